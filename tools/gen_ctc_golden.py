"""Write tests/golden/ctc_tiny.npz: the CTC recognition model (`CTCRecModel`, models/model_builder.py:8-38) and its string rule
(`ctc_get_str_list` / `CTCAccuracy`, evaluation_metric/metrics.py:205-251) from the UNMODIFIED reference.  The class is the reference's own; only
the encoder factory it calls is pointed at the TINY encoder of finetune_tiny.npz (dig_oracle.TINY: no registered factory has that width).
B = 4, nb_classes = 37 (+ 1 blank), every drop rate 0.  The file holds

  * the state dict as names, shapes, norms and eight samples per tensor -- the values themselves are the deterministic tensors of
    tests/ctc_model.state(seed_enc, seed_head): in full they would pass the size cap of a committed file;
  * images (by seed), targets and lengths; the reference's logits (fp32);
  * fp64: `F.ctc_loss` per sample on the reference model run in double (`nll`), the loss under this project's reduction (sum / B), and the norm and
    eight samples of every parameter's gradient of that loss;
  * for the evaluation, with the last Linear scaled by `cls_scale` (evaluation only): the reference's logits, the per-frame arg-max, which frames
    are clear of a tie (top-2 probability margin above MARGIN), the reference's strings and CTCAccuracy;
  * the same strings and accuracy for a hand-made [6, 32] matrix of frame classes: runs, blank-separated repeats, EOS in the middle, UNKNOWN,
    all blank, 32 distinct symbols;
  * key names and shapes of the reference's full-size CTCRecModel(args) for the three encoders.
At most 1/8 of the frames may be unclear: the seed and the scale are searched until the reference alone meets that, and it is asserted.  Asserts
that tests/ctc_model.py reproduces the reference before writing.  Data only.

    python tools/gen_ctc_golden.py        # needs the reference checkout (oracle/ref_harness/refenv.py); runs on the CPU
"""
import os
import sys
import types
from functools import partial

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "oracle", "ref_harness"), os.path.join(ROOT, "tests")]
import dig_oracle as O  # noqa: E402
import refenv  # noqa: E402
from gen_finetune_golden import sample_index  # noqa: E402
import ctc_model as S  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
B, T, NB, MAX_LEN, MARGIN = 4, 32, 37, 8, 6e-2
VOC = list("0123456789abcdefghijklABCDEFGHIJKL") + ["EOS", "PADDING", "UNKNOWN"]      # 34 characters + the three special classes = NB
EOS, PAD, UNK, BLANK = 34, 35, 36, 37
FULL = ("simmim_vit_tiny_patch4_32x128", "simmim_vit_small_patch4_32x128", "simmim_vit_base_patch4_32x128")


def samples(t):
    return np.resize(t.reshape(-1)[sample_index(t.numel())].numpy(), 8)


class Dataset:
    """What ctc_get_str_list reads of a dataset (dataset/dataset_lmdb.py:75-97)."""
    classes = VOC
    class_to_idx = dict(zip(VOC, range(len(VOC))))
    idx_to_class = dict(zip(range(len(VOC)), VOC))


def hand_made():
    a, b, c = VOC.index("a"), VOC.index("b"), VOC.index("C")
    rows = torch.full((6, T), BLANK, dtype=torch.int64)
    rows[0, :12] = torch.tensor([a, a, a, b, b, BLANK, BLANK, c, c, c, c, 3])                       # runs
    rows[1, :9] = torch.tensor([a, BLANK, a, BLANK, BLANK, a, b, BLANK, b])                          # blank-separated repeats
    rows[2, 2:12] = torch.tensor([a, b, EOS, EOS, c, BLANK, EOS, a, a, 7])                           # EOS in the middle: dropped, not a cut
    rows[3, 1:10] = torch.tensor([UNK, a, UNK, UNK, b, PAD, c, UNK, c])                              # UNKNOWN (and PADDING) frames
    rows[5] = torch.arange(T)                                                                        # 32 distinct symbols; row 4: all blank
    words = ["aabc3", "aaabb", "abca7", "abcd", "", "".join(VOC[:T])]
    targets = torch.full((6, T + 2), PAD, dtype=torch.int64)
    for i, w in enumerate(words):
        targets[i, :len(w)] = torch.tensor([VOC.index(ch) for ch in w])
        targets[i, len(w)] = EOS
    targets[3, 1] = UNK                                                                              # an UNKNOWN inside a target: dropped there too
    return rows, targets


def main():
    refenv.setup()
    torch.manual_seed(0)
    import models.model_builder as MB
    import modeling_pretrain_vit as V
    try:
        import editdistance  # noqa: F401
    except ImportError:
        # metrics.py imports it at the top; the two functions read here never call it, so where it is not installed a stand-in that refuses
        # to compute anything lets the module import (the way refenv's shims stand in for timm)
        def refuse(*a, **k):
            raise RuntimeError("editdistance is not installed")
        sys.modules["editdistance"] = types.SimpleNamespace(eval=refuse)
    from evaluation_metric.metrics import CTCAccuracy, ctc_get_str_list
    ecfg = O.DiGConfig(**O.TINY)
    tiny = lambda args: V.PretrainVisionTransformerEncoder(img_size=(32, 128), patch_size=4, embed_dim=ecfg.embed_dim, depth=ecfg.depth,
                                                           num_heads=ecfg.heads, mlp_ratio=4, qkv_bias=True, norm_layer=partial(nn.LayerNorm, eps=1e-6),
                                                           num_classes=0, drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.0)
    args = types.SimpleNamespace(model="tiny", nb_classes=NB, max_len=MAX_LEN, drop=0.0, drop_path=0.0, attn_drop_rate=0.0, use_mean_pooling=False,
                                 init_scale=0.001, use_seq_cls_token=False)
    factory, MB.create_encoder = MB.create_encoder, tiny
    try:
        model = MB.CTCRecModel(args)
    finally:
        MB.create_encoder = factory
    fin = np.load(os.path.join(GOLD, "finetune_tiny.npz"))
    seed_enc, batch_seed = int(fin["seed_enc"]), int(fin["batch_seed"])
    images = O.synthetic_batch(B, ecfg, batch_seed)[0]
    ds = Dataset()

    def load(P):
        sd = model.state_dict()
        assert set(P) <= set(sd) and all(k in P or k.startswith(("patch_embed.", "pos_embed")) for k in sd), sorted(set(sd) - set(P))
        for k, v in P.items():
            assert sd[k].shape == v.shape, k
            sd[k].copy_(v)

    found = None
    for scale in (1.0, 2.0, 4.0, 8.0, 16.0, 32.0):                          # the smallest scale first, then the seeds
        for seed in range(71, 111):
            P0 = S.state(ecfg, NB, seed_enc, seed)
            P = dict(P0)
            P["ctc_classifier.3.weight"], P["ctc_classifier.3.bias"] = P0["ctc_classifier.3.weight"] * scale, P0["ctc_classifier.3.bias"] * scale
            load(P)
            model.eval()
            with torch.no_grad():
                ev = model((images, None, None))
            top2 = ev.softmax(-1).topk(2, -1).values
            clear = (top2[..., 0] - top2[..., 1]) > MARGIN
            if int((~clear).sum()) * 8 <= clear.numel():
                found = (seed, scale, P0, P, ev, clear)
                break
        if found:
            break
    assert found
    seed, scale, P0, P, ev, clear = found
    assert int((~clear).sum()) * 8 <= clear.numel()
    print(f"head seed {seed}, classifier scale {scale}: {int(clear.sum())} of {clear.numel()} frames clear of a tie (margin {MARGIN})")
    frames = ev.argmax(-1)
    # ---- targets: an empty word, a repeated character, a full row, a mixed one; lengths count the closing EOS
    words = [[], [5, 5, 12], [3, 9, 9, 20, 33, 1, 0], [14, 2, 14, 2]]
    targets = torch.full((B, MAX_LEN), PAD, dtype=torch.int64)
    for b, w in enumerate(words):
        targets[b, :len(w)] = torch.tensor(w, dtype=torch.int64)
        targets[b, len(w)] = EOS
    lens = torch.tensor([len(w) + 1 for w in words], dtype=torch.int64)
    pred, targ = ctc_get_str_list(frames, targets, ds)
    acc = CTCAccuracy(frames, targets, ds)
    assert pred == S.frames_to_strings(frames, VOC, BLANK)
    assert (S.logits(P, ecfg, images) - ev).abs().max() < 3e-5 * scale
    # ---- the training step with the head as seeded: the reference's logits in fp32, loss and gradients from the model run in double
    load(P0)
    model.train()
    ref_logits = model((images, targets, lens)).detach().clone()
    model.double()
    load({k: v.double() for k, v in P0.items()})
    lg = model((images.double(), targets, lens))
    nll = TF.ctc_loss(TF.log_softmax(lg, -1).transpose(0, 1), targets, torch.full((B,), T, dtype=torch.int64), lens - 1, blank=BLANK,
                      reduction="none", zero_infinity=True)
    loss = nll.sum() / B
    model.zero_grad()
    loss.backward()
    seen = set()
    ref_grads = {}
    for n_, p in model.named_parameters():                                  # (the aliases patch_embed / pos_embed repeat encoder tensors)
        if p.grad is not None and n_ in P0 and id(p) not in seen:
            ref_grads[n_] = p.grad.detach().clone()
            seen.add(id(p))
    assert set(ref_grads) == set(P0) - {"encoder.mask_token"}, sorted(set(P0) - set(ref_grads))
    P64 = {k: v.double() for k, v in P0.items()}
    o_loss, o_grads, o_logits = S.loss_and_grads(P64, ecfg, images.double(), targets, lens, BLANK)
    assert abs(o_loss - loss.item()) < 1e-9 * abs(loss.item()), (o_loss, loss.item())
    assert (o_logits - lg.detach()).abs().max() < 1e-9 and (S.logits(P0, ecfg, images) - ref_logits).abs().max() < 3e-5
    worst = max((o_grads[n_] - g).abs().max().item() / (g.abs().max().item() + 1e-300) for n_, g in ref_grads.items())
    assert worst < 1e-7, worst
    print(f"tests/ctc_model.py == reference (loss {loss.item():.6f}, nll {nll.tolist()}, worst gradient rel-to-max err {worst:.2e})")
    model.float()
    names = [n_ for n_ in P0 if n_ in ref_grads]
    hand, hand_targets = hand_made()
    h_pred, h_targ = ctc_get_str_list(hand, hand_targets, ds)
    h_acc = CTCAccuracy(hand, hand_targets, ds)
    assert h_pred == S.frames_to_strings(hand, VOC, BLANK)
    print("hand-made rows:", h_pred, h_targ, h_acc)
    out = {"margin": MARGIN, "voc": np.array(VOC), "nb_classes": NB, "B": B, "T": T, "max_len": MAX_LEN, "seed_enc": seed_enc, "seed_head": seed,
           "batch_seed": batch_seed, "cls_scale": scale,
           "state_names": np.array(list(P0)), "state_shapes": np.array([list(v.shape) + [0] * (4 - v.dim()) for v in P0.values()], dtype=np.int64),
           "state_norms": np.array([v.double().norm().item() for v in P0.values()]), "state_samples": np.stack([samples(v) for v in P0.values()]),
           "targets": targets.numpy(), "lens": lens.numpy(), "logits": ref_logits.numpy(), "nll": nll.detach().numpy(), "loss": np.float64(loss.item()),
           "grad_names": np.array(names), "grad_norms": np.array([ref_grads[n_].norm().item() for n_ in names]),
           "grad_samples": np.stack([samples(ref_grads[n_]) for n_ in names]),
           "eval_logits": ev.numpy(), "eval_frames": frames.numpy(), "eval_clear": clear.numpy(), "eval_pred_strings": np.array(pred),
           "eval_targ_strings": np.array(targ), "eval_ctc_accuracy": np.float64(acc),
           "hand_frames": hand.numpy(), "hand_targets": hand_targets.numpy(), "hand_pred_strings": np.array(h_pred),
           "hand_targ_strings": np.array(h_targ), "hand_ctc_accuracy": np.float64(h_acc)}
    # ---- the real CTCRecModel(args) on the three encoders: key names and shapes of its state_dict
    for encoder in FULL:
        a = types.SimpleNamespace(model=encoder, nb_classes=97, max_len=25, drop=0.0, drop_path=0.0, attn_drop_rate=0.0, use_mean_pooling=False,
                                  init_scale=0.001, use_seq_cls_token=False)
        sd = MB.CTCRecModel(a).state_dict()
        out["keys/" + encoder] = np.array(list(sd.keys()))
        out["shapes/" + encoder] = np.array([list(v.shape) + [0] * (4 - v.dim()) for v in sd.values()], dtype=np.int64)
        print(f"CTCRecModel on {encoder}: {len(sd)} state_dict entries")
    out["keys/tiny"] = np.array(list(model.state_dict().keys()))
    out["shapes/tiny"] = np.array([list(v.shape) + [0] * (4 - v.dim()) for v in model.state_dict().values()], dtype=np.int64)
    path = os.path.join(GOLD, "ctc_tiny.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size <= 128 << 10, size                                          # (two logit tensors and the three key lists; a committed file stays small)
    print(f"wrote {path} ({size} bytes)")


if __name__ == "__main__":
    main()
