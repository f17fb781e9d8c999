"""Write tests/golden/corres_decoder_tiny.npz: the recognition decoder at head dims 24 and 48 (the `corres_*_tf_decoder` family, models/decoder.py:35-72)
from the UNMODIFIED reference classes.  Two tiny configurations on dig_oracle.TINY's encoder, both 2 layers, d_model 192, d_inner 64, max_seq_len 8:
`h8k24` (8 heads x d_k 24) and `h4k48` (4 heads x d_k 48).  Per configuration, from the reference's TFDecoder with every drop rate 0: one
teacher-forced training step (logits, loss, sampled gradients and the norm of every tensor), greedy decoding (probabilities, tokens, sampled
attention maps) and beam search at width 2 (the best hypothesis per sample).  Also the state_dict key names and shapes of the reference's own
RecModel(args) for the three `corres_*` names.  Asserts that oracle/decode_oracle.py and oracle/finetune_oracle.py reproduce the reference at these
configurations (the bounds of the other generators) before writing.  Data only.

Tokens are compared across precisions only where the reference is not near a tie (MARGIN, as tools/gen_text_cond_golden.py).  Greedy: a position
is clear when the top-2 margin of its probabilities exceeds MARGIN.  Beam search: a sample is clear when at every step the two best of the
beam_width * classes candidates, as probabilities normalised over the step's candidates, are more than MARGIN apart (with one live slot this is
the greedy rule) and its best hypothesis is the chain of those best candidates.  At most 1/8 of the positions may be unclear under either rule:
the seeds and the classifier scale (applied for the evaluation only) are searched until that holds.

    python tools/gen_corres_decoder_golden.py        # needs the reference checkout (oracle/ref_harness/refenv.py); runs on the CPU
"""
import os
import sys
import types
from functools import partial

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "oracle", "ref_harness")]
import decode_oracle as D  # noqa: E402
import dig_oracle as O  # noqa: E402
import finetune_oracle as F  # noqa: E402
import refenv  # noqa: E402
from gen_finetune_golden import TinyRec, sample_index  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
CONFIGS = {"h8k24": dict(n_layers=2, d_model=192, n_head=8, d_k=24, d_inner=64, max_seq_len=8, enc_dim=128),
           "h4k48": dict(n_layers=2, d_model=192, n_head=4, d_k=48, d_inner=64, max_seq_len=8, enc_dim=128)}
FULL = {"corres_tiny_tf_decoder": "simmim_vit_tiny_patch4_32x128", "corres_small_tf_decoder": "simmim_vit_small_patch4_32x128",
        "corres_base_tf_decoder": "simmim_vit_base_patch4_32x128"}
B, BW, EOS, MARGIN = 2, 2, 94, 6e-2


def samples(t):
    return np.resize(t.reshape(-1)[sample_index(t.numel())].numpy(), 8)


def beam_clear(step_logits, ids, nb, bw, eos, margin):
    """The rule of the module docstring on the classifier outputs [T, nb*bw, C] of the reference's search: per sample, every step's two best
    candidates more than `margin` apart as normalised probabilities, and `ids` the chain of the best candidates."""
    T, S, C = step_logits.shape
    seq = torch.full((S, 1), -float("inf")); seq[torch.arange(nb) * bw] = 0.0
    ok = torch.ones(nb, dtype=torch.bool)
    for t in range(T):
        cand = (seq.repeat(1, C) + step_logits[t].log_softmax(-1)).view(nb, -1)
        top = cand.softmax(-1).topk(2, -1).values
        sc, ci = cand.topk(bw, dim=1)
        sym = (ci % C).view(S)
        ok &= (top[:, 0] - top[:, 1]) > margin
        ok &= sym.view(nb, bw)[:, 0] == ids[:, t]
        if t:
            ok &= (ci // C)[:, 0] == 0                                   # the best candidate continues the best slot
        seq = sc.view(S, 1).masked_fill(sym.view(-1, 1).eq(eos), -float("inf"))
    return ok


def one_config(tag, cfg, V, TFDecoder, ref_ce):
    c, ecfg = D.DecoderConfig(**cfg), O.DiGConfig(**O.TINY)
    enc = V.PretrainVisionTransformerEncoder(img_size=(32, 128), patch_size=4, embed_dim=ecfg.embed_dim, depth=ecfg.depth, num_heads=ecfg.heads,
                                             mlp_ratio=4, qkv_bias=True, norm_layer=partial(nn.LayerNorm, eps=1e-6), num_classes=0, drop_rate=0.0,
                                             attn_drop_rate=0.0, drop_path_rate=0.0)
    dec = TFDecoder(n_layers=c.n_layers, d_embedding=c.d_model, n_head=c.n_head, d_k=c.d_k, d_v=c.d_k, d_model=c.d_model, d_inner=c.d_inner,
                    num_classes=c.num_classes, max_seq_len=c.max_seq_len, dropout=0.0)
    ln = nn.Sequential(nn.Linear(ecfg.embed_dim, c.d_model), nn.LayerNorm(c.d_model))
    model = TinyRec(enc, ln, dec)
    T = c.max_seq_len
    found = None
    # the smallest classifier scale first (the bf16 error of the logits grows with it), then the seeds
    for scale in (1.0, 2.0, 4.0, 8.0, 16.0, 32.0):
        for seed in range(61, 101):                                     # (seed_enc, seed_dec, batch_seed) = (seed + 1, seed, 500 + seed)
            P0 = {**D.det_encoder_state(ecfg, seed + 1), **D.det_decoder_state(c, seed)}
            images = O.synthetic_batch(B, ecfg, 500 + seed)[0]
            P = dict(P0)
            P["decoder.classifier.weight"] = P0["decoder.classifier.weight"] * scale
            sd = model.state_dict()
            for k, v in P.items():
                sd[k].copy_(v)
            model.eval()
            with torch.no_grad():
                probs, _, _, maps = model((images, None, None))
                top2 = probs.topk(2, -1).values
                clear = (top2[..., 0] - top2[..., 1]) > MARGIN
                if int((~clear).sum()) * 8 > clear.numel():
                    continue
                mem_ref = model.linear_norm(model.encoder(images))
                rec = []
                h = dec.classifier.register_forward_hook(lambda _m, _i, out: rec.append(out.detach().clone()))
                ids, _ = dec.beam_search(None, mem_ref, None, None, None, BW, eos=EOS)
                h.remove()
            bclear = beam_clear(torch.stack(rec), ids, B, BW, EOS, MARGIN)
            if int((~bclear).sum()) * 8 <= B:
                found = (seed, scale, P0, P, images, probs, maps, clear, ids, bclear)
                break
        if found:
            break
    assert found, tag
    seed, scale, P0, P, images, probs, maps, clear, ids, bclear = found
    print(f"{tag}: seed {seed}, classifier scale {scale}: {int(clear.sum())} of {clear.numel()} greedy positions and {int(bclear.sum())} of {B} "
          f"beam samples clear of a tie (margin {MARGIN})")
    tokens = probs.argmax(-1)
    # ---- the oracles reproduce the reference's evaluation
    o_probs, o_maps, o_tok = D.recognize(P, ecfg, c, images, cached=True)
    assert (o_probs - probs).abs().max() < 2e-5 and (o_maps - maps).abs().max() < 2e-5 and torch.equal(o_tok, tokens), tag
    e = D.encoder_features(P, ecfg, images)
    mem = torch.nn.functional.layer_norm(e @ P["linear_norm.0.weight"].t() + P["linear_norm.0.bias"], (c.d_model,), P["linear_norm.1.weight"],
                                         P["linear_norm.1.bias"], 1e-5)
    assert torch.equal(D.beam_search(P, c, mem, BW, EOS), ids), tag
    # ---- teacher-forced training step, with the classifier as seeded (`cls_scale` applies to the evaluation only: the bounds below are the
    # other generators', which hold for logits of their size)
    P = P0
    sd = model.state_dict()
    for k, v in P.items():
        sd[k].copy_(v)
    rng = np.random.RandomState(seed)
    lens = torch.from_numpy(rng.randint(1, T + 1, size=B))
    lens[0], lens[1] = 1, T                                               # both extremes
    targets = torch.from_numpy(rng.randint(0, 94, size=(B, T)))
    for b in range(B):
        targets[b, int(lens[b]) - 1] = 94
        targets[b, int(lens[b]):] = 95
    model.train()
    outputs, _, _, _ = model((images, targets, lens))
    loss = ref_ce.SeqCrossEntropyLoss()(outputs, targets, lens)
    model.zero_grad()
    loss.backward()
    ref_grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    assert set(ref_grads) == set(P) - {"encoder.mask_token"}
    o_loss, o_grads, o_logits = F.loss_and_grads(P, ecfg, c, images, targets, lens)
    assert abs(o_loss - loss.item()) < 1e-5 * abs(loss.item()), (o_loss, loss.item())
    assert (o_logits - outputs.detach()).abs().max() < 3e-5
    worst = max((o_grads[n] - g).abs().max().item() / (g.abs().max().item() + 1e-12) for n, g in ref_grads.items())
    assert worst < 2e-3, (tag, worst)
    print(f"{tag}: oracles == reference (loss {loss.item():.6f}, worst gradient rel-to-max err {worst:.2e}; greedy and beam-{BW} tokens equal)")
    names = [n for n in P if n in ref_grads]
    pre = tag + "/"
    return {pre + "config": np.array([c.n_layers, c.d_model, c.n_head, c.d_k, c.d_inner, c.max_seq_len, c.enc_dim]), pre + "seed_enc": seed + 1,
            pre + "seed_dec": seed, pre + "batch_seed": 500 + seed, pre + "B": B, pre + "cls_scale": scale, pre + "targets": targets.numpy(),
            pre + "lens": lens.numpy(), pre + "loss": np.float64(loss.item()), pre + "logits": outputs.detach().numpy(),
            pre + "grad_names": np.array(names), pre + "grad_norms": np.array([ref_grads[n].double().norm().item() for n in names]),
            pre + "grad_samples": np.stack([samples(ref_grads[n]) for n in names]), pre + "greedy_probs": probs.numpy(),
            pre + "greedy_tokens": tokens.numpy(), pre + "greedy_clear": clear.numpy(),
            pre + "greedy_map_norms": maps.double().norm(dim=-1).numpy(),
            pre + "greedy_map_samples": np.stack([samples(m) for m in maps.reshape(-1, maps.shape[-1])]),
            pre + "beam_ids": ids.numpy(), pre + "beam_clear": bclear.numpy()}


def main():
    refenv.setup()
    torch.manual_seed(0)
    from models.decoder import TFDecoder
    from models.model_builder import RecModel
    import modeling_pretrain_vit as V
    import importlib.util
    spec = importlib.util.spec_from_file_location("ref_seq_ce", os.path.join(refenv.REF, "loss", "seqCrossEntropyLoss.py"))
    ref_ce = importlib.util.module_from_spec(spec); spec.loader.exec_module(ref_ce)
    out = {"margin": MARGIN, "beam_width": BW, "eos": EOS, "tags": np.array(list(CONFIGS))}
    for tag, cfg in CONFIGS.items():
        out.update(one_config(tag, cfg, V, TFDecoder, ref_ce))
    # ---- the real RecModel with the three decoders: key names and shapes of its state_dict (a list of names and shapes)
    for name, encoder in FULL.items():
        args = types.SimpleNamespace(model=encoder, decoder_name=name, nb_classes=97, max_len=25, drop=0.0, drop_path=0.0, attn_drop_rate=0.0,
                                     use_mean_pooling=False, init_scale=0.001, use_seq_cls_token=False, use_1d_attdec=False, text_cond_vis=False,
                                     beam_width=0)
        sd = RecModel(args).state_dict()
        out["keys/" + name] = np.array(list(sd.keys()))
        out["shapes/" + name] = np.array([list(v.shape) + [0] * (4 - v.dim()) for v in sd.values()], dtype=np.int64)
        out["encoder/" + name] = encoder
        print(f"{name} on {encoder}: {len(sd)} state_dict entries")
    path = os.path.join(GOLD, "corres_decoder_tiny.npz")
    np.savez_compressed(path, **out)
    size, cap = os.path.getsize(path), 2 * os.path.getsize(os.path.join(GOLD, "finetune_tiny.npz"))
    assert size <= cap, (size, cap)
    print(f"wrote {path} ({size} bytes)")


if __name__ == "__main__":
    main()
