"""Write tests/golden/text_cond_tiny.npz: the recognition decoder with `--text_cond_vis` from the UNMODIFIED reference classes (TFDecoder with
TextConditionalMultiHeadAttention cross-attention, models/decoder.py / models/transformer_layer.py:284-383) at decode_oracle.TINY widths --
one teacher-forced training step (logits, loss, every gradient), greedy decoding (probabilities, tokens, attention maps), beam search (width 2:
the symbols of every step and the result, plain and with forced classifier outputs; the step logits are asserted here, not stored), one attention module alone (output, map, gradients) and the
state_dict key list.  Asserts that tests/textcond_model.py, literal and folded, equals the reference before writing.  Data only.

    python tools/gen_text_cond_golden.py        # needs the reference checkout (oracle/ref_harness/refenv.py); runs on the CPU
"""
import os
import sys
from functools import partial

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "oracle", "ref_harness")]
import decode_oracle as D  # noqa: E402
import dig_oracle as O  # noqa: E402
import refenv  # noqa: E402
import textcond_model as TC  # noqa: E402
from gen_finetune_golden import TinyRec, sample_index  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
SEED_ENC, SEED_DEC, SEED_TCV, BATCH_SEED, B, BW, EOS, MARGIN = 52, 51, 53, 575, 2, 2, 94, 6e-2


def samples(t):
    return np.resize(t.reshape(-1)[sample_index(t.numel())].numpy(), 8)


def rel_to_max(a, b):
    return (a - b).abs().max().item() / (b.abs().max().item() + 1e-12)


def main():
    refenv.setup()
    torch.manual_seed(0)
    from models.decoder import TFDecoder
    from models.transformer_layer import TextConditionalMultiHeadAttention
    import modeling_pretrain_vit as V
    import importlib.util
    spec = importlib.util.spec_from_file_location("ref_seq_ce", os.path.join(refenv.REF, "loss", "seqCrossEntropyLoss.py"))
    ref_ce = importlib.util.module_from_spec(spec); spec.loader.exec_module(ref_ce)
    c, ecfg = D.DecoderConfig(**D.TINY), O.DiGConfig(**O.TINY)
    enc = V.PretrainVisionTransformerEncoder(img_size=(32, 128), patch_size=4, embed_dim=ecfg.embed_dim, depth=ecfg.depth, num_heads=ecfg.heads,
                                             mlp_ratio=4, qkv_bias=True, norm_layer=partial(nn.LayerNorm, eps=1e-6), num_classes=0, drop_rate=0.0,
                                             attn_drop_rate=0.0, drop_path_rate=0.0)
    dec = TFDecoder(n_layers=c.n_layers, d_embedding=c.d_model, n_head=c.n_head, d_k=c.d_k, d_v=c.d_k, d_model=c.d_model, d_inner=c.d_inner,
                    num_classes=c.num_classes, max_seq_len=c.max_seq_len, dropout=0.0, text_cond_vis=True)
    ln = nn.Sequential(nn.Linear(ecfg.embed_dim, c.d_model), nn.LayerNorm(c.d_model))
    model = TinyRec(enc, ln, dec)
    keys = [k for k in model.state_dict() if not k.endswith("position_table")]
    P0 = {**D.det_encoder_state(ecfg, SEED_ENC), **D.det_decoder_state(c, SEED_DEC), **TC.det_text_cond_state(c, SEED_TCV)}
    assert set(keys) == set(P0), sorted(set(keys) ^ set(P0))
    images = O.synthetic_batch(B, ecfg, BATCH_SEED)[0]

    def load(P):
        sd = model.state_dict()
        for k, v in P.items():
            sd[k].copy_(v)

    # the classifier scale: the smallest power of two at which at least half of the greedy positions have a top-2 margin above MARGIN
    for scale in (1.0, 2.0, 4.0, 8.0, 16.0, 32.0):
        P = dict(P0)
        P["decoder.classifier.weight"] = P0["decoder.classifier.weight"] * scale
        load(P)
        model.eval()
        with torch.no_grad():
            probs, _, _, maps = model((images, None, None))
        top2 = probs.topk(2, -1).values
        clear = (top2[..., 0] - top2[..., 1]) > MARGIN
        if int(clear.sum()) * 2 >= clear.numel():
            break
    assert int(clear.sum()) * 2 >= clear.numel(), int(clear.sum())
    print(f"classifier scale {scale}: {int(clear.sum())} of {clear.numel()} greedy positions with a top-2 margin above {MARGIN}")
    tokens = probs.argmax(-1)
    mem = TC.memory_of(P, ecfg, c, images)
    for attn in (TC.attn_folded, TC.attn_literal):
        o_probs, o_maps, o_tok = TC.greedy_decode(P, c, mem, attn=attn)
        assert (o_probs - probs).abs().max() < 2e-5 and (o_maps - maps).abs().max() < 2e-5 and torch.equal(o_tok, tokens), attn.__name__

    # ---- teacher-forced training step
    rng = np.random.RandomState(29)
    lens = torch.from_numpy(rng.randint(2, c.max_seq_len + 1, size=B))
    targets = torch.from_numpy(rng.randint(0, 94, size=(B, c.max_seq_len)))
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
    for attn in (TC.attn_folded, TC.attn_literal):
        o_loss, o_grads, o_logits = TC.loss_and_grads(P, ecfg, c, images, targets, lens, attn=attn)
        assert abs(o_loss - loss.item()) < 1e-5 * abs(loss.item()), (o_loss, loss.item())
        assert (o_logits - outputs.detach()).abs().max() < 3e-5
        worst = max(rel_to_max(o_grads[n], g) for n, g in ref_grads.items())
        assert worst < 2e-3, (attn.__name__, worst)
    print(f"training step: specification == reference (loss {loss.item():.6f}, worst gradient rel-to-max err {worst:.2e})")
    names = [n for n in P if n in ref_grads]

    # ---- beam search, width BW: the classifier's outputs of every step are recorded (plain) or replaced (forced) by a forward hook
    model.eval()
    T, S = c.max_seq_len, B * BW
    forced = O.det_tensor("beam_force", (T, S, c.num_classes), SEED_TCV, 2.0)
    mem_ref = model.linear_norm(model.encoder(images)).detach()
    rec, step = [], [0]

    def hook(_m, _i, out, force=None):
        rec.append(out.detach().clone())
        step[0] += 1
        return None if force is None else force[step[0] - 1]

    beams = {}
    for tag, force in (("plain", None), ("forced", forced)):
        rec.clear(); step[0] = 0
        h = dec.classifier.register_forward_hook(partial(hook, force=force))
        with torch.no_grad():
            ids, _ = dec.beam_search(None, mem_ref, None, None, None, BW, eos=EOS)
        h.remove()
        mine, lg, syms = TC.beam_search(P, c, mem, BW, EOS, force_logits=force)
        assert torch.equal(mine, ids), tag
        assert (lg - torch.stack(rec)).abs().max() < 3e-5, tag
        beams[tag] = (ids.numpy(), torch.stack(rec), syms.numpy())
    print("beam search: specification == reference; plain", beams["plain"][0][0].tolist(), "forced", beams["forced"][0][0].tolist())

    # ---- one attention module alone
    mod = TextConditionalMultiHeadAttention(n_head=c.n_head, d_model=c.d_model, d_k=c.d_k, d_v=c.d_k, dropout=0.0)
    pre = "decoder.layer_stack.0.enc_attn."
    msd = mod.state_dict()
    for k in msd:
        msd[k].copy_(P[pre + k])
    q_in = O.det_tensor("tcv_q", (1, 3, c.d_model), SEED_TCV, 1.0).requires_grad_(True)
    kv_in = O.det_tensor("tcv_mem", (1, 5, c.d_model), SEED_TCV, 1.0).requires_grad_(True)
    dout = O.det_tensor("tcv_dout", (1, 3, c.d_model), SEED_TCV, 1.0)
    out, amap = mod(q_in, kv_in, kv_in, return_attn_map=True)
    (out * dout).sum().backward()
    mgrads = {pre + n: p.grad.detach() for n, p in mod.named_parameters()}
    mgrads["q_in"], mgrads["mem_in"] = q_in.grad, kv_in.grad
    for attn in (TC.attn_folded, TC.attn_literal):
        Q = {k: v.detach().clone().requires_grad_(True) for k, v in P.items() if k.startswith(pre)}
        q2, m2 = q_in.detach().clone().requires_grad_(True), kv_in.detach().clone().requires_grad_(True)
        o2, map2 = attn(Q, pre, c, q2, m2)
        (o2 * dout).sum().backward()
        assert (o2 - out).abs().max() < 2e-5 and (map2 - amap).abs().max() < 2e-6
        got = {**{k: v.grad for k, v in Q.items()}, "q_in": q2.grad, "mem_in": m2.grad}
        worst = max(rel_to_max(got[n], g) for n, g in mgrads.items())
        assert worst < 1e-3, (attn.__name__, worst)
    print(f"attention module: specification == reference (worst gradient rel-to-max err {worst:.2e})")
    mnames = list(mgrads)

    path = os.path.join(GOLD, "text_cond_tiny.npz")
    np.savez_compressed(
        path, seed_enc=SEED_ENC, seed_dec=SEED_DEC, seed_tcv=SEED_TCV, batch_seed=BATCH_SEED, B=B, cls_scale=scale, state_keys=np.array(keys),
        targets=targets.numpy(), lens=lens.numpy(), loss=np.float64(loss.item()), logits=outputs.detach().numpy(), grad_names=np.array(names),
        grad_norms=np.array([ref_grads[n].double().norm().item() for n in names]), grad_samples=np.stack([samples(ref_grads[n]) for n in names]),
        greedy_probs=probs.numpy(), greedy_tokens=tokens.numpy(), greedy_clear=clear.numpy(), n_clear=int(clear.sum()), margin=MARGIN,
        greedy_map_norms=maps.double().norm(dim=-1).numpy(), greedy_map_samples=np.stack([samples(m) for m in maps.reshape(-1, maps.shape[-1])]),
        beam_width=BW, eos=EOS, beam_ids_plain=beams["plain"][0],
        beam_syms_plain=beams["plain"][2], beam_ids_forced=beams["forced"][0], beam_force_scale=2.0,
        mod_out=out.detach().numpy(), mod_map=amap.detach().numpy(), mod_grad_names=np.array(mnames),
        mod_grad_norms=np.array([mgrads[n].double().norm().item() for n in mnames]), mod_grad_samples=np.stack([samples(mgrads[n]) for n in mnames]))
    size, cap = os.path.getsize(path), os.path.getsize(os.path.join(GOLD, "finetune_tiny.npz"))
    assert size <= cap, (size, cap)
    print(f"wrote {path} ({size} bytes)")


if __name__ == "__main__":
    main()
