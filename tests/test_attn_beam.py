"""Beam search of the GRU attention head (`--decoder_type attention --beam_width K`): the two kernels that make it (`dig_addattn_fwd_slots`,
csrc/gru_attn.hip; `dig_attn_beam_advance`, csrc/decode.hip) on both builds of the ABI, the specification (tests/attn_beam_model.py) on its
own, `AttnRecModelTrain.beam_search` on the MI355X against the specification, and the host / driver wiring.

1. dig_addattn_fwd_slots against float64 on bf16-rounded operands, criterion and helpers of tests/test_gru_attn_kernels.py.  Bound per
   output = max(that module's TAU[backend], 2 x the term dig_addattn_fwd reaches on the same case with the tokens inflated K times), never
   above TAU_CAP; the factor 2 is for the other summation order of the softmax (a wave per slot) only.  Largest terms measured:
       output         MI355X      CPU build
       alpha (fp32)   5.112e-07   6.731e-06      (TAU 3e-06 / 3e-05)
       ctx (bf16)     1.851e-08   1.060e-06      (TAU 4e-07 / 2e-06)
   On the device the largest alpha term is dig_addattn_fwd's own on that case (5.112e-07 both); where the two differ the slots kernel is at
   most 1.4 x dig_addattn_fwd's term (3.537e-07 against 2.610e-07).  The CPU build runs dig_addattn_fwd's loops per slot and reaches its bits.
2. dig_attn_beam_advance: bit-equal to dig_beam_step in what both compute; the gathers and the embedding rows bit-exact.
3. The specification: width 1 = the greedy head_sample; its restated back-tracking = dig_amd.recognizer.beam_backtrack.
4. The model.  Yardstick e_bf = the largest |score difference| between the specification under torch.autocast("cpu", bfloat16) and in
   float64 along the float64 decisions (computed and printed by the tests); bound 4 x e_bf (the device rounds the same operands to bf16
   but sums in fp32 and in another order).  Measured on the tiny fixture model, widths 1 / 3 / 5 / 8: e_bf 2.3e-2 (2.3e-2 .. 2.5e-2 with the
   host's bf16 GEMM path); forced decisions: max |score - specification| 2.0e-2 .. 2.2e-2 against a bound of 9e-2; free run: worst shortfall
   -2.9e-1 (width 1: the greedy margin) / 3.1e-3 / -7.4e-4 / 4.2e-3; with eos = 18 (width 5: 37 masked slots, every best hypothesis ends at
   length 1) 2.0e-2 and 8.4e-4; greedy top-2 margin 0.287 against 8 e_bf = 0.18.  Full-size head (ViT-S tokens, sDim = attDim = 512, B = 4,
   K = 5): e_bf 3.1e-2, forced 1.9e-2, free 1.2e-3 against a bound of 1.2e-1.
5. Host and driver."""
import math
import os
import types

import numpy as np
import pytest
import torch

import attn_decoder_oracle as AD
import decode_oracle as D
import dig_oracle as O
import attn_beam_model as SPEC
from test_gru_attn_kernels import BF, F32, TAU, TAU_CAP, _backend, _is_poison, _poisoned, _tau_term

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
I64 = torch.int64
NEG_INF = float("-inf")


def _sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 1. dig_addattn_fwd_slots
SLOT_CASES = [(2, 256, 512, 384, 5, 512),     # the workload's shape, ldc > X, split-token contexts
              (1, 512, 1024, 768, 8, 0),      # the LDS maximum: 53,248 B; one-thread-per-pair contexts
              (1, 7, 520, 520, 8, 8),         # partial passes of the score loop, N below the 8 waves
              (3, 1, 8, 8, 2, 0),             # N = 1: alpha exactly 1
              (2, 65, 72, 40, 3, 24),         # odd shape
              (2, 70, 64, 128, 1, 0)]         # K = 1; partial contexts (K * X floats) larger than the sproj rows they overwrite
_REF = {}


def _slots_ref(case, amp):
    key = (case, amp)
    if key not in _REF:
        B, N, A, X, K, E = case
        g = torch.Generator().manual_seed(2000 * amp + N + A + X + K)
        xproj = (torch.randn(B, N, A, generator=g) * amp).bfloat16()
        sproj = (torch.randn(B * K, A, generator=g) * amp).bfloat16()
        w = (torch.randn(A, generator=g) * (amp * 2 / math.sqrt(A))).bfloat16().float()
        x = torch.randn(B, N, X, generator=g).bfloat16()
        v = torch.tanh(sproj.double().view(B, K, 1, A) + xproj.double()[:, None]) @ w.double()          # [B, K, N]
        alpha = v.softmax(-1)
        ctx = torch.einsum("bkn,bnc->bkc", alpha, x.double())
        _REF[key] = ((xproj, sproj, w, x), {"alpha": alpha.reshape(B * K, N), "ctx": ctx.reshape(B * K, X)})
    return _REF[key]


def _slots_run(L, dev, case, ops, with_alpha=True):
    B, N, A, X, K, E = case
    xproj, sproj, w, x = ops
    ld = E + X
    inp = _poisoned(dev, (B * K + 1, ld), BF)
    alpha = _poisoned(dev, (B * K + 1, N), F32)
    L.call("dig_addattn_fwd_slots", L.ptr(xproj), L.ptr(sproj), L.ptr(w), L.ptr(x), L.ptr(alpha) if with_alpha else None, L.ptr(inp[:, E:]), ld,
           B, N, A, X, K, L.stream())
    _sync(dev)
    assert _is_poison(inp[:B * K, :E]) and _is_poison(inp[B * K:]) and _is_poison(alpha[B * K:] if with_alpha else alpha)
    return alpha[:B * K], inp[:B * K, E:]


@pytest.mark.parametrize("amp", [1, 4])
@pytest.mark.parametrize("case", SLOT_CASES, ids=lambda c: "x".join(map(str, c)))
def test_addattn_fwd_slots_vs_fp64(abi_dev, case, amp):
    """alpha and ctx at (B, N, A, X, K, E) against float64; the bound is taken beside dig_addattn_fwd on the K-times inflated tokens of the
    same case.  alpha = NULL gives the same context bits, margins keep their poison, a second run is bit-equal."""
    from dig_amd import _lib as L
    dev = abi_dev
    B, N, A, X, K, E = case
    ops, ref = _slots_ref(case, amp)
    ops = tuple(t.to(dev) for t in ops)
    xproj, sproj, w, x = ops
    alpha, ctx = _slots_run(L, dev, case, ops)
    # the existing entry point, one row per (sample, slot) over inflated tokens
    xp_inf, x_inf = xproj.repeat_interleave(K, 0).contiguous(), x.repeat_interleave(K, 0).contiguous()
    alpha0, ctx0 = torch.empty(B * K, N, device=dev), torch.empty(B * K, X, device=dev, dtype=BF)
    L.call("dig_addattn_fwd", L.ptr(xp_inf), L.ptr(sproj), L.ptr(w), L.ptr(x_inf), L.ptr(alpha0), L.ptr(ctx0), X, B * K, N, A, X, L.stream())
    be = _backend(dev)
    terms = {"alpha": _tau_term(alpha, ref["alpha"], False), "ctx": _tau_term(ctx, ref["ctx"], True)}
    base = {"alpha": _tau_term(alpha0, ref["alpha"], False), "ctx": _tau_term(ctx0, ref["ctx"], True)}
    bounds = {k: min(max(TAU[be][k], 2 * base[k]), TAU_CAP) for k in terms}
    for k in terms:
        print(f"tau {be} slots {k} {terms[k]:.3e}  dig_addattn_fwd {base[k]:.3e}  bound {bounds[k]:.3e}")
    for k in terms:
        assert terms[k] <= bounds[k], (k, terms[k], bounds[k])
    if N == 1:
        assert bool((alpha == 1).all())
    alpha2, ctx2 = _slots_run(L, dev, case, ops)
    assert torch.equal(alpha, alpha2) and torch.equal(ctx, ctx2)
    _, ctx3 = _slots_run(L, dev, case, ops, with_alpha=False)
    assert torch.equal(ctx, ctx3)


@pytest.mark.parametrize("case", [(2, 65, 72, 40, 3, 24), (1, 7, 520, 520, 8, 8), (2, 256, 512, 384, 5, 512)], ids=lambda c: "x".join(map(str, c)))
def test_addattn_fwd_slots_identical_slots_are_bit_identical(abi_dev, case):
    from dig_amd import _lib as L
    dev = abi_dev
    B, N, A, X, K, E = case
    (xproj, sproj, w, x), _ = _slots_ref(case, 1)
    same = sproj.view(B, K, A)[:, :1].expand(B, K, A).reshape(B * K, A).contiguous()
    alpha, ctx = _slots_run(L, dev, case, tuple(t.to(dev) for t in (xproj, same, w, x)))
    alpha, ctx = alpha.view(B, K, N), ctx.reshape(B, K, X)
    for k in range(1, K):
        assert torch.equal(alpha[:, k], alpha[:, 0]) and torch.equal(ctx[:, k], ctx[:, 0]), k


def test_addattn_fwd_slots_rejects_bad_arguments(abi_dev):
    from dig_amd import _lib as L
    dev = abi_dev
    B, N, A, X = 2, 16, 16, 16
    z = lambda *s, dt=BF: torch.zeros(*s, dtype=dt, device=dev)
    xproj, sproj, w, x = z(B * 513, 1032), z(B * 9, 1032), z(1032, dt=F32), z(B * 513, 1032)
    alpha, ctx = _poisoned(dev, (B * 9, 513), F32), _poisoned(dev, (B * 9, 1040), BF)

    def call(N=N, A=A, X=X, K=2, ldc=1040, **null):
        p = {k: L.ptr(t) for k, t in dict(xproj=xproj, sproj=sproj, w=w, x=x, alpha=alpha, ctx=ctx).items()}
        p.update(null)
        L.call("dig_addattn_fwd_slots", p["xproj"], p["sproj"], p["w"], p["x"], p["alpha"], p["ctx"], ldc, B, N, A, X, K, L.stream())

    for kw in ({"K": 0}, {"K": 9}, {"N": 513}, {"A": 1032}, {"A": 516}):
        with pytest.raises(L.DigHipError, match="unsupported"):
            call(**kw)
    for kw in ({"X": 15}, {"ldc": 25}, {"xproj": None}, {"sproj": None}, {"w": None}, {"x": None}, {"ctx": None}):
        with pytest.raises(L.DigHipError, match="bad argument"):
            call(**kw)
    with pytest.raises(L.DigHipError, match="misaligned"):
        call(xproj=type(L.ptr(w))(xproj.data_ptr() + 8))
    _sync(dev)
    assert _is_poison(alpha) and _is_poison(ctx)
    call()                                                                  # the unmodified arguments are accepted


# ------------------------------------------------------------------------------------------------ 2. dig_attn_beam_advance
ADV_CASES = [(3, 1, 97), (2, 5, 97), (1, 8, 38), (4, 3, 256)]
ADV_S, ADV_E = 40, 24


def _advance_inputs(B, K, C, kind):
    """Seeded logits [B*K, C + 3] and running scores: `step0` only slot 0 of a sample live; `later` finite scores with some slots at -inf;
    `ties` slots with equal scores and equal logit rows (every candidate of one ties with one of the other), and repeated values in a row."""
    g = torch.Generator().manual_seed(97 * B + 13 * K + C + len(kind))
    logits = torch.randn(B * K, C + 3, generator=g) * 3
    seq = torch.full((B * K,), NEG_INF)
    if kind == "step0":
        seq[::K] = 0.0
    else:
        seq = -torch.rand(B * K, generator=g) * 5
        if kind == "later" and K > 1:
            seq[1::K] = NEG_INF
            if K > 3:
                seq[3::K] = NEG_INF
        if kind == "ties":
            logits[:, 1] = logits[:, 0]
            logits[:, C - 1] = logits[:, 0]
            if K > 1:
                lg = logits.view(B, K, C + 3)
                lg[:, 1:] = lg[:, :1]
                seq = seq.view(B, K)[:, :1].expand(B, K).reshape(-1).clone()
    return logits, seq


@pytest.mark.parametrize("kind", ["step0", "later", "ties"])
@pytest.mark.parametrize("B,K,C", ADV_CASES)
def test_attn_beam_advance_vs_beam_step(abi_dev, B, K, C, kind):
    """The ranking and its bookkeeping are dig_beam_step's bits; the state rows follow their predecessors and the embedding rows their symbols,
    bit for bit; nothing else is written."""
    from dig_amd import _lib as L
    dev = abi_dev
    S, E, R = ADV_S, ADV_E, B * K
    logits, seq = _advance_inputs(B, K, C, kind)
    ld = logits.shape[1]
    eos = C - 3
    lg = logits.to(dev)
    seq_a, seq_b = seq.clone().to(dev), seq.clone().to(dev)
    sym_a, pred_a, sc_a = (torch.full((R,), -7, dtype=I64, device=dev), torch.full((R,), -7, dtype=I64, device=dev), _poisoned(dev, (R,), F32))
    L.call("dig_beam_step", L.ptr(lg), ld, L.ptr(seq_a), B, K, C, eos, L.ptr(sym_a), L.ptr(pred_a), L.ptr(sc_a), L.stream())
    g = torch.Generator().manual_seed(5)
    s_in = torch.randn(R, S, generator=g)
    table = torch.randn(C + 1, E, generator=g)
    s_in_d, sbf_in_d, table_d = s_in.to(dev), s_in.bfloat16().to(dev), table.to(dev)
    s_out, sbf_out = _poisoned(dev, (R + 1, S), F32), _poisoned(dev, (R + 1, S), BF)
    inp = _poisoned(dev, (R + 1, E + 8), BF)
    sym_b, pred_b, sc_b = (torch.full((R + 1,), -7, dtype=I64, device=dev), torch.full((R + 1,), -7, dtype=I64, device=dev), _poisoned(dev, (R + 1,), F32))
    L.call("dig_attn_beam_advance", L.ptr(lg), ld, L.ptr(seq_b), B, K, C, eos, L.ptr(sym_b), L.ptr(pred_b), L.ptr(sc_b), None, L.ptr(s_in_d),
           L.ptr(sbf_in_d), L.ptr(s_out), L.ptr(sbf_out), S, L.ptr(table_d), E, L.ptr(inp), E + 8, L.stream())
    _sync(dev)
    assert torch.equal(sym_b[:R], sym_a) and torch.equal(pred_b[:R], pred_a)
    assert torch.equal(sc_b[:R].view(torch.int32), sc_a.view(torch.int32)) and torch.equal(seq_b.view(torch.int32), seq_a.view(torch.int32))
    assert int(sym_b[R]) == -7 and int(pred_b[R]) == -7 and _is_poison(sc_b[R:])
    pred = pred_a.cpu()
    assert bool(((pred // K) == torch.arange(R) // K).all())                 # a predecessor is a slot of the same sample
    if kind == "later" and K > 1:
        assert bool((seq[pred] > NEG_INF).all())                            # dead slots are never expanded (>= K finite candidates)
    assert torch.equal(s_out[:R].cpu(), s_in[pred]) and torch.equal(sbf_out[:R].cpu(), s_in.bfloat16()[pred])
    assert torch.equal(inp[:R, :E].cpu(), table[sym_a.cpu()].bfloat16())
    assert _is_poison(s_out[R:]) and _is_poison(sbf_out[R:]) and _is_poison(inp[:, E:]) and _is_poison(inp[R:])
    assert torch.equal(seq_b.cpu() == NEG_INF, sym_a.cpu() == eos)


def test_attn_beam_advance_follows_forced_candidates(abi_dev):
    from dig_amd import _lib as L
    dev = abi_dev
    B, K, C, S, E = 2, 5, 97, ADV_S, ADV_E
    R = B * K
    logits, seq = _advance_inputs(B, K, C, "later")
    g = torch.Generator().manual_seed(11)
    forced = torch.stack([torch.randperm(K * C, generator=g)[:K] for _ in range(B)]).reshape(-1)
    forced[0] = 2 * C + (C - 3)                                                # slot 2 emits eos
    cand = (seq.double()[:, None] + logits[:, :C].double().log_softmax(-1)).view(B, K * C)
    want = cand.gather(1, forced.view(B, K)).view(-1)
    s_in, table = torch.randn(R, S, generator=g), torch.randn(C + 1, E, generator=g)
    lg, seq_d, forced_d, s_in_d, sbf_in_d, table_d = (t.to(dev) for t in (logits, seq, forced, s_in, s_in.bfloat16(), table))
    sym, pred, sc = torch.empty(R, dtype=I64, device=dev), torch.empty(R, dtype=I64, device=dev), torch.empty(R, device=dev)
    s_out, sbf_out, inp = torch.empty(R, S, device=dev), torch.empty(R, S, device=dev, dtype=BF), torch.empty(R, E, device=dev, dtype=BF)
    L.call("dig_attn_beam_advance", L.ptr(lg), C + 3, L.ptr(seq_d), B, K, C, C - 3, L.ptr(sym), L.ptr(pred), L.ptr(sc), L.ptr(forced_d), L.ptr(s_in_d),
           L.ptr(sbf_in_d), L.ptr(s_out), L.ptr(sbf_out), S, L.ptr(table_d), E, L.ptr(inp), E, L.stream())
    base = (torch.arange(R) // K) * K
    assert torch.equal(sym.cpu(), forced % C) and torch.equal(pred.cpu(), forced // C + base)
    got = sc.cpu().double()
    fin = torch.isfinite(want)
    assert torch.equal(torch.isfinite(got), fin) and float((got[fin] - want[fin]).abs().max()) <= 1e-5 * float(want[fin].abs().max())
    assert torch.equal(s_out.cpu(), s_in[pred.cpu()]) and torch.equal(inp.cpu(), table[sym.cpu()].bfloat16())
    assert float(seq_d[0]) == NEG_INF and torch.equal(seq_d.cpu()[1:], sc.cpu()[1:])


def test_attn_beam_advance_rejects_bad_arguments(abi_dev):
    from dig_amd import _lib as L
    dev = abi_dev
    B, C, S, E = 2, 38, 16, 8
    lg, seq = torch.zeros(B * 9, C, device=dev), torch.zeros(B * 9, device=dev)
    sym, pred, sc = torch.full((B * 9,), -7, dtype=I64, device=dev), torch.full((B * 9,), -7, dtype=I64, device=dev), _poisoned(dev, (B * 9,), F32)
    state, sbf = torch.zeros(2 * B * 9, S, device=dev), torch.zeros(2 * B * 9, S, device=dev, dtype=BF)
    s_out, sbf_out = _poisoned(dev, (B * 9, S), F32), _poisoned(dev, (B * 9, S), BF)
    table, inp = torch.zeros(C + 1, E, device=dev), _poisoned(dev, (B * 9, E), BF)

    def call(K=3, s_in=state, s_o=s_out, b_in=sbf, b_o=sbf_out, **null):
        p = {k: L.ptr(t) for k, t in dict(lg=lg, seq=seq, sym=sym, pred=pred, sc=sc, s_in=s_in, b_in=b_in, s_o=s_o, b_o=b_o, table=table, inp=inp).items()}
        p.update(null)
        L.call("dig_attn_beam_advance", p["lg"], C, p["seq"], B, K, C, C - 3, p["sym"], p["pred"], p["sc"], None, p["s_in"], p["b_in"], p["s_o"], p["b_o"],
               S, p["table"], E, p["inp"], E, L.stream())

    for K in (0, 9):
        with pytest.raises(L.DigHipError, match="unsupported"):
            call(K=K)
    with pytest.raises(L.DigHipError, match="unsupported"):                 # 8 * 2000 * 4 B of candidates: dig_beam_step's LDS condition
        L.call("dig_attn_beam_advance", L.ptr(lg), 2000, L.ptr(seq), 1, 8, 2000, 5, L.ptr(sym), L.ptr(pred), L.ptr(sc), None, L.ptr(state), L.ptr(sbf),
               L.ptr(s_out), L.ptr(sbf_out), S, L.ptr(table), E, L.ptr(inp), E, L.stream())
    # a gather in place, or into rows that overlap the source's, is refused: fp32 and bf16 states alike
    for kw in ({"s_o": state}, {"b_o": sbf}, {"s_o": state[3:]}, {"b_o": sbf[B * 3 - 1:]}):
        with pytest.raises(L.DigHipError, match="bad argument"):
            call(**kw)
    for name in ("lg", "seq", "sym", "pred", "sc", "s_in", "b_in", "s_o", "b_o", "table", "inp"):
        with pytest.raises(L.DigHipError, match="bad argument"):
            call(**{name: None})
    _sync(dev)
    assert _is_poison(sc) and _is_poison(s_out) and _is_poison(sbf_out) and _is_poison(inp) and int(sym.max()) == -7
    call(s_in=state[B * 9:], s_o=state[:B * 9].contiguous())                 # adjacent, disjoint rows are fine
    call()


# ------------------------------------------------------------------------------------------------ 3. the specification on its own
def _attn_fixture():
    """The tiny AttnRecModel of tests/golden/attn_decoder_tiny.npz (as tests/test_finetune.py builds it): weights, images, configuration."""
    g = np.load(os.path.join(GOLD, "attn_decoder_tiny.npz"))
    ecfg = O.DiGConfig(**O.TINY)
    c = AD.AttnDecConfig(**{**AD.TINY, "in_planes": ecfg.embed_dim})
    P = {**D.det_encoder_state(ecfg, int(g["seed_enc"])), **AD.det_state(c, int(g["seed_dec"]))}
    images = O.synthetic_batch(int(g["B"]), ecfg, int(g["batch_seed"]))[0]
    return g, c, ecfg, P, images


_TINY = {}


def _tiny():
    """Fixture model, its oracle tokens, and per width the float64 specification run + e_bf; computed once, not modified."""
    if not _TINY:
        g, c, ecfg, P, images = _attn_fixture()
        _TINY.update(g=g, c=c, ecfg=ecfg, P=P, images=images, x=D.encoder_features(P, ecfg, images), eos=c.num_classes - 3, runs={})
    return types.SimpleNamespace(**_TINY)


def _e_bf(P, c, x, K, eos, ref):
    """Largest |score difference| between the specification under CPU bf16 autocast and in float64, along the float64 decisions."""
    with torch.autocast("cpu", dtype=torch.bfloat16):
        bf = SPEC.beam_search(P, c, x, K, eos, force_decisions=ref.candidates, dtype=torch.float32)
    fin = torch.isfinite(ref.scores)
    assert torch.equal(torch.isfinite(bf.scores), fin)
    return float((bf.scores[fin] - ref.scores[fin]).abs().max())


def _tiny_run(K):
    t = _tiny()
    if K not in t.runs:
        ref = SPEC.beam_search(t.P, t.c, t.x, K, t.eos)
        t.runs[K] = (ref, _e_bf(t.P, t.c, t.x, K, t.eos, ref))
    return t.runs[K]


def _backtrack(r, B, K, eos):
    from dig_amd.recognizer import beam_backtrack
    return beam_backtrack(r.scores.float().numpy(), r.preds.numpy(), r.syms.numpy(), B, K, eos)


def test_spec_width_1_is_the_greedy_sample():
    t = _tiny()
    ref, _ = _tiny_run(1)
    greedy = AD.head_sample(t.P, t.c, t.x).argmax(-1)
    assert torch.equal(greedy, torch.from_numpy(t.g["sample_probs"]).argmax(-1))
    for b in range(greedy.shape[0]):
        row = greedy[b].tolist()
        n = row.index(t.eos) + 1 if t.eos in row else len(row)
        assert ref.ids[b, :n].tolist() == row[:n], b


def test_spec_backtracking_is_beam_backtrack():
    """Forced classifier outputs that end hypotheses at different steps (sample b: an EOS 2 above the row's maximum in slot b % K at step
    b + 1, and a weaker one, 1 below the maximum, in the next slot two steps later): the back-tracking restated from the reference and
    dig_amd.recognizer.beam_backtrack pick the same strings, and the best hypotheses end at different lengths."""
    t = _tiny()
    K, C, T, eos = 3, t.c.num_classes, t.c.max_len, t.eos
    B = t.x.shape[0]
    g = torch.Generator().manual_seed(3)
    fl = torch.randn(T, B * K, C, generator=g, dtype=torch.float64)
    fl[:, :, eos] = -20.0
    for b in range(B):
        row = b * K + b % K
        fl[b + 1, row, eos] = fl[b + 1, row].max() + 2.0
        if b + 3 < T:
            row = b * K + (b + 1) % K
            fl[b + 3, row, eos] = fl[b + 3, row].max() - 1.0
    r = SPEC.beam_search(t.P, t.c, t.x, K, eos, force_logits=fl)
    print("spec: best lengths", r.lens, "masked slots", int(r.masked.sum()))
    assert bool(r.masked.any()) and min(r.lens) < T and len(set(r.lens)) > 2
    assert torch.equal(r.ids, _backtrack(r, B, K, eos))
    for b in range(B):
        if r.lens[b] < T:
            assert int(r.ids[b, r.lens[b] - 1]) == eos
    free = SPEC.beam_search(t.P, t.c, t.x, K, eos)
    assert torch.equal(free.ids, _backtrack(free, B, K, eos))
    again = SPEC.beam_search(t.P, t.c, t.x, K, eos, force_decisions=free.candidates)
    assert torch.equal(again.scores, free.scores) and torch.equal(again.ids, free.ids)


# ------------------------------------------------------------------------------------------------ 4. the model on the MI355X
WIDTHS = [1, 3, 5, 8]


def _device_model(c, ecfg, P):
    from dig_amd.attn_recognizer import AttnRecModelTrain
    m = AttnRecModelTrain(embed_dim=ecfg.embed_dim, depth=ecfg.depth, num_heads=ecfg.heads, nb_classes=c.num_classes, max_len=c.max_len, sDim=c.sDim,
                          attDim=c.attDim)
    m.load_state_dict(P)
    m.to("cuda:0")
    return m.eval()


def _candidates(preds, syms, B, K, C):
    """[T, B, K] candidate indices k*C + c of device decisions [T, B*K]."""
    base = (torch.arange(B * K) // K) * K
    return ((preds.cpu() - base) * C + syms.cpu()).view(-1, B, K)


def _check_forced(m, images, K, eos, ref, e_bf, tag):
    """a. the specification's decisions forced on the device: every finite stored score within 4 e_bf of the specification's."""
    _, _, scores, preds, syms = m.beam_search(images, K, eos=eos, force_decisions=ref.candidates, return_logits=True)
    assert torch.equal(preds.cpu(), ref.preds) and torch.equal(syms.cpu(), ref.syms)
    got, fin = scores.cpu().double(), torch.isfinite(ref.scores)
    assert torch.equal(torch.isfinite(got), fin)
    err = float((got[fin] - ref.scores[fin]).abs().max())
    print(f"{tag} K={K} forced: e_bf {e_bf:.3e}  max |score - spec| {err:.3e}  bound {4 * e_bf:.3e}")
    assert err <= 4 * e_bf


def _check_free(m, images, K, eos, spec, e_bf, tag):
    """b. the device's own decisions re-scored by the float64 specification along the device's path: no excluded candidate beats a chosen one
    by more than 4 e_bf; the ids are beam_backtrack of the device's decisions; two runs are bit-identical.  spec(cands) -> specification run."""
    from dig_amd.recognizer import beam_backtrack
    ids, logits, scores, preds, syms = m.beam_search(images, K, eos=eos, return_logits=True)
    B, C = images.shape[0], logits.shape[-1]
    cands = _candidates(preds, syms, B, K, C)
    r = spec(cands)
    chosen = r.cand_scores.gather(2, cands)
    rest = r.cand_scores.scatter(2, cands, NEG_INF)
    best_out, worst_in = rest.max(-1)[0], chosen.min(-1)[0]
    live = torch.isfinite(best_out)
    short = float((best_out[live] - worst_in[live]).max())
    print(f"{tag} K={K} free: e_bf {e_bf:.3e}  worst shortfall {short:.3e}  bound {4 * e_bf:.3e}")
    assert short <= 4 * e_bf
    assert torch.equal(ids.cpu(), beam_backtrack(scores.cpu().numpy(), preds.cpu().numpy(), syms.cpu().numpy(), B, K, eos))
    ids2, logits2, scores2, preds2, syms2 = m.beam_search(images, K, eos=eos, return_logits=True)
    assert all(torch.equal(a, b) for a, b in ((ids, ids2), (logits, logits2), (scores.view(torch.int32), scores2.view(torch.int32)), (preds, preds2),
                                              (syms, syms2)))
    assert torch.equal(m.beam_search(images, K, eos=eos), ids)
    return ids


@pytest.fixture(scope="module")
def tiny_device_model():
    t = _tiny()
    return _device_model(t.c, t.ecfg, t.P), t.images.to("cuda:0")


@pytest.mark.gpu
@pytest.mark.parametrize("K", WIDTHS)
def test_device_beam_search_vs_specification(tiny_device_model, K):
    m, images = tiny_device_model
    t = _tiny()
    ref, e_bf = _tiny_run(K)
    _check_forced(m, images, K, t.eos, ref, e_bf, "tiny")
    ids = _check_free(m, images, K, t.eos, lambda cands: SPEC.beam_search(t.P, t.c, t.x, K, t.eos, force_decisions=cands), e_bf, "tiny")
    m.beam_width = K
    try:
        out = m((images, None, None))
    finally:
        m.beam_width = 0
    assert out[1] is None and out[2] is None and torch.equal(out[0], ids) and out[0].dtype == I64 and tuple(out[0].shape) == (images.shape[0], t.c.max_len)
    assert torch.equal(out[3], torch.ones_like(ids))


@pytest.mark.gpu
def test_device_width_1_is_the_greedy_sample(tiny_device_model):
    """c. precondition on the specification: the greedy top-2 log-probability margin is at least 8 e_bf at every step."""
    m, images = tiny_device_model
    t = _tiny()
    ref, e_bf = _tiny_run(1)
    top2 = ref.logits.log_softmax(-1).topk(2, -1)[0]
    margin = float((top2[..., 0] - top2[..., 1]).min())
    print(f"tiny K=1: greedy top-2 margin {margin:.3e}  8 e_bf {8 * e_bf:.3e}")
    assert margin >= 8 * e_bf
    ids = m.beam_search(images, 1).cpu()
    greedy = m.sample(images).argmax(-1).cpu()
    for b in range(ids.shape[0]):
        row = greedy[b].tolist()
        n = row.index(t.eos) + 1 if t.eos in row else len(row)
        assert ids[b, :n].tolist() == row[:n], b


def _ending_eos(t, K):
    """d. a class the specification ranks inside the top K but not first at some step, with which (on the specification alone) a slot is masked
    and a best hypothesis ends before max_len.  The first such class in (step, sample, rank) order."""
    ref, _ = _tiny_run(K)
    T, B = ref.syms.shape[0], t.x.shape[0]
    ranked = ref.syms.view(T, B, K)                                          # (top-K order: slot 0 holds the best candidate)
    tried = set(ranked[:, :, 0].reshape(-1).tolist())                        # never a class that is first anywhere
    for step in range(T - 1):
        for b in range(B):
            for rank in range(1, K):
                cls = int(ranked[step, b, rank])
                if cls in tried:
                    continue
                tried.add(cls)
                r = SPEC.beam_search(t.P, t.c, t.x, K, cls)
                if bool(r.masked.any()) and min(r.lens) < T:
                    return cls, r
    raise AssertionError("no class ends a hypothesis early")


@pytest.mark.gpu
def test_device_beam_search_with_hypotheses_that_end(tiny_device_model):
    m, images = tiny_device_model
    t = _tiny()
    K = 5
    eos, r = _ending_eos(t, K)
    assert bool(r.masked.any()) and min(r.lens) < t.c.max_len              # (on the specification alone)
    e_bf = _e_bf(t.P, t.c, t.x, K, eos, r)
    print(f"tiny K={K} eos={eos}: masked slots {int(r.masked.sum())}, best lengths {r.lens}")
    _check_forced(m, images, K, eos, r, e_bf, f"tiny eos={eos}")
    _check_free(m, images, K, eos, lambda cands: SPEC.beam_search(t.P, t.c, t.x, K, eos, force_decisions=cands), e_bf, f"tiny eos={eos}")


@pytest.mark.gpu
def test_device_beam_search_full_size_head():
    """e. ViT-S tokens, sDim = attDim = 512, max_len 25, B = 4, K = 5; the specification reads the device's own encoder tokens."""
    from dig_amd.attn_recognizer import AttnRecModelTrain
    torch.manual_seed(31)
    args = types.SimpleNamespace(model="simmim_vit_small_patch4_32x128", nb_classes=97, max_len=25, drop=0.0, attn_drop_rate=0.0, drop_path=0.0)
    m = AttnRecModelTrain(args)
    P = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    m.to("cuda:0").eval()
    B, K = 4, 5
    c = AD.AttnDecConfig(num_classes=97, in_planes=m.D, sDim=512, attDim=512, max_len=25)
    images = (torch.rand(B, 3, 32, 128, generator=torch.Generator().manual_seed(4)) * 2 - 1).to("cuda:0")
    x = m.eval_tokens(images)[1].view(B, m.N, m.D).cpu().double()
    ref = SPEC.beam_search(P, c, x, K, m.eos)
    e_bf = _e_bf(P, c, x, K, m.eos, ref)
    _check_forced(m, images, K, m.eos, ref, e_bf, "full")
    _check_free(m, images, K, m.eos, lambda cands: SPEC.beam_search(P, c, x, K, m.eos, force_decisions=cands), e_bf, "full")


# ------------------------------------------------------------------------------------------------ 5. host and driver
def test_beam_width_argument():
    from dig_amd.attn_recognizer import AttnRecModelTrain
    args = dict(model="simmim_vit_tiny_patch4_32x128", nb_classes=97, max_len=25, drop=0.0, attn_drop_rate=0.0, drop_path=0.0)
    for bad in (9, -1):
        with pytest.raises(ValueError, match="beam_width"):
            AttnRecModelTrain(types.SimpleNamespace(beam_width=bad, **args))
    assert AttnRecModelTrain(types.SimpleNamespace(beam_width=0, **args)).beam_width == 0
    assert AttnRecModelTrain(types.SimpleNamespace(**args)).beam_width == 0
    m = AttnRecModelTrain(types.SimpleNamespace(beam_width=8, **args))
    assert m.beam_width == 8 and m.eos == 94
    with pytest.raises(ValueError, match="beam_width"):
        m.beam_search(torch.zeros(1, 3, 32, 128), 9)


from test_finetune_driver import COMMON, _driver  # noqa: E402

ATT = COMMON + " --decoder_type attention"


def test_driver_attention_beam_width_flag():
    drv = _driver()
    assert drv.get_args(ATT.split()).beam_width == 0
    assert drv.get_args((ATT + " --beam_width 8").split()).beam_width == 8
    for bad in ("9", "-1"):
        with pytest.raises(SystemExit, match="1..8"):
            drv.get_args((ATT + " --beam_width " + bad).split())
    with pytest.raises(SystemExit, match="--decoder_type ctc"):                # --ctc_beam_width is handled as before
        drv.get_args((ATT + " --ctc_beam_width 4").split())
    assert drv.get_args((COMMON + " --beam_width 12").split()).beam_width == 12  # (the transformer decoder's beam has its own limit)


@pytest.mark.gpu
def test_evaluate_reads_the_beam_ids():
    """evaluate() with args.beam_width = 5 over the synthetic evaluation set, on a model built with that width from the driver's arguments: the
    model returns ids, the loss meter reads 0, acc and recognition_fmeasure are those of `beam_search`'s ids, batch by batch."""
    from dig_amd.attn_recognizer import AttnRecModelTrain
    from dig_amd.engine_for_finetuning import _vocabulary, evaluate
    from dig_amd.rec_datasets import build_dataset, device_loader
    from dig_amd.recognizer import accuracy, recognition_f_measure
    drv = _driver()
    args = drv.get_args((ATT + " --beam_width 5").split())
    dev = torch.device("cuda", 0)
    torch.manual_seed(args.seed)
    data = build_dataset(False, args)[0]
    loader = device_loader(data, args, False, dev, seed=args.seed)
    m = AttnRecModelTrain(args)
    assert m.beam_width == 5
    m.to(dev)
    ev = evaluate(loader, m, dev, args=args)
    voc = _vocabulary(data)
    n = acc = fm = 0.0
    for batch in loader:
        images, target = batch[0].to(dev), batch[1].to(dev)
        ids = m.beam_search(images, 5)
        assert tuple(ids.shape) == (images.shape[0], args.max_len)
        acc += float(accuracy(ids, target, voc)) * images.shape[0]
        fm += float(recognition_f_measure(ids, target, voc)) * images.shape[0]
        n += images.shape[0]
    assert n == len(data) > args.batch_size                                 # (more than one batch)
    assert ev["loss"] == 0.0
    assert ev["acc"] == pytest.approx(acc / n, abs=1e-9) and ev["recognition_fmeasure"] == pytest.approx(fm / n, abs=1e-9)
    with pytest.raises(RuntimeError, match="beam_width"):                    # a model built with another width is refused, as before
        evaluate(loader, m, dev, args=types.SimpleNamespace(beam_width=3))


@pytest.mark.gpu
def test_attention_driver_evaluates_with_the_beam(tmp_path):
    """--decoder_type attention --beam_width 5 through the driver: a two-epoch run evaluates through the beam after every epoch (log.txt, loss
    meter 0), and --eval --resume of its last checkpoint prints the meters log.txt ends with.  The line naming the decoder is printed once, by
    the runs that use it; --beam_width 0 on the same checkpoint is the greedy evaluation (a loss, no such line)."""
    import contextlib
    import io
    import json
    drv = _driver()
    out = str(tmp_path)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res = drv.main(drv.get_args((ATT + " --beam_width 5 --save_ckpt --output_dir " + out).split()))
    assert buf.getvalue().count("beam search of the GRU attention head") == 1 and "Model = AttnRecModelTrain" in buf.getvalue()
    ck = os.path.join(out, "checkpoint-1.pth")
    assert os.path.exists(ck)
    lines = [json.loads(l) for l in open(os.path.join(out, "log.txt"))]
    assert [l["epoch"] for l in lines] == [0, 1] and all(l["test_loss"] == 0.0 for l in lines)
    last = lines[-1]
    got = {}
    for width in (5, 0):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            got[width] = drv.main(drv.get_args((ATT + f" --eval --resume {ck} --beam_width {width}").split()))["test_stats"]
        assert buf.getvalue().count("beam search of the GRU attention head") == (1 if width else 0)
        assert ("width 5" in buf.getvalue()) == bool(width)
        assert set(got[width]) == {"loss", "acc", "recognition_fmeasure", "edit_distance"} and all(math.isfinite(v) for v in got[width].values())
    for k in ("acc", "loss", "recognition_fmeasure", "edit_distance"):
        assert got[5][k] == last["test_" + k] == res["test_stats"][k], k
    assert got[5]["loss"] == 0.0 and got[0]["loss"] > 0.0


# ------------------------------------------------------------------------------------------------ 6. the build
def test_attn_beam_kernels_use_no_scratch():
    from dig_amd import build
    build.build(verbose=False)
    rows = [r for r in build.kernel_resources() if r["name"].startswith(("addattn_fwd_slots_kernel", "attn_beam_advance_kernel"))]
    assert len(rows) == 9 and all(r["scratch"] == 0 and r["hot"] for r in rows), rows
    # two 512-thread workgroups of the K-slot attention share a CU (4 waves per SIMD) while a wave stays within 128 registers
    assert all(r["vgpr"] <= 128 for r in rows if r["name"].startswith("addattn_fwd_slots_kernel")), rows
