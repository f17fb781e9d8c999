"""Every branch of the GRU attention head kernels (dig_amd/csrc/gru_attn.hip: dig_addattn_fwd / _bwd / _bwd_tokens, dig_gru_cell_fwd / _bwd,
dig_embed_rows) against float64 torch on the same bf16-rounded operands, on both builds of the ABI (`abi_dev`: libdig_hip.so on the MI355X and
cpu_abi/libdig_cpu.so).

Criterion, per element:   fp32 outputs   |out - ref| <= tau * max|ref|
                          bf16 outputs   |out - ref| <= 2^-8 * |ref| + tau * max|ref|
(2^-8 |ref| is one bf16 ulp of the element: half an ulp of rounding plus half for a value that lands on the other side of a rounding boundary;
max|ref| is taken over the whole output of the case, all steps together.)  The `tau` term of an output is the largest
(|out - ref| [- 2^-8 |ref|]) / max|ref| over its elements; each test prints it (`tau <backend> <output> <value>`) before it asserts.

tau: the largest term measured over all cases of this module (seeded inputs, deterministic kernels), and the bound = 4 x that, rounded up to
one significant digit (the factor is for a later compiler's reassociation only); each build is held to the bound from its own figures (the
device's tree reductions are closer to float64 than the CPU build's serial sums over N, its exp-based gates a little further).  No bound may exceed TAU_CAP = 1e-4,
the linear worst case of a 3e-7 tanh error summed over sum|w| ~ 200 at A = 1024, amp = 4.

    output           MI355X     bound     CPU build  bound
    alpha (fp32)     7.145e-07  3e-06     5.139e-06  3e-05
    ctx (bf16)       7.509e-08  4e-07     4.433e-07  2e-06
    dv (fp32)        1.194e-06  5e-06     5.335e-06  3e-05
    dsproj (bf16)    1.133e-07  5e-07     2.359e-07  1e-06
    dw (fp32)        1.132e-06  5e-06     4.228e-06  2e-05
    dxproj (bf16)    1.943e-07  8e-07     7.182e-08  3e-07
    dx (bf16)        2.281e-08  1e-07     3.184e-07  2e-06
    s (fp32)         2.814e-07  2e-06     3.405e-07  2e-06
    r (fp32)         8.524e-08  4e-07     8.524e-08  4e-07
    z (fp32)         8.719e-08  4e-07     8.719e-08  4e-07
    n (fp32)         9.608e-07  4e-06     1.482e-06  6e-06
    dgi (bf16)       7.195e-07  3e-06     2.703e-07  2e-06
    dgh (bf16)       8.693e-07  4e-06     2.703e-07  2e-06
    ds_prev (fp32)   1.359e-07  6e-07     1.359e-07  6e-07

Attention chain rows -> branches of gru_attn.hip (fwd: `if (CP <= NT / 2)`; bwd: `if (AP <= NT / 2)`; token_score / dalpha: `a0 += 512`,
`c0 += 512`; dxproj / dx: `n0 + j < N`):
    (3, 256, 512, 384, 3, 512)  CP = 192 < 256 and AP = 256 == 256: both split-token paths, AP with every thread busy; one score pass; ldc > X
    (2, 256, 512, 512, 2, 0)    CP == 256 and AP == 256: both half-blocks fully occupied; dalpha in exactly one pass of 512 channels
    (2, 70, 1024, 768, 2, 64)   CP = 384, AP = 512: both one-thread-per-pair paths; full second score pass, half second dalpha pass; N % 8, N % 64 != 0
    (2, 7, 520, 520, 2, 8)      pair paths with 260 pairs (4 threads past the half); second passes of one lane; odd N below the 8 waves
    (3, 1, 8, 8, 1, 0)          N == 1: the first half-block's token range is empty, alpha == 1 and every score gradient is exactly 0
    (1, 512, 64, 128, 2, 0)     N == MAXN: the softmax loops' last thread, 8 full token tiles
    (2, 65, 72, 40, 25, 24)     T = 25 steps; second token tile of dxproj / dx holds one token; A, X of a single partial pass
"""
import math

import pytest
import torch

POISON = 768.0                    # (exact in bf16)
TAU_CAP = 1e-4
BF, F32 = torch.bfloat16, torch.float32

# bounds per backend and output: 4 x the measured maximum (docstring table), one significant digit, rounded up
TAU = {
    "hip": {"alpha": 3e-06, "ctx": 4e-07, "dv": 5e-06, "dsproj": 5e-07, "dw": 5e-06, "dxproj": 8e-07, "dx": 1e-07,
           "s": 2e-06, "r": 4e-07, "z": 4e-07, "n": 4e-06, "dgi": 3e-06, "dgh": 4e-06, "ds_prev": 6e-07},
    "cpu_abi": {"alpha": 3e-05, "ctx": 2e-06, "dv": 3e-05, "dsproj": 1e-06, "dw": 2e-05, "dxproj": 3e-07, "dx": 2e-06,
               "s": 2e-06, "r": 4e-07, "z": 4e-07, "n": 6e-06, "dgi": 2e-06, "dgh": 2e-06, "ds_prev": 6e-07},
}
_BF16_OUT = {"ctx", "dsproj", "dxproj", "dx", "dgi", "dgh"}


def _backend(dev):
    return "hip" if dev.type == "cuda" else "cpu_abi"


def _tau_term(out, ref, bf16):
    """Largest tau term of `out` against the float64 `ref` (see the module docstring); inf where the output is not finite, or differs at all
    from a reference that is zero everywhere."""
    out = out.detach().cpu().double().reshape(ref.shape)
    if not bool(torch.isfinite(out).all()):
        return math.inf
    err = (out - ref).abs()
    if bf16:
        err = (err - ref.abs() * 2.0 ** -8).clamp_min(0)
    e, m = err.max().item(), ref.abs().max().item()
    if m == 0:
        return 0.0 if e == 0 else math.inf
    return e / m


def _check(dev, terms):
    """terms: {output: tau term}.  Prints every figure, then asserts every bound."""
    be = _backend(dev)
    for name, t in terms.items():
        print(f"tau {be} {name} {t:.3e}")
    for name, t in terms.items():
        bound = TAU[be][name]
        assert bound <= TAU_CAP
        assert t <= bound, (name, t, bound)


def _poisoned(dev, shape, dtype):
    return torch.full(shape, POISON, dtype=dtype, device=dev)


def _is_poison(t):
    return bool((t.float() == POISON).all())


# ------------------------------------------------------------------------------------------------ 1. attention chain
CHAIN = [(3, 256, 512, 384, 3, 512), (2, 256, 512, 512, 2, 0), (2, 70, 1024, 768, 2, 64), (2, 7, 520, 520, 2, 8), (3, 1, 8, 8, 1, 0),
         (1, 512, 64, 128, 2, 0), (2, 65, 72, 40, 25, 24)]
_REF = {}


def _chain_ref(case, amp):
    """Operands (bf16-rounded) and the float64 autograd reference of one case; computed once, shared by both backends, not modified."""
    key = ("chain", case, amp)
    if key not in _REF:
        B, N, A, X, T, E = case
        g = torch.Generator().manual_seed(1000 * amp + N + A + X)
        xproj = (torch.randn(B, N, A, generator=g) * amp).bfloat16()
        sproj = (torch.randn(T, B, A, generator=g) * amp).bfloat16()
        w = (torch.randn(A, generator=g) * (amp * 2 / math.sqrt(A))).bfloat16().float()
        x = torch.randn(B, N, X, generator=g).bfloat16()
        dinp = torch.randn(T, B, E + X, generator=g).bfloat16()             # [dyProj | dctx]: the kernels read columns [E, E + X)
        xp, xx, ww, sp = (t.double().requires_grad_(True) for t in (xproj, x, w, sproj))
        vs, als, cs = [], [], []
        for t in range(T):
            v = torch.tanh(sp[t][:, None, :] + xp) @ ww
            v.retain_grad()
            al = v.softmax(1)
            vs.append(v); als.append(al); cs.append(torch.bmm(al[:, None, :], xx)[:, 0])
        torch.autograd.backward(cs, [dinp[t][:, E:].double() for t in range(T)])
        ref = {"alpha": torch.stack(als).detach(), "ctx": torch.stack(cs).detach(), "dv": torch.stack([v.grad for v in vs]), "dsproj": sp.grad,
               "dw": ww.grad, "dxproj": xp.grad, "dx": xx.grad}
        _REF[key] = ((xproj, sproj, w, x, dinp), ref)
    return _REF[key]


def _chain_run(L, dev, case, ops):
    """The engine's call sequence: fwd + bwd per step (dw_acc zeroed once), then bwd_tokens.  Every output has a poisoned row behind what the
    next call may write, checked after that call; the context lands in columns [E, E + X) of a poisoned [T, B, E + X] buffer."""
    B, N, A, X, T, E = case
    xproj, sproj, w, x, dinp = (t.to(dev) for t in ops)
    ld = E + X
    inp = _poisoned(dev, (T + 1, B, ld), BF)
    alpha, dv = _poisoned(dev, (T * B + 1, N), F32), _poisoned(dev, (T * B + 1, N), F32)
    dsproj = _poisoned(dev, (T * B + 1, A), BF)
    dw_acc = torch.zeros(B, A, device=dev)
    for t in range(T):
        r0, r1 = t * B, (t + 1) * B
        L.call("dig_addattn_fwd", L.ptr(xproj), L.ptr(sproj[t]), L.ptr(w), L.ptr(x), L.ptr(alpha[r0:]), L.ptr(inp[t][:, E:]), ld, B, N, A, X, L.stream())
        assert _is_poison(alpha[r1:]) and _is_poison(inp[t][:, :E]) and _is_poison(inp[t + 1:])
        L.call("dig_addattn_bwd", L.ptr(xproj), L.ptr(sproj[t]), L.ptr(w), L.ptr(x), L.ptr(alpha[r0:]), L.ptr(dinp[t][:, E:]), ld, L.ptr(dv[r0:]),
               L.ptr(dsproj[r0:]), L.ptr(dw_acc), B, N, A, X, L.stream())
        assert _is_poison(dv[r1:]) and _is_poison(dsproj[r1:])
    dxproj, dx = _poisoned(dev, (B * N + 1, A), BF), _poisoned(dev, (B * N + 1, X), BF)
    L.call("dig_addattn_bwd_tokens", L.ptr(xproj), L.ptr(sproj), L.ptr(w), L.ptr(dv), L.ptr(alpha), L.ptr(dinp[0][:, E:]), ld, L.ptr(dxproj), L.ptr(dx),
           T, B, N, A, X, L.stream())
    assert _is_poison(dxproj[B * N:]) and _is_poison(dx[B * N:]) and _is_poison(alpha[T * B:]) and _is_poison(dv[T * B:])
    return {"alpha": alpha[:T * B], "ctx": inp[:T, :, E:], "dv": dv[:T * B], "dsproj": dsproj[:T * B], "dw": dw_acc.sum(0), "dxproj": dxproj[:B * N],
            "dx": dx[:B * N]}


@pytest.mark.parametrize("amp", [1, 4])
@pytest.mark.parametrize("case", CHAIN, ids=lambda c: "x".join(map(str, c)))
def test_attention_chain_vs_fp64(abi_dev, case, amp):
    """dig_addattn_fwd -> _bwd per step -> _bwd_tokens at (B, N, A, X, T, E) with ldc = ldd = E + X, against float64 autograd of the literal
    formula; amp = 4 saturates tanh and spikes the softmax.  dw = dw_acc.sum(0) with dw_acc zeroed once: the += contract.  Margins stay
    poisoned and a second run is bit-equal."""
    from dig_amd import _lib as L
    dev = abi_dev
    ops, ref = _chain_ref(case, amp)
    out = _chain_run(L, dev, case, ops)
    _check(dev, {k: _tau_term(out[k], ref[k], k in _BF16_OUT) for k in ref})
    again = _chain_run(L, dev, case, ops)
    for k in out:
        assert torch.equal(out[k], again[k]), k


# ------------------------------------------------------------------------------------------------ 2. bwd_tokens alone, large dynamic LDS
def _tokens_ref(dims):
    key = ("tokens", dims)
    if key not in _REF:
        T, B, N, A, X = dims
        g = torch.Generator().manual_seed(T + N + A + X)
        xproj, sproj = torch.randn(B, N, A, generator=g).bfloat16(), torch.randn(T, B, A, generator=g).bfloat16()
        w = (torch.randn(A, generator=g) * (2 / math.sqrt(A))).bfloat16().float()
        dv, alpha = torch.randn(T, B, N, generator=g), torch.randn(T, B, N, generator=g).softmax(-1)
        dctx = torch.randn(T, B, X + 8, generator=g).bfloat16()             # ldd = X + 8, the kernels read columns [0, X)
        th = torch.tanh(sproj.double()[:, :, None, :] + xproj.double()[None])                          # [T, B, N, A]
        ref = {"dxproj": (dv.double()[..., None] * (1 - th * th)).sum(0) * w.double(),
               "dx": torch.einsum("tbn,tbc->bnc", alpha.double(), dctx[:, :, :X].double())}
        _REF[key] = ((xproj, sproj, w, dv, alpha, dctx), ref)
    return _REF[key]


def _tokens_run(L, dev, dims):
    T, B, N, A, X = dims
    ops, ref = _tokens_ref(dims)
    xproj, sproj, w, dv, alpha, dctx = (t.to(dev) for t in ops)
    dxproj, dx = _poisoned(dev, (B * N + 1, A), BF), _poisoned(dev, (B * N + 1, X), BF)
    L.call("dig_addattn_bwd_tokens", L.ptr(xproj), L.ptr(sproj), L.ptr(w), L.ptr(dv), L.ptr(alpha), L.ptr(dctx), X + 8, L.ptr(dxproj), L.ptr(dx),
           T, B, N, A, X, L.stream())
    assert _is_poison(dxproj[B * N:]) and _is_poison(dx[B * N:])
    _check(dev, {k: _tau_term(o[:B * N], ref[k], True) for k, o in (("dxproj", dxproj), ("dx", dx))})


LARGE = (30, 1, 65, 1024, 768)    # 130,560 B and 99,840 B of dynamic LDS: above the 64 KB default, below the 150 KB limit


@pytest.mark.parametrize("small_first", [False, True], ids=["large", "small_then_large"])
def test_bwd_tokens_large_lds_vs_fp64(abi_dev, small_first):
    """dig_addattn_bwd_tokens as a function of random dv_all / alpha_all, with more dynamic LDS than a launch gets by default; after a small
    launch in the same process the limit has to grow."""
    from dig_amd import _lib as L
    if small_first:
        _tokens_run(L, abi_dev, (2, 1, 65, 64, 64))
    _tokens_run(L, abi_dev, LARGE)


def test_bwd_tokens_rejects_lds_above_limit(abi_dev):
    from dig_amd import _lib as L
    dev = abi_dev
    T, B, N, A, X = 40, 1, 8, 1024, 64                                      # (40 * 1024 + 40 * 64) * 4 = 174,080 B > 150 KB
    z = lambda *s, dt=BF: torch.zeros(*s, dtype=dt, device=dev)
    xproj, sproj, w, dv, alpha, dctx = z(B * N, A), z(T * B, A), z(A, dt=F32), z(T * B, N, dt=F32), z(T * B, N, dt=F32), z(T * B, X)
    dxproj, dx = _poisoned(dev, (B * N, A), BF), _poisoned(dev, (B * N, X), BF)
    with pytest.raises(L.DigHipError, match="unsupported"):
        L.call("dig_addattn_bwd_tokens", L.ptr(xproj), L.ptr(sproj), L.ptr(w), L.ptr(dv), L.ptr(alpha), L.ptr(dctx), X, L.ptr(dxproj), L.ptr(dx),
               T, B, N, A, X, L.stream())
    assert _is_poison(dxproj) and _is_poison(dx)


# ------------------------------------------------------------------------------------------------ 3. GRU cell
def _gru_ref(B, S, with_prev, sat):
    """gi, gh (bf16), s_prev, four ds terms (fp32) and the float64 reference of torch.nn.GRU's cell (gates r | z | n) with its autograd
    gradients.  sat: pre-activation terms up to 40 in magnitude, and planted pairs whose sum is +-96, +-80 (exp overflows to inf past 88.7)."""
    key = ("gru", B, S, with_prev, sat)
    if key not in _REF:
        g = torch.Generator().manual_seed(7 * B + S + 2 * with_prev + sat)
        if sat:
            gi, gh = ((torch.randn(B, 3 * S, generator=g) * 12).clamp(-40, 40) for _ in range(2))
            for j, val in enumerate((-48.0, 48.0, -40.0, 40.0)):
                for plane in range(3):                                           # elements j of r, z and n of every sample
                    gi[:, plane * S + j] = val
                    gh[:, plane * S + j] = val
        else:
            gi, gh = torch.randn(B, 3 * S, generator=g), torch.randn(B, 3 * S, generator=g)
        gi, gh = gi.bfloat16(), gh.bfloat16()
        s0 = torch.randn(B, S, generator=g) if with_prev else None
        ds = [torch.randn(B, S, generator=g) * f for f in (1.0, 0.5, -0.25, 2.0)]
        gid, ghd = gi.double().requires_grad_(True), gh.double().requires_grad_(True)
        s0d = s0.double().requires_grad_(True) if with_prev else torch.zeros(B, S, dtype=torch.float64)
        r = torch.sigmoid(gid[:, :S] + ghd[:, :S])
        z = torch.sigmoid(gid[:, S:2 * S] + ghd[:, S:2 * S])
        n = torch.tanh(gid[:, 2 * S:] + r * ghd[:, 2 * S:])
        s1 = (1 - z) * n + z * s0d
        fwd = {"s": s1.detach(), "r": r.detach(), "z": z.detach(), "n": n.detach()}
        bwd = []
        for k in range(1, 5):
            dsum = sum(d.double() for d in ds[:k])
            grads = torch.autograd.grad(s1, [gid, ghd], dsum, retain_graph=True)
            bwd.append({"dgi": grads[0], "dgh": grads[1], "ds_prev": dsum * z.detach()})     # (the direct z path; also d s1 / d s_prev)
        _REF[key] = ((gi, gh, s0, ds), fwd, bwd)
    return _REF[key]


@pytest.mark.parametrize("sat", [False, True], ids=["unit", "saturated"])
@pytest.mark.parametrize("with_prev", [True, False], ids=["s_prev", "null_s_prev"])
@pytest.mark.parametrize("B,S", [(5, 128), (3, 512), (1, 64), (7, 192)])
def test_gru_cell_vs_fp64(abi_dev, B, S, with_prev, sat):
    """dig_gru_cell_fwd (s, r | z | n | gh_n, the bf16 copy of s) and dig_gru_cell_bwd with 1..4 ds terms on the forward's own saved gates, with
    and without s_prev, against float64; saturated gates stay finite and within the same bounds."""
    from dig_amd import _lib as L
    dev = abi_dev
    (gi, gh, s0, ds), fwd, bwd = _gru_ref(B, S, with_prev, sat)
    gid, ghd, s0d = gi.to(dev), gh.to(dev), (s0.to(dev) if with_prev else None)
    s, sbf, gates = _poisoned(dev, (B + 1, S), F32), _poisoned(dev, (B + 1, S), BF), _poisoned(dev, (B + 1, 4 * S), F32)
    L.call("dig_gru_cell_fwd", L.ptr(gid), L.ptr(ghd), L.ptr(s0d), L.ptr(s), L.ptr(sbf), L.ptr(gates), B, S, L.stream())
    assert _is_poison(s[B:]) and _is_poison(sbf[B:]) and _is_poison(gates[B:])
    gt = gates[:B]
    terms = {"s": _tau_term(s[:B], fwd["s"], False)}
    for i, k in enumerate("rzn"):
        terms[k] = _tau_term(gt[:, i * S:(i + 1) * S], fwd[k], False)
    assert torch.equal(gt[:, 3 * S:].cpu(), gh[:, 2 * S:].float())                # gh_n: the bf16 input, exactly
    assert torch.equal(sbf[:B], s[:B].bfloat16())
    _check(dev, terms)
    dsd = [d.to(dev) for d in ds]
    for k in range(1, 5):
        dgi, dgh, dsp = _poisoned(dev, (B + 1, 3 * S), BF), _poisoned(dev, (B + 1, 3 * S), BF), _poisoned(dev, (B + 1, S), F32)
        p = [L.ptr(d) for d in dsd[:k]] + [None] * (4 - k)
        L.call("dig_gru_cell_bwd", *p, L.ptr(gates), L.ptr(s0d), L.ptr(dgi), L.ptr(dgh), L.ptr(dsp), B, S, L.stream())
        assert _is_poison(dgi[B:]) and _is_poison(dgh[B:]) and _is_poison(dsp[B:])
        ref = bwd[k - 1]
        _check(dev, {"dgi": _tau_term(dgi[:B], ref["dgi"], True), "dgh": _tau_term(dgh[:B], ref["dgh"], True),
                     "ds_prev": _tau_term(dsp[:B], ref["ds_prev"], False)})


# ------------------------------------------------------------------------------------------------ 4. embedding rows
@pytest.mark.parametrize("rows,cols", [(57, 40), (64, 512)])
def test_embed_rows_exact(abi_dev, rows, cols):
    """out[r, :cols] = bf16(table[clamp(token[r], 0, vocab - 1)]) bit for bit into a wider poisoned buffer; tokens below 0 and at or past
    vocab.  (The table has two rows behind `vocab`, so a clamp to `vocab` would read defined, different values.)"""
    from dig_amd import _lib as L
    dev = abi_dev
    vocab, ld = 99, cols + 24
    g = torch.Generator().manual_seed(rows + cols)
    table = torch.randn(vocab + 2, cols, generator=g)
    tok = torch.randint(0, vocab, (rows,), generator=g)
    tok[:5] = torch.tensor([-3, 0, vocab - 1, vocab, vocab + 1000])
    out = _poisoned(dev, (rows + 1, ld), BF)
    tok_d, table_d = tok.to(dev), table.to(dev)
    L.call("dig_embed_rows", L.ptr(tok_d), L.ptr(table_d), L.ptr(out), ld, rows, cols, vocab, L.stream())
    assert torch.equal(out[:rows, :cols].cpu(), table[tok.clamp(0, vocab - 1)].bfloat16())
    assert _is_poison(out[:rows, cols:]) and _is_poison(out[rows:])


# ------------------------------------------------------------------------------------------------ 5. host-side argument rejection
class _Args:
    """Valid arguments of the six entry points at one small shape, in buffers large enough for every shape a test below asks to have rejected
    (N <= 513, A, X <= 1032): inputs zero, outputs (and dw_acc) poisoned."""

    def __init__(self, dev):
        z = lambda n, dt=BF: torch.zeros(n, dtype=dt, device=dev)
        p = lambda n, dt=BF: _poisoned(dev, (n,), dt)
        B, N, A, X, T = self.dims = (2, 16, 16, 16, 2)
        MN, MA = 513, 1032
        self.xproj, self.sproj, self.w, self.x = z(B * MN * MA + 8), z(T * B * MA), z(MA, F32), z(B * MN * MA + 8)
        self.alpha_in, self.dv_in, self.dctx = z(T * B * MN, F32), z(T * B * MN, F32), z(T * B * (MA + 8))
        self.alpha, self.ctx, self.dv, self.dsproj, self.dw_acc = p(B * MN, F32), p(B * (MA + 8)), p(B * MN, F32), p(B * MA), p(B * MA, F32)
        self.dxproj, self.dx = p(B * MN * MA), p(B * MN * MA)
        S = 16
        self.gi, self.gh, self.s_prev, self.ds = z(B * 3 * S), z(B * 3 * S), z(B * S, F32), z(B * S, F32)
        self.s, self.sbf, self.gates, self.gates_in = p(B * S, F32), p(B * S), p(B * 4 * S, F32), z(B * 4 * S, F32)
        self.dgi, self.dgh, self.dsp = p(B * 3 * S), p(B * 3 * S), p(B * S, F32)
        self.tok, self.table, self.emb = torch.zeros(4, dtype=torch.int64, device=dev), z(8 * 16, F32), p(4 * 24)
        self.S = S
        self.outputs = [self.alpha, self.ctx, self.dv, self.dsproj, self.dw_acc, self.dxproj, self.dx, self.s, self.sbf, self.gates, self.dgi, self.dgh,
                        self.dsp, self.emb]

    def fwd(self, L, N=None, A=None, X=None, ldc=None, xproj=None):
        B, N0, A0, X0, _ = self.dims
        N, A, X = N or N0, A or A0, X or X0
        return "dig_addattn_fwd", [xproj or L.ptr(self.xproj), L.ptr(self.sproj), L.ptr(self.w), L.ptr(self.x), L.ptr(self.alpha), L.ptr(self.ctx),
                                   ldc or 1040, B, N, A, X, L.stream()], 6

    def bwd(self, L, N=None, A=None, X=None, xproj=None):
        B, N0, A0, X0, _ = self.dims
        N, A, X = N or N0, A or A0, X or X0
        return "dig_addattn_bwd", [xproj or L.ptr(self.xproj), L.ptr(self.sproj), L.ptr(self.w), L.ptr(self.x), L.ptr(self.alpha_in), L.ptr(self.dctx),
                                   1040, L.ptr(self.dv), L.ptr(self.dsproj), L.ptr(self.dw_acc), B, N, A, X, L.stream()], 10

    def tokens(self, L):
        B, N, A, X, T = self.dims
        return "dig_addattn_bwd_tokens", [L.ptr(self.xproj), L.ptr(self.sproj), L.ptr(self.w), L.ptr(self.dv_in), L.ptr(self.alpha_in), L.ptr(self.dctx),
                                          X + 8, L.ptr(self.dxproj), L.ptr(self.dx), T, B, N, A, X, L.stream()], 9

    def gru_fwd(self, L):
        return "dig_gru_cell_fwd", [L.ptr(self.gi), L.ptr(self.gh), L.ptr(self.s_prev), L.ptr(self.s), L.ptr(self.sbf), L.ptr(self.gates), self.dims[0],
                                    self.S, L.stream()], 6

    def gru_bwd(self, L):
        return "dig_gru_cell_bwd", [L.ptr(self.ds), None, None, None, L.ptr(self.gates_in), L.ptr(self.s_prev), L.ptr(self.dgi), L.ptr(self.dgh),
                                    L.ptr(self.dsp), self.dims[0], self.S, L.stream()], 9

    def embed(self, L):
        return "dig_embed_rows", [L.ptr(self.tok), L.ptr(self.table), L.ptr(self.emb), 24, 4, 16, 8, L.stream()], 3

    def rejected(self, L, call, match):
        name, args, _ = call
        with pytest.raises(L.DigHipError, match=match):
            L.call(name, *args)
        if self.alpha.device.type == "cuda":
            torch.cuda.synchronize()
        assert all(_is_poison(o) for o in self.outputs), name


# optional pointers (NULL is a documented value): s_prev of both GRU calls, ds_b..ds_d of the backward
_OPTIONAL = {"dig_gru_cell_fwd": {2}, "dig_gru_cell_bwd": {1, 2, 3, 5}}


def test_gru_attention_entry_points_reject_bad_arguments(abi_dev):
    """The host-side checks in front of the launches (mirrored by the CPU build): shapes past the kernels' LDS arrays, channel counts that
    break the 16-byte / 4-byte loads, null required pointers, a misaligned xproj.  A rejected call writes nothing."""
    from dig_amd import _lib as L
    a = _Args(abi_dev)
    bad = "bad argument"
    for kw in ({"N": 513}, {"A": 1032}, {"A": 516}, {"X": 15}, {"ldc": 25}):
        a.rejected(L, a.fwd(L, **kw), bad)
    for kw in ({"N": 513}, {"A": 1032}, {"A": 516}, {"X": 1032}, {"X": 516}):
        a.rejected(L, a.bwd(L, **kw), bad)
    for make in (a.fwd, a.bwd, a.tokens, a.gru_fwd, a.gru_bwd, a.embed):
        name, args, n_ptr = make(L)
        for i in range(n_ptr):
            if i in _OPTIONAL.get(name, ()) or isinstance(args[i], int):            # (ldd sits among the pointers)
                continue
            nulled = list(args)
            nulled[i] = None
            a.rejected(L, (name, nulled, n_ptr), bad)
    off8 = type(L.ptr(a.w))(a.xproj.data_ptr() + 8)
    a.rejected(L, a.fwd(L, xproj=off8), "misaligned")
    a.rejected(L, a.bwd(L, xproj=off8), "misaligned")
    for make in (a.fwd, a.bwd, a.tokens, a.gru_fwd, a.gru_bwd, a.embed):            # and the unmodified arguments are accepted
        name, args, _ = make(L)
        L.call(name, *args)
