"""Every fused GELU site (dig_amd/csrc/common.h: gelu_f / erf_poly, gelu_fast_f / gelu_fast2, dgelu_f / dgelu2, dgelu_acc_f, compiled into the
epilogues of the three GEMM kernel families of gemm.hip, the fused MLP chain of mlp_chain.hip and LayerNorm + GELU of norm.hip) at every finite
bf16 pre-activation against float64 torch, on both builds of the ABI (`abi_dev`: libdig_hip.so on the MI355X and cpu_abi/libdig_cpu.so, whose
GELU is std::erf and leaves excesses near 1e-7).

Reference and bounds (derived, not measured on the kernels)
-----------------------------------------------------------
The reference is torch float64 with x the pre-activation the kernel actually saw:

    G(x) = x / 2 (1 + erf(x / sqrt 2))          G'(x) = Phi(x) + x phi(x)

    GELU value, bf16 output                 |got - G|        <= 2^-8 |G| + E_g |x|
    GELU value, fp32 output                 |got - G|        <= 2^-22 |G| + E_g |x|
    derivative, dgelu_f / dgelu2, bf16      |got - d G'|     <= 2^-8 |d G'| + |d| E_d
    derivative, dgelu_f, fp32 output        |got - d G'|     <= 2^-22 |d G'| + |d| E_d
    64-row column sums of d G' (fp32)       |got - sum d G'| <= sum |d| (E_d + 2^-22)
    derivative, dgelu_acc_f (fp32 dbeta)    |got - sum d G'| <= sum |d| (E_a + 2^-22)

E_g = 5e-5: the approximation error of the two fitted GELU forms, relative to |x| (an fp32-FMA restatement of the coefficients gives 4.86e-5 |x|
for gelu_f and 4.73e-5 |x| for gelu_fast_f, both beyond the clamp, |x| > 4.24, where erf_poly(3) = 0.99990284 stands for 1; fp32 effects are
near 1e-7).  E_d = 2.8e-4 and E_a = 5e-5 are the bounds common.h documents (restatement: 2.71e-4 at x = 3.924, 4.86e-5 at x ~ 6.03).
2^-8 is one bf16 rounding of the result (the allowance of test_gelu_bwd_every_finite_bf16), 2^-22 four fp32 roundings (0.5 x (1 + erf); the
product and the sums of a column); where the result is a subnormal of its format the rounding allowance is half the subnormal spacing instead
(2^-134 for bf16, 2^-150 for fp32: round-to-nearest is absolute there, G(x) = x / 2 of the smallest normal x loses a bit whatever computes
it).  `test_polynomial_restatement_is_inside_the_bounds` holds a torch restatement of the four polynomials
(every Horner step a float64 multiply-add rounded to fp32) to E_g |x|, E_d and E_a over the sweep and over 2,000,001 fp32 points of [-8, 8],
and requires it to reach 0.8 of each: the bounds are not vacuous and the reference is not broken.  Every output must be finite, +-3.39e38
included.  For large negative x the kernels return about -4.9e-5 |x| where erf-GELU is -0 (-3e-3 at x = -64): inside E_g |x|, a stated property.
A bound that a kernel exceeds is a finding to investigate, not a number to raise.

Inputs
------
`sweep`: the 65,280 finite bf16 bit patterns.  A matrix holds value[slot] = sweep[(slot * 7919 + off) mod 65280] (7919 is prime and coprime to
65280 = 2^8 3 5 17: every value once per 65,280 slots, and every tile position -- wave, lane, tick, quad -- sees values of the whole range);
each matrix-shaped case runs with off = 0 and 11.

Cases -> the branch each exists for
-----------------------------------
1. GEMM forward epilogue, act 1 (gelu_f): A = layout [256, 768], B = identity, so C = GELU(A) and `pre` = A as numbers (-0 comes back +0; a
   subnormal input may come back as itself or as 0 -- how the matrix core treats bf16 subnormals is not documented -- and x is read from the
   returned `pre`; the other 65,026 values must come back as they went in).
       tiles 64, 32 (gemm_kernel), 244, 264, 212, 221 (gemm_wide_kernel: 16 / 12 / 2 / 2 waves)     bf16 and fp32 output
       tiles 544, 564 (gemm_pwide_kernel, persistent)                                              bf16 output, with and without `pre`
       every tile without `pre`: bit-equal to the run with it (the side store does not change the arithmetic)
       dense: tile 64, fp32 output, A = 0, bias = linspace(-8, 8, 8192) + k / 4 step, k = 0..3 (I = 128, J = 8192, R = 64): pre-activations that
       are not bf16 values, as in real use
   The output is a view of a buffer with one poisoned row behind row I, which must survive.
2. GEMM data-gradient epilogue, act 2 (dgelu_f): trans_b, dy[:, 0] = d, w[0, :] = 1 (R = 64): the product is exactly d; resid = layout [256, 768],
   read directly, so all 65,280 values count.  d = 1 and a random bf16 column.
       tiles 32, 64    bf16 and fp32 output;   244, 264, 212, 221    bf16 output;   32, 64, 244 also with colsum_partials (fp32, per 64 rows)
3. LayerNorm + GELU forward (gelu_f) and backward (dgelu_acc_f): gamma = 0 and x = 0 make the normalised row vanish: y = GELU(beta[c]) in every
   row, and dbeta[c] = sum_r dy[r, c] G'(beta[c]) in fp32 with no bf16 rounding; dx = 0 and dgamma = 0 exactly.
       D = 512: 128 launches, beta = the sweep widened to fp32; forward rows = 5 (a last row group shorter than the 2 rows a wave keeps in
       flight); backward rows = 1 with dy = 1 and rows = 3 with random bf16 dy
       D = 64, 128, 192, 256, 384: linspace(-8, 8, D), and +-0, +-1e-30, +-3, +-4.2426, +-6, +-64, +-3.39e38 repeated to D
4. Fused MLP chain forward (gelu_fast2), D = 384, F = 1536, R = 256: x = layout, w1[f, f mod 384] = 1, w2[d, d] = 1, biases and residual 0:
   `pre` = x tiled four times (rule of 1), `act` against G, `out` bit-equal to act[:, :384] (a -0 in `act`, the half of the smallest negative
   subnormal, leaves the second GEMM as +0: zeros compare as numbers); save=False bit-equal; the same through dig_mlp_chain_fwd_ln with rows
   that are normalised already (ln_g = None, resid = 0), F = 1536 and 2048.
5. Fused MLP chain backward (dgelu2), R = 128, F = 1536: pre = layout [128, 1536], dy[:, 0] = d, w2t[:, 0] = 1, d = 1 and random; dpre against
   d G' from dig_mlp_chain_bwd, dig_mlp_chain_bwd_ln and dig_mlp_chain_bwd_ln_proj (printed: whether the three are bit-equal).
6. The restatement (CPU only), above.

Largest excess per site on the MI355X (the printed figure: (|err| - the rounding allowance) / the scale its E multiplies), E in brackets
-----------------------------------------------------------------------------------------------------------------------------------
The device agrees with the restatement at every site; no kernel exceeded a bound.  (A bf16 value output adds up to 2^-8 of the spurious
-4.86e-5 |x| itself, which 2^-8 |G| does not cover where G is -0: 4.858e-5 (1 + 2^-8) = 4.877e-5.)
    1. GEMM act 1, every tile (64, 32, 244, 264, 212, 221, 544, 564), both offsets     bf16 out 4.876e-5 |x| at x = -1352 / -1.4e9   [5e-5]
                                                                                       fp32 out 4.858e-5 |x| at x = -2.4e15
       dense fp32 bias, k = 0..3                                                       4.858e-5 |x| at x = -7.51
       `pre` came back equal to the input for every value, subnormals included
    2. GEMM act 2, every tile (32, 64, 244, 264, 212, 221)                             bf16 out 2.569e-4 (d = 1) / 2.575e-4 (random d) at
                                                                                       x = -3.921875; fp32 out 2.584e-4 at x = -3.34375 [2.8e-4]
       colsum_partials (32, 64, 244)                                                   1.52e-5 (d = 1) / 6.86e-5 (random d) per unit of sum |d|
    3. LayerNorm + GELU forward                                                        4.876e-5 |x| at x = -10.5625 (D = 512), 4.870e-5 ..
                                                                                       4.873e-5 |x| at the other widths                 [5e-5]
       backward (dbeta)                                                                4.860e-5 at x = 6.0625 (rows 1), 4.867e-5 (rows 3, D = 512),
                                                                                       4.859e-5 .. 4.869e-5 at the other widths  [5e-5 + 2^-22]
    4. mlp_chain_fwd, mlp_chain_fwd_ln (F = 1536, 2048)                                4.739e-5 |x| at x = -1.9e14 / -7.3e11           [5e-5]
    5. mlp_chain_bwd, _bwd_ln, _bwd_ln_proj                                            2.569e-4 (d = 1), 2.548e-4 / 2.578e-4 (random d) at
                                                                                       x = -3.921875; the three dpre are bit-equal    [2.8e-4]
    6. restatement: gelu_f 4.863e-5 |x| (4.350e-5 for |x| <= 4.24), gelu_fast_f 4.726e-5 |x| (4.573e-5), dgelu_f 2.709e-4 at x = 3.92396,
       dgelu_acc_f 4.861e-5 at x = 6.03444; 1 - erf_poly(3) = 9.716e-5
On the CPU build (std::erf) every figure is below 2e-7.
"""
import math

import numpy as np
import pytest
import torch

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
E_G, E_D, E_A = 5e-5, 2.8e-4, 5e-5
R8, R22 = 2.0 ** -8, 2.0 ** -22
POISON = 768.0                    # (exact in bf16)
N = 65280
STRIDE = 7919
OFFS = (0, 11)


def _backend(dev):
    return "hip" if dev.type == "cuda" else "cpu_abi"


def _make_sweep():
    bits = np.arange(65536, dtype=np.uint32)
    bits = bits[((bits >> 7) & 0xff) != 0xff]
    assert bits.size == N and math.gcd(STRIDE, N) == 1
    return torch.from_numpy(bits.astype(np.uint16).view(np.int16).copy()).view(BF)


SWEEP = _make_sweep()             # computed once, never modified
TINY = 2.0 ** -126                # below it a bf16 value is subnormal
assert int(((SWEEP.float() == 0) | (SWEEP.float().abs() >= TINY)).sum()) == 65026


def _layout(rows, cols, off):
    """[rows, cols] bf16, value[slot] = sweep[(slot * 7919 + off) mod n]."""
    slot = torch.arange(rows * cols, dtype=torch.int64)
    return SWEEP[(slot * STRIDE + off) % N].view(rows, cols).clone()


def G(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def Gp(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def _check(tag, dev, got, ref, rel, scale, E, x):
    """|got - ref| <= max(rel |ref|, floor) + E scale, element-wise, in float64; prints the largest (|err| - the rounding allowance) / scale and
    the x where it occurs."""
    floor = 2.0 ** -134 if got.dtype == BF else 2.0 ** -150            # half the spacing of the format's subnormals: where RNE is absolute
    got, ref, scale, x = got.detach().cpu().double().reshape(-1), ref.reshape(-1), scale.reshape(-1), x.reshape(-1)
    assert bool(torch.isfinite(ref).all()) and got.shape == ref.shape == scale.shape == x.shape
    assert bool(torch.isfinite(got).all()), (tag, "non-finite output at x =", x[~torch.isfinite(got)][:8].tolist())
    rest = (got - ref).abs() - torch.clamp_min(rel * ref.abs(), floor)  # what the approximation has to explain
    ratio = rest / scale.clamp_min(1e-300)                              # (inf-like where a zero scale meets any error)
    i = int(ratio.argmax())
    print(f"{tag} {_backend(dev)}: largest (|err| - {rel:.1e} |ref|) / scale = {float(ratio[i]):.3e} at x = {float(x[i]):.7g} (E = {E:.3g})")
    bad = rest > E * scale
    assert not bool(bad.any()), (tag, int(bad.sum()), float(ratio[i]), float(x[i]), float(got[i]), float(ref[i]))
    return float(ratio[i])


def _check_pre(tag, pre, want):
    """The returned pre-activation equals the input as numbers; a subnormal input may also come back as 0.  Returns x = pre in float64."""
    p, w = pre.detach().cpu().float(), want.float()
    sub = (w != 0) & (w.abs() < TINY)
    assert bool((p[~sub] == w[~sub]).all()), (tag, "a normal pre-activation changed")
    assert bool(((p[sub] == w[sub]) | (p[sub] == 0)).all()), (tag, "a subnormal pre-activation is neither itself nor 0")
    print(f"{tag}: {int((p[sub] == 0).sum())} of {int(sub.sum())} subnormal pre-activations came back as 0")
    return p.double()


def _same_bits(a, b):
    return torch.equal(a.detach().cpu().contiguous().view(torch.int16 if a.dtype == BF else torch.int32),
                       b.detach().cpu().contiguous().view(torch.int16 if b.dtype == BF else torch.int32))


# ------------------------------------------------------------------------------------------------ 1. GEMM forward epilogue (gelu_f)
I1, J1 = 256, 768
FWD_CASES = [(bk, ok) for bk in (64, 32, 244, 264, 212, 221) for ok in (0, 1)] + [(544, 0), (564, 0)]


@pytest.mark.parametrize("off", OFFS)
@pytest.mark.parametrize("bk,out_kind", FWD_CASES)
def test_gemm_fwd_gelu_every_finite_bf16(abi_dev, bk, out_kind, off):
    from dig_amd import ops
    dev = abi_dev
    a = _layout(I1, J1, off)
    A, B = a.to(dev), torch.eye(J1).bfloat16().to(dev)
    dt = BF if out_kind == 0 else F32
    buf = torch.full((I1 + 1, J1), POISON, dtype=dt, device=dev)
    pbuf = torch.full((I1 + 1, J1), POISON, dtype=BF, device=dev)
    ops.gemm(A, B, I1, J1, J1, act=1, pre=pbuf[:I1], out=buf[:I1], out_kind=out_kind, bk=bk)
    x = _check_pre(f"gemm fwd {bk}", pbuf[:I1], a)
    _check(f"gemm fwd act=1 tile {bk} out {'bf16' if out_kind == 0 else 'fp32'} off {off}", dev, buf[:I1], G(x), R8 if out_kind == 0 else R22,
           x.abs(), E_G, x)
    assert bool((buf[I1].float() == POISON).all()) and bool((pbuf[I1].float() == POISON).all())
    buf2 = torch.full((I1 + 1, J1), POISON, dtype=dt, device=dev)
    ops.gemm(A, B, I1, J1, J1, act=1, out=buf2[:I1], out_kind=out_kind, bk=bk)
    assert _same_bits(buf2, buf), "the result without `pre` differs from the result with it"


def test_gemm_fwd_gelu_dense_fp32(abi_dev):
    from dig_amd import ops
    dev = abi_dev
    I, J, R = 128, 8192, 64
    A, B = torch.zeros(I, R, dtype=BF, device=dev), torch.zeros(J, R, dtype=BF, device=dev)
    step = 16.0 / (J - 1)
    worst = 0.0
    for k in range(4):
        bias = (torch.linspace(-8, 8, J, dtype=F64) + k * step / 4).float()
        buf = torch.full((I + 1, J), POISON, dtype=F32, device=dev)
        ops.gemm(A, B, I, J, R, act=1, bias=bias.to(dev), out=buf[:I], out_kind=ops.OUT_F32, bk=64)
        x = bias.double().expand(I, J).contiguous()
        worst = max(worst, _check(f"gemm fwd act=1 dense fp32 k {k}", dev, buf[:I], G(x), R22, x.abs(), E_G, x))
        assert bool((buf[I] == POISON).all())


# ------------------------------------------------------------------------------------------------ 2. GEMM data-gradient epilogue (dgelu_f)
DGRAD_CASES = [(32, 0, False), (32, 1, False), (64, 0, False), (64, 1, False), (244, 0, False), (264, 0, False), (212, 0, False),
               (221, 0, False), (32, 0, True), (64, 0, True), (244, 0, True)]


def _dcol(kind, rows):
    if kind == "ones":
        return torch.ones(rows, dtype=BF)
    return torch.randn(rows, generator=torch.Generator().manual_seed(rows)).bfloat16()


@pytest.mark.parametrize("dkind", ["ones", "random"])
@pytest.mark.parametrize("off", OFFS)
@pytest.mark.parametrize("bk,out_kind,colsum", DGRAD_CASES)
def test_gemm_dgrad_dgelu_every_finite_bf16(abi_dev, bk, out_kind, colsum, off, dkind):
    from dig_amd import ops
    dev = abi_dev
    R = 64
    pre = _layout(I1, J1, off)
    d = _dcol(dkind, I1)
    dy = torch.zeros(I1, R, dtype=BF)
    dy[:, 0] = d
    w = torch.zeros(R, J1, dtype=BF)
    w[0, :] = 1
    dt = BF if out_kind == 0 else F32
    buf = torch.full((I1 + 1, J1), POISON, dtype=dt, device=dev)
    parts = torch.full((I1 // 64 + 1, J1), POISON, dtype=F32, device=dev) if colsum else None
    ops.gemm(dy.to(dev), w.to(dev), I1, J1, R, tb=True, act=2, resid=pre.to(dev), out=buf[:I1], out_kind=out_kind, bk=bk,
             colsum_partials=parts[:I1 // 64] if colsum else None)
    x = pre.double()
    dd = d.double()[:, None].expand(I1, J1)
    ref = dd * Gp(x)
    tag = f"gemm dgrad act=2 tile {bk} out {'bf16' if out_kind == 0 else 'fp32'}{' colsum' if colsum else ''} off {off} d {dkind}"
    _check(tag, dev, buf[:I1], ref, R8 if out_kind == 0 else R22, dd.abs().contiguous(), E_D, x)
    assert bool((buf[I1].float() == POISON).all())
    if colsum:
        _check(tag + " partials", dev, parts[:I1 // 64], ref.view(I1 // 64, 64, J1).sum(1), 0.0,
               dd.abs().reshape(I1 // 64, 64, J1).sum(1), E_D + R22, x.view(I1 // 64, 64, J1)[:, 0].contiguous())
        assert bool((parts[I1 // 64] == POISON).all())


# ------------------------------------------------------------------------------------------------ 3. LayerNorm + GELU (gelu_f, dgelu_acc_f)
SPECIALS = [s * v for v in (0.0, 1e-30, 3.0, 4.2426, 6.0, 64.0, 3.39e38) for s in (1.0, -1.0)]


def _ln_case(dev, betas, tag):
    """betas [launches, D] fp32: forward rows = 5, backward rows = 1 (dy = 1) and rows = 3 (random bf16 dy), gamma = 0, x = 0."""
    from dig_amd import ops
    L, D = betas.shape
    eps = 1e-6
    gamma = torch.zeros(D, device=dev)
    x5 = torch.zeros(5, D, dtype=BF, device=dev)
    _, mean, rstd = ops.layernorm_fwd(x5, gamma, gamma, eps)
    assert bool((mean == 0).all()) and bool(torch.isfinite(rstd).all())
    dy3 = torch.randn(3, D, generator=torch.Generator().manual_seed(D)).bfloat16()
    dy1 = torch.ones(1, D, dtype=BF)
    dy3d, dy1d = dy3.to(dev), dy1.to(dev)
    bd = betas.to(dev)
    ys, dx_zero = [], True
    dg = torch.zeros(2, L, D, device=dev)
    db = torch.zeros(2, L, D, device=dev)
    for l in range(L):
        ys.append(ops.layernorm_fwd(x5, gamma, bd[l], eps, gelu=True)[0])
        dx1 = ops.layernorm_bwd(dy1d, x5[:1], gamma, bd[l], mean[:1], rstd[:1], None, dg[0, l], db[0, l], gelu=True)
        dx3 = ops.layernorm_bwd(dy3d, x5[:3], gamma, bd[l], mean[:3], rstd[:3], None, dg[1, l], db[1, l], gelu=True)
        if l % 16 == 0 or l == L - 1:
            dx_zero = dx_zero and bool((dx1.float() == 0).all()) and bool((dx3.float() == 0).all())
    assert dx_zero and bool((dg == 0).all()), (tag, "dx / dgamma must vanish with gamma = 0 and x = 0")
    xb = betas.double()
    y = torch.stack(ys).cpu()                                            # [L, 5, D]
    xr = xb[:, None, :].expand(L, 5, D).contiguous()
    _check(f"layernorm+gelu fwd D {D} {tag}", dev, y, G(xr), R8, xr.abs(), E_G, xr)
    gp = Gp(xb)
    _check(f"layernorm+gelu bwd D {D} {tag} rows 1", dev, db[0], gp, 0.0, torch.ones_like(gp), E_A + R22, xb)
    d3 = dy3.double()                                                    # [3, D]
    ref3 = (d3[None] * gp[:, None, :]).sum(1)
    _check(f"layernorm+gelu bwd D {D} {tag} rows 3", dev, db[1], ref3, 0.0, d3.abs().sum(0)[None].expand(L, D).contiguous(), E_A + R22, xb)


def test_layernorm_gelu_every_finite_bf16(abi_dev):
    D = 512
    L = (N + D - 1) // D
    assert L == 128
    idx = torch.arange(L * D) % N
    _ln_case(abi_dev, SWEEP[idx].float().view(L, D), "sweep")


@pytest.mark.parametrize("D", [64, 128, 192, 256, 384])
def test_layernorm_gelu_other_widths(abi_dev, D):
    lin = torch.linspace(-8, 8, D, dtype=F64).float()
    sp = torch.tensor(SPECIALS, dtype=F64).float()
    assert bool(torch.isfinite(sp).all())
    _ln_case(abi_dev, torch.stack([lin, sp[torch.arange(D) % sp.numel()]]), "linspace + specials")


# ------------------------------------------------------------------------------------------------ 4. fused MLP chain forward (gelu_fast2)
def _chain_weights(D, Fh, dev):
    w1 = torch.zeros(Fh, D, dtype=BF)
    w1[torch.arange(Fh), torch.arange(Fh) % D] = 1
    w2 = torch.zeros(D, Fh, dtype=BF)
    w2[torch.arange(D), torch.arange(D)] = 1
    return w1.to(dev), torch.zeros(Fh, device=dev), w2.to(dev), torch.zeros(D, device=dev)


def _check_chain_fwd(tag, dev, xin, out, pre, act, Fh):
    D = xin.shape[1]
    want = xin.repeat(1, (Fh + D - 1) // D)[:, :Fh]
    x = _check_pre(tag, pre, want)
    _check(tag, dev, act, G(x), R8, x.abs(), E_G, x)
    o, a = out.detach().cpu(), act.detach().cpu()[:, :D].contiguous()
    z = (a.float() == 0)                                                 # (a -0 hidden value leaves fc2's sum as +0)
    assert bool((o.float()[z] == 0).all()) and _same_bits(torch.where(z, torch.zeros_like(o), o), torch.where(z, torch.zeros_like(a), a)), \
        (tag, "out is not act[:, :D]")


@pytest.mark.parametrize("off", OFFS)
def test_mlp_chain_fwd_every_finite_bf16(abi_dev, off):
    from dig_amd import ops
    dev = abi_dev
    R, D, Fh = 256, 384, 1536
    xin = _layout(R, D, off)
    xd = xin.to(dev)
    w1, b1, w2, b2 = _chain_weights(D, Fh, dev)
    res = torch.zeros(R, D, dtype=BF, device=dev)
    out, pre, act = ops.mlp_chain_fwd(xd, w1, b1, w2, b2, res, save=True)
    _check_chain_fwd(f"mlp_chain_fwd F {Fh} off {off}", dev, xin, out, pre, act, Fh)
    assert _same_bits(ops.mlp_chain_fwd(xd, w1, b1, w2, b2, res), out), "save=False changes the result"


@pytest.mark.parametrize("off", OFFS)
@pytest.mark.parametrize("Fh", [1536, 2048])
def test_mlp_chain_fwd_ln_every_finite_bf16(abi_dev, Fh, off):
    from dig_amd import ops
    dev = abi_dev
    R, D = 256, 384
    xin = _layout(R, D, off)
    xd = xin.to(dev)
    w1, b1, w2, b2 = _chain_weights(D, Fh, dev)
    res = torch.zeros(R, D, dtype=BF, device=dev)
    r = ops.mlp_chain_fwd_ln(xd, None, None, 1e-6, w1, b1, w2, b2, save=True, resid=res)
    _check_chain_fwd(f"mlp_chain_fwd_ln F {Fh} off {off}", dev, xin, r["out"], r["pre"], r["act"], Fh)
    q = ops.mlp_chain_fwd_ln(xd, None, None, 1e-6, w1, b1, w2, b2, resid=res)
    assert _same_bits(q["out"], r["out"]), "save=False changes the result"


# ------------------------------------------------------------------------------------------------ 5. fused MLP chain backward (dgelu2)
@pytest.mark.parametrize("dkind", ["ones", "random"])
@pytest.mark.parametrize("off", OFFS)
def test_mlp_chain_bwd_every_finite_bf16(abi_dev, off, dkind):
    from dig_amd import ops
    dev = abi_dev
    R, D, Fh = 128, 384, 1536
    g = torch.Generator().manual_seed(5 + off)
    pre = _layout(R, Fh, off)
    d = _dcol(dkind, R)
    dy = torch.zeros(R, D, dtype=BF)
    dy[:, 0] = d
    w2t = torch.zeros(Fh, D, dtype=BF)
    w2t[:, 0] = 1
    w1t = (torch.randn(D, Fh, generator=g) * 0.06).bfloat16().to(dev)
    x_mid = (torch.randn(R, D, generator=g) * 1.3 + 0.2).bfloat16().to(dev)
    gam, bet = (1.0 + 0.3 * torch.randn(D, generator=g)).to(dev), (0.1 * torch.randn(D, generator=g)).to(dev)
    projt = (torch.randn(D, D, generator=g) * 0.05).bfloat16().to(dev)
    _, mu, rs = ops.layernorm_fwd(x_mid, gam, bet, 1e-6)
    dyd, w2d, pred = dy.to(dev), w2t.to(dev), pre.to(dev)
    x = pre.double()
    dd = d.double()[:, None].expand(R, Fh).contiguous()
    ref = dd * Gp(x)
    got = {"bwd": ops.mlp_chain_bwd(dyd, w2d, pred, w1t)[1],
           "bwd_ln": ops.mlp_chain_bwd_ln(dyd, w2d, pred, w1t, x_mid, gam, mu, rs)[1],
           "bwd_ln_proj": ops.mlp_chain_bwd_ln(dyd, w2d, pred, w1t, x_mid, gam, mu, rs, projt=projt)[1]}
    for name, dpre in got.items():
        _check(f"mlp_chain_{name} dpre off {off} d {dkind}", dev, dpre, ref, R8, dd.abs(), E_D, x)
    print(f"mlp_chain_bwd dpre {_backend(dev)} off {off} d {dkind}: bwd_ln bit-equal to bwd: {_same_bits(got['bwd_ln'], got['bwd'])}, "
          f"bwd_ln_proj bit-equal to bwd: {_same_bits(got['bwd_ln_proj'], got['bwd'])}")


# ------------------------------------------------------------------------------------------------ 6. the bounds are not vacuous (CPU only)
def _fma(a, b, c):
    """fp32 fma(a, b, c): the float64 multiply-add (the product of two fp32 values is exact in float64) rounded to fp32."""
    return (a.double() * b.double() + c).float()


def _horner(t, coeffs):
    p = torch.full_like(t, np.float32(coeffs[0]))
    for c in coeffs[1:]:
        p = _fma(p, t, float(np.float32(c)))
    return p


ERF_POLY = (-4.055360137e-07, 1.715983126e-05, -3.145953815e-04, 3.318710718e-03, -2.268579789e-02, 1.077178270e-01, -3.732314110e-01,
            1.127895713e+00)
GELU_FAST = (-1.120145568e-09, 9.479557069e-08, -3.475820744e-06, 7.333383917e-05, -1.002580095e-03, 9.521000741e-03, -6.597861542e-02,
             3.987713536e-01)
DGELU = (-1.763060760e+01, 8.145713806e+01, -1.613111115e+02, 1.802621155e+02, -1.259510422e+02, 5.725678253e+01, -1.676991081e+01,
         3.186886549e+00)
RSQRT2, RSQRT2PI = float(np.float32(0.70710678118654752)), float(np.float32(0.39894228040143268))


def _erf_poly(z):
    zc = z.clamp(-3.0, 3.0)
    return _horner(zc * zc, ERF_POLY) * zc


def _gelu_f(x):
    return 0.5 * x * (1.0 + _erf_poly(x * RSQRT2))


def _gelu_fast_f(x):
    c = float(np.float32(4.2426405))
    xc = x.clamp(-c, c)
    return x * _fma(xc, _horner(xc * xc, GELU_FAST), 0.5)


def _dgelu_f(x):
    z = (x * 0.25).clamp(-1.0, 1.0)
    return _fma(_horner(z * z, DGELU), z, 0.5)


def _dgelu_acc_f(x):
    cdf = 0.5 * (1.0 + _erf_poly(x * RSQRT2))
    pdf = RSQRT2PI * torch.exp(-0.5 * x * x)
    return cdf + x * pdf


def test_polynomial_restatement_is_inside_the_bounds():
    """The four polynomials of common.h, restated in torch fp32 with emulated FMAs, against float64 over the sweep and a 2,000,001-point fp32
    grid on [-8, 8]: inside E_g |x|, E_d, E_a and reaching 0.8 of each.  Expected: gelu_f 4.86e-5 |x|, gelu_fast_f 4.73e-5 |x| (both beyond
    the clamp), dgelu_f 2.71e-4 at x = 3.924, dgelu_acc_f 4.86e-5 at x ~ 6.03; erf_poly(3) = 0.99990284."""
    x = torch.cat([SWEEP.float(), torch.linspace(-8, 8, 2000001, dtype=F64).float()])
    assert x.dtype == F32
    xd = x.double()
    e3 = float(_erf_poly(torch.tensor([3.0]))[0])
    print(f"erf_poly(3) = {e3:.8f}, 1 - erf_poly(3) = {1 - e3:.3e}")
    assert 9.6e-5 < 1 - e3 < 9.8e-5
    nz = xd != 0
    inside = xd.abs() <= 4.24
    for name, fn, ref, rel, E in (("gelu_f", _gelu_f, G(xd), True, E_G), ("gelu_fast_f", _gelu_fast_f, G(xd), True, E_G),
                                  ("dgelu_f", _dgelu_f, Gp(xd), False, E_D), ("dgelu_acc_f", _dgelu_acc_f, Gp(xd), False, E_A)):
        got = fn(x).double()
        assert bool(torch.isfinite(got).all()), name
        err = (got - ref).abs()
        if rel:
            assert bool((err[~nz] == 0).all())
            err = torch.where(nz, err / xd.abs().clamp_min(1e-300), torch.zeros_like(err))
        i = int(err.argmax())
        msg = f"restatement {name}: largest error {float(err[i]):.3e}{' |x|' if rel else ''} at x = {float(x[i]):.6g} (E = {E:.3g})"
        if rel:
            big = inside & (xd.abs() >= 2.0 ** -100)
            msg += f"; {float(err[big].max()):.3e} |x| inside the clamp"
        print(msg)
        assert float(err[i]) <= E and float(err[i]) >= 0.8 * E, msg
