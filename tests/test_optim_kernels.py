"""Every entry point of the optimizer and arena kernels (dig_amd/csrc/optim.hip: dig_adamw_step / _dev / _groups / _tr, dig_ema_update / _dev,
dig_sumsq, the cast / fill / scale / axpy / pad helpers; dig_amd/csrc/elementwise.hip: dig_add_bf16, dig_gelu_bwd) against float64 torch on the
same fp32 inputs, on both builds of the ABI (`abi_dev`: libdig_hip.so on the MI355X and cpu_abi/libdig_cpu.so).

Reference and bounds (derived, not measured on the kernels)
-----------------------------------------------------------
The reference is torch float64 on the same fp32 inputs, with the hyper-parameters as the fp32 values the ABI receives, widened to float64:
1 - beta is exact in fp32 for 0.9 and 0.999 (1 - b is exact for every fp32 b in [0.5, 1]), the bias corrections are 1 / (1 - b1^t) and
1 / sqrt(1 - b2^t) in double, rounded to fp32 as the library does.  With u = 2^-24 and the per-element scales

    sM = |m| b1 + |g gs| (1 - b1)         sV = v b2 + (g gs)^2 (1 - b2)         sP = |p| + step_size sM / denom

(step_size = lr / (1 - b1^t), denom = sqrt(V64) / sqrt(1 - b2^t) + eps) the bounds are

    |M - M64| <= 4 u sM          |V - V64| <= 6 u sV          |P - P64| <= 16 u sP

worst-case counts of the roundings of `adamw_elem` (each at most u relative to its result, which the scale bounds):
M: g gs, two products, one sum; V: g gs twice, three products, one sum; P: M / denom inherits M (4), the square root of V (3), 1/sqrt(bc2),
+ eps, the division, step_size (its own rounding and the product), the final difference, and on the |p| side decay and p decay; a few ulp
of slack for division and square root are included; FMA contraction only removes roundings.  Where a scale is 0 (g = m = v = 0) the bound is
0: M and V are exactly 0 and P is p decay.  A plain fp32 restatement of the same formula (torch, no library) measures P 3.4 u sP, M 2.5 u sM,
V 3.3 u sV against float64 (steps 1, 3, 1000, 100000, both grad scales, n = 2^20, zeros in g / m / v included): `test_fp32_restatement_is_inside_the_bounds`
holds the restatement to the bounds, so the bounds are not vacuous and the reference is not broken.  A bound that a kernel exceeds is a
finding to investigate, not a number to raise.

A sequence of launches is checked launch by launch: the float64 step starts from the library's own fp32 state before that launch (exact in
float64), since the bounds count the roundings of ONE launch; a free-running float64 recurrence would also carry the earlier launches'
roundings through 1 / sqrt(v), which no per-launch count covers.

    EMA                        |pm' - ref| <= 3 u (|pm| m + |p| (1 - m))           two products, one sum
    sumsq                      |out - S64| <= (t + 16) u S64, t = ceil(n / 2^20)   float4 groups one thread sums; squares, the 3 adds of a group,
                                                                                   6 tree levels, 3 adds, the final rounding; covers the CPU
                                                                                   build's double accumulation
    axpy                       2 u (|y| + |a x|)                                   one product, one sum
    scale_by_device_scalar     3 u |ref|                                           scalar * extra, x * s
    gelu_bwd                   2^-8 |ref| + |dact| E, E = 4e-5                     one bf16 ulp of the result + four times the "~1e-5" that
                                                                                   common.h documented for the derivative
Everything else is bit-exact.

Cases -> the branch or loop trip they exist for
-----------------------------------------------
adamw_kernel / adamw_groups_kernel (`flat_grid`: min(4096, n4 / 256) blocks of 256 float4 lanes; `group[i >> 6]`):
    n = 256                one granule, one block of which 64 lanes work; once per flag 0 / 1 / 2 (grouped: 254 / 0 / 255)
    n = 1280               a partial last block (320 float4); flags 0 1 2 1 0; granule 1 has g = m = v = 0 (0 / (0 + eps): M = V = 0 exactly, P finite),
                           granule 3 has v = 0, g != 0
    n = 4 * 2^20 + 768     three granules past the 4096-block cap: the grid-stride loop's second trip.  Its flags are 0 1 2 (a group boundary
                           and a no-gradient granule), the first trip's flags of the same threads are 1 2 0: a lookup that is not redone per trip
                           updates with the wrong group.  Granules 5 / 6 are the zero cases.
    steps 1, 2, 3          carried forward in place (bias corrections 10 / 5.26 / 3.69 and 31.6 / 22.4 / 18.3); then 1000 and 100000 (bc -> 1)
    grad_scale 1 / 0.37    gs enters M once and V twice
    shadow / None          `if (shadow)`: bf16(p) RNE over the whole range, the no-gradient granules' unchanged values included; p / m / v do not
                           depend on it
    _dev                   `if (dev_scalars)`: six scalars from memory == the host-scalar launch, and again after an in-place overwrite (the
                           captured-graph replay contract)
    _groups                256-entry tables, NaN in every unused slot; 7 groups with distinct (lr, wd), indices 0 1 2 7 64 129 254 and 255 = no
                           gradient; with two groups mapped to (lr0, wd0) / (lr1, wd1) bit-equal to dig_adamw_step (one copy of the arithmetic)
    _tr                    flat granules + a 64 x 64 tile weight of group 0 + one flagged no-gradient (0x80 | 2): p / m / v untouched, shadow and
                           W^T of the unchanged values
    finite_gate            None / 1.0 run; +inf / -inf / NaN leave p, m, v, a poisoned shadow and tr_out as they were, on all four launches
    refusals               n % 256, step 0, null tables, p + 4 bytes: bad argument / misaligned, nothing written
ema_kernel:                n = 4 (one lane), 1028 (partial block), 4 * 2^20 + 20 (second trip of 5 lanes); m = 0.996 and 0.3 (1 - m not exact in
                           fp32 without the double subtraction's single rounding); _dev == host form; shadow exact, None
sumsq_partial / _final:    n = 4, 1024 (one block), 2^20 + 1332 (second trip at the 1024-block cap, 333 lanes); a poisoned workspace (NaN: a
                           partial the final kernel reads but nobody wrote shows); one dominating element; inf as the last element; one NaN;
                           and its output as dig_adamw_step's gate without a host round trip
cast_kernel:               ties to even in both directions, carries into the next binade, +-0, +-inf, the largest finite -> inf, 1e-30 .. 1e30
cast_back_kernel:          all 65536 bit patterns
fill / scale (float4):     n = 4, 1028, 4 * 2^20 + 4 (second trip of one lane)
scale_dev / axpy (scalar): n = 1, 5, 1027, 4 * 2^20 + 3: grids of (n + 3) / 4 / 256 blocks walking n scalars, n % 4 != 0, four and five trips
pad_cast_kernel:           pad rows and pad columns, odd sizes, a single element
add_bf16_kernel:           n = 8, 4104, 8 * 2^20 + 8 (second trip past the 4096-block cap); out-of-place, out is a, out is b
gelu_bwd_kernel:           every finite bf16 pre-activation (subnormals, +-3.4e38: exp(-x^2 / 2) of an overflowed square), dact = 1 and random
Every output buffer has poisoned guard elements behind the range, which must survive.
"""
import ctypes
import math
import struct

import numpy as np
import pytest
import torch

U = 2.0 ** -24
GUARD = 256                       # poisoned elements behind every output range
POISON = 768.0                    # (exact in bf16)
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
cf, cll = ctypes.c_float, ctypes.c_longlong


def f32(x):
    return float(np.float32(x))


B1, B2, EPS = f32(0.9), f32(0.999), f32(1e-8)
LR0, WD0, LR1, WD1 = f32(1e-3), f32(0.1), f32(2.5e-3), f32(0.02)
GS = {"gs1": 1.0, "gs0.37": f32(0.37)}
K_P, K_M, K_V = 16, 4, 6
BIG = 4 * (1 << 20) + 768
SIZES = [256, 1280, BIG]
STEPS = (1, 2, 3, 1000, 100000)


def _backend(dev):
    return "hip" if dev.type == "cuda" else "cpu_abi"


def _sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize()


def _bias(step):
    """(1 / (1 - b1^t), 1 / sqrt(1 - b2^t)) in double, rounded to fp32: dig_adamw_bias_corrections' arithmetic."""
    return f32(1.0 / (1.0 - B1 ** step)), f32(1.0 / math.sqrt(1.0 - B2 ** step))


def _ref_step(p, g, m, v, lr, wd, upd, step, gs):
    """One float64 AdamW step on fp32 state.  lr, wd: float64 per element; upd: which elements receive a gradient.  Returns (P, M, V) and the
    bounds' scales (sP, sM, sV), all float64; where `upd` is false the values are the inputs' and the scales 0."""
    c1, c2 = _bias(step)
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    gk = g * gs
    M = m * B1 + gk * (1.0 - B1)
    V = v * B2 + gk * gk * (1.0 - B2)
    sM = m.abs() * B1 + gk.abs() * (1.0 - B1)
    denom = V.sqrt() * c2 + EPS
    ss = lr * c1
    P = p * (1.0 - lr * wd) - ss * (M / denom)
    sP = p.abs() + ss * sM / denom
    zero = torch.zeros((), dtype=F64)
    return ((torch.where(upd, P, p), torch.where(upd, M, m), torch.where(upd, V, v)),
            (torch.where(upd, sP, zero), torch.where(upd, sM, zero), torch.where(upd, V, zero)))


def _check_bounds(tag, got, ref, scales):
    """Prints the largest error of P, M, V in units of u * scale, then asserts the per-element bounds (exact where the scale is 0)."""
    worst, ok = {}, {}
    for name, k, x, r, s in zip("PMV", (K_P, K_M, K_V), got, ref, scales):
        x = x.detach().cpu().double()
        assert bool(torch.isfinite(x).all()), (tag, name, "non-finite")
        err = (x - r).abs()
        worst[name] = float((err / (U * s).clamp_min(1e-300)).max())          # (inf-like where a zero scale meets any error)
        ok[name] = bool((err <= k * U * s).all())
    print(f"adamw {tag} P {worst['P']:.2f} u sP  M {worst['M']:.2f} u sM  V {worst['V']:.2f} u sV")
    for name, k in zip("PMV", (K_P, K_M, K_V)):
        assert ok[name], (tag, name, worst[name], k)
    return worst


# ------------------------------------------------------------------------------------------------ layouts and inputs (computed once, never modified)
def _layout(n, variant=0):
    """(flags [n / 256] of dig_adamw_step, [(start, end, kind)] zero ranges: kind 'all' -> g = m = v = 0, 'v' -> v = 0)."""
    G = n // 256
    if n == 256:
        return np.array([variant], np.uint8), [(0, 64, "all"), (64, 128, "v")]
    if n == 1280:
        return np.array([0, 1, 2, 1, 0], np.uint8), [(256, 512, "all"), (768, 1024, "v")]
    rng = np.random.RandomState(G)
    fl = rng.randint(0, 2, G).astype(np.uint8)
    fl[10::11] = 2
    fl[:3] = (1, 2, 0)                                  # the first trip of the threads whose second trip is ...
    fl[5], fl[6] = 0, 1
    fl[-3:] = (0, 1, 2)                                 # ... a group boundary and a no-gradient granule
    return fl, [(5 * 256, 6 * 256, "all"), (6 * 256, 7 * 256, "v")]


_INPUTS = {}


def _inputs(n, variant=0):
    key = (n, variant)
    if key not in _INPUTS:
        flags, zeros = _layout(n, variant)
        g = torch.Generator().manual_seed(n + variant)
        p, gr = torch.randn(n, generator=g), torch.randn(n, generator=g) * 1e-2
        m, v = torch.randn(n, generator=g) * 1e-3, torch.rand(n, generator=g) * 1e-5
        for a, b, kind in zeros:
            v[a:b] = 0
            if kind == "all":
                gr[a:b] = 0
                m[a:b] = 0
        _INPUTS[key] = (flags, p, gr, m, v)
    return _INPUTS[key]


G7 = (0, 1, 2, 7, 64, 129, 254)                        # group indices of the 7-group table (254: the highest legal one)
GA, GB = 3, 254                                         # the two groups that stand for flags 0 / 1 in the mapped table


def _tables(kind):
    """(lr_tab, wd_tab) fp32 [256], NaN in every slot no granule may use."""
    lr, wd = torch.full((256,), math.nan), torch.full((256,), math.nan)
    if kind == "groups7":
        for k, gi in enumerate(G7):
            lr[gi], wd[gi] = 1e-3 * 0.75 ** k, 0.05 + 0.01 * k
    else:
        lr[GA], wd[GA], lr[GB], wd[GB] = LR0, WD0, LR1, WD1
    return lr, wd


def _group_idx(kind, flags):
    """Granule indices of the grouped launch: the flags mapped (0 -> GA, 1 -> GB, 2 -> 255), or 7 groups and 255 scattered."""
    if kind != "groups7":
        return np.array([GA, GB, 255], np.uint8)[flags]
    G = len(flags)
    pool = np.array(G7 + (255,), np.uint8)
    if G == 1:
        return pool[[(6, 0, 7)[int(flags[0])]]]
    if G == 5:
        return np.array([254, 0, 255, 129, 7], np.uint8)
    idx = pool[np.random.RandomState(G + 1).randint(0, 8, G)]
    idx[:3] = (255, 0, 254)
    idx[5], idx[6] = 2, 64
    idx[-3:] = (254, 7, 255)
    return idx


class _Arena:
    """p / g / m / v (+ a poisoned bf16 shadow) on the device with GUARD poisoned elements behind each, the flags or the group table of `kind`,
    and the float64 per-element (lr, wd, upd) the reference uses."""

    def __init__(self, dev, kind, n, variant=0):
        flags, p, g, m, v = _inputs(n, variant)
        self.dev, self.kind, self.n = dev, kind, n
        pad = lambda t: torch.cat([t, torch.full((GUARD,), POISON)]).to(dev)
        self.p, self.g, self.m, self.v = pad(p), pad(g), pad(m), pad(v)
        self.shadow = torch.full((n + GUARD,), POISON, dtype=BF, device=dev)
        self.flags = torch.from_numpy(flags).to(dev)
        self.flags_np = flags
        if kind.startswith("groups"):
            idx = _group_idx(kind, flags)
            lr, wd = _tables(kind)
            self.idx, self.lr_tab, self.wd_tab = torch.from_numpy(idx).to(dev), lr.to(dev), wd.to(dev)
            safe = torch.from_numpy(np.where(idx == 255, G7[0] if kind == "groups7" else GA, idx).astype(np.int64))
            self.lr64 = lr.double()[safe].repeat_interleave(256)
            self.wd64 = wd.double()[safe].repeat_interleave(256)
            self.upd = torch.from_numpy(idx != 255).repeat_interleave(256)
        else:
            fl = torch.from_numpy(flags.astype(np.int64))
            self.lr64 = torch.tensor([LR0, LR1, LR1], dtype=F64)[fl].repeat_interleave(256)
            self.wd64 = torch.tensor([WD0, WD1, WD1], dtype=F64)[fl].repeat_interleave(256)
            self.upd = (fl != 2).repeat_interleave(256)
        self.s6 = None

    def state(self):
        n = self.n
        return tuple(t[:n].to("cpu", copy=True) for t in (self.p, self.m, self.v))

    def guards_intact(self, shadow=True):
        n = self.n
        ok = all(bool((t[n:] == POISON).all()) for t in (self.p, self.g, self.m, self.v))
        return ok and (not shadow or bool((self.shadow[n:].float() == POISON).all()))

    def launch(self, step, gs, shadow=True, gate=None, lrs=None):
        from dig_amd import _lib as L, ops
        n = self.n
        lr0, wd0, lr1, wd1 = lrs or (LR0, WD0, LR1, WD1)
        sh = L.ptr(self.shadow) if shadow else None
        head = (L.ptr(self.p), L.ptr(self.g), L.ptr(self.m), L.ptr(self.v), sh, cll(n))
        if self.kind == "plain":
            L.call("dig_adamw_step", *head, L.ptr(self.flags), cf(lr0), cf(wd0), cf(lr1), cf(wd1), cf(B1), cf(B2), cf(EPS), int(step), cf(gs),
                   L.ptr(gate), L.stream())
        elif self.kind == "dev":
            six = torch.tensor([lr0, wd0, lr1, wd1, *ops.adamw_bias_corrections(B1, B2, step)], dtype=F32)
            if self.s6 is None:
                self.s6 = six.to(self.dev)
            else:
                self.s6.copy_(six)                      # in place: the address a captured launch would keep reading
            L.call("dig_adamw_step_dev", *head, L.ptr(self.flags), L.ptr(self.s6), cf(B1), cf(B2), cf(EPS), cf(gs), L.ptr(gate), L.stream())
        else:
            L.call("dig_adamw_step_groups", *head, L.ptr(self.idx), L.ptr(self.lr_tab), L.ptr(self.wd_tab), cf(B1), cf(B2), cf(EPS), int(step),
                   cf(gs), L.ptr(gate), L.stream())


# ------------------------------------------------------------------------------------------------ 1. the bounds themselves
def test_fp32_restatement_is_inside_the_bounds():
    """The same formula in plain fp32 torch (no library) against the float64 reference: inside the bounds, and within a factor 32 of them (the
    bounds are neither broken nor vacuous).  Its figures are the docstring's."""
    n = 1 << 20
    g = torch.Generator().manual_seed(11)
    p, gr = torch.randn(n, generator=g), torch.randn(n, generator=g) * 1e-2
    m, v = torch.randn(n, generator=g) * 1e-3, torch.rand(n, generator=g) * 1e-5
    v[:4096] = 0
    gr[:2048] = 0
    m[:2048] = 0
    lr = torch.full((n,), LR0, dtype=F64)
    lr[n // 2:] = LR1
    wd = torch.full((n,), WD0, dtype=F64)
    wd[n // 2:] = WD1
    upd = torch.ones(n, dtype=torch.bool)
    one = np.float32(1)
    top = {"P": 0.0, "M": 0.0, "V": 0.0}
    for step in (1, 3, 1000, 100000):
        for gs in GS.values():
            c1, c2 = _bias(step)
            gk = gr * gs
            M = m * B1 + gk * float(one - np.float32(B1))
            V = v * B2 + gk * gk * float(one - np.float32(B2))
            denom = V.sqrt() * c2 + EPS
            P = torch.empty(n)
            for sl, l, w in ((slice(0, n // 2), LR0, WD0), (slice(n // 2, n), LR1, WD1)):
                decay, ss = float(one - np.float32(l) * np.float32(w)), float(np.float32(l) * np.float32(c1))
                P[sl] = p[sl] * decay - ss * (M[sl] / denom[sl])
            ref, scales = _ref_step(p, gr, m, v, lr, wd, upd, step, gs)
            w = _check_bounds(f"fp32-torch step {step} gs {gs:.2f}", (P, M, V), ref, scales)
            for k in top:
                top[k] = max(top[k], w[k])
            assert bool((M[:2048] == 0).all()) and bool((V[:2048] == 0).all())
    for k, bound in zip("PMV", (K_P, K_M, K_V)):
        assert bound / 32 <= top[k] <= bound, (k, top[k])


# ------------------------------------------------------------------------------------------------ 2. AdamW against float64
def _variants(n):
    return (0, 1, 2) if n == 256 else (0,)


@pytest.mark.parametrize("gs", list(GS), ids=list(GS))
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["plain", "dev", "groups2", "groups7"])
def test_adamw_vs_fp64(abi_dev, kind, n, gs):
    """Steps 1, 2, 3, 1000, 100000 in place on one arena with a shadow and, in lockstep, on a second one without: every launch within the bounds
    of the float64 step from the state before it, M = V = 0 exactly where g = m = v = 0, the shadow == bf16(p) over the whole range, p / m / v
    independent of the shadow, guards intact."""
    dev, gsv = abi_dev, GS[gs]
    for variant in _variants(n):
        a, b = _Arena(dev, kind, n, variant), _Arena(dev, kind, n, variant)
        before = a.state()
        for step in STEPS:
            a.launch(step, gsv, shadow=True)
            b.launch(step, gsv, shadow=False)
            after = a.state()
            ref, scales = _ref_step(*before[:1], a.g[:n].cpu(), *before[1:], a.lr64, a.wd64, a.upd, step, gsv)
            _check_bounds(f"{_backend(dev)} {kind} n {n} v{variant} step {step} {gs}", after, ref, scales)
            frozen = ~a.upd
            for x, y in zip(after, before):
                assert torch.equal(x[frozen], y[frozen])                 # a granule without a gradient: untouched
            assert torch.equal(a.shadow[:n].cpu(), after[0].bfloat16())
            for x, y in zip(after, b.state()):
                assert torch.equal(x, y)
            assert a.guards_intact() and b.guards_intact() and bool((b.shadow.float() == POISON).all())
            before = after


@pytest.mark.parametrize("n", SIZES)
def test_adamw_entry_points_bit_equal(abi_dev, n):
    """dig_adamw_step_dev with scalars built from ops.adamw_bias_corrections, and dig_adamw_step_groups with two table entries standing for the
    flags, give dig_adamw_step's p / m / v / shadow bit for bit; so does a second launch after the six device scalars were overwritten in place
    with the next step's (another lr and wd): the captured-graph replay contract."""
    dev, gs = abi_dev, GS["gs0.37"]
    nxt = (f32(0.9e-3), f32(0.11), f32(2.2e-3), f32(0.03))
    for variant in _variants(n):
        arenas = {k: _Arena(dev, k, n, variant) for k in ("plain", "dev", "groups2")}
        for step, lrs in ((3, None), (4, nxt)):
            for k, a in arenas.items():
                if k == "groups2" and lrs:
                    a.lr_tab[GA], a.wd_tab[GA], a.lr_tab[GB], a.wd_tab[GB] = lrs
                a.launch(step, gs, lrs=lrs)
            if lrs is None:
                s6_ptr = arenas["dev"].s6.data_ptr()
            want = arenas["plain"]
            for k in ("dev", "groups2"):
                for x, y in zip(arenas[k].state(), want.state()):
                    assert torch.equal(x, y), (k, step)
                assert torch.equal(arenas[k].shadow, want.shadow), (k, step)
        assert arenas["dev"].s6.data_ptr() == s6_ptr
        assert variant == 2 or not torch.equal(want.p[:n].cpu(), _inputs(n, variant)[1])


# ------------------------------------------------------------------------------------------------ 3. the gate, and the refusals, on all four launches
TR_N = 256 + 2 * 4096 + 256       # a flat granule, two listed 64 x 64 weights, a flat granule


class _Small:
    """One launch of each kind at a small size, called through the ABI with any argument replaceable (None -> NULL)."""

    def __init__(self, dev, kind):
        from dig_amd import _lib as L
        self.dev, self.kind = dev, kind
        n = self.n = TR_N if kind == "tr" else 1280
        g = torch.Generator().manual_seed(31)
        mk = lambda t: torch.cat([t, torch.full((GUARD,), POISON)]).to(dev)
        self.p, self.g = mk(torch.randn(n, generator=g)), mk(torch.randn(n, generator=g) * 1e-2)
        self.m, self.v = mk(torch.randn(n, generator=g) * 1e-3), mk(torch.rand(n, generator=g) * 1e-5)
        self.shadow = torch.full((n + GUARD,), POISON, dtype=BF, device=dev)
        if kind == "tr":
            fl = np.array([1] + [0x80] * 16 + [0x80 | 2] * 16 + [0], np.uint8)
            recs = [struct.pack("<qqiiii", 256, 0, 64, 64, 0, 0), struct.pack("<qqiiii", 256 + 4096, 4096, 64, 64, 1, 0)]
            self.mats = torch.frombuffer(bytearray(b"".join(recs)), dtype=torch.uint8).to(dev)
            self.tr_out = torch.full((2 * 4096 + GUARD,), POISON, dtype=BF, device=dev)
        else:
            fl = np.array([0, 1, 2, 1, 0], np.uint8)
        self.flags_np = fl
        self.flags = torch.from_numpy(fl).to(dev)
        lr, wd = _tables("groups2")
        self.idx = torch.from_numpy(fl if kind == "tr" else np.array([GA, GB, 255], np.uint8)[fl]).to(dev)     # (the grouped launch's granule indices)
        self.lr_tab, self.wd_tab = lr.to(dev), wd.to(dev)
        self.s6 = None
        self.L = L

    def buffers(self):
        out = [self.p, self.g, self.m, self.v, self.shadow]
        return out + [self.tr_out] if self.kind == "tr" else out

    def snapshot(self):
        return [t.clone() for t in self.buffers()]

    def call(self, step=3, gate=None, **over):
        """over: p / flags / tab (lr_tab) / wd_tab / s6 / mats / tr_out -> a replacement pointer (None = NULL); n -> another element count."""
        from dig_amd import ops
        L = self.L
        if self.kind == "dev" and self.s6 is None:
            self.s6 = torch.tensor([LR0, WD0, LR1, WD1, *ops.adamw_bias_corrections(B1, B2, step)], dtype=F32).to(self.dev)
        arg = lambda name, t: over[name] if name in over else L.ptr(t)
        n = over.get("n", self.n)
        head = (arg("p", self.p), L.ptr(self.g), L.ptr(self.m), L.ptr(self.v), L.ptr(self.shadow), cll(n))
        hyp = (cf(LR0), cf(WD0), cf(LR1), cf(WD1), cf(B1), cf(B2), cf(EPS), int(step), cf(0.5), L.ptr(gate))
        if self.kind == "plain":
            L.call("dig_adamw_step", *head, arg("flags", self.flags), *hyp, L.stream())
        elif self.kind == "tr":
            L.call("dig_adamw_step_tr", *head, arg("flags", self.flags), *hyp, arg("mats", self.mats), 2, 2, arg("tr_out", self.tr_out), L.stream())
        elif self.kind == "dev":
            L.call("dig_adamw_step_dev", *head, arg("flags", self.flags), arg("s6", self.s6), cf(B1), cf(B2), cf(EPS), cf(0.5), L.ptr(gate), L.stream())
        else:
            L.call("dig_adamw_step_groups", *head, arg("flags", self.idx), arg("tab", self.lr_tab), arg("wd_tab", self.wd_tab), cf(B1), cf(B2),
                   cf(EPS), int(step), cf(0.5), L.ptr(gate), L.stream())
        _sync(self.dev)


KINDS4 = ["plain", "dev", "groups", "tr"]


@pytest.mark.parametrize("kind", KINDS4)
def test_adamw_finite_gate(abi_dev, kind):
    """finite_gate None and 1.0: the step runs, with the same result; +inf, -inf, NaN: p, m, v, the poisoned shadow (and tr_out) keep their
    bits.  The `_tr` launch that runs: the flat launch's p / m / v / shadow, the flagged no-gradient weight untouched, W^T == shadow^T."""
    dev = abi_dev
    ran = {}
    for gv in (None, 1.0):
        s = _Small(dev, kind)
        before = s.snapshot()
        s.call(gate=None if gv is None else torch.tensor([gv], device=dev))
        n = s.n
        assert not torch.equal(s.p[:256], before[0][:256]) and not torch.equal(s.m[:n], before[2][:n]) and not torch.equal(s.v[:n], before[3][:n])
        assert torch.equal(s.shadow[:n], s.p[:n].bfloat16()) and torch.equal(s.g, before[1])
        assert all(bool((t[n:].float() == POISON).all()) for t in (s.p, s.m, s.v, s.shadow))
        ran[gv] = s
    for x, y in zip(ran[None].buffers(), ran[1.0].buffers()):
        assert torch.equal(x, y)
    if kind == "tr":
        s = ran[None]
        fresh = _Small(dev, "tr")
        flat = _Small(dev, "tr")                                               # the same arena through the flat launch, bit 7 cleared
        flat.kind, flat.flags = "plain", torch.from_numpy(s.flags_np & 0x7f).to(dev)
        flat.call()
        for x, y in zip(flat.buffers(), s.buffers()[:5]):
            assert torch.equal(x, y)
        lo, hi = 256 + 4096, 256 + 8192                                        # the flagged no-gradient weight
        for x, y in zip((s.p, s.m, s.v), (fresh.p, fresh.m, fresh.v)):
            assert torch.equal(x[lo:hi], y[lo:hi])
        assert not torch.equal(s.p[256:lo], fresh.p[256:lo])
        for k, o in enumerate((256, lo)):
            assert torch.equal(s.tr_out[k * 4096:(k + 1) * 4096].view(64, 64), s.shadow[o:o + 4096].view(64, 64).t())
        assert bool((s.tr_out[8192:].float() == POISON).all())
    for gv in (math.inf, -math.inf, math.nan):
        s = _Small(dev, kind)
        before = s.snapshot()
        s.call(gate=torch.tensor([gv], device=dev))
        for x, y in zip(s.buffers(), before):
            assert torch.equal(x, y), (kind, gv)


@pytest.mark.parametrize("kind", KINDS4)
def test_adamw_refusals(abi_dev, kind):
    """n that is no multiple of 256, step 0, a null table, p offset by one element: the `_lib` error of the argument / alignment code, and
    no buffer is written."""
    from dig_amd import _lib as L
    dev = abi_dev
    s = _Small(dev, kind)
    before = s.snapshot()
    bad = [({"n": s.n - 4}, "bad argument"), ({"n": s.n + 100}, "bad argument"), ({"flags": None}, "bad argument"),
           ({"p": ctypes.c_void_p(s.p.data_ptr() + 4)}, "misaligned")]
    if kind != "dev":
        bad.append(({"step": 0}, "bad argument"))
    bad += {"dev": [({"s6": None}, "bad argument")], "groups": [({"tab": None}, "bad argument"), ({"wd_tab": None}, "bad argument")],
            "tr": [({"mats": None}, "bad argument"), ({"tr_out": None}, "bad argument")], "plain": []}[kind]
    for kw, match in bad:
        with pytest.raises(L.DigHipError, match=match):
            s.call(**kw)
        _sync(dev)
        for x, y in zip(s.buffers(), before):
            assert torch.equal(x, y), (kind, kw)
    s.call()                                                                    # and the unmodified arguments are accepted
    assert not torch.equal(s.p, before[0])


# ------------------------------------------------------------------------------------------------ 4. EMA
@pytest.mark.parametrize("n", [4, 1028, 4 * (1 << 20) + 20])
def test_ema_vs_fp64(abi_dev, n):
    """dig_ema_update and _dev ([m, float32(1 - double(m))] on the device) against float64; bit-equal to each other; the shadow == bf16(pm'),
    and pm' does not depend on it."""
    from dig_amd import ops
    dev = abi_dev
    g = torch.Generator().manual_seed(n)
    pm0, p = torch.randn(n, generator=g), torch.randn(n, generator=g) * 3
    pd = p.to(dev)
    mk = lambda: torch.cat([pm0, torch.full((GUARD,), POISON)]).to(dev)
    for m in (f32(0.996), f32(0.3)):
        om = f32(1.0 - m)
        ref = pm0.double() * m + p.double() * om
        scale = pm0.double().abs() * m + p.double().abs() * om
        a, b, c = mk(), mk(), mk()
        sa, sc = (torch.full((n + GUARD,), POISON, dtype=BF, device=dev) for _ in range(2))
        ops.ema_update(a, pd, sa, n, m)
        ops.ema_update(b, pd, None, n, m)
        ops.ema_update(c, pd, sc, n, torch.tensor([m, om], dtype=F32).to(dev))
        err = (a[:n].cpu().double() - ref).abs()
        print(f"ema {_backend(dev)} n {n} m {m:.3f}: {float((err / (U * scale)).max()):.2f} u scale")
        assert bool((err <= 3 * U * scale).all())
        assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(sa, sc)
        assert torch.equal(sa[:n], a[:n].bfloat16())
        assert bool((a[n:] == POISON).all()) and bool((sa[n:].float() == POISON).all())


# ------------------------------------------------------------------------------------------------ 5. sum of squares, and the gate it feeds
def _sumsq(dev, x):
    from dig_amd import ops
    ws = torch.full((1024 + GUARD,), math.nan, device=dev)
    out = torch.full((1 + GUARD,), POISON, device=dev)
    ops.sumsq(x, ws, out)
    assert bool(torch.isnan(ws[1024:]).all()) and bool((out[1:] == POISON).all())
    return out


@pytest.mark.parametrize("n", [4, 1024, (1 << 20) + 1332])
def test_sumsq_vs_fp64(abi_dev, n):
    """dig_sumsq with a poisoned workspace: random values; one element that dominates the sum; inf as the last element; one NaN."""
    dev = abi_dev
    g = torch.Generator().manual_seed(n)
    t = -(-n // (1 << 20))
    x = torch.randn(n, generator=g) * 1e-2
    big = torch.randn(n, generator=g) * 1e-3
    big[n // 2] = 1e3
    for tag, h in (("random", x), ("dominated", big)):
        S = float((h.double() ** 2).sum())
        got = float(_sumsq(dev, h.to(dev))[0])
        print(f"sumsq {_backend(dev)} n {n} {tag}: {abs(got - S) / (U * S):.2f} u S (bound {t + 16})")
        assert abs(got - S) <= (t + 16) * U * S
    xi = x.clone()
    xi[-1] = math.inf
    assert float(_sumsq(dev, xi.to(dev))[0]) == math.inf
    xn = x.clone()
    xn[n // 3] = math.nan
    assert math.isnan(float(_sumsq(dev, xn.to(dev))[0]))


def test_sumsq_output_gates_adamw(abi_dev):
    """A gradient with one inf in dig_sumsq's second trip -> its output, still on the device, as dig_adamw_step's finite_gate: nothing changes;
    with the finite gradient's norm the step runs."""
    dev = abi_dev
    n = (1 << 20) + 1536
    g = torch.Generator().manual_seed(3)
    p, gr = torch.randn(n, generator=g), torch.randn(n, generator=g) * 1e-2
    flags = torch.zeros(n // 256, dtype=torch.uint8, device=dev)
    from dig_amd import ops
    for poison_grad in (True, False):
        gh = gr.clone()
        if poison_grad:
            gh[n - 2] = math.inf
        pd, gd, m, v = p.clone().to(dev), gh.to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        sh = torch.full((n,), POISON, dtype=BF, device=dev)
        out = _sumsq(dev, gd)
        ops.adamw_step(pd, gd, m, v, sh, flags, LR0, WD0, LR1, WD1, B1, B2, EPS, 1, 1.0, out[:1])
        if poison_grad:
            assert torch.equal(pd.cpu(), p) and not bool(m.any()) and not bool(v.any()) and bool((sh.float() == POISON).all())
        else:
            assert not torch.equal(pd.cpu(), p) and bool(m.any()) and torch.equal(sh, pd.bfloat16())


# ------------------------------------------------------------------------------------------------ 6. casts
def _cast_inputs():
    g = torch.Generator().manual_seed(17)
    base = torch.randn(4096, generator=g)
    rng = np.random.RandomState(17)
    k = 4096
    sign, exp, man7 = (rng.randint(0, 2, k).astype(np.uint32) << 31), rng.randint(1, 254, k).astype(np.uint32) << 23, rng.randint(0, 128, k).astype(np.uint32) << 16
    man7[:128] = np.arange(128, dtype=np.uint32) << 16                         # every kept mantissa, even and odd
    hi = sign | exp | man7
    parts = [hi | 0x8000,                                                      # exact ties: down to an even, up to an even mantissa
             hi | 0x7fff, hi | 0x8001,                                         # either side of a tie
             sign | exp | 0x7fffff, sign | exp | 0x7f8000, sign | exp | 0x7f7fff,   # all-ones mantissa: up into the next binade (the tie too); just below
             hi]                                                               # already bf16
    special = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7f7fffff, 0xff7fffff, 0x7f7f8000, 0x7f7f7fff,
                        0x00800000, 0x80800000, 0x00ffffff, 0x3f7fffff], np.uint32)    # +-0, +-inf, largest finite -> inf, smallest normals
    bits = np.concatenate(parts + [special])
    x = torch.cat([base * 1e-30, base, base * 1e30, torch.from_numpy(bits.view(np.float32).copy())])
    assert x.numel() % 4 == 0 and not bool(torch.isnan(x).any())
    assert bool((x.abs()[x != 0] >= 2.0 ** -126).all())                        # normal range only
    return x


def test_cast_f32_to_bf16_exact(abi_dev):
    from dig_amd import ops
    dev = abi_dev
    x = _cast_inputs()
    n = x.numel()
    want = x.bfloat16()
    assert bool(torch.isinf(want[x == torch.finfo(F32).max]).all())
    y = torch.full((n + GUARD,), POISON, dtype=BF, device=dev)
    ops.cast_f32_to_bf16(x.to(dev), y, n)
    assert torch.equal(y[:n].cpu().view(torch.int16), want.view(torch.int16))
    assert bool((y[n:].float() == POISON).all())


def test_cast_bf16_to_f32_all_patterns(abi_dev):
    from dig_amd import ops
    dev = abi_dev
    bits = np.arange(65536, dtype=np.uint32)
    x = torch.from_numpy(bits.astype(np.uint16).view(np.int16).copy()).view(BF).to(dev)
    y = torch.full((65536 + GUARD,), POISON, device=dev)
    ops.cast_bf16_to_f32(x, y, 65536)
    assert torch.equal(y[:65536].cpu().view(torch.int32), torch.from_numpy((bits << 16).view(np.int32).copy()))
    assert bool((y[65536:] == POISON).all())


# ------------------------------------------------------------------------------------------------ 7. element-wise helpers
@pytest.mark.parametrize("n", [4, 1028, 4 * (1 << 20) + 4])
def test_fill_and_scale_exact(abi_dev, n):
    from dig_amd import ops
    dev = abi_dev
    x = torch.randn(n, generator=torch.Generator().manual_seed(n))
    buf = torch.cat([x, torch.full((GUARD,), POISON)]).to(dev)
    ops.scale_f32(buf[:n], f32(0.37))
    assert torch.equal(buf[:n].cpu(), x * f32(0.37)) and bool((buf[n:] == POISON).all())
    ops.fill_f32(buf[:n], -1.25)
    assert bool((buf[:n] == -1.25).all()) and bool((buf[n:] == POISON).all())


@pytest.mark.parametrize("n", [1, 5, 1027, 4 * (1 << 20) + 3])
def test_scale_by_device_scalar_and_axpy_vs_fp64(abi_dev, n):
    from dig_amd import ops
    dev = abi_dev
    g = torch.Generator().manual_seed(n)
    x, y = torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.1
    sc = f32(1.7)
    scalar = torch.tensor([sc, POISON], dtype=F32).to(dev)
    for extra in (1.0, f32(0.3)):
        buf = torch.cat([x, torch.full((GUARD,), POISON)]).to(dev)
        ops.scale_by_device_scalar(buf[:n], scalar, extra)
        ref = x.double() * sc * extra
        err = (buf[:n].cpu().double() - ref).abs()
        print(f"scale_dev {_backend(dev)} n {n} extra {extra:.1f}: {float((err / (U * ref.abs())).max()):.2f} u |ref|")
        assert bool((err <= 3 * U * ref.abs()).all()) and bool((buf[n:] == POISON).all())
    a = f32(-0.37)
    buf = torch.cat([y, torch.full((GUARD,), POISON)]).to(dev)
    ops.axpy_f32(buf[:n], x.to(dev), a)
    ref, scale = y.double() + a * x.double(), y.double().abs() + (a * x.double()).abs()
    err = (buf[:n].cpu().double() - ref).abs()
    print(f"axpy {_backend(dev)} n {n}: {float((err / (U * scale)).max()):.2f} u scale")
    assert bool((err <= 2 * U * scale).all()) and bool((buf[n:] == POISON).all())


@pytest.mark.parametrize("M,C,M_pad,ld", [(333, 48, 384, 64), (5, 7, 8, 24), (1, 1, 1, 1)])
def test_pad_cast_rows_exact(abi_dev, M, C, M_pad, ld):
    from dig_amd import _lib as L
    dev = abi_dev
    src = torch.randn(M, C, generator=torch.Generator().manual_seed(M + C))
    dst = torch.full((M_pad * ld + GUARD,), POISON, dtype=BF, device=dev)
    srcd = src.to(dev)
    L.call("dig_pad_cast_rows", L.ptr(srcd), L.ptr(dst), M, C, M_pad, ld, L.stream())
    want = torch.zeros(M_pad, ld, dtype=BF)
    want[:M, :C] = src.bfloat16()
    got = dst[:M_pad * ld].cpu().view(M_pad, ld)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))          # (bit for bit: the padding is +0)
    assert bool((dst[M_pad * ld:].float() == POISON).all())


@pytest.mark.parametrize("n", [8, 4104, 8 * (1 << 20) + 8])
def test_add_bf16_exact_and_in_place(abi_dev, n):
    """Bit-equal to bf16(float(a) + float(b)); `out is a` and `out is b` (the fine-tune gradient adds) give the same bits."""
    from dig_amd import ops
    dev = abi_dev
    g = torch.Generator().manual_seed(n)
    a = (torch.randn(n, generator=g) * 100).bfloat16()
    b = torch.randn(n, generator=g).bfloat16()
    want = (a.float() + b.float()).bfloat16()
    guard = torch.full((GUARD,), POISON, dtype=BF)
    ad, bd = torch.cat([a, guard]).to(dev), torch.cat([b, guard]).to(dev)
    out = torch.full((n + GUARD,), POISON, dtype=BF, device=dev)
    ops.add_bf16(ad[:n], bd[:n], out[:n])
    assert torch.equal(out[:n].cpu(), want) and bool((out[n:].float() == POISON).all())
    a2, b2 = ad.clone(), bd.clone()
    ops.add_bf16(a2[:n], bd[:n], a2[:n])
    ops.add_bf16(ad[:n], b2[:n], b2[:n])
    assert torch.equal(a2, out) and torch.equal(b2, out)
    assert torch.equal(ad[:n].cpu(), a) and torch.equal(bd[:n].cpu(), b)


def test_gelu_bwd_every_finite_bf16(abi_dev):
    """dpre = dact * gelu'(pre) at every finite bf16 pre-activation, dact = 1 and random, against Phi(x) + x phi(x) in float64."""
    from dig_amd import ops
    dev = abi_dev
    E = 4e-5
    bits = np.arange(65536, dtype=np.uint32)
    bits = bits[((bits >> 7) & 0xff) != 0xff]
    n = bits.size
    assert n == 65280 and n % 8 == 0
    pre = torch.from_numpy(bits.astype(np.uint16).view(np.int16).copy()).view(BF)
    x = pre.double()
    gp = 0.5 * (1 + torch.erf(x / math.sqrt(2))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)
    assert bool(torch.isfinite(gp).all())
    pred = pre.to(dev)
    for tag, dact in (("ones", torch.ones(n).bfloat16()), ("random", torch.randn(n, generator=torch.Generator().manual_seed(1)).bfloat16())):
        out = torch.full((n + GUARD,), POISON, dtype=BF, device=dev)
        ops.gelu_bwd(dact.to(dev), pred, out[:n])
        got = out[:n].cpu().double()
        ref = dact.double() * gp
        assert bool(torch.isfinite(got).all())
        excess = (got - ref).abs() - 2.0 ** -8 * ref.abs()
        i = int(excess.argmax())
        print(f"gelu_bwd {_backend(dev)} {tag}: largest |err| - 2^-8 |ref| = {float(excess[i]):.3e} at x = {float(x[i]):.4g} (E = {E:.0e})")
        assert bool((excess <= dact.double().abs() * E).all())
        assert bool((out[n:].float() == POISON).all())
