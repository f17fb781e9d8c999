"""Every entry point of the kernels that compute statistics -- dig_amd/csrc/norm.hip (LayerNorm, BatchNorm), dig_amd/csrc/loss.hip (L2 normalise, the
fp32 GEMM, the InfoNCE row kernel) and the MSE and column-sum kernels of dig_amd/csrc/elementwise.hip -- against float64 torch on the same bf16 /
fp32 inputs, on both builds of the ABI (`abi_dev`: libdig_hip.so on the MI355X and cpu_abi/libdig_cpu.so).

Reference and bounds (derived, not measured on the kernels)
-----------------------------------------------------------
The reference is torch float64 on the same inputs; eps, momentum, gscale, alpha are the fp32 values the ABI receives, widened.  Every reduction is
checked twice.

1. Exact arithmetic.  Integers in [-8, 8] or multiples of 1/4 in [-8, 8]: every product and every partial sum is a small dyadic number that fp32
   holds exactly, in ANY summation order, so the library's sums must equal the float64 sums bit for bit on both builds: BatchNorm sums[2, C], the
   backward sums, dbeta / dgamma (mean an integer, rstd a power of two: they are inputs of the backward); the LayerNorm mean at D = 64 / 128 /
   256 / 512 (1 / D exact) and the fused BatchNorm mean at rows 2 / 64 / 4096; dgamma / dbeta / dcolsum of the LayerNorm backward; every
   column-sum entry point; out3[1] / out3[2] of dig_ce_rows; dig_sgemm with integer operands.  The largest sum is 32 769 rows x 160 < 2^24.

2. Random and adversarial data, bounds from counting roundings: u = 2^-24 per fp32 operation (FMA contraction only removes roundings), 2^-8 |ref|
   for a bf16 result.  `a` is the number of additions an element passes through in a sum, which depends on the build's documented order:

       LayerNorm row sums   hip: D / 64 - 1 in the lane + 6 shuffle levels        cpu: D - 1 (one chain)
       LayerNorm columns    hip: 2 ceil(rows / (8 parts)) in the wave + 3 waves + ceil(parts / 64) + 6 tree levels + 1 (the += )
                            cpu: ceil(rows / parts) + parts + 1                   parts = min(1024, ceil(rows / 16))
       BatchNorm columns    hip: rows_per_block + 1 (the strip, rows in flight folded in order) + ceil(strips / 32) + 32 (finalize)
                            cpu: rows (one chain)        one-launch path, both builds: ceil(rows / 64) + 64
       l2norm rows          hip: ceil(C / 64) - 1 + 6    cpu: C - 1
       ce_rows              hip: ceil(m / 256) - 1 + 6 + 3                        cpu: m - 1
       mse (both)           ceil(M ld / 65536) + 6 + 3 + 2 + min(256, ceil(M ld / 256))   (the cpu build accumulates in double)

   LayerNorm forward (i = 1 where 1 / D is inexact, D = 192 / 384):
       mean    |err| <= dmu = (a + 2 + i) u sum|x| / D                        the adds, the multiply by 1 / D (its rounding at D = 192 / 384), one spare
       rstd    |err| <= rstd64 (R + dmu^2 / (var + eps)),  R = (a + 8 + i) u + E_FAST
               x - mean (2 u in the square), the square, the adds, 1 / D, + eps, the inverse root; the centred sum about the ROUNDED mean
               is var + (mean error)^2 exactly, which is the second term (a constant row of 100 at D = 192 lives on it)
       y       |err| <= 2^-8 |y64| + 1.01 F,   F = |gamma| rstd64 (dmu + (R' + 4 u) (|x - mean| + dmu)) + 3 u (|v64| + |beta|),  R' = the rstd bound / rstd64
               (1.01: the bf16 rounding of a value that F moved);  with GELU 2^-8 |G| + 1.01 * 1.14 F + E_G (|v64| + F): max |G'| = 1.13, E_G = 5e-5
               relative to the pre-activation (tests/test_gelu_sites.py)
   LayerNorm backward (mean / rstd are fp32 inputs; d = dy' gamma, dy' = dy G'(xhat gamma + beta) with GELU, error of dy' at most
   dp = |dy| (E_A + 8 u (1 + |xhat gamma| + |beta|)), E_A = 5e-5 (dgelu_acc_f, common.h), 0 without GELU):
       dx      |err| <= 2^-8 |dx64| + 1.01 rstd (|gamma| dp + e1 + |xhat| e2 + 8 u (|d| + |c1| + |xhat c2|)) [+ 2 u |dx64| with dres]
               e1 = (a + 3) u mean|d| + mean(|gamma| dp),  e2 = (a + 6) u mean|d xhat| + mean(|gamma| dp |xhat|)
       dgamma  |err| <= (k + 4) u (sum_r |dy' xhat| + |start|) + sum_r dp |xhat|      k = the column count above
       dbeta   |err| <= (k + 2) u (sum_r |dy'| + |start|) + sum_r dp       dcolsum   |err| <= (k + 1) u (sum_r |dres| + |start|)
   BatchNorm (one pass, E[x^2] - mean^2 in fp32; k = the column count):
       sums    |err| <= k u sum|x|,  (k + 1) u sum x^2
       mean    |err| <= dmu = (k + 2) u sum|x| / n
       var     |err| <= dvar = (3 k + 8) u E[x^2]: the sum of squares (k + 2), mean^2 (2 k + 4 of its own), product and difference
       rstd    inside [(1 - 4 u - E_FAST) / sqrt(var + dvar + eps), (1 + 4 u + E_FAST) / sqrt(max(var - dvar, 0) + eps)]; to first order that is
               k' u kappa / 2 relative with kappa = E[x^2] / (var + eps), k' = 3 k + 8.  kappa per column kind: randn 2 + 0.5: 1.06; constant 0: 0;
               constant 1.7: 2.9e5; constant 100: 1e9 (var = 0, the clamp: rstd anywhere between 1 / sqrt(eps) and 1 / sqrt(dvar + eps), and y = beta
               to within |gamma| dmu rstd); mean 16, std 0.25: 4.1e3 (each test prints its largest kappa and its k)
       y       |err| <= 2^-8 |y64| + 1.01 (|gamma| (|x - mean| B_rstd + dmu rstd_hi + 4 u (|x - mean| + dmu) rstd_hi) + 3 u (|v64| + |beta|))
       running mean  m dmu + 4 u (|rm| + |mean| m)          running var  1.001 m n / (n - 1) dvar + 6 u (|rv| + var n / (n - 1) m)
       the `_running` form against dig_bn_update_running on the same fp32 sums: twice the expression's own roundings, 8 u (|rm| + |mean| m) and
       2 (5 u E[x^2] n / (n - 1) m + 6 u (|rv| + var n / (n - 1) m)) (two kernels: contraction may differ, the bits need not agree)
       backward sums  (k + 1) u sum|g| + A1,  (k + 4) u sum|g xhat| + A2;  A: |dy| (and |dy xhat|) of the elements whose pre-activation
               gamma xhat + beta is within 8 u (|gamma xhat| + |beta|) of 0: they may fall either side of the mask `> 0` (none on dyadic data)
       dx      2^-8 |dx64| + 1.01 |gamma rstd| (8 u (|g| + |S1 / n| + |xhat S2 / n|) + A), S the fp32 sums the call read; the one-launch path
               does not return its sums: float64 sums, plus |gamma rstd| (b_S1 + |xhat| b_S2) / n
   l2norm      inv_norm, y: (a + 6) u and (a + 7) u relative (squares, adds, root, reciprocal, product).  dx: inv (|y| (a + 2) u sum|y dy| + 4 u (|dy| + |y s|))
   sgemm       integer operands exact; random: (K + 2) u |alpha| sum |a| |b| over the slab's K range
   ce_rows     rank = #{j : z_j > z_label}: top-1 iff rank == 0, top-5 iff rank < 5; entries EQUAL to the label's logit do not count (torch.topk's
               order among ties is unspecified, so the reference is built from this rule)
               s = sum exp(z - max): relative R_s = (a + 4) u + 3 u sum_j p_j |z_j - max| + E_FAST (the subtraction's rounding enters exp as an
               absolute error of its argument);  loss: sum_rows (R_s + E_FAST + 3 u (|max| + |lse| + |z_label|)) + (n + 1) u sum|loss_i| + u |out|
               dlogits: gscale (p (R_s + 3 u |z - max| + 4 u + E_FAST) + 2 u |p - onehot| + 2^-125) (2^-125: a probability below the smallest normal
               number, exp(-160) of the +-80 row, may come out as 0); each row of dlogits sums to 0 within the sum of its bounds;
               with a workspace: the same bound, and within twice it of the plain form (another order)
   mse         loss: (a + 6) u (sum df^2 / count) + u |loss|;  dpred: (2^-8 + 5 u) |ref|, pad columns exactly 0
   E_FAST = 4 x 9.2e-8: __expf / __logf / rsqrtf are not correctly rounded; exp, log and 1 / sqrt in plain fp32 torch measure 9.16e-8 relative
   against float64 on 2^22 arguments each (restatement test), and the intrinsics are allowed four times that.

`test_fp32_restatement_is_inside_the_bounds` / `..._of_the_other_kernels_...` hold a plain fp32 torch restatement of each formula to the same bounds
(the cpu counts: no chain in torch is longer).  Their worst |err| / bound: LayerNorm mean 0.045, rstd 0.033, y 0.995, dx 0.996, dgamma 0.034,
dbeta 0.0014, dcolsum 0.0016; BatchNorm mean 0.0018, rstd 0.069, y 0.97, running mean 0.19, running var 0.16, sum g 8e-5, sum g xhat 3e-4, dx 0.995;
l2norm inv_norm 0.16, y 0.14; ce_rows loss 0.013, dlogits 0.24; mse loss 0.008, dpred 0.996.  (y, dx, dpred: the bf16 rounding is reached; the
column sums are worst-case counts over up to 1003 additions that blocked summation does not come near.)  A bound that a kernel exceeds is a finding
to investigate, not a number to raise.  Every output buffer carries 256 poisoned elements behind its range, which must survive; every workspace is
NaN before the call.

Cases -> the branch or loop trip they exist for
-----------------------------------------------
dig_layernorm_fwd                D in 64 128 192 256 384 512 x GELU: twelve instantiations, load_row 16-byte (512), dword (128 256 384), scalar (64 192)
    rows 1 2 3 5 17              the clamp min(r0 + u, rows - 1) with rows < U (U = 4 rows in flight, 2 with GELU), a first full group, a second workgroup
    rows 32768 + 5 / 16384 + 3   D = 64 without / with GELU: the second grid-stride trip past the 2048-block cap, with a partial group
    row kinds (index mod 7)      randn; constant 0 / 1.7 / 100 (var = 0; y = beta exactly for 0); mean 64 std 0.5 (a one-pass variance fails here);
                                 std 1e-3 (var ~ eps: the wrong eps, or none, fails here); one 1e4 outlier; 3 randn + 1
    eps 1e-6 and 1e-5            the encoder blocks' and the text-conditional LayerNorm's; mean and rstd compared
    refusals                     D = 320 unsupported, x + 2 bytes misaligned, rows = 0: poisoned outputs untouched
dig_layernorm_bwd, dig_layernorm_bwd_partials + dig_layernorm_bwd_finalize
    rows 1 2 3 16 17 1003        one row of a pair, a pair, the odd last pair, one full part, a second part, many parts
    rows 16384 + 25 (D = 64)     the third trip past the 1024-part cap with an odd last pair
    dres None / given, dcolsum None / given, beta None without GELU; accumulators start non-zero; one call == partials + finalize == a second run, bit
    for bit; dyadic data: dgamma / dbeta / dcolsum exact
    refusals                     dcolsum without dres, GELU without beta, D = 320, rows = 0, x + 2 bytes, D % 16 != 0 in both finalize forms
dig_layernorm_bwd_parts, dig_layernorm_bwd_workspace_bytes      min(1024, ceil(rows / 16)) [x 3 D 4] at rows 1 16 17 16384 10^6
dig_layernorm_bwd_finalize_parts parts 1 63 64 65 1024 1500 (one row group, 64-way walk of 1 / 2 / 16 / 24 trips), D = 64 and 192 (16-column blocks meet the
                                 boundaries between the three vectors), NaN behind row `parts`, dcolsum None, exact
dig_bn_stats, dig_bn_fwd_apply, dig_bn_fwd_apply_running, dig_bn_update_running, dig_bn_bwd_stats, dig_bn_bwd_stats_acc, dig_bn_bwd_apply,
dig_bn_stats_workspace_bytes
    C 8 64 288 2048 2056         one column group with 256 rows in flight; 32 rows in flight; c8 = 36: 7 rows in flight, four idle threads, the apply grid's
                                 gcd rule at unit 9; exactly one full column block; a second column block with a single live thread
    rows 1 2 31 33 1000          fewer rows than rows in flight, a strip boundary at 32, many strips
    rows 32 * 1024 + 1, C = 8    the rows-per-block doubling (64), 513 strips: the finalize walks more than its 32-wide fold
    gamma / beta None and given, ReLU on and off (exact zeros of the pre-activation: constant columns without affine, column 0 of the dyadic data)
    n_total = 2 rows             the sums doubled: the same bits in y / mean / rstd / dx, the running variance with the n / (n - 1) of 2 rows
    column kinds (index mod 5)   randn 2 + 0.5; constant 0 / 1.7 / 100; mean 16 std 0.25 (kappa 4.1e3)
    refusals                     C % 8, n_total <= 1 with running statistics, one of running mean / var, one of gamma / beta, one of dbeta_acc / dgamma_acc,
                                 misaligned sums / mean: outputs untouched
dig_bn_fused_supported, dig_bn_fwd_fused, dig_bn_bwd_fused
    rows 2 63 64 65 1000 4096    fewer rows than the 64 row lanes, one short, exact, one over, many trips, the limit
    C 256 288 4096               the smallest, 9 slabs (not a multiple of 8 slabs), the widest layer
    against float64, against the three-launch path (the sum of the two bounds), with and without running statistics / accumulators
    refusals                     rows 1 and 4097, C 224 and 264: supported() false, unsupported; gamma / beta / mean / rstd / running mean / running var /
                                 dbeta_acc / dgamma_acc one float into a buffer: misaligned, nothing launched, outputs untouched
dig_l2norm_fwd, dig_l2norm_bwd   n 1 5 512 (n % 4 != 0, 128 blocks), C 1 65 256 (one lane, C % 64 != 0, four trips); an all-zero row (y = 0, inv = 1 / eps,
                                 dx = dy / eps: the clamp has no gradient), a row of norm 1e-13 (below eps), a row of 1e18 (the squares sum to C 1e36, below
                                 3.4e38 up to C = 340: no overflow, and F.normalize in fp32 gives the same x / |x|, which the test holds the kernel to)
dig_sgemm (through the ABI: ops.sgemm picks the split itself)
    (1,1,1) (33,31,65) (100,520,200) (64,64,256), both trans_b, alpha 1 and 5, lda / ldb / ldc eight larger than the extents with poison in the pad
    r_splits 2 at R = 200 (a ragged second slab of 72), 3 at R = 130, 4 at R = 256: every slab the float64 product of its K range
    refusals                     r_splits = 3 at R = 128 (ceil(R / per) == r_splits fails), r_splits 0, I = 0
dig_ce_rows, dig_ce_rows_ws      n 1 7 (7 rows do not fit m = 5 / 6: refused, then n = m), m 5 6 255 256 257 1000 (every row a top-5 hit at m = 5, the sixth
                                 row not at m = 6; less than one trip of the 256 threads, exactly one, a second)
                                 label_offset 0 and m - n; randn 5, a row of +-80, ties at the label's logit: (above, equal) = (0,3) (1,2) (4,3) (5,0) (0,6);
                                 out3 starts non-zero; the workspace form twice on one zeroed workspace: the same bits, ticket word 0
                                 refusal: label_offset + n > m
dig_infonce_finish, dig_step_meters   test_gpu_kernels.py::test_scalar_tails_of_infonce_and_the_log_line (grad_norm None -> NaN is asserted there)
dig_mse_fwd_bwd, dig_mse_fwd_bwd_ws   (M, C, ld_pred, ld_dpred) (1,1,1,1) (895,48,64,64) (300,48,48,56) (2000,48,48,48: M ld > 65536, the 256-block grid strides);
                                 loss only, gradient only, gscale 0.7, loss += onto 0.5, pad columns zero, the workspace form three times: the same bits
dig_colsum, dig_colsum_masked, dig_colsum_workspace_bytes
    C 8 520 1536                 one lane; a second column block 8 wide; three blocks
    rows 1 3 4 13 16 17 64 65    the 16-row unrolled loop (r + 12 < r1), its 4-row tail, a second row block; rows 32768 + 70 at C = 8: the doubling (128)
    ld = C and C + 8 with poison in the pad; out starts non-zero; masks all 0, all 1 (any non-zero byte), random
dig_colsum_partials              n_parts 1 127 128 129 (the 128 row groups: one short, exact, a second trip), NaN behind the last part; C % 8, partials + 4 bytes refused
dig_colsum_partials_multi        thirteen segments of widths % 32 == 0 (the 32-column kernel), the same with one width of 40 (the 8-column kernel), strides 3 C

Largest |err| / bound on the MI355X (printed by every test; no kernel exceeded a bound)
---------------------------------------------------------------------------------------
    LayerNorm    mean 0.41, rstd 0.13, y 0.996, dx 0.996, dgamma 0.91, dbeta 0.91 (both with GELU: E_A), dcolsum 0.07
    BatchNorm    sum x 0.015, sum x^2 0.08, mean 0.026, rstd 0.83, y 0.995, running mean 0.40, running var 0.21, sum g 0.004, sum g xhat 0.05, dx 0.996;
                 `_running` against dig_bn_update_running: mean 0 (the same bits), var 0.15 (NOT the same bits: two kernels, two contractions)
                 one launch: mean 0.03, rstd 0.28, y 0.994, running mean 0.32, running var 0.21, dbeta 0.27, dgamma 0.45, dx 0.996; against three launches 0.02
    l2norm       inv_norm 0.13, y 0.18, dx 0.46          sgemm 0.19          mse loss 0.02, dpred 0.994
    ce_rows      loss 0.14, dlogits 0.43, row sums 0.09, with a workspace 0.08, against the plain form 0.05
On the cpu build: LayerNorm mean 0.06, rstd 0.09, dgamma 0.32, dbeta 0.20, dcolsum 0.25; y, dx at the bf16 rounding (0.995).

Seeded faults (each a one-line arithmetic change to cpu_abi/dig_cpu.cpp, on a scratch copy) and the tests that failed
---------------------------------------------------------------------------------------------------------------------
    LayerNorm eps ignored; variance as E[x^2] - mean^2; rstd output off by 1 + 2^-12     test_layernorm_fwd_vs_fp64
    the last LayerNorm row's dx taken from the row before                                 test_layernorm_bwd_vs_fp64
    dgamma missing its last part        test_layernorm_bwd_finalize_parts, test_layernorm_bwd_sums_are_exact_on_dyadic_data, test_layernorm_bwd_vs_fp64
    BatchNorm ReLU mask >= instead of > test_batchnorm_sums_are_exact_on_integers, test_batchnorm_fused_is_exact_on_integers, the two vs_fp64 tests
    n / (n - 1) dropped; BatchNorm eps ignored        test_batchnorm_three_launch_vs_fp64, test_batchnorm_fused_vs_fp64_and_three_launch
    top-5 threshold 5.5                 test_ce_rows_vs_fp64              l2norm eps clamp removed        test_l2norm_vs_fp64
    sgemm alpha on the first slab only  test_sgemm_vs_fp64                colsum skipping row rows - 1    test_colsum_and_masked_are_exact
"""
import ctypes
import math

import numpy as np
import pytest
import torch

U = 2.0 ** -24
BF_ULP = 2.0 ** -8                # one bf16 rounding of a result, as test_optim_kernels.py allows it
GUARD = 256                       # poisoned elements behind every output range
POISON = 768.0                    # (exact in bf16)
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
cf = ctypes.c_float
E_G, E_A = 5e-5, 5e-5             # gelu_f (relative to |x|) and dgelu_acc_f (absolute): tests/test_gelu_sites.py
E_FAST_R = 9.2e-8                 # worst relative error of exp / log / 1 / sqrt in plain fp32 torch against float64 (the restatement test measures it)
E_FAST = 4 * E_FAST_R             # the allowance for __expf / __logf / rsqrtf: four times that
ARG, ALIGN, UNSUP = -1, -2, -4


def f32(x):
    return float(np.float32(x))


def _backend(dev):
    return "hip" if dev.type == "cuda" else "cpu_abi"


def _sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize()


def _L():
    from dig_amd import _lib
    return _lib


def _buf(dev, n, dtype=F32, fill=POISON):
    """n elements of `fill` with GUARD poisoned ones behind them."""
    b = torch.full((n + GUARD,), POISON, dtype=dtype, device=dev)
    if fill != POISON:
        b[:n] = fill
    return b


def _put(dev, t):
    """A host tensor on the device, flattened, with the guard behind it."""
    t = t.contiguous().reshape(-1)
    b = torch.full((t.numel() + GUARD,), POISON, dtype=t.dtype, device=dev)
    b[:t.numel()] = t.to(dev)
    return b


def _ws(dev, nfloats):
    """A workspace of NaN (a partial that is read but was never written shows) with the guard behind it."""
    b = torch.full((nfloats + GUARD,), POISON, dtype=F32, device=dev)
    b[:nfloats] = math.nan
    return b


def _get(b, n, *shape):
    return b[:n].detach().cpu().reshape(*shape) if shape else b[:n].detach().cpu()


def _guard_ok(b, n):
    return bool((b[n:].float() == POISON).all())


def _untouched(b):
    return bool((b.float() == POISON).all())


def _refused(code, name, *args):
    L = _L()
    with pytest.raises(L.DigHipError) as e:
        L.call(name, *args)
    assert f"rc={code})" in str(e.value), (name, str(e.value))


def _inside(tag, got, ref, bound):
    """Prints the worst |got - ref| / bound, then asserts the element-wise bound; every value finite."""
    got, ref, bound = got.double(), ref.double(), bound.double()
    assert bool(torch.isfinite(got).all()), (tag, "non-finite")
    err = (got - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print(f"{tag}: worst |err| / bound = {ratio:.3g}")
    bad = err > bound
    if bool(bad.any()):
        i = int(torch.nonzero(bad.reshape(-1))[0])
        raise AssertionError((tag, ratio, i, float(got.reshape(-1)[i]), float(ref.reshape(-1)[i]), float(bound.reshape(-1)[i])))
    return ratio


def _gelu64(v):
    return 0.5 * v * (1.0 + torch.erf(v * math.sqrt(0.5)))


def _dgelu64(v):
    return 0.5 * (1.0 + torch.erf(v * math.sqrt(0.5))) + v * torch.exp(-0.5 * v * v) / math.sqrt(2.0 * math.pi)


def _ints(gen, *shape, lo=-8, hi=8):
    return torch.randint(lo, hi + 1, shape, generator=gen).float()


def _quarters(gen, *shape):
    return torch.randint(-32, 33, shape, generator=gen).float() / 4


# ================================================================================================ LayerNorm
LN_D = [64, 128, 192, 256, 384, 512]
LN_EPS = (f32(1e-6), f32(1e-5))


def _ln_adds(backend, D):
    """Additions an element passes through in a row sum: the lane's sequential adds and six shuffle levels, or one chain of D."""
    return (D // 64 - 1 + 6) if backend == "hip" else D - 1


def _ln_rows(rows, D, seed):
    """[rows, D] bf16, the row kinds by row index mod 7."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, D, generator=g)
    r = torch.arange(rows)
    const = torch.tensor([0.0, 1.7, 100.0])[(r // 7) % 3]
    k = r % 7
    x = torch.where((k == 1)[:, None], const[:, None].expand(rows, D), x)
    x = torch.where((k == 2)[:, None], 64.0 + 0.5 * x, x)
    x = torch.where((k == 3)[:, None], 1e-3 * x, x)
    out = (r * 13) % D
    sel = k == 4
    x[r[sel], out[sel]] = 1e4
    x = torch.where((k == 5)[:, None], 3.0 * x + 1.0, x)
    return x.bfloat16()


_LN_PARAMS = {}


def _ln_params(D):
    if D not in _LN_PARAMS:
        g = torch.Generator().manual_seed(D)
        _LN_PARAMS[D] = (torch.randn(D, generator=g) * 0.5 + 1.0, torch.randn(D, generator=g) * 0.3)
    return _LN_PARAMS[D]


def _ln_fwd_ref(x, gamma, beta, eps, gelu, backend):
    """float64 outputs and the bounds of the docstring: (mean, rstd, y), (b_mean, b_rstd, b_y)."""
    D = x.shape[1]
    na, inexact = _ln_adds(backend, D), int(D in (192, 384))
    x, g, b = x.double(), gamma.double(), beta.double()
    mu = x.mean(1, keepdim=True)
    xc = x - mu
    var = (xc * xc).mean(1, keepdim=True)
    rs = 1.0 / torch.sqrt(var + eps)
    v = xc * rs * g + b
    dmu = (na + 2 + inexact) * U * x.abs().mean(1, keepdim=True)
    rel = (na + 8 + inexact) * U + E_FAST + dmu * dmu / (var + eps)
    fp = g.abs() * rs * (dmu + (rel + 4 * U) * (xc.abs() + dmu)) + 3 * U * (v.abs() + b.abs())
    if gelu:
        y = _gelu64(v)
        by = BF_ULP * y.abs() + 1.01 * 1.14 * fp + E_G * (v.abs() + fp)
    else:
        y = v
        by = BF_ULP * y.abs() + 1.01 * fp
    return (mu[:, 0], rs[:, 0], y), (dmu[:, 0], (rel * rs)[:, 0], by)


def _ln_fwd(dev, x, gamma, beta, eps, gelu):
    L = _L()
    rows, D = x.shape
    xd, gd, bd = _put(dev, x), _put(dev, gamma), _put(dev, beta)
    y, mean, rstd = _buf(dev, rows * D, BF), _buf(dev, rows), _buf(dev, rows)
    L.call("dig_layernorm_fwd", L.ptr(xd), L.ptr(gd), L.ptr(bd), L.ptr(y), L.ptr(mean), L.ptr(rstd), rows, D, cf(eps), int(gelu), L.stream())
    _sync(dev)
    assert _guard_ok(y, rows * D) and _guard_ok(mean, rows) and _guard_ok(rstd, rows)
    return _get(mean, rows), _get(rstd, rows), _get(y, rows * D, rows, D)


def _ln_fwd_rows(D, gelu):
    big = {(64, 0): [32768 + 5], (64, 1): [16384 + 3]}.get((D, gelu), [])
    return [1, 2, 3, 5, 17] + big


@pytest.mark.parametrize("gelu", [0, 1], ids=["plain", "gelu"])
@pytest.mark.parametrize("D", LN_D)
def test_layernorm_fwd_vs_fp64(abi_dev, D, gelu):
    dev, be = abi_dev, _backend(abi_dev)
    gamma, beta = _ln_params(D)
    for rows in _ln_fwd_rows(D, gelu):
        x = _ln_rows(rows, D, rows + D)
        for eps in (LN_EPS if rows <= 17 else LN_EPS[:1]):
            mean, rstd, y = _ln_fwd(dev, x, gamma, beta, eps, gelu)
            ref, bnd = _ln_fwd_ref(x, gamma, beta, eps, gelu, be)
            tag = f"ln_fwd {be} D {D} gelu {gelu} rows {rows} eps {eps:.0e}"
            _inside(tag + " mean", mean, ref[0], bnd[0])
            _inside(tag + " rstd", rstd, ref[1], bnd[1])
            _inside(tag + " y", y, ref[2], bnd[2])
            const0 = (torch.arange(rows) % 21) == 1                                   # the all-zero rows: y is beta (or its GELU), whatever eps
            if bool(const0.any()) and not gelu:
                assert torch.equal(y[const0], beta.bfloat16().expand(int(const0.sum()), D))


@pytest.mark.parametrize("D", [64, 128, 256, 512])
def test_layernorm_fwd_mean_is_exact_on_integers(abi_dev, D):
    """Integers in [-8, 8]: every partial sum is exact in fp32 in any order and 1 / D is a power of two, so `mean` equals the float64 mean bit for
    bit; rows 1 .. 17 and, at D = 64, the second grid-stride trip."""
    dev = abi_dev
    gamma, beta = _ln_params(D)
    for rows in [1, 2, 3, 5, 17] + ([32768 + 5] if D == 64 else []):
        x = _ints(torch.Generator().manual_seed(rows), rows, D).bfloat16()
        for gelu in (0, 1):
            mean, rstd, _ = _ln_fwd(dev, x, gamma, beta, LN_EPS[0], gelu)
            assert torch.equal(mean.double(), x.double().mean(1)), (D, rows, gelu)


def test_layernorm_fwd_refusals(abi_dev):
    dev = abi_dev
    L = _L()
    x, g, b = _put(dev, _ln_rows(4, 320, 1)), _put(dev, torch.ones(320)), _put(dev, torch.zeros(320))
    y, mean, rstd = _buf(dev, 4 * 320, BF), _buf(dev, 4), _buf(dev, 4)
    out = (L.ptr(y), L.ptr(mean), L.ptr(rstd))
    _refused(UNSUP, "dig_layernorm_fwd", L.ptr(x), L.ptr(g), L.ptr(b), *out, 4, 320, cf(1e-6), 0, L.stream())
    _refused(UNSUP, "dig_layernorm_fwd", L.ptr(x), L.ptr(g), L.ptr(b), *out, 4, 320, cf(1e-6), 1, L.stream())
    _refused(ALIGN, "dig_layernorm_fwd", ctypes.c_void_p(x.data_ptr() + 2), L.ptr(g), L.ptr(b), *out, 4, 256, cf(1e-6), 0, L.stream())
    _refused(ARG, "dig_layernorm_fwd", L.ptr(x), L.ptr(g), L.ptr(b), *out, 0, 256, cf(1e-6), 0, L.stream())
    _sync(dev)
    assert _untouched(y) and _untouched(mean) and _untouched(rstd)


# ------------------------------------------------------------------------------------------------ LayerNorm backward
LN_BWD_ROWS = [1, 2, 3, 16, 17, 1003]
LN_BWD_BIG = 16384 + 25


def _ln_parts(rows):
    return max(1, min(1024, (rows + 15) // 16))


def _ln_col_adds(backend, rows):
    """Additions a row's term passes through on its way into dgamma / dbeta / dcolsum (the docstring's k(rows))."""
    parts = _ln_parts(rows)
    if backend == "hip":
        return 2 * -(-rows // (8 * parts)) + 3 + -(-parts // 64) + 6 + 1
    return -(-rows // parts) + parts + 1


def _ln_bwd_ref(dy, x, gamma, beta, mean, rstd, dres, gelu, backend, start):
    """float64 (dx, dgamma, dbeta, dcolsum) from the fp32 / bf16 inputs and their bounds; `start`: the three accumulators' values before."""
    rows, D = x.shape
    na, kc = _ln_adds(backend, D), _ln_col_adds(backend, rows)
    x, dy, g, b = x.double(), dy.double(), gamma.double(), beta.double()
    mu, rs = mean.double()[:, None], rstd.double()[:, None]
    xh = (x - mu) * rs
    if gelu:
        v = xh * g + b
        dyp = dy * _dgelu64(v)
        dp = dy.abs() * (E_A + 8 * U * (1 + (xh * g).abs() + b.abs()))          # error of dy' : the derivative's own and that of its argument
    else:
        dyp, dp = dy, torch.zeros_like(dy)
    d, dd = dyp * g, dp * g.abs()
    c1, c2 = d.mean(1, keepdim=True), (d * xh).mean(1, keepdim=True)
    dx = rs * (d - c1 - xh * c2)
    e1 = (na + 3) * U * d.abs().mean(1, keepdim=True) + dd.mean(1, keepdim=True)
    e2 = (na + 6) * U * (d * xh).abs().mean(1, keepdim=True) + (dd * xh.abs()).mean(1, keepdim=True)
    fp = rs * (dd + e1 + xh.abs() * e2 + 8 * U * (d.abs() + c1.abs() + (xh * c2).abs()))
    if dres is not None:
        dx = dx + dres.double()
        fp = fp + 2 * U * dx.abs()
    bdx = BF_ULP * dx.abs() + 1.01 * fp
    t_g, t_b = dyp * xh, dyp
    sg, sb, sc = (s.double() for s in start)
    dgamma, dbeta = sg + t_g.sum(0), sb + t_b.sum(0)
    bg = (kc + 4) * U * (t_g.abs().sum(0) + sg.abs()) + (dp * xh.abs()).sum(0)
    bb = (kc + 2) * U * (t_b.abs().sum(0) + sb.abs()) + dp.sum(0)
    if dres is not None:
        dcol = sc + dres.double().sum(0)
        bc = (kc + 1) * U * (dres.double().abs().sum(0) + sc.abs())
    else:
        dcol, bc = sc, torch.zeros_like(sc)
    return (dx, dgamma, dbeta, dcol), (bdx, bg, bb, bc)


class _LnBwd:
    """One LayerNorm backward problem on the device: every buffer guarded, the workspace NaN, the accumulators non-zero."""

    def __init__(self, dev, dy, x, gamma, beta, mean, rstd, dres, start, with_col):
        L = self.L = _L()
        self.dev, (self.rows, self.D) = dev, x.shape
        self.dy, self.x, self.g, self.b = _put(dev, dy), _put(dev, x), _put(dev, gamma), (_put(dev, beta) if beta is not None else None)
        self.mean, self.rstd = _put(dev, mean), _put(dev, rstd)
        self.dres = _put(dev, dres) if dres is not None else None
        self.with_col = with_col
        self.nws = L.query("dig_layernorm_bwd_workspace_bytes", self.rows, self.D) // 4
        self.start = start
        self.reset()

    def reset(self):
        dev, n, D = self.dev, self.rows * self.D, self.D
        self.dx, self.ws = _buf(dev, n, BF), _ws(dev, self.nws)
        self.dg, self.db, self.dc = (_put(dev, s) for s in self.start)

    def args(self):
        L = self.L
        return (L.ptr(self.dy), L.ptr(self.x), L.ptr(self.g), L.ptr(self.b), L.ptr(self.mean), L.ptr(self.rstd), L.ptr(self.dres), L.ptr(self.dx))

    def acc(self):
        L = self.L
        return (L.ptr(self.dg), L.ptr(self.db), L.ptr(self.dc) if self.with_col else None)

    def one_call(self, gelu):
        L = self.L
        L.call("dig_layernorm_bwd", *self.args(), *self.acc(), L.ptr(self.ws), self.rows, self.D, int(gelu), L.stream())
        return self.result()

    def two_calls(self, gelu):
        L = self.L
        L.call("dig_layernorm_bwd_partials", *self.args(), L.ptr(self.ws), self.rows, self.D, int(gelu), L.stream())
        L.call("dig_layernorm_bwd_finalize", L.ptr(self.ws), self.rows, self.D, *self.acc(), L.stream())
        return self.result()

    def result(self):
        _sync(self.dev)
        n, D = self.rows * self.D, self.D
        assert _guard_ok(self.dx, n) and _guard_ok(self.ws, self.nws) and all(_guard_ok(t, D) for t in (self.dg, self.db, self.dc))
        return _get(self.dx, n, self.rows, D), _get(self.dg, D), _get(self.db, D), _get(self.dc, D)


def _ln_bwd_inputs(rows, D, gelu, seed):
    g = torch.Generator().manual_seed(seed)
    x = _ln_rows(rows, D, seed)
    dy = torch.randn(rows, D, generator=g).bfloat16()
    dres = torch.randn(rows, D, generator=g).bfloat16()
    gamma, beta = _ln_params(D)
    ref, _ = _ln_fwd_ref(x, gamma, beta, LN_EPS[0], gelu, "hip")
    start = tuple(torch.randn(D, generator=g) for _ in range(3))
    return dy, x, gamma, beta, ref[0].float(), ref[1].float(), dres, start


@pytest.mark.parametrize("gelu", [0, 1], ids=["plain", "gelu"])
@pytest.mark.parametrize("D", LN_D)
def test_layernorm_bwd_vs_fp64(abi_dev, D, gelu):
    """dig_layernorm_bwd against float64 for every (dres, dcolsum) form; dig_layernorm_bwd_partials + dig_layernorm_bwd_finalize and a second
    run give the same bits."""
    dev, be = abi_dev, _backend(abi_dev)
    for rows in LN_BWD_ROWS + ([LN_BWD_BIG] if D == 64 else []):
        dy, x, gamma, beta, mean, rstd, dres, start = _ln_bwd_inputs(rows, D, gelu, rows + D + gelu)
        for use_res, use_col in ((False, False), (True, False), (True, True)):
            p = _LnBwd(dev, dy, x, gamma, beta if (gelu or use_col) else None, mean, rstd, dres if use_res else None, start, use_col)
            got = p.one_call(gelu)
            ref, bnd = _ln_bwd_ref(dy, x, gamma, beta, mean, rstd, dres if use_res else None, gelu, be, start)
            tag = f"ln_bwd {be} D {D} gelu {gelu} rows {rows} dres {int(use_res)} dcol {int(use_col)}"
            for name, a, r, b in zip(("dx", "dgamma", "dbeta", "dcolsum"), got, ref, bnd):
                if name == "dcolsum" and not use_col:
                    assert torch.equal(a, start[2])                                 # not given to the call: as it was
                else:
                    _inside(f"{tag} {name}", a, r, b)
            p.reset()
            again = p.one_call(gelu)
            p.reset()
            split = p.two_calls(gelu)
            for a, b2, c in zip(got, again, split):
                assert torch.equal(a, b2) and torch.equal(a, c), tag


@pytest.mark.parametrize("D", LN_D)
def test_layernorm_bwd_sums_are_exact_on_dyadic_data(abi_dev, D):
    """dy integers, x integers, mean an integer per row and rstd a power of two (they are inputs): xhat, dy xhat and every partial sum are exact
    in fp32 in any order, so dbeta, dgamma and dcolsum equal the float64 sums bit for bit, on top of non-zero dyadic accumulators."""
    dev = abi_dev
    for rows in LN_BWD_ROWS + ([LN_BWD_BIG] if D == 64 else []):
        g = torch.Generator().manual_seed(rows * 7 + D)
        x, dy = _ints(g, rows, D).bfloat16(), _ints(g, rows, D).bfloat16()
        dres = _quarters(g, rows, D).bfloat16()
        mean = _ints(g, rows, lo=-2, hi=2)
        rstd = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (rows,), generator=g)]
        gamma = _quarters(g, D)
        start = tuple(_quarters(g, D) for _ in range(3))
        xh = (x.double() - mean.double()[:, None]) * rstd.double()[:, None]
        want = (start[0].double() + (dy.double() * xh).sum(0), start[1].double() + dy.double().sum(0), start[2].double() + dres.double().sum(0))
        for form in ("one", "two"):
            p = _LnBwd(dev, dy, x, gamma, None, mean, rstd, dres, start, True)
            _, dg, db, dc = p.one_call(0) if form == "one" else p.two_calls(0)
            for name, a, w in zip(("dgamma", "dbeta", "dcolsum"), (dg, db, dc), want):
                assert torch.equal(a.double(), w), (D, rows, form, name, float((a.double() - w).abs().max()))


def test_layernorm_bwd_refusals_and_sizes(abi_dev):
    dev = abi_dev
    L = _L()
    for rows in (1, 16, 17, 16384, 10 ** 6):
        parts = max(1, min(1024, (rows + 15) // 16))
        assert L.query("dig_layernorm_bwd_parts", rows) == parts
        for D in (64, 192, 512):
            assert L.query("dig_layernorm_bwd_workspace_bytes", rows, D) == parts * 3 * D * 4
    dy, x, gamma, beta, mean, rstd, dres, start = _ln_bwd_inputs(5, 128, 0, 3)

    def fresh(**kw):
        a = dict(dev=dev, dy=dy, x=x, gamma=gamma, beta=beta, mean=mean, rstd=rstd, dres=dres, start=start, with_col=True)
        a.update(kw)
        return _LnBwd(**a)

    def untouched(p):
        _sync(dev)
        assert _untouched(p.dx) and all(torch.equal(_get(t, 128), s) for t, s in zip((p.dg, p.db, p.dc), start))

    p = fresh(dres=None)                                                        # dcolsum without dres
    _refused(ARG, "dig_layernorm_bwd", *p.args(), *p.acc(), L.ptr(p.ws), 5, 128, 0, L.stream())
    untouched(p)
    p = fresh(beta=None)                                                        # GELU without beta
    _refused(ARG, "dig_layernorm_bwd", *p.args(), *p.acc(), L.ptr(p.ws), 5, 128, 1, L.stream())
    _refused(ARG, "dig_layernorm_bwd_partials", *p.args(), L.ptr(p.ws), 5, 128, 1, L.stream())
    untouched(p)
    p = fresh()
    _refused(UNSUP, "dig_layernorm_bwd", *p.args(), *p.acc(), L.ptr(p.ws), 2, 320, 0, L.stream())
    _refused(ARG, "dig_layernorm_bwd", *p.args(), *p.acc(), L.ptr(p.ws), 0, 128, 0, L.stream())
    a = list(p.args())
    a[1] = ctypes.c_void_p(p.x.data_ptr() + 2)
    _refused(ALIGN, "dig_layernorm_bwd", *a, *p.acc(), L.ptr(p.ws), 4, 128, 0, L.stream())
    _refused(ARG, "dig_layernorm_bwd_finalize", L.ptr(p.ws), 5, 72, *p.acc(), L.stream())
    _refused(ARG, "dig_layernorm_bwd_finalize_parts", L.ptr(p.ws), 5, 72, *p.acc(), L.stream())
    _refused(ARG, "dig_layernorm_bwd_finalize_parts", L.ptr(p.ws), 0, 64, *p.acc(), L.stream())
    untouched(p)


@pytest.mark.parametrize("D", [64, 192])
@pytest.mark.parametrize("parts", [1, 63, 64, 65, 1024, 1500])
def test_layernorm_bwd_finalize_parts(abi_dev, D, parts):
    """A synthetic [parts][3][D] workspace of multiples of 1/4 with NaN behind row `parts`: dgamma / dbeta / dcolsum += the float64 column sums,
    bit for bit (exact in any order); dcolsum None leaves it alone."""
    dev = abi_dev
    L = _L()
    g = torch.Generator().manual_seed(parts + D)
    w = _quarters(g, parts, 3, D)
    ws = torch.cat([w.reshape(-1), torch.full((8 * 3 * D,), math.nan)])
    wsd = _put(dev, ws)
    start = [_quarters(g, D) for _ in range(3)]
    for with_col in (True, False):
        acc = [_put(dev, s) for s in start]
        L.call("dig_layernorm_bwd_finalize_parts", L.ptr(wsd), parts, D, L.ptr(acc[0]), L.ptr(acc[1]), L.ptr(acc[2]) if with_col else None, L.stream())
        _sync(dev)
        for v in range(3):
            want = start[v].double() + (w[:, v].double().sum(0) if (v < 2 or with_col) else 0.0)
            assert torch.equal(_get(acc[v], D).double(), want), (parts, D, v, with_col)
            assert _guard_ok(acc[v], D)


# ================================================================================================ the bounds themselves
def test_fp32_restatement_is_inside_the_bounds():
    """The LayerNorm formulas in plain fp32 torch (no library) against the float64 reference, held to the bounds of the build with the longest
    summation chain (torch's own sums are blocked: no chain is longer).  The printed ratios are the docstring's."""
    for D in LN_D:
        gamma, beta = _ln_params(D)
        x = _ln_rows(1003, D, D)
        for eps in LN_EPS:
            xf = x.float()
            mu = xf.sum(1, keepdim=True) / D
            xc = xf - mu
            rs = 1.0 / torch.sqrt((xc * xc).sum(1, keepdim=True) / D + eps)
            v = xc * rs * gamma + beta
            for gelu in (0, 1):
                y = (torch.nn.functional.gelu(v) if gelu else v).bfloat16()
                ref, bnd = _ln_fwd_ref(x, gamma, beta, eps, gelu, "cpu_abi")
                tag = f"restatement ln_fwd D {D} gelu {gelu} eps {eps:.0e}"
                _inside(tag + " mean", mu[:, 0], ref[0], bnd[0])
                _inside(tag + " rstd", rs[:, 0], ref[1], bnd[1])
                _inside(tag + " y", y, ref[2], bnd[2])
        for gelu in (0, 1):
            dy, x, gamma, beta, mean, rstd, dres, start = _ln_bwd_inputs(1003, D, gelu, D + 1)
            xh = (x.float() - mean[:, None]) * rstd[:, None]
            dyp = dy.float()
            if gelu:
                vv = xh * gamma + beta
                dyp = dyp * (0.5 * (1 + torch.erf(vv * f32(math.sqrt(0.5)))) + vv * torch.exp(-0.5 * vv * vv) * f32(1 / math.sqrt(2 * math.pi)))
            d = dyp * gamma
            c1, c2 = d.sum(1, keepdim=True) / D, (d * xh).sum(1, keepdim=True) / D
            dx = (rstd[:, None] * (d - c1 - xh * c2) + dres.float()).bfloat16()
            got = (dx, start[0] + (dyp * xh).sum(0), start[1] + dyp.sum(0), start[2] + dres.float().sum(0))
            ref, bnd = _ln_bwd_ref(dy, x, gamma, beta, mean, rstd, dres, gelu, "cpu_abi", start)
            for name, a, r, b in zip(("dx", "dgamma", "dbeta", "dcolsum"), got, ref, bnd):
                _inside(f"restatement ln_bwd D {D} gelu {gelu} {name}", a, r, b)


# ================================================================================================ BatchNorm
BN_EPS, BN_MOM = f32(1e-5), f32(0.1)
BN_C = [8, 64, 288, 2048, 2056]
BN_ROWS = [1, 2, 31, 33, 1000]
BN_BIG = (32 * 1024 + 1, 8)
BN_OPTS = [(False, 0), (False, 1), (True, 0), (True, 1)]           # (gamma / beta given, ReLU)


def _bn_rpb(rows, C):
    cb, rpb = -(-(C // 8) // 256), 32
    while cb * -(-rows // rpb) > 1024:
        rpb *= 2
    return rpb


def _bn_adds(backend, rows, C, fused=False):
    """Additions a row's term passes through in a column sum: the docstring's k."""
    if fused:
        return -(-rows // 64) + 64                                  # a row lane's walk, then the 64 lanes in order (both builds)
    if backend == "hip":
        rpb = _bn_rpb(rows, C)
        return rpb + 1 + -(-(-(-rows // rpb)) // 32) + 32            # the strip (rows in flight folded in order), the finalize walk, its 32-way fold
    return rows                                                     # one chain


def _bn_cols(rows, C, seed, ints=False):
    """[rows, C] bf16, the column kinds by column index mod 5."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, C, generator=g) * 2 + 0.5
    c = torch.arange(C)
    const = torch.tensor([0.0, 1.7, 100.0])[(c // 5) % 3]
    k = c % 5
    x = torch.where((k == 1)[None, :], const[None, :].expand(rows, C), x)
    x = torch.where((k == 2)[None, :], 16.0 + 0.25 * torch.randn(rows, C, generator=g), x)
    return x.bfloat16()


_BN_PARAMS = {}


def _bn_params(C):
    if C not in _BN_PARAMS:
        g = torch.Generator().manual_seed(C)
        _BN_PARAMS[C] = (torch.randn(C, generator=g) * 0.5 + 1.0, torch.randn(C, generator=g) * 0.3, torch.randn(C, generator=g),
                         torch.rand(C, generator=g) + 0.5)
    return _BN_PARAMS[C]


def _bn_fwd_ref(x, eps, gamma, beta, relu, k, n_total=None, running=None):
    """float64 (mean, rstd, y[, running_mean, running_var]) of the columns of x and their bounds; k: `_bn_adds`."""
    x = x.double()
    mu = x.mean(0)
    xc = x - mu
    var, ex2 = (xc * xc).mean(0), (x * x).mean(0)
    dmu = (k + 2) * U * x.abs().mean(0)
    dvar = (3 * k + 8) * U * ex2
    rs = 1.0 / torch.sqrt(var + eps)
    rs_hi = (1 + 4 * U + E_FAST) / torch.sqrt((var - dvar).clamp_min(0) + eps)
    rs_lo = (1 - 4 * U - E_FAST) / torch.sqrt(var + dvar + eps)
    brs = torch.maximum(rs_hi - rs, rs - rs_lo)
    g = gamma.double() if gamma is not None else torch.ones_like(mu)
    b = beta.double() if gamma is not None else torch.zeros_like(mu)
    v = xc * rs * g + b
    fp = g.abs() * (xc.abs() * brs + dmu * rs_hi + 4 * U * (xc.abs() + dmu) * rs_hi) + 3 * U * (v.abs() + b.abs())
    y = v.clamp_min(0) if relu else v
    ref, bnd = [mu, rs, y], [dmu, brs, BF_ULP * y.abs() + 1.01 * fp]
    if running is not None:
        rm, rv = running[0].double(), running[1].double()
        n, m = float(n_total), float(BN_MOM)
        unb = var * (n / (n - 1))
        ref += [rm * (1 - m) + mu * m, rv * (1 - m) + unb * m]
        bnd += [m * dmu + 4 * U * (rm.abs() + mu.abs() * m), 1.001 * m * (n / (n - 1)) * dvar + 6 * U * (rv.abs() + unb * m)]
    return ref, bnd


def _bn_bwd_ref(dy, x, mean, rstd, gamma, beta, relu, k, exact=False):
    """float64 (sum g, sum g xhat) under the ReLU mask `gamma xhat + beta > 0`, their bounds, and what the apply's reference needs.  An element
    whose pre-activation is within its own fp32 rounding of zero may fall either side of the mask (`exact`: dyadic operands, fp32 computes the
    pre-activation without a rounding: nothing is ambiguous)."""
    x, dy, mu, rs = x.double(), dy.double(), mean.double(), rstd.double()
    g = gamma.double() if gamma is not None else torch.ones_like(mu)
    b = beta.double() if gamma is not None else torch.zeros_like(mu)
    xh = (x - mu) * rs
    pre = g * xh + b
    amb = torch.zeros_like(pre, dtype=torch.bool)
    gm = dy
    if relu:
        gm = torch.where(pre > 0, dy, torch.zeros_like(dy))
        if not exact:
            amb = pre.abs() < 8 * U * ((g * xh).abs() + b.abs())
    a = torch.where(amb, dy.abs(), torch.zeros_like(dy))
    s1, s2 = gm.sum(0), (gm * xh).sum(0)
    b1 = (k + 1) * U * gm.abs().sum(0) + a.sum(0)
    b2 = (k + 4) * U * (gm * xh).abs().sum(0) + (a * xh.abs()).sum(0)
    return (s1, s2), (b1, b2), (gm, xh, g, rs, a)


def _bn_dx_ref(parts, sums, n_total):
    """dx = gamma rstd (g - S1 / n - xhat S2 / n) in float64 from the fp32 sums the call received, and its bound."""
    gm, xh, g, rs, a = parts
    s1, s2 = sums[0].double() / n_total, sums[1].double() / n_total
    dx = g * rs * (gm - s1 - xh * s2)
    fp = (g * rs).abs() * (8 * U * (gm.abs() + s1.abs() + (xh * s2).abs()) + a)
    return dx, BF_ULP * dx.abs() + 1.01 * fp


def _col_chunks(C, step=1024):
    return [(c0, min(C, c0 + step)) for c0 in range(0, C, step)]


def _sl(t, c0, c1):
    return None if t is None else t[..., c0:c1]


def _bn_check_fwd(tag, x, got, eps, gamma, beta, relu, k, n_total=None, running=None, got_running=None):
    C = x.shape[1]
    for c0, c1 in _col_chunks(C):
        run = None if running is None else (running[0][c0:c1], running[1][c0:c1])
        ref, bnd = _bn_fwd_ref(x[:, c0:c1], eps, _sl(gamma, c0, c1), _sl(beta, c0, c1), relu, k, n_total, run)
        names = ["mean", "rstd", "y"] + (["running_mean", "running_var"] if running is not None else [])
        outs = list(got) + (list(got_running) if running is not None else [])
        for name, a, r, b in zip(names, outs, ref, bnd):
            _inside(f"{tag} {name}", _sl(a, c0, c1), r, b)


class _Bn:
    """One BatchNorm layer on the device, every buffer guarded."""

    def __init__(self, dev, x, gamma, beta):
        L = self.L = _L()
        self.dev, (self.rows, self.C) = dev, x.shape
        self.x = _put(dev, x)
        self.g = _put(dev, gamma) if gamma is not None else None
        self.b = _put(dev, beta) if gamma is not None else None
        self.nws = L.query("dig_bn_stats_workspace_bytes", self.rows, self.C) // 4

    def stats(self):
        L, C = self.L, self.C
        sums, ws = _buf(self.dev, 2 * C), _ws(self.dev, self.nws)
        L.call("dig_bn_stats", L.ptr(self.x), L.ptr(sums), L.ptr(ws), self.rows, C, L.stream())
        _sync(self.dev)
        assert _guard_ok(sums, 2 * C) and _guard_ok(ws, self.nws)
        return sums

    def apply(self, sums, n_total, relu, running=None):
        """-> (mean, rstd, y), (running_mean, running_var) or None; running: host (rm, rv) start values -> dig_bn_fwd_apply_running."""
        L, C, n = self.L, self.C, self.rows * self.C
        y, mean, rstd = _buf(self.dev, n, BF), _buf(self.dev, C), _buf(self.dev, C)
        head = (L.ptr(self.x), L.ptr(sums), cf(n_total), cf(BN_EPS), L.ptr(self.g), L.ptr(self.b), int(relu), L.ptr(y), L.ptr(mean), L.ptr(rstd))
        run = None
        if running is None:
            L.call("dig_bn_fwd_apply", *head, self.rows, C, L.stream())
        else:
            rm, rv = _put(self.dev, running[0]), _put(self.dev, running[1])
            L.call("dig_bn_fwd_apply_running", *head, cf(BN_MOM), L.ptr(rm), L.ptr(rv), self.rows, C, L.stream())
        _sync(self.dev)
        assert _guard_ok(y, n) and _guard_ok(mean, C) and _guard_ok(rstd, C)
        if running is not None:
            assert _guard_ok(rm, C) and _guard_ok(rv, C)
            run = (_get(rm, C), _get(rv, C))
        return (_get(mean, C), _get(rstd, C), _get(y, n, self.rows, C)), run

    def update_running(self, sums, n_total, running):
        L, C = self.L, self.C
        rm, rv = _put(self.dev, running[0]), _put(self.dev, running[1])
        L.call("dig_bn_update_running", L.ptr(sums), cf(n_total), cf(BN_MOM), L.ptr(rm), L.ptr(rv), C, L.stream())
        _sync(self.dev)
        assert _guard_ok(rm, C) and _guard_ok(rv, C)
        return _get(rm, C), _get(rv, C)

    def bwd_stats(self, dy, mean, rstd, relu, acc=None):
        """-> sums buffer (device), (dbeta, dgamma) or None; acc: host start values -> dig_bn_bwd_stats_acc."""
        L, C = self.L, self.C
        self.dy, self.mean, self.rstd = _put(self.dev, dy), _put(self.dev, mean), _put(self.dev, rstd)
        sums, ws = _buf(self.dev, 2 * C), _ws(self.dev, self.nws)
        head = (L.ptr(self.dy), L.ptr(self.x), L.ptr(self.mean), L.ptr(self.rstd), L.ptr(self.g), L.ptr(self.b), int(relu), L.ptr(sums))
        out = None
        if acc is None:
            L.call("dig_bn_bwd_stats", *head, L.ptr(ws), self.rows, C, L.stream())
        else:
            db, dg = _put(self.dev, acc[0]), _put(self.dev, acc[1])
            L.call("dig_bn_bwd_stats_acc", *head, L.ptr(db), L.ptr(dg), L.ptr(ws), self.rows, C, L.stream())
        _sync(self.dev)
        assert _guard_ok(sums, 2 * C) and _guard_ok(ws, self.nws)
        if acc is not None:
            assert _guard_ok(db, C) and _guard_ok(dg, C)
            out = (_get(db, C), _get(dg, C))
        return sums, out

    def bwd_apply(self, sums, n_total, relu):
        L, C, n = self.L, self.C, self.rows * self.C
        dx = _buf(self.dev, n, BF)
        L.call("dig_bn_bwd_apply", L.ptr(self.dy), L.ptr(self.x), L.ptr(self.mean), L.ptr(self.rstd), L.ptr(self.g), L.ptr(self.b), int(relu),
               L.ptr(sums), cf(n_total), L.ptr(dx), self.rows, C, L.stream())
        _sync(self.dev)
        assert _guard_ok(dx, n)
        return _get(dx, n, self.rows, C)

    def fwd_fused(self, relu, running=None):
        L, C, n = self.L, self.C, self.rows * self.C
        y, mean, rstd = _buf(self.dev, n, BF), _buf(self.dev, C), _buf(self.dev, C)
        rm = rv = None
        if running is not None:
            rm, rv = _put(self.dev, running[0]), _put(self.dev, running[1])
        L.call("dig_bn_fwd_fused", L.ptr(self.x), cf(BN_EPS), L.ptr(self.g), L.ptr(self.b), int(relu), L.ptr(y), L.ptr(mean), L.ptr(rstd), cf(BN_MOM),
               L.ptr(rm), L.ptr(rv), self.rows, C, L.stream())
        _sync(self.dev)
        assert _guard_ok(y, n) and _guard_ok(mean, C) and _guard_ok(rstd, C) and (rm is None or (_guard_ok(rm, C) and _guard_ok(rv, C)))
        return (_get(mean, C), _get(rstd, C), _get(y, n, self.rows, C)), (None if rm is None else (_get(rm, C), _get(rv, C)))

    def bwd_fused(self, dy, mean, rstd, relu, acc=None):
        L, C, n = self.L, self.C, self.rows * self.C
        self.dy, self.mean, self.rstd = _put(self.dev, dy), _put(self.dev, mean), _put(self.dev, rstd)
        dx = _buf(self.dev, n, BF)
        db = dg = None
        if acc is not None:
            db, dg = _put(self.dev, acc[0]), _put(self.dev, acc[1])
        L.call("dig_bn_bwd_fused", L.ptr(self.dy), L.ptr(self.x), L.ptr(self.mean), L.ptr(self.rstd), L.ptr(self.g), L.ptr(self.b), int(relu),
               L.ptr(db), L.ptr(dg), L.ptr(dx), self.rows, C, L.stream())
        _sync(self.dev)
        assert _guard_ok(dx, n) and (db is None or (_guard_ok(db, C) and _guard_ok(dg, C)))
        return _get(dx, n, self.rows, C), (None if db is None else (_get(db, C), _get(dg, C)))


def _bn_shapes():
    return [(r, c) for c in BN_C for r in BN_ROWS] + [BN_BIG]


def _doubled(dev, sums, n):
    return _put(dev, _get(sums, n) * 2)


@pytest.mark.parametrize("rows,C", _bn_shapes())
def test_batchnorm_three_launch_vs_fp64(abi_dev, rows, C):
    """dig_bn_stats -> dig_bn_fwd_apply / _running (and dig_bn_update_running), dig_bn_bwd_stats / _acc -> dig_bn_bwd_apply, every option, with
    n_total = rows and with the sums doubled and n_total = 2 rows (the two-rank form: the same bits)."""
    dev, be = abi_dev, _backend(abi_dev)
    k = _bn_adds(be, rows, C)
    x = _bn_cols(rows, C, rows + C)
    gamma, beta, rm0, rv0 = _bn_params(C)
    gen = torch.Generator().manual_seed(rows * 3 + C)
    dy = torch.randn(rows, C, generator=gen).bfloat16()
    acc0 = (torch.randn(C, generator=gen), torch.randn(C, generator=gen))
    x64 = x.double()
    ref0, _ = _bn_fwd_ref(x, BN_EPS, None, None, 0, k)
    mean_in, rstd_in = ref0[0].float(), ref0[1].float()
    print(f"bn {be} rows {rows} C {C}: k = {k}, largest kappa = E[x^2] / (var + eps) = {float(((x64 * x64).mean(0) / (x64.var(0, unbiased=False) + BN_EPS)).max()):.3g}")
    for affine, relu in BN_OPTS:
        bn = _Bn(dev, x, gamma if affine else None, beta if affine else None)
        ga, ba = (gamma, beta) if affine else (None, None)
        tag = f"bn {be} rows {rows} C {C} affine {int(affine)} relu {relu}"
        sums = bn.stats()
        s = _get(sums, 2 * C, 2, C)
        _inside(tag + " sum x", s[0], x64.sum(0), k * U * x64.abs().sum(0))
        _inside(tag + " sum x^2", s[1], (x64 * x64).sum(0), (k + 1) * U * (x64 * x64).sum(0))
        base = None
        for mult in (1, 2):
            n_total = float(rows * mult)
            sm = sums if mult == 1 else _doubled(dev, sums, 2 * C)
            got, _ = bn.apply(sm, n_total, relu)
            _bn_check_fwd(f"{tag} n_total {int(n_total)}", x, got, BN_EPS, ga, ba, relu, k)
            if base is None:
                base = got
            assert all(torch.equal(a, b) for a, b in zip(got, base)), tag          # sums and n_total doubled: the same bits
            if n_total > 1:
                got_r, run = bn.apply(sm, n_total, relu, running=(rm0, rv0))
                assert all(torch.equal(a, b) for a, b in zip(got_r, base)), tag
                _bn_check_fwd(f"{tag} n_total {int(n_total)} running", x, got_r, BN_EPS, ga, ba, relu, k, n_total, (rm0, rv0), run)
                upd = bn.update_running(sm, n_total, (rm0, rv0))
                # one expression, two kernels: the compiler may contract a product and a sum in one and not in the other, so each is within
                # its own roundings of the expression's exact value on the fp32 sums they both read, and the two within twice that
                s64 = _get(sm, 2 * C, 2, C).double() / n_total
                unb = (s64[1] - s64[0] * s64[0]).clamp_min(0) * (n_total / (n_total - 1))
                m = float(BN_MOM)
                _inside(f"{tag} n_total {int(n_total)} running_mean against dig_bn_update_running", run[0], upd[0],
                        2 * 4 * U * (rm0.double().abs() + s64[0].abs() * m))
                _inside(f"{tag} n_total {int(n_total)} running_var against dig_bn_update_running", run[1], upd[1],
                        2 * (5 * U * s64[1] * (n_total / (n_total - 1)) * m + 6 * U * (rv0.double().abs() + unb * m)))
        # backward
        (r1, r2), (b1, b2), parts = _bn_bwd_ref(dy, x, mean_in, rstd_in, ga, ba, relu, k)
        bs, _ = bn.bwd_stats(dy, mean_in, rstd_in, relu)
        t = _get(bs, 2 * C, 2, C)
        _inside(tag + " sum g", t[0], r1, b1)
        _inside(tag + " sum g xhat", t[1], r2, b2)
        bs2, acc = bn.bwd_stats(dy, mean_in, rstd_in, relu, acc=acc0)
        assert torch.equal(_get(bs2, 2 * C), _get(bs, 2 * C)), tag
        assert torch.equal(acc[0], acc0[0] + t[0]) and torch.equal(acc[1], acc0[1] + t[1]), tag
        dx_base = None
        for mult in (1, 2):
            n_total = float(rows * mult)
            sm = bs if mult == 1 else _doubled(dev, bs, 2 * C)
            dx = bn.bwd_apply(sm, n_total, relu)
            ref, bnd = _bn_dx_ref(parts, t, float(rows))
            _inside(f"{tag} n_total {int(n_total)} dx", dx, ref, bnd)
            if dx_base is None:
                dx_base = dx
            assert torch.equal(dx, dx_base), tag


def _bn_exact_inputs(rows, C, seed):
    """Dyadic everything: integer x and dy, integer means, power-of-two rstd, quarter gamma / beta; column 0 has gamma 1, beta 0, mean 0, rstd 1,
    so every x == 0 there has a pre-activation of exactly 0 (the mask is `> 0`: its dy does not count)."""
    g = torch.Generator().manual_seed(seed)
    x, dy = _ints(g, rows, C).bfloat16(), _ints(g, rows, C).bfloat16()
    x[::3, 0] = 0
    dy[:, 0] = dy[:, 0].abs() + 1
    mean = _ints(g, C, lo=-2, hi=2)
    rstd = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (C,), generator=g)]
    gamma, beta = _quarters(g, C), _quarters(g, C)
    mean[0], rstd[0], gamma[0], beta[0] = 0.0, 1.0, 1.0, 0.0
    acc = (_quarters(g, C), _quarters(g, C))
    return x, dy, mean, rstd, gamma, beta, acc


def _bn_exact_ref(x, dy, mean, rstd, gamma, beta, relu):
    xh = (x.double() - mean.double()) * rstd.double()
    g = dy.double()
    if relu:
        pre = (gamma.double() * xh + beta.double()) if gamma is not None else xh
        g = torch.where(pre > 0, g, torch.zeros_like(g))
    return g.sum(0), (g * xh).sum(0)


@pytest.mark.parametrize("rows,C", _bn_shapes())
def test_batchnorm_sums_are_exact_on_integers(abi_dev, rows, C):
    """sums[2, C] of dig_bn_stats and of dig_bn_bwd_stats / _acc, and dbeta / dgamma, equal the float64 sums bit for bit on dyadic data, with
    pre-activations that are exactly zero under the ReLU mask."""
    dev = abi_dev
    x, dy, mean, rstd, gamma, beta, acc0 = _bn_exact_inputs(rows, C, rows + 7 * C)
    x64 = x.double()
    for affine, relu in BN_OPTS:
        ga, ba = (gamma, beta) if affine else (None, None)
        bn = _Bn(dev, x, ga, ba)
        s = _get(bn.stats(), 2 * C, 2, C)
        assert torch.equal(s[0].double(), x64.sum(0)) and torch.equal(s[1].double(), (x64 * x64).sum(0)), (rows, C)
        w1, w2 = _bn_exact_ref(x, dy, mean, rstd, ga, ba, relu)
        bs, _ = bn.bwd_stats(dy, mean, rstd, relu)
        t = _get(bs, 2 * C, 2, C)
        assert torch.equal(t[0].double(), w1) and torch.equal(t[1].double(), w2), (rows, C, affine, relu)
        bs2, acc = bn.bwd_stats(dy, mean, rstd, relu, acc=acc0)
        assert torch.equal(_get(bs2, 2 * C), _get(bs, 2 * C))
        assert torch.equal(acc[0].double(), acc0[0].double() + w1) and torch.equal(acc[1].double(), acc0[1].double() + w2), (rows, C, affine, relu)
        if relu and not affine and rows > 1:
            assert float(t[0][0]) == float(dy.double()[:, 0][x64[:, 0] > 0].sum())          # column 0: the zeros of x carry dy >= 1 and are masked
        dx = bn.bwd_apply(bs, float(rows), relu)
        _, _, parts = _bn_bwd_ref(dy, x, mean, rstd, ga, ba, relu, 1, exact=True)
        ref, bnd = _bn_dx_ref(parts, t, float(rows))
        _inside(f"bn exact rows {rows} C {C} affine {int(affine)} relu {relu} dx", dx, ref, bnd)


def test_batchnorm_three_launch_refusals_and_sizes(abi_dev):
    dev, be = abi_dev, _backend(abi_dev)
    L = _L()
    for rows, C in [(1, 8), (1000, 64), (1000, 2056), BN_BIG, (10 ** 6, 4096)]:
        want = -(-rows // _bn_rpb(rows, C)) if be == "hip" else -(-rows // 64)
        assert L.query("dig_bn_stats_workspace_bytes", rows, C) == want * 2 * C * 4
    rows, C = 4, 16
    x = _bn_cols(rows, C, 1)
    gamma, beta, rm0, rv0 = _bn_params(C)
    bn = _Bn(dev, x, gamma, beta)
    sums = bn.stats()
    y, mean, rstd, dx = _buf(dev, rows * C, BF), _buf(dev, C), _buf(dev, C), _buf(dev, rows * C, BF)
    rm, rv, db, dg = _buf(dev, C), _buf(dev, C), _buf(dev, C), _buf(dev, C)
    s2, ws = _buf(dev, 2 * C + 4), _ws(dev, bn.nws)
    off = lambda t: ctypes.c_void_p(t.data_ptr() + 4)                           # a view that starts one float into the buffer
    P = L.ptr

    def fwd(sums_p=P(sums), n=float(rows), g=P(bn.g), b=P(bn.b), c=C, rmp=P(rm), rvp=P(rv)):
        return (P(bn.x), sums_p, cf(n), cf(BN_EPS), g, b, 1, P(y), P(mean), P(rstd), cf(BN_MOM), rmp, rvp, rows, c, L.stream())

    _refused(ARG, "dig_bn_stats", P(bn.x), P(s2), P(ws), rows, 12, L.stream())
    _refused(ARG, "dig_bn_fwd_apply_running", *fwd(c=12))
    _refused(ARG, "dig_bn_fwd_apply_running", *fwd(n=1.0))                       # running statistics need n_total > 1
    _refused(ARG, "dig_bn_fwd_apply_running", *fwd(rvp=None))
    _refused(ARG, "dig_bn_fwd_apply_running", *fwd(b=None))                      # only one of gamma / beta
    _refused(ARG, "dig_bn_fwd_apply_running", *fwd(g=None))
    _refused(ALIGN, "dig_bn_fwd_apply_running", *fwd(sums_p=off(s2)))
    _refused(ARG, "dig_bn_update_running", P(sums), cf(1.0), cf(BN_MOM), P(rm), P(rv), C, L.stream())
    bn.dy, bn.mean, bn.rstd = _put(dev, x), _put(dev, torch.zeros(C + 4)), _put(dev, torch.ones(C + 4))
    bhead = (P(bn.dy), P(bn.x), P(bn.mean), P(bn.rstd), P(bn.g), P(bn.b), 1, P(s2))
    _refused(ARG, "dig_bn_bwd_stats_acc", *bhead, P(db), None, P(ws), rows, C, L.stream())      # only one of the accumulators
    _refused(ARG, "dig_bn_bwd_stats_acc", *bhead, None, P(dg), P(ws), rows, C, L.stream())
    _refused(ARG, "dig_bn_bwd_stats", *bhead, P(ws), rows, 12, L.stream())
    _refused(ALIGN, "dig_bn_bwd_stats", P(bn.dy), P(bn.x), off(bn.mean), P(bn.rstd), P(bn.g), P(bn.b), 1, P(s2), P(ws), rows, C, L.stream())
    _refused(ALIGN, "dig_bn_bwd_apply", P(bn.dy), P(bn.x), P(bn.mean), P(bn.rstd), P(bn.g), P(bn.b), 1, off(s2), cf(rows), P(dx), rows, C, L.stream())
    _refused(ARG, "dig_bn_bwd_apply", P(bn.dy), P(bn.x), P(bn.mean), P(bn.rstd), P(bn.g), P(bn.b), 1, P(sums), cf(rows), P(dx), rows, 12, L.stream())
    _sync(dev)
    assert all(_untouched(t) for t in (y, mean, rstd, dx, rm, rv, db, dg, s2))


# ------------------------------------------------------------------------------------------------ the one-launch path
BNF_ROWS = [2, 63, 64, 65, 1000, 4096]
BNF_C = [256, 288, 4096]


@pytest.mark.parametrize("C", BNF_C)
@pytest.mark.parametrize("rows", BNF_ROWS)
def test_batchnorm_fused_vs_fp64_and_three_launch(abi_dev, rows, C):
    """dig_bn_fwd_fused / dig_bn_bwd_fused against float64 and against the three-launch path (statistics within the sum of the two paths' bounds)."""
    dev, be = abi_dev, _backend(abi_dev)
    L = _L()
    assert L.query("dig_bn_fused_supported", rows, C) == 1
    kf, k3 = _bn_adds(be, rows, C, fused=True), _bn_adds(be, rows, C)
    x = _bn_cols(rows, C, rows + C + 1)
    gamma, beta, rm0, rv0 = _bn_params(C)
    gen = torch.Generator().manual_seed(rows * 5 + C)
    dy = torch.randn(rows, C, generator=gen).bfloat16()
    acc0 = (torch.randn(C, generator=gen), torch.randn(C, generator=gen))
    opts = BN_OPTS if rows * C < (1 << 22) else [(True, 1)]
    for affine, relu in opts:
        ga, ba = (gamma, beta) if affine else (None, None)
        bn = _Bn(dev, x, ga, ba)
        tag = f"bn fused {be} rows {rows} C {C} affine {int(affine)} relu {relu}"
        got, run = bn.fwd_fused(relu, running=(rm0, rv0))
        _bn_check_fwd(tag, x, got, BN_EPS, ga, ba, relu, kf, float(rows), (rm0, rv0), run)
        plain, _ = bn.fwd_fused(relu)
        assert all(torch.equal(a, b) for a, b in zip(got, plain)), tag          # the running statistics do not change the outputs
        three, _ = bn.apply(bn.stats(), float(rows), relu)
        for c0, c1 in _col_chunks(C):
            _, bf = _bn_fwd_ref(x[:, c0:c1], BN_EPS, None, None, 0, kf)
            _, b3 = _bn_fwd_ref(x[:, c0:c1], BN_EPS, None, None, 0, k3)
            for i, name in enumerate(("mean", "rstd")):
                _inside(f"{tag} {name} against three-launch", got[i][c0:c1], three[i][c0:c1], bf[i] + b3[i])
        mean_in, rstd_in = got[0], got[1]                                       # the backward of this forward: its own statistics are the inputs
        dx, acc = bn.bwd_fused(dy, mean_in, rstd_in, relu, acc=acc0)
        dx2, _ = bn.bwd_fused(dy, mean_in, rstd_in, relu)
        assert torch.equal(dx, dx2), tag
        for c0, c1 in _col_chunks(C):
            sl = lambda t: _sl(t, c0, c1)
            (r1, r2), (b1, b2), parts = _bn_bwd_ref(sl(dy), sl(x), sl(mean_in), sl(rstd_in), sl(ga), sl(ba), relu, kf)
            _inside(f"{tag} dbeta", sl(acc[0]), sl(acc0[0]).double() + r1, b1 + 2 * U * (sl(acc0[0]).double().abs() + r1.abs()))
            _inside(f"{tag} dgamma", sl(acc[1]), sl(acc0[1]).double() + r2, b2 + 2 * U * (sl(acc0[1]).double().abs() + r2.abs()))
            # dx uses the kernel's own fp32 sums, which it does not return: the reference takes the float64 sums, the bound their error
            gm, xh, g, rs, a = parts
            ref, bnd = _bn_dx_ref(parts, torch.stack([r1, r2]), float(rows))
            bnd = bnd + 1.01 * (g * rs).abs() * (b1 / rows + xh.abs() * b2 / rows)
            _inside(f"{tag} dx", sl(dx), ref, bnd)


@pytest.mark.parametrize("rows", [2, 64, 4096])
def test_batchnorm_fused_is_exact_on_integers(abi_dev, rows):
    """rows a power of two, integer x: the fused forward's mean equals the float64 mean bit for bit; dyadic backward inputs: dbeta / dgamma
    equal the float64 sums bit for bit, exactly-zero pre-activations under the mask included."""
    dev, C = abi_dev, 288
    x, dy, mean, rstd, gamma, beta, acc0 = _bn_exact_inputs(rows, C, rows + 11)
    for affine, relu in BN_OPTS:
        ga, ba = (gamma, beta) if affine else (None, None)
        bn = _Bn(dev, x, ga, ba)
        got, _ = bn.fwd_fused(relu)
        assert torch.equal(got[0].double(), x.double().mean(0)), (rows, affine, relu)
        w1, w2 = _bn_exact_ref(x, dy, mean, rstd, ga, ba, relu)
        _, acc = bn.bwd_fused(dy, mean, rstd, relu, acc=acc0)
        assert torch.equal(acc[0].double(), acc0[0].double() + w1) and torch.equal(acc[1].double(), acc0[1].double() + w2), (rows, affine, relu)


def test_batchnorm_fused_refusals(abi_dev):
    """Unsupported shapes and misaligned parameter vectors (a view one float into a buffer) are refused before anything is launched."""
    dev = abi_dev
    L = _L()
    P = L.ptr
    off = lambda t: ctypes.c_void_p(t.data_ptr() + 4)
    for rows, C in [(1, 256), (4097, 256), (8, 224), (8, 264)]:
        assert L.query("dig_bn_fused_supported", rows, C) == 0
    rows, C = 8, 256
    x = _bn_cols(rows, C, 2)
    xs = _put(dev, _bn_cols(8, 264, 2))                                         # large enough for every refused shape but rows 4097, which reads nothing
    gamma, beta, rm0, rv0 = _bn_params(C)
    g, b = _put(dev, torch.cat([gamma, gamma[:4]])), _put(dev, torch.cat([beta, beta[:4]]))
    y, dx = _buf(dev, 8 * 264, BF), _buf(dev, 8 * 264, BF)
    mean, rstd, rm, rv, db, dg = (_buf(dev, C + 8) for _ in range(6))
    mi, ri = _put(dev, torch.zeros(C + 4)), _put(dev, torch.ones(C + 4))

    def fwd(rows=rows, C=C, g=P(g), b=P(b), mean=P(mean), rstd=P(rstd), rm=P(rm), rv=P(rv)):
        return (P(xs), cf(BN_EPS), g, b, 1, P(y), mean, rstd, cf(BN_MOM), rm, rv, rows, C, L.stream())

    def bwd(rows=rows, C=C, g=P(g), b=P(b), mean=P(mi), rstd=P(ri), db=P(db), dg=P(dg)):
        return (P(xs), P(xs), mean, rstd, g, b, 1, db, dg, P(dx), rows, C, L.stream())

    for r, c in [(1, 256), (4097, 256), (8, 224), (8, 264)]:
        _refused(UNSUP, "dig_bn_fwd_fused", *fwd(rows=r, C=c))
        _refused(UNSUP, "dig_bn_bwd_fused", *bwd(rows=r, C=c))
    for kw in (dict(g=off(g)), dict(b=off(b)), dict(mean=off(mean)), dict(rstd=off(rstd)), dict(rm=off(rm)), dict(rv=off(rv))):
        _refused(ALIGN, "dig_bn_fwd_fused", *fwd(**kw))
    for kw in (dict(g=off(g)), dict(b=off(b)), dict(mean=off(mi)), dict(rstd=off(ri)), dict(db=off(db)), dict(dg=off(dg))):
        _refused(ALIGN, "dig_bn_bwd_fused", *bwd(**kw))
    _refused(ARG, "dig_bn_fwd_fused", *fwd(b=None))
    _refused(ARG, "dig_bn_fwd_fused", *fwd(rv=None))
    _refused(ARG, "dig_bn_bwd_fused", *bwd(dg=None))
    _sync(dev)
    assert all(_untouched(t) for t in (y, dx, mean, rstd, rm, rv, db, dg))
    L.call("dig_bn_fwd_fused", *fwd())                                          # the aligned call runs
    L.call("dig_bn_bwd_fused", *bwd())
    _sync(dev)
    assert not _untouched(y) and not _untouched(dx) and _guard_ok(y, rows * C) and _guard_ok(dx, rows * C)


# ================================================================================================ L2 normalise
L2_EPS = f32(1e-12)


def _row_adds(backend, C):
    """Additions an element passes through in a row sum of l2norm: lane strides of 64 and six shuffle levels, or one chain."""
    return (-(-C // 64) - 1 + 6) if backend == "hip" else C - 1


def _l2_rows(n, C, seed):
    """Row kinds by row index mod 5: randn, all zero, norm 1e-13 (below eps), all 1e18, randn * 3."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, C, generator=g)
    k = torch.arange(n) % 5
    x[k == 1] = 0
    tiny = x[k == 2]
    x[k == 2] = tiny / tiny.norm(dim=1, keepdim=True) * 1e-13
    x[k == 3] = 1e18
    x[k == 4] *= 3
    return x, k


@pytest.mark.parametrize("C", [1, 65, 256])
@pytest.mark.parametrize("n", [1, 5, 512])
def test_l2norm_vs_fp64(abi_dev, n, C):
    dev, be = abi_dev, _backend(abi_dev)
    L = _L()
    na = _row_adds(be, C)
    x, kind = _l2_rows(n, C, n + C)
    xd, y, inv = _put(dev, x), _buf(dev, n * C), _buf(dev, n)
    L.call("dig_l2norm_fwd", L.ptr(xd), L.ptr(y), L.ptr(inv), n, C, cf(L2_EPS), L.stream())
    _sync(dev)
    assert _guard_ok(y, n * C) and _guard_ok(inv, n)
    y, inv = _get(y, n * C, n, C), _get(inv, n)
    x64 = x.double()
    inv64 = 1.0 / x64.norm(dim=1).clamp_min(L2_EPS)
    y64 = x64 * inv64[:, None]
    rel = (na + 6) * U
    tag = f"l2norm {be} n {n} C {C}"
    _inside(tag + " inv_norm", inv, inv64, rel * inv64)
    _inside(tag + " y", y, y64, (rel + U) * y64.abs())
    clamp = f32(np.float32(1) / np.float32(L2_EPS))
    assert bool((y[kind == 1] == 0).all()) and bool((inv[(kind == 1) | (kind == 2)] == clamp).all())       # the eps clamp: inv_norm = 1 / eps exactly
    # a row of 1e18: the squares sum to C 1e36 < 3.4e38 for C <= 340, so nothing overflows and F.normalize in fp32 gives x / |x| as well
    if bool((kind == 3).any()):
        t = torch.nn.functional.normalize(x[kind == 3], dim=1, eps=L2_EPS)
        assert bool(torch.isfinite(t).all())
        _inside(tag + " against F.normalize(fp32) on the 1e18 rows", y[kind == 3], t, (rel + (C + 6) * U) * y64[kind == 3].abs())
    # backward: dx = (dy - y <y, dy>) inv_norm from fp32 (dy, y, inv_norm)
    dy = torch.randn(n, C, generator=torch.Generator().manual_seed(n * C))
    yin, invin = y64.float(), inv64.float()
    dyd, yd, invd, dx = _put(dev, dy), _put(dev, yin), _put(dev, invin), _buf(dev, n * C)
    L.call("dig_l2norm_bwd", L.ptr(dyd), L.ptr(yd), L.ptr(invd), L.ptr(dx), n, C, L.stream())
    _sync(dev)
    assert _guard_ok(dx, n * C)
    dx = _get(dx, n * C, n, C)
    s = (yin.double() * dy.double()).sum(1, keepdim=True)
    es = (na + 2) * U * (yin.double() * dy.double()).abs().sum(1, keepdim=True)
    ref = (dy.double() - yin.double() * s) * invin.double()[:, None]
    bnd = invin.double()[:, None] * (yin.double().abs() * es + 4 * U * (dy.double().abs() + (yin.double() * s).abs()))
    _inside(tag + " dx", dx, ref, bnd)
    z = kind == 1                                                               # the all-zero rows: the clamp has no gradient of its own, dx = dy / eps
    if bool(z.any()):
        _inside(tag + " dx of a zero row against dy / eps", dx[z], dy[z].double() / L2_EPS, 3 * U * dy[z].double().abs() / L2_EPS)


# ================================================================================================ the fp32 GEMM
def _sgemm_per(R, splits):
    return -(-(-(-R // splits)) // 64) * 64


def _sgemm(dev, A, B, I, J, R, trans_b, alpha, splits, pad=8):
    """-> C [splits, I, J] as the library wrote it; A / B / C carry `pad` poisoned columns behind every row, C also the guard."""
    L = _L()
    lda, ldb, ldc = R + pad, (J if trans_b else R) + pad, J + pad
    Ap, Bp = torch.full((I, lda), POISON), torch.full(B.shape[:1] + (ldb,), POISON)
    Ap[:, :R] = A
    Bp[:, :B.shape[1]] = B
    Ad, Bd, Cd = _put(dev, Ap), _put(dev, Bp), _buf(dev, splits * I * ldc)
    L.call("dig_sgemm", L.ptr(Ad), L.ptr(Bd), L.ptr(Cd), I, J, R, lda, ldb, ldc, int(trans_b), cf(alpha), splits, L.stream())
    _sync(dev)
    assert _guard_ok(Cd, splits * I * ldc)
    C = _get(Cd, splits * I * ldc, splits, I, ldc)
    assert bool((C[:, :, J:] == POISON).all())
    return C[:, :, :J]


def _sgemm_ref(A, B, R, trans_b, alpha, splits):
    """float64 slabs [splits, I, J] and sum |a| |b| per slab."""
    per = _sgemm_per(R, splits)
    A, B = A.double(), (B.double() if trans_b else B.double().t())
    out, mag = [], []
    for s in range(splits):
        k0, k1 = s * per, min(R, (s + 1) * per)
        out.append(alpha * (A[:, k0:k1] @ B[k0:k1]))
        mag.append(abs(alpha) * (A[:, k0:k1].abs() @ B[k0:k1].abs()))
    return torch.stack(out), torch.stack(mag), per


SGEMM_CASES = [(1, 1, 1, 1), (33, 31, 65, 1), (100, 520, 200, 1), (64, 64, 256, 1), (33, 31, 200, 2), (33, 31, 130, 3), (64, 64, 256, 4)]


@pytest.mark.parametrize("alpha", [1.0, 5.0])
@pytest.mark.parametrize("trans_b", [0, 1])
@pytest.mark.parametrize("I,J,R,splits", SGEMM_CASES)
def test_sgemm_vs_fp64(abi_dev, I, J, R, splits, trans_b, alpha):
    """Integer operands: every slab equals the float64 product of its K range bit for bit; random operands: within (K + 2) u alpha sum |a| |b|."""
    dev, be = abi_dev, _backend(abi_dev)
    g = torch.Generator().manual_seed(I + J + R + splits)
    bshape = (R, J) if trans_b else (J, R)
    A, B = _ints(g, I, R), _ints(g, *bshape)
    ref, _, per = _sgemm_ref(A, B, R, trans_b, alpha, splits)
    assert -(-R // per) == splits
    assert torch.equal(_sgemm(dev, A, B, I, J, R, trans_b, alpha, splits).double(), ref), (I, J, R, splits)
    A, B = torch.randn(I, R, generator=g), torch.randn(*bshape, generator=g)
    ref, mag, per = _sgemm_ref(A, B, R, trans_b, alpha, splits)
    _inside(f"sgemm {be} {I}x{J}x{R} splits {splits} tb {trans_b} alpha {alpha}", _sgemm(dev, A, B, I, J, R, trans_b, alpha, splits), ref,
            (min(per, R) + 2) * U * mag)


def test_sgemm_refusals(abi_dev):
    dev = abi_dev
    L = _L()
    A, B, C = _put(dev, torch.ones(4, 128)), _put(dev, torch.ones(4, 128)), _buf(dev, 3 * 16)
    _refused(ARG, "dig_sgemm", L.ptr(A), L.ptr(B), L.ptr(C), 4, 4, 128, 128, 128, 4, 0, cf(1.0), 3, L.stream())      # ceil(R / per) == r_splits fails: per = 64
    _refused(ARG, "dig_sgemm", L.ptr(A), L.ptr(B), L.ptr(C), 4, 4, 128, 128, 128, 4, 0, cf(1.0), 0, L.stream())
    _refused(ARG, "dig_sgemm", L.ptr(A), L.ptr(B), L.ptr(C), 0, 4, 128, 128, 128, 4, 0, cf(1.0), 1, L.stream())
    _sync(dev)
    assert _untouched(C)


# ================================================================================================ the InfoNCE row kernel
CE_M = [5, 6, 255, 256, 257, 1000]
CE_TIES = [(0, 3), (1, 2), (4, 3), (5, 0), (0, 6)]                  # (entries above the label's logit, entries equal to it), rows 2 .. 6


def _ce_adds(backend, m):
    return (-(-m // 256) - 1 + 6 + 3) if backend == "hip" else m - 1


def _ce_logits(n, m, off, seed):
    """Row kinds: 0 randn * 5; 1 a row of +-80; 2 .. 6 the label's logit 1.0 with CE_TIES entries above it / equal to it, the rest below."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(n, m, generator=g) * 5
    for i in range(1, n):
        label = i + off
        if i == 1:
            z[i] = torch.where(torch.rand(m, generator=g) < 0.5, 80.0, -80.0)
            continue
        above, ties = CE_TIES[(i - 2) % len(CE_TIES)]
        above = min(above, m - 1)
        ties = min(ties, m - 1 - above)
        z[i] = torch.randn(m, generator=g) * 0.5 - 3.0
        others = [j for j in range(m) if j != label]
        perm = torch.randperm(len(others), generator=g).tolist()
        for q in range(above):
            z[i, others[perm[q]]] = 2.0 + 0.25 * q
        for q in range(above, above + ties):
            z[i, others[perm[q]]] = 1.0
        z[i, label] = 1.0
    return z


def _ce_ref(z, off, gscale, backend):
    """float64 (sum of losses, #top1, #top5, dlogits) with the kernel's rule rank = #{z > z_label} (top-1: rank 0, top-5: rank < 5; entries equal
    to the label's logit do not count, whatever order a sort would give them), and the bounds."""
    n, m = z.shape
    na = _ce_adds(backend, m)
    z = z.double()
    lab = torch.arange(n) + off
    zl = z[torch.arange(n), lab]
    mx = z.max(1).values
    e = torch.exp(z - mx[:, None])
    s = e.sum(1)
    lse = mx + torch.log(s)
    p = e / s[:, None]
    one = torch.zeros_like(z)
    one[torch.arange(n), lab] = 1
    rank = (z > zl[:, None]).sum(1)
    w = (p * (z - mx[:, None]).abs()).sum(1)
    rel_s = (na + 4) * U + 3 * U * w + E_FAST
    li = lse - zl
    b_loss = (rel_s + E_FAST + 3 * U * (mx.abs() + lse.abs() + zl.abs())).sum() + (n + 1) * U * li.abs().sum()
    # (2^-125: a probability below the smallest normal fp32 number comes out as a subnormal or as 0, e.g. exp(-160) of the +-80 row)
    b_d = gscale * (p * (rel_s[:, None] + 3 * U * (z - mx[:, None]).abs() + 4 * U + E_FAST) + 2 * U * (p - one).abs() + 2.0 ** -125)
    return li.sum(), float((rank == 0).sum()), float((rank < 5).sum()), gscale * (p - one), b_loss, b_d


def _ce_run(dev, z, off, gscale, start, ws=None):
    L = _L()
    n, m = z.shape
    zd, out = _put(dev, z), _put(dev, start)
    if ws is None:
        L.call("dig_ce_rows", L.ptr(zd), n, m, off, cf(gscale), L.ptr(out), L.stream())
    else:
        L.call("dig_ce_rows_ws", L.ptr(zd), n, m, off, cf(gscale), L.ptr(out), L.ptr(ws), L.stream())
    _sync(dev)
    assert _guard_ok(zd, n * m) and _guard_ok(out, 3)
    return _get(out, 3), _get(zd, n * m, n, m)


@pytest.mark.parametrize("m", CE_M)
@pytest.mark.parametrize("n", [1, 7])
def test_ce_rows_vs_fp64(abi_dev, n, m):
    dev, be = abi_dev, _backend(abi_dev)
    if n > m:
        L = _L()
        z, out = _put(dev, torch.zeros(n, m)), _buf(dev, 3)
        _refused(ARG, "dig_ce_rows", L.ptr(z), n, m, 0, cf(1.0), L.ptr(out), L.stream())          # label_offset + n > m
        _refused(ARG, "dig_ce_rows_ws", L.ptr(z), n, m, 0, cf(1.0), L.ptr(out), None, L.stream())
        _refused(ARG, "dig_ce_rows", L.ptr(z), 3, m, m - 2, cf(1.0), L.ptr(out), L.stream())
        _sync(dev)
        assert _untouched(out) and bool((z[:n * m] == 0).all())
        n = m                                                                    # m = 5 / 6: as many rows as fit, so the tie rows run at these widths too
    gscale, start = f32(0.25), torch.tensor([0.5, 2.0, 3.0])
    for off in sorted({0, m - n}):
        z = _ce_logits(n, m, off, n + m + off)
        loss, top1, top5, d64, b_loss, b_d = _ce_ref(z, off, gscale, be)
        out, d = _ce_run(dev, z, off, gscale, start)
        tag = f"ce_rows {be} n {n} m {m} offset {off}"
        _inside(tag + " loss", out[:1], (0.5 + loss).reshape(1), (b_loss + U * (0.5 + loss.abs())).reshape(1))
        assert float(out[1]) == 2.0 + top1 and float(out[2]) == 3.0 + top5, (tag, out, top1, top5)
        if m == 5:
            assert top5 == n                                                    # four other entries: every row is a top-5 hit
        if m == 6 and n == 6:
            assert top5 == n - 1                                                # row 5 has all five other entries above its label
        _inside(tag + " dlogits", d, d64, b_d)
        _inside(tag + " dlogits row sums", d.double().sum(1), torch.zeros(n, dtype=F64), b_d.sum(1))
        ws = _put(dev, torch.zeros(1 + 3 * n))
        first = _ce_run(dev, z, off, gscale, start, ws)
        second = _ce_run(dev, z, off, gscale, start, ws)
        assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1]), tag
        assert int(_get(ws, 1).view(torch.int32)[0]) == 0 and _guard_ok(ws, 1 + 3 * n)              # the ticket word is left at 0
        assert torch.equal(first[1], d) and torch.equal(first[0][1:], out[1:]), tag
        _inside(tag + " loss with a workspace against the plain form", first[0][:1], out[:1], (2 * b_loss + 2 * U * (0.5 + loss.abs())).reshape(1))
        _inside(tag + " loss with a workspace", first[0][:1], (0.5 + loss).reshape(1), (b_loss + U * (0.5 + loss.abs())).reshape(1))


# ================================================================================================ MSE
MSE_CASES = [(1, 1, 1, 1), (895, 48, 64, 64), (300, 48, 48, 56), (2000, 48, 48, 48)]          # the last: M ld_dpred > 65536, the 256-block grid strides


def _mse_adds(M, ldd):
    total = M * ldd
    return -(-total // 65536) + 6 + 3 + 2 + min(256, -(-total // 256))        # a thread's walk, the wave, the four waves, 1 / count, the blocks


@pytest.mark.parametrize("M,C,ldp,ldd", MSE_CASES)
def test_mse_vs_fp64(abi_dev, M, C, ldp, ldd):
    dev, be = abi_dev, _backend(abi_dev)
    L = _L()
    g = torch.Generator().manual_seed(M + C)
    pred = torch.full((M, ldp), POISON)
    pred[:, :C] = torch.randn(M, C, generator=g)
    target = torch.randn(M, C, generator=g)
    gscale, start = f32(0.7), 0.5
    df = pred[:, :C].double() - target.double()
    inv = 1.0 / (M * C)
    loss64 = start + (df * df).sum() * inv
    g64 = torch.zeros(M, ldd, dtype=F64)
    g64[:, :C] = 2.0 * df * inv * gscale
    pd, td = _put(dev, pred), _put(dev, target)
    tag = f"mse {be} M {M} C {C} ld {ldp} / {ldd}"

    def run(name, with_loss, with_grad, ws=None):
        loss = _put(dev, torch.tensor([start]))
        dp = _buf(dev, M * ldd, BF)
        tail = (L.ptr(ws), L.stream()) if name.endswith("_ws") else (L.stream(),)
        L.call(name, L.ptr(pd), ldp, L.ptr(td), M, C, cf(gscale), L.ptr(loss) if with_loss else None, L.ptr(dp) if with_grad else None, ldd, *tail)
        _sync(dev)
        assert _guard_ok(loss, 1) and _guard_ok(dp, M * ldd)
        if with_loss:
            k = _mse_adds(M, ldd if with_grad else C)
            _inside(f"{tag} {name} loss", _get(loss, 1), loss64.reshape(1), ((k + 6) * U * (loss64 - start) + U * loss64).reshape(1))
        else:
            assert float(_get(loss, 1)) == start
        if with_grad:
            d = _get(dp, M * ldd, M, ldd)
            _inside(f"{tag} {name} dpred", d, g64, (BF_ULP + 5 * U) * g64.abs())
            assert bool((d[:, C:] == 0).all())                                  # pad columns are zeroed
        else:
            assert _untouched(dp)
        return _get(loss, 1)

    run("dig_mse_fwd_bwd", True, True)
    run("dig_mse_fwd_bwd", True, False)                                         # loss only
    run("dig_mse_fwd_bwd", False, True)                                         # gradient only
    ws = _put(dev, torch.zeros(257))
    vals = [run("dig_mse_fwd_bwd_ws", True, True, ws) for _ in range(3)]
    assert torch.equal(vals[0], vals[1]) and torch.equal(vals[1], vals[2]), tag
    assert int(_get(ws, 1).view(torch.int32)[0]) == 0 and _guard_ok(ws, 257)
    _refused(ARG, "dig_mse_fwd_bwd", L.ptr(pd), C - 1, L.ptr(td), M, C, cf(gscale), None, None, ldd, L.stream())


# ================================================================================================ column sums
CS_C = [8, 520, 1536]
CS_ROWS = [1, 3, 4, 13, 16, 17, 64, 65]
CS_BIG = (32768 + 70, 8)


def _colsum_rpb(rows, C):
    cb, rpb = -(-C // 512), 64
    while cb * -(-rows // rpb) > 512:
        rpb *= 2
    return rpb


def _cs_shapes():
    return [(r, c) for c in CS_C for r in CS_ROWS] + [CS_BIG]


@pytest.mark.parametrize("rows,C", _cs_shapes())
def test_colsum_and_masked_are_exact(abi_dev, rows, C):
    """Multiples of 1/4: dig_colsum (ld = C + 8, poison in the pad) and dig_colsum_masked (masks all 0, all 1, random) add the float64 column sums
    onto non-zero accumulators bit for bit."""
    dev, be = abi_dev, _backend(abi_dev)
    L = _L()
    want_ws = (-(-rows // _colsum_rpb(rows, C)) if be == "hip" else -(-rows // 64)) * C * 4
    assert L.query("dig_colsum_workspace_bytes", rows, C) == want_ws
    nws = want_ws // 4
    g = torch.Generator().manual_seed(rows + C)
    x = _quarters(g, rows, C).bfloat16()
    start = _quarters(g, C)
    for ld in (C, C + 8):
        xp = torch.full((rows, ld), POISON, dtype=BF)
        xp[:, :C] = x
        xd, out, ws = _put(dev, xp), _put(dev, start), _ws(dev, nws)
        L.call("dig_colsum", L.ptr(xd), L.ptr(out), L.ptr(ws), rows, C, ld, L.stream())
        _sync(dev)
        assert _guard_ok(out, C) and _guard_ok(ws, nws)
        assert torch.equal(_get(out, C).double(), start.double() + x.double().sum(0)), (rows, C, ld)
    xd = _put(dev, x)
    for kind in ("zeros", "ones", "random"):
        mask = {"zeros": torch.zeros(rows), "ones": torch.full((rows,), 3.0), "random": (torch.rand(rows, generator=g) < 0.4) * 7.0}[kind].to(torch.uint8)
        md = torch.cat([mask, torch.full((GUARD,), 1, dtype=torch.uint8)]).to(dev)
        o0, o1, ws = _put(dev, start), _put(dev, start * 2), _ws(dev, 2 * nws)
        L.call("dig_colsum_masked", L.ptr(xd), L.ptr(md), L.ptr(o0), L.ptr(o1), L.ptr(ws), rows, C, L.stream())
        _sync(dev)
        assert _guard_ok(o0, C) and _guard_ok(o1, C) and _guard_ok(ws, 2 * nws)
        m = mask != 0
        assert torch.equal(_get(o0, C).double(), start.double() + x.double()[~m].sum(0)), (rows, C, kind)
        assert torch.equal(_get(o1, C).double(), 2 * start.double() + x.double()[m].sum(0)), (rows, C, kind)


@pytest.mark.parametrize("C", CS_C)
@pytest.mark.parametrize("n_parts", [1, 127, 128, 129])
def test_colsum_partials_is_exact(abi_dev, n_parts, C):
    dev = abi_dev
    L = _L()
    g = torch.Generator().manual_seed(n_parts + C)
    p, start = _quarters(g, n_parts, C), _quarters(g, C)
    pd = _put(dev, torch.cat([p.reshape(-1), torch.full((4 * C,), math.nan)]))          # NaN behind row n_parts
    out = _put(dev, start)
    L.call("dig_colsum_partials", L.ptr(pd), n_parts, C, L.ptr(out), L.stream())
    _sync(dev)
    assert _guard_ok(out, C) and torch.equal(_get(out, C).double(), start.double() + p.double().sum(0))
    _refused(ARG, "dig_colsum_partials", L.ptr(pd), n_parts, C + 4, L.ptr(out), L.stream())
    _refused(ALIGN, "dig_colsum_partials", ctypes.c_void_p(pd.data_ptr() + 4), n_parts, C, L.ptr(out), L.stream())


@pytest.mark.parametrize("odd", [False, True], ids=["widths % 32 == 0", "one width of 40"])
def test_colsum_partials_multi_is_exact(abi_dev, odd):
    """Thirteen segments (more than twelve selects the 32-column kernel when every width is a multiple of 32; one width of 40 sends the launch to
    the 8-column kernel), interleaved strides, multiples of 1/4: out += the float64 column sums bit for bit."""
    from dig_amd import ops
    dev = abi_dev
    L = _L()
    g = torch.Generator().manual_seed(13 + int(odd))
    segs, outs, want, keep = [], [], [], []
    for k in range(13):
        C = 40 if (odd and k == 6) else (64, 384, 32, 1536, 512)[k % 5]
        n_parts = (1, 5, 33, 64, 65, 129, 300)[k % 7]
        vecs = 3 if k % 4 == 0 else 1
        w = _quarters(g, n_parts, vecs, C)
        wd = _put(dev, torch.cat([w.reshape(-1), torch.full((vecs * C,), math.nan)]))
        keep.append(wd)
        start = _quarters(g, C)
        out = _put(dev, start)
        outs.append((out, C))
        want.append(start.double() + w[:, vecs - 1].double().sum(0))
        segs.append(ops._ColsumSeg(wd.data_ptr() + 4 * (vecs - 1) * C, out.data_ptr(), vecs * C, n_parts, C))
    arr = (ops._ColsumSeg * len(segs))(*segs)
    L.call("dig_colsum_partials_multi", arr, len(segs), L.stream())
    _sync(dev)
    for (out, C), w in zip(outs, want):
        assert _guard_ok(out, C) and torch.equal(_get(out, C).double(), w), (odd, C)


def test_fp32_restatement_of_the_other_kernels_is_inside_the_bounds():
    """BatchNorm (one pass, as the library), L2 normalise, the row softmax / cross entropy and the MSE in plain fp32 torch against the float64
    reference, held to the same bounds; and the figure behind E_FAST: exp, log and 1 / sqrt in fp32 torch against float64 on the same arguments."""
    g = torch.Generator().manual_seed(0)
    a = -(torch.rand(1 << 22, generator=g) * 20)
    s = torch.rand(1 << 22, generator=g) * 1000 + 1
    v = torch.rand(1 << 22, generator=g) * 100 + 1e-6
    worst = max(float(((torch.exp(a).double() - torch.exp(a.double())).abs() / torch.exp(a.double())).max()),
                float(((torch.log(s).double() - torch.log(s.double())).abs() / torch.log(s.double())).max()),
                float((((1.0 / torch.sqrt(v)).double() - 1.0 / torch.sqrt(v.double())).abs() * torch.sqrt(v.double())).max()))
    print(f"restatement exp / log / 1 / sqrt: worst relative error {worst:.3g}")
    assert E_FAST_R / 4 <= worst <= E_FAST_R
    # BatchNorm
    rows, C = 1000, 64
    x = _bn_cols(rows, C, 5)
    gamma, beta, rm0, rv0 = _bn_params(C)
    xf = x.float()
    inv_n = f32(1.0 / rows)
    mu = xf.sum(0) * inv_n
    var = ((xf * xf).sum(0) * inv_n - mu * mu).clamp_min(0)
    rs = 1.0 / torch.sqrt(var + BN_EPS)
    n = float(rows)
    run = (rm0 * f32(1 - BN_MOM) + mu * BN_MOM, rv0 * f32(1 - BN_MOM) + var * f32(n / (n - 1)) * BN_MOM)
    for relu in (0, 1):
        y = (xf - mu) * rs * gamma + beta
        y = (y.clamp_min(0) if relu else y).bfloat16()
        _bn_check_fwd(f"restatement bn relu {relu}", x, (mu, rs, y), BN_EPS, gamma, beta, relu, _bn_adds("cpu_abi", rows, C), n, (rm0, rv0), run)
        dy = torch.randn(rows, C, generator=g).bfloat16()
        ref0, _ = _bn_fwd_ref(x, BN_EPS, None, None, 0, rows)
        mean_in, rstd_in = ref0[0].float(), ref0[1].float()
        xh = (xf - mean_in) * rstd_in
        gm = dy.float()
        if relu:
            gm = torch.where(gamma * xh + beta > 0, gm, torch.zeros_like(gm))
        s1, s2 = gm.sum(0), (gm * xh).sum(0)
        (r1, r2), (b1, b2), parts = _bn_bwd_ref(dy, x, mean_in, rstd_in, gamma, beta, relu, rows)
        _inside(f"restatement bn relu {relu} sum g", s1, r1, b1)
        _inside(f"restatement bn relu {relu} sum g xhat", s2, r2, b2)
        dx = (gamma * rstd_in * (gm - s1 * inv_n - xh * (s2 * inv_n))).bfloat16()
        ref, bnd = _bn_dx_ref(parts, torch.stack([s1, s2]), n)
        _inside(f"restatement bn relu {relu} dx", dx, ref, bnd)
    # L2 normalise
    for C in (1, 65, 256):
        x, kind = _l2_rows(512, C, C)
        inv = 1.0 / torch.sqrt((x * x).sum(1)).clamp_min(L2_EPS)
        inv64 = 1.0 / x.double().norm(dim=1).clamp_min(L2_EPS)
        rel = (_row_adds("cpu_abi", C) + 6) * U
        _inside(f"restatement l2norm C {C} inv_norm", inv, inv64, rel * inv64)
        _inside(f"restatement l2norm C {C} y", x * inv[:, None], x.double() * inv64[:, None], (rel + U) * (x.double() * inv64[:, None]).abs())
    # cross entropy rows
    for m in CE_M[2:]:
        z = _ce_logits(7, m, 0, m)
        loss, top1, top5, d64, b_loss, b_d = _ce_ref(z, 0, 0.25, "cpu_abi")
        mx = z.max(1, keepdim=True).values
        e = torch.exp(z - mx)
        ssum = e.sum(1, keepdim=True)
        li = (mx + torch.log(ssum))[:, 0] - z[torch.arange(7), torch.arange(7)]
        one = torch.zeros_like(z)
        one[torch.arange(7), torch.arange(7)] = 1
        _inside(f"restatement ce_rows m {m} loss", li.sum().reshape(1), loss.reshape(1), b_loss.reshape(1))
        _inside(f"restatement ce_rows m {m} dlogits", 0.25 * (e / ssum - one), d64, b_d)
    # MSE
    M, C = 895, 48
    pred, target = torch.randn(M, C, generator=g), torch.randn(M, C, generator=g)
    df = pred - target
    inv = f32(1.0 / (M * C))
    loss64 = (df.double() ** 2).sum() / (M * C)
    _inside("restatement mse loss", ((df * df).sum() * inv).reshape(1), loss64.reshape(1), ((_mse_adds(M, C) + 6) * U * loss64).reshape(1))
    g64 = 2.0 * df.double() / (M * C) * f32(0.7)
    _inside("restatement mse dpred", (2.0 * df * inv * f32(0.7)).bfloat16(), g64, (BF_ULP + 5 * U) * g64.abs())
