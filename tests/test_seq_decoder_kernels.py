"""Every entry point of the Transformer recognition decoder's kernels -- dig_amd/csrc/seq_attn.hip (whole-sequence attention forward / backward, the
token embedding and its gradient), dig_amd/csrc/seq_loss.hip (the sequence cross-entropy criteria and their gradients) and the per-step decode kernels
of dig_amd/csrc/decode.hip -- against float64 torch on the same bf16 / fp32 / int64 inputs, on both builds of the ABI (`abi_dev`: libdig_hip.so on the
MI355X and cpu_abi/libdig_cpu.so).  cpu_abi/dig_cpu_rec.cpp restates the formulas with the kernels' conventions, so the pairing of the two builds cannot
see an error they share; the float64 reference here is written from the definitions alone.

Reference and bounds (derived, not measured on the kernels)
-----------------------------------------------------------
The reference is torch float64 on the same inputs; `scale`, `smoothing`, the dropout factor 1 / (1 - p) and *gscalar are the fp32 values the ABI
receives, widened.  Every reduction is checked twice.

1. Exact arithmetic, no tolerance.
   routing    key j is the +-64 sign code of the bits of j over the first 9 (13 for n_mem = 8192) channels, the other channels 0, and q_i = k_pi(i)
              with pi(i) a key the mask allows: logit(i, j) = scale 4096 (nbits - 2 hamming(pi(i), j)), the gap to every other key at least
              8192 scale >= 1024, exp(-gap) = 0 on both builds and exp(0) = 1: the probabilities are exactly one-hot.  out[i] == v[pi(i)] bit for
              bit; lse[i] is the logit within (a_dot + 2) u nbits 4096 scale (bit for bit where scale is a power of two); for the backward, lse is the
              test's own fl(fl(q . k) scale), the value the backward forms, so P is exactly one-hot: dV[j] == the sum of the integer dO rows routed
              to j, dQ == dK == 0 -- where scale is a power of two (head dim 64, or scale = 1); elsewhere the fp32 lse is a rounded logit
              and the compiler may contract fl(q . k) scale - lse into one FMA, so P = exp(logit - lse) is 1 + 2.6e-4 at head dim 48 (seen on the
              MI355X): there the backward is held to the float64 reference on that lse and the bounds of 2. instead.  The same for dig_decode_self_attn (its online softmax multiplies everything before the target by exp(-gap) = 0)
              and dig_decode_cross_attn (`weights` exactly one-hot, the beam slots of one memory routed to different keys).
   counting   q = 0: every allowed logit is 0, s = n_i exactly (a sum of ones), lse[i] = log n_i within (a + 2) u + E_FAST, which separates n from
              n +- 1 up to Lk = 512 (log(513 / 512) = 2e-3); out[i] = the mean of the allowed v rows (multiples of 1/4: the sum is exact), bit for bit
              the bf16 rounding of the float64 mean where n_i is a power of two and within (2^-8 + 4 u) |mean| elsewhere.  The off-by-one test of
              `causal & (key < lens)`.
   losses     integer logits in [-8, 8] with one class at 200: exp(-192) = 0, s = 1, log s = 0; the row term is exactly 0 where the target is the
              dominant class and the integer gap elsewhere; with B a power of two dig_seq_cross_entropy is exact, and with C a power of two and
              smoothing 1/4 so is dig_seq_ls_cross_entropy.  A second launch gives the same bits.
   embedding gradient   dx multiples of 1/4 in [-8, 8], up to 15 360 rows of one token (|sum| <= 491 520 quarters < 2^24): demb exact on a non-zero
              dyadic start, in any order.

2. Random and adversarial data, bounds from counting roundings: u = 2^-24 per fp32 operation (FMA contraction only removes roundings), 2^-8 |ref|
   for a bf16 result, E_FAST = 4 x 9.2e-8 for __expf / __logf (tests/test_norm_loss_kernels.py: exp and log in plain fp32 torch measure 9.16e-8, the
   intrinsics are allowed four times that; a logarithm's error is E_FAST (1 + max(1, |log s|)): relative above 1, absolute below), TINY = 2^-125
   absolute for a probability below the smallest normal number, which may come out as 0.  `a` = the additions an element passes through:

       q . k            hip: 8 terms + 3 shuffles = 11 (Lk <= 64: dot8_reduce), four chains of dk / 4 + 2 (dot_row), 6 shuffle levels (decode self),
                             8 + 3 = 11 (decode cross)                                        cpu: dk (one chain)
       row max / sum    hip: ceil(Lk / 64) - 1 in the lane + 6 shuffle levels; decode cross ceil(n_mem / 256) + 6 + 3 (four waves)   cpu: Lk
       P V, dS K        hip: Lk in one chain (rows_times_x); decode cross ceil(n_mem / 32) + 3 + 3                                   cpu: Lk
       dS^T Q, P^T dO   both: Lq in one chain
       decode self      hip: the online softmax: 2 (t + 1) for the sum and the output (a multiply and an add per step), and the t rescalings
                             c = exp(m_old - m_new) each carry E_FAST + u |m_old - m_new|; the differences telescope to max - min of the scores:
                             2 (t E_FAST + u (max - min)) more on every weight (once in the numerator, once in the denominator)
       logit rows       hip: ceil(C / 64) - 1 + 6      cpu: C - 1           row terms   hip: ceil(B T / 256) - 1 + 8   cpu: a double accumulator

   forward (s the float64 logit, m the row's maximum, p the float64 probability, f the dropout factor 0 or 1 / (1 - p_drop), 1 without):
       score   |err| <= es = (a_dot + 3) u scale sum_c |q_c k_c|        q scale (exact only at head dim 64, scale = 2^-3), the products, the adds
               it enters exp as an absolute error of its argument, with the subtraction's rounding:  eta_j = es_j + u |s_j - m|
       p       relative rho_j = eta_j + sum_k p_k eta_k + 2 E_FAST + (a_sum + 3) u         its own exp, then the sum's bound, 1 / s, the product
       out     |err| <= 2^-8 |out64| + 1.01 sum_j p_j f_j |v_j| (rho_j + (a_out + 2) u) + Lk TINY max|v|
       lse     |err| <= sum_k p_k eta_k + (a_sum + 1) u + E_FAST (1 + max(1, log s)) + 2 u (|lse| + |m|)
       weights (decode cross)   1.01 p rho + TINY; each row sums to 1 within the sum of its bounds
   backward (lse is an INPUT, as mean / rstd are for the LayerNorm backward: the reference uses the fp32 lse the forward wrote, widened;
   P = exp(s - lse), dP = f (dO . v), del = sum_j P dP, dS = P (dP - del), dV = (P f)^T dO, dK = scale dS^T Q, dQ = scale dS K):
       P       eP = P (es' + u |s - lse| + E_FAST) + TINY,   es' = (a_dot + 2) u scale sum_c |q_c k_c|   (the dot product, then scale)
       dP      eD = (a_dot + 2) u f sum_c |dO_c v_c|
       del     eDel = sum_j (eP |dP| + P eD + (a_sum + 1) u P |dP|)
       dS      eS = eP |dP - del| + P (eD + eDel) + 2 u |dS|
       dV      2^-8 |dV64| + 1.01 sum_i f |dO| (eP + (Lq + 2) u P)
       dK      2^-8 |dK64| + 1.01 scale sum_i |q| (eS + (Lq + 2) u |dS|)         dQ   2^-8 |dQ64| + 1.01 scale sum_j |k| (eS + (Lk + 2) u |dS|)
       forward + backward against float64 autograd: lse is the float64 one and the forward's lse bound is added to P's relative error
   softmax_argmax   probs: 1.01 p (u |x - m| + sum_k p_k u |x_k - m| + 2 E_FAST + (a + 3) u) + TINY, rows sum to 1 within the sum; token exact
   embedding        out == bf16(fp32(emb + pos)): the float64 sum of two fp32 numbers of these magnitudes is exact, so its fp32 rounding is THE
                    correctly rounded sum and the comparison has no tolerance
   seq_cross_entropy   R_s = (a + 4) u + 3 u sum_j p_j |x_j - m| + E_FAST (the row sum, relative); row term r = R_s + E_FAST (1 + max(1, log s))
                    + 3 u (|m| + |lse| + |x_y|); loss: (sum r + (k + 1) u sum|term|) / B + 3 u |loss|
       gradient     2^-8 |ref| + 1.01 sc (p (R_s + 3 u |x - m| + 4 u + E_FAST) + 2 u |p - onehot| + TINY) + 3 u |ref|,  sc = g / B; masked rows and
                    pad columns exactly 0; every other row sums to 0 within the sum of its bounds
   seq_ls_cross_entropy   s_j = lse_j - mean_c x_jc: e_j = R_s + E_FAST (1 + max(1, log s)) + 2 u (|m| + |lse|) + (a + 2) u mean|x| + u |s_j|;
                    loss: ((1 - sm) n (sum r + (k + 1) u sum|nll|) + sm cnt (sum e + (k + 1) u sum|s_j|)) / B + 8 u (|term 1| + |term 2|)
       gradient     v = sc (wn (p - onehot) + ws (p - 1 / C)), wn = (1 - sm) B T on a counted row, ws = sm cnt:
                    2^-8 |ref| + 1.01 sc (wn + ws) eP + 8 u sc (wn |p - onehot| + ws |p - 1 / C| + ws / C); every row sums to 0 within the sum
                    at smoothing 0 the loss is B T times the plain loss within the two bounds

`test_fp32_restatement_is_inside_the_bounds` holds a plain fp32 torch restatement of each formula to the same bounds on the CPU (the cpu counts: no
chain in torch is longer).  Its worst |err| / bound: out 0.983, lse 0.040, dQ 0.971, dK 0.979, dV 0.985, probs 0.20, ce rows 0.11, ce loss 0.094,
ce gradient 0.993, ls loss 0.029, ls gradient 0.986 (the bf16 outputs reach their rounding: half an ulp is 2^-8 just above a power of two).  A bound that a kernel exceeds is a finding to
investigate, not a number to raise.  Every output buffer carries 256 poisoned elements behind its range and in its pad columns, which must survive;
every workspace is NaN before the call; every refusal leaves the poisoned outputs untouched.

Cases -> the branch or loop trip they exist for       (B = 3 and three heads unless named: a wrong head or sample stride lands in other columns)
-----------------------------------------------
dig_seq_attn_fwd_hd, dig_seq_attn_bwd_hd        head dim 24 48 64: G = 10 / 5 / 4 groups in rows_times_x (threads 240..255 idle at 48), 3 / 6 / 8 live lanes
    dig_seq_attn_fwd, dig_seq_attn_bwd,         of a key's group on the 8-lane path
    dig_seq_attn_fwd_dropout,                   at head dim 64 every case is repeated through the four wrappers: the same bits
    dig_seq_attn_bwd_dropout
    Lq 1 4 5 31 32                              fewer queries than groups, G at head dim 64, G at 48, the last NU trip partial, full; Lq = 33 refused
    Lk 1 8 31 32 33 64 65 100 255 256 257 384   one / two / three passes of the 32-key 8-lane path, the switch at Lk <= 64, the second trip of j += 256,
                                                384: the largest backward at head dim 64 (exactly 160 KiB of LDS)
    Lk 512, forward alone                       all three head dims (139 392 bytes at 64)
    masks                                       causal with Lq == Lk <= 32; causal + lens holding 1, Lk, Lk + 3 and a mid value (B = 4); none;
                                                lens without causal (cross-attention: lens alone is honoured); lens holding 0 and -3: fully masked rows
                                                give out = 0, lse = -inf and exactly zero dQ / dK / dV
    layout                                      q k v out dout dq dk dv are views of wider poisoned buffers: eight different leading dimensions, columns
                                                from a non-zero 16-byte aligned offset
    scale dk^-0.5 and 1; one spiked row (its target logit near 100: most of its probabilities underflow)
    dropout                                     p = 0.1 at Lk = 25 (8-lane path) and 100: the keep mask rebuilt from the keys of dig_amd/dropout.py and the hash of
                                                include/dig_hip.h; lse the bits of the run without; thr = 0 the bits of the run without
    refusals                                    Lq = 33, Lk = 513 (argument); head dim 32, the backward at Lk 385 / 431 for head dim 64 / 48 (unsupported); k + 2 bytes,
                                                ldk = hk + 4, dk / dv + 2 bytes, lddk / lddv = hk + 4 (alignment); after them a backward at Lk = 256 still runs
dig_decode_self_attn                            head dim 24 48 64; (T, t) (1, 0) (26, 0) (26, 1) (26, 25); cache rows above t NaN; t = T, t < 0, head dim 32 refused
dig_decode_cross_attn                           n_mem 1 31 32 33 255 256 257 8192 (fewer keys than slots, one pass, a second, the 256-thread loops' second trip, the
                                                limit), slots_per_mem 1 and 5 with B = 10, weights None / given; n_mem 8193, B % slots_per_mem, head dim 32,
                                                kv_mem + 2 bytes, q + 2 bytes refused
dig_softmax_argmax                              C 1 63 64 65 97 200, ld = C + 3 with NaN pads; ties inside a lane's stride (6, 70), across lanes (3, 65), first and
                                                last column, -inf beside finite entries, a row of -inf (token 0), a +-80 row
dig_seq_embed_fwd, dig_decode_embed             d 1 255 256 257 640; tokens -3, -1, vocab, vocab + 7 read the nearest row
dig_seq_embed_bwd, dig_seq_embed_bwd_lens       n_tok 1 255 256 257 15 360 (the 256-token ballot chunks: one short, exact, a second; the LDS list's limit), d 1 256 257 640
                                                (a second channel block with one live thread), every token equal, a token without hits, out-of-range tokens
                                                (their gradient goes to the clamped row), lens 0 1 T T + 2, a non-zero start, two runs the same bits;
                                                n_tok = 15 361 and n_tok % T != 0 with lens refused
dig_seq_cross_entropy, dig_seq_cross_entropy_bwd,   C 1 63 64 65 97 200; (B, T) (1, 1) (7, 25) (4, 65) (70, 5): B T = 260 takes the fixed-order sum past one 256
dig_seq_ls_cross_entropy, dig_seq_ls_cross_entropy_bwd   trip, B = 70 the count loop past 64 lanes; lengths 0, T, T + 3, -2, mid; targets -1 and C + 5; ld = C + 3
                                                with NaN pads, ldd = C + 5 with zero pads; gscalar None / given; smoothing 0 0.1 1, -0.1 and 1.1 refused; +-80 rows
dig_beam_step, dig_attn_beam_advance            tests/test_decode.py and tests/test_attn_beam.py

Largest |err| / bound on the MI355X (printed by every test; no kernel exceeded a bound)
---------------------------------------------------------------------------------------
    seq attention   out 0.992, lse 0.14, dQ 0.987, dK 0.992, dV 0.995; with dropout out 0.985, dQ 0.984, dK 0.986, dV 0.991; counting lse 0.44;
                    routing lse 0.054, and at an inexact scale dQ / dK 2e-4, dV 0.029
    decode          self 0.977; cross out 0.983, weights 0.10, weight sums 0.022; softmax_argmax probs 0.58, prob sums 0.073
    losses          ce row terms 0.18, loss 0.069, gradient 0.995, row sums 0.68; ls nll rows 0.18, smooth rows 0.20, loss 0.082, gradient 0.996, row sums 0.73
On the cpu build: out 0.99, lse 0.061, dQ 0.982, dK 0.984, dV 0.994, counting lse 0.055, decode self 0.974, cross out 0.965, weights 0.049, probs 0.17,
ce loss 0.063, ls loss 0.043; the gradients at the bf16 rounding.

Seeded faults (each a one-line change to cpu_abi/dig_cpu_rec.cpp, on a scratch copy) and the tests that failed
---------------------------------------------------------------------------------------------------------------
    j <= i -> j < i (forward and backward)      test_seq_attn_counting, test_seq_attn_routing_is_exact, test_seq_attn_vs_fp64, test_seq_attn_dropout,
                                                test_seq_attn_fwd_then_bwd_vs_fp64_autograd
    j < len -> j <= len (both)                  test_seq_attn_counting, test_seq_attn_vs_fp64, test_seq_attn_dropout, test_seq_attn_fwd_then_bwd_vs_fp64_autograd
    head 1's keys read 8 columns further        test_seq_attn_routing_is_exact, test_seq_attn_vs_fp64, test_seq_attn_dropout, test_seq_attn_fwd_then_bwd_vs_fp64_autograd
    the * scale of dK dropped                   test_seq_attn_vs_fp64, test_seq_attn_fwd_then_bwd_vs_fp64_autograd, test_seq_attn_dropout, test_seq_attn_refusals
    dropout before the row sum                  test_seq_attn_dropout
"""
import ctypes
import math

import numpy as np
import pytest
import torch

U = 2.0 ** -24
BF_ULP = 2.0 ** -8
TINY = 2.0 ** -125
GUARD = 256
POISON = 768.0
BF, F32, F64, I64 = torch.bfloat16, torch.float32, torch.float64, torch.int64
cf = ctypes.c_float
E_FAST_R = 9.2e-8
E_FAST = 4 * E_FAST_R
ARG, ALIGN, UNSUP = -1, -2, -4
HEAD_DIMS = [24, 48, 64]
INF = math.inf


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
    b = torch.full((n + GUARD,), POISON, dtype=dtype, device=dev)
    if fill != POISON:
        b[:n] = fill
    return b


def _put(dev, t):
    t = t.contiguous().reshape(-1)
    if t.dtype == I64:
        return t.to(dev)
    b = torch.full((t.numel() + GUARD,), POISON, dtype=t.dtype, device=dev)
    b[:t.numel()] = t.to(dev)
    return b


def _ws(dev, nfloats):
    b = torch.full((nfloats + GUARD,), POISON, dtype=F32, device=dev)
    b[:nfloats] = math.nan
    return b


def _get(b, n, *shape):
    return b[:n].detach().cpu().reshape(*shape) if shape else b[:n].detach().cpu()


def _guard_ok(b, n):
    return bool((b[n:].float() == POISON).all())


def _untouched(b):
    return bool((b.float() == POISON).all())


def _off(t, nbytes):
    return ctypes.c_void_p(t.data_ptr() + nbytes)


def _refused(code, name, *args):
    L = _L()
    with pytest.raises(L.DigHipError) as e:
        L.call(name, *args)
    assert f"rc={code})" in str(e.value), (name, str(e.value))


def _inside(tag, got, ref, bound):
    """Prints the worst |got - ref| / bound, then asserts the element-wise bound; every value finite."""
    got, ref, bound = got.double(), ref.double(), bound.double()
    assert got.shape == ref.shape == bound.shape, (tag, got.shape, ref.shape, bound.shape)
    assert bool(torch.isfinite(got).all()), (tag, "non-finite")
    err = (got - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print(f"{tag}: worst |err| / bound = {ratio:.3g}")
    bad = err > bound
    if bool(bad.any()):
        i = int(torch.nonzero(bad.reshape(-1))[0])
        raise AssertionError((tag, ratio, i, float(got.reshape(-1)[i]), float(ref.reshape(-1)[i]), float(bound.reshape(-1)[i])))
    return ratio


class _View:
    """A [rows, cols] matrix inside a wider poisoned buffer: leading dimension ld, first column `off`, GUARD poisoned elements behind."""

    def __init__(self, dev, rows, cols, ld, off, src=None, dtype=BF):
        self.rows, self.cols, self.ld, self.off = rows, cols, ld, off
        self.buf = torch.full((rows * ld + GUARD,), POISON, dtype=dtype, device=dev)
        self.mat = self.buf[:rows * ld].view(rows, ld)
        if src is not None:
            self.mat[:, off:off + cols] = src.to(dev)

    def ptr(self, extra_bytes=0):
        return ctypes.c_void_p(self.buf.data_ptr() + self.off * self.buf.element_size() + extra_bytes)

    def get(self):
        return self.mat[:, self.off:self.off + self.cols].detach().cpu().clone()

    def outside_ok(self):
        m = self.mat.detach().cpu().float().clone()
        m[:, self.off:self.off + self.cols] = POISON
        return bool((m == POISON).all()) and _guard_ok(self.buf, self.rows * self.ld)

    def untouched(self):
        return _untouched(self.buf)


# ================================================================================================ the float64 references
def _split(t, B, L, H, dk):
    """[B * L, H * dk] -> float64 [B, H, L, dk]"""
    return t.double().reshape(B, L, H, dk).permute(0, 2, 1, 3)


def _merge(t):
    """[B, H, L, dk] -> [B * L, H * dk]"""
    B, H, L, dk = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * L, H * dk)


def _allow(B, Lq, Lk, causal, lens):
    """[B, 1, Lq, Lk] bool: (causal ? key <= query : 1) & (lens ? key < lens[sample] : 1)"""
    j, i = torch.arange(Lk)[None, None, :], torch.arange(Lq)[None, :, None]
    a = torch.ones(B, Lq, Lk, dtype=torch.bool)
    if causal:
        a = a & (j <= i)
    if lens is not None:
        a = a & (j < lens.reshape(B, 1, 1))
    return a[:, None]


def _attn_adds(be, kind, dk, Lk):
    """(a_dot, a_sum, a_out) of the docstring's table; kind: seq, self (Lk = t + 1), cross (Lk = n_mem)."""
    if be != "hip":
        return dk, Lk, Lk
    if kind == "seq":
        return (11 if Lk <= 64 else dk // 4 + 2), -(-Lk // 64) - 1 + 6, Lk
    if kind == "self":
        return 6, 2 * Lk, 2 * Lk
    return 11, -(-Lk // 256) + 6 + 3, -(-Lk // 32) + 3 + 3


def _fwd_ref(q, k, v, scale, allow, adds, keep=None, extra=0.0):
    """float64 attention of [B, H, L, dk] operands and the forward bounds of the docstring."""
    a_dot, a_sum, a_out = adds
    Lk = k.shape[2]
    s = (q @ k.transpose(-1, -2)) * scale
    es = (a_dot + 3) * U * (q.abs() @ k.abs().transpose(-1, -2)) * abs(scale)
    allow = allow.expand_as(s)
    zero = torch.zeros_like(s)
    sm = torch.where(allow, s, torch.full_like(s, -INF))
    dead = ~allow.any(-1, keepdim=True)
    m = torch.where(dead, zero[..., :1], sm.amax(-1, keepdim=True))
    e = torch.where(allow, torch.exp((s - m).clamp_max(0.0)), zero)
    sig = torch.where(dead, 1.0 + zero[..., :1], e.sum(-1, keepdim=True))
    p = e / sig
    eta = torch.where(allow, es + U * (s - m).abs(), zero)
    avg = (p * eta).sum(-1, keepdim=True)
    rho = eta + avg + 2 * E_FAST + (a_sum + 3) * U + extra
    pf = p if keep is None else p * keep
    out = pf @ v
    f_out = (pf * (rho + (a_out + 2) * U)) @ v.abs() + Lk * TINY * float(v.abs().max())
    logs = torch.log(sig)
    lse = torch.where(dead, torch.full_like(m, -INF), m + logs)
    b_lse = avg + (a_sum + 1) * U + E_FAST * (1 + logs.clamp_min(1.0)) + 2 * U * ((m + logs).abs() + m.abs())
    return dict(out=out, b_out=BF_ULP * out.abs() + 1.01 * f_out, lse=lse[..., 0], b_lse=b_lse[..., 0], p=p, b_p=1.01 * p * rho + TINY,
                dead=dead[..., 0], s=s)


def _bwd_ref(q, k, v, do, scale, allow, lse, a_dot, a_sum, keep=None, extra=None):
    """float64 (dQ, dK, dV) from the given lse [B, H, Lq] (float64) and the backward bounds of the docstring; `extra` [B, H, Lq]: added to P's
    relative error (the forward's lse bound, when lse is the float64 one)."""
    Lq, Lk = q.shape[2], k.shape[2]
    s = (q @ k.transpose(-1, -2)) * scale
    es = (a_dot + 2) * U * (q.abs() @ k.abs().transpose(-1, -2)) * abs(scale)
    allow = allow.expand_as(s)
    zero = torch.zeros_like(s)
    l = torch.where(torch.isfinite(lse), lse, torch.zeros_like(lse))[..., None]
    P = torch.where(allow, torch.exp(torch.where(allow, s - l, zero)), zero)
    rP = es + U * (s - l).abs() + E_FAST + (0.0 if extra is None else extra[..., None])
    eP = torch.where(allow, P * rP + TINY, zero)
    f = torch.ones_like(s) if keep is None else keep
    dP = torch.where(allow, (do @ v.transpose(-1, -2)) * f, zero)
    eD = torch.where(allow, (a_dot + 2) * U * (do.abs() @ v.abs().transpose(-1, -2)) * f, zero)
    dl = (P * dP).sum(-1, keepdim=True)
    eDel = (eP * dP.abs() + P * eD + (a_sum + 1) * U * P * dP.abs()).sum(-1, keepdim=True)
    dS = P * (dP - dl)
    eS = eP * (dP - dl).abs() + P * (eD + eDel) + 2 * U * dS.abs()
    dV = (P * f).transpose(-1, -2) @ do
    eV = (f * (eP + (Lq + 2) * U * P)).transpose(-1, -2) @ do.abs()
    dK = scale * (dS.transpose(-1, -2) @ q)
    eK = abs(scale) * ((eS + (Lq + 2) * U * dS.abs()).transpose(-1, -2) @ q.abs())
    dQ = scale * (dS @ k)
    eQ = abs(scale) * ((eS + (Lk + 2) * U * dS.abs()) @ k.abs())
    return (dQ, dK, dV), tuple(BF_ULP * r.abs() + 1.01 * e for r, e in ((dQ, eQ), (dK, eK), (dV, eV)))


# ================================================================================================ whole-sequence attention
LAYOUT = dict(q=(8, 8), k=(16, 8), v=(24, 16), out=(32, 8), dout=(8, 0), dq=(16, 16), dk=(24, 8), dv=(40, 24))       # (ld - hk, first column)


class _Seq:
    """One attention problem on the device: every operand a view of a wider poisoned buffer (LAYOUT), lse with a guard behind it."""

    def __init__(self, dev, dk, B, H, Lq, Lk, q, k, v, dout=None):
        self.dev, self.dk, self.B, self.H, self.Lq, self.Lk, self.hk = dev, dk, B, H, Lq, Lk, H * dk
        hk = self.hk
        mk = lambda name, rows, src: _View(dev, rows, hk, hk + LAYOUT[name][0], LAYOUT[name][1], src)
        self.q, self.k, self.v = mk("q", B * Lq, q), mk("k", B * Lk, k), mk("v", B * Lk, v)
        self.dout = mk("dout", B * Lq, dout) if dout is not None else None
        self._mk = mk

    FWD = {"_hd": "dig_seq_attn_fwd_hd", "_dropout": "dig_seq_attn_fwd_dropout", "": "dig_seq_attn_fwd"}
    BWD = {"_hd": "dig_seq_attn_bwd_hd", "_dropout": "dig_seq_attn_bwd_dropout", "": "dig_seq_attn_bwd"}

    def _tail(self, form, drop):
        tail = (ctypes.byref(drop) if drop is not None else None,) if form != "" else ()
        return tail + ((self.dk,) if form == "_hd" else ())

    def fwd_args(self, out, lse, scale, causal, lens, form, drop):
        L = _L()
        return (self.q.ptr(), self.q.ld, self.k.ptr(), self.k.ld, self.v.ptr(), self.v.ld, out.ptr(), out.ld, L.ptr(lse), self.B, self.H, self.Lq, self.Lk,
                cf(scale), int(causal), L.ptr(lens), *self._tail(form, drop), L.stream())

    def fwd(self, scale, causal, lens, drop=None, form="_hd"):
        L = _L()
        n = self.B * self.H * self.Lq
        out, lse = self._mk("out", self.B * self.Lq, None), _buf(self.dev, n)
        ld = lens.to(self.dev) if lens is not None else None
        L.call(self.FWD[form], *self.fwd_args(out, lse, scale, causal, ld, form, drop))
        _sync(self.dev)
        assert out.outside_ok() and _guard_ok(lse, n)
        return out.get(), _get(lse, n, self.B, self.H, self.Lq)

    def grads(self):
        return self._mk("dq", self.B * self.Lq, None), self._mk("dk", self.B * self.Lk, None), self._mk("dv", self.B * self.Lk, None)

    def bwd_args(self, g, lse, scale, causal, lens, form, drop, Lk=None):
        L = _L()
        dq, dk_, dv = g
        return (self.q.ptr(), self.q.ld, self.k.ptr(), self.k.ld, self.v.ptr(), self.v.ld, self.dout.ptr(), self.dout.ld, L.ptr(lse), dq.ptr(), dq.ld,
                dk_.ptr(), dk_.ld, dv.ptr(), dv.ld, self.B, self.H, self.Lq, Lk or self.Lk, cf(scale), int(causal), L.ptr(lens), *self._tail(form, drop),
                L.stream())

    def bwd(self, scale, causal, lens, lse, drop=None, form="_hd"):
        L = _L()
        g = self.grads()
        lsed = lse.reshape(-1).to(self.dev)
        ld = lens.to(self.dev) if lens is not None else None
        L.call(self.BWD[form], *self.bwd_args(g, lsed, scale, causal, ld, form, drop))
        _sync(self.dev)
        assert all(t.outside_ok() for t in g)
        return tuple(t.get() for t in g)


def _seq_data(dk, B, H, Lq, Lk, seed, spike=False, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    hk = H * dk
    q, k = torch.randn(B * Lq, hk, generator=g), torch.randn(B * Lk, hk, generator=g)
    v, do = torch.randn(B * Lk, hk, generator=g), torch.randn(B * Lq, hk, generator=g)
    if spike:                                                                            # query 0 of the last sample, head 1: along its key Lk // 2
        kr = k[(B - 1) * Lk + Lk // 2, dk:2 * dk]
        q[(B - 1) * Lq, dk:2 * dk] = kr * (100.0 / (scale * float(kr.double().pow(2).sum())))
    return q.bfloat16(), k.bfloat16(), v.bfloat16(), do.bfloat16()


def _lens_for(kind, B, Lk):
    if kind in ("causal", "none"):
        return None
    if kind == "dead":
        return torch.tensor([0, max(1, Lk // 2), -3][:B] + [Lk] * max(0, B - 3), dtype=I64)
    return torch.tensor([1, Lk, Lk + 3, max(1, (Lk + 1) // 2)][:B], dtype=I64)


# (Lq, Lk, mask, scale = 1?, spike, backward?)
SEQ_CASES = [(1, 1, "causal", 0, 0, 1), (8, 8, "causal", 0, 0, 1), (8, 8, "causal+lens", 1, 0, 1), (31, 31, "causal+lens", 0, 0, 1), (32, 32, "causal", 1, 0, 1),
             (32, 32, "causal+lens", 0, 1, 1), (25, 25, "causal+dead", 0, 0, 1), (5, 1, "none", 0, 0, 1), (5, 8, "lens", 0, 0, 1), (4, 31, "none", 0, 0, 1),
             (5, 32, "lens", 0, 0, 1), (1, 33, "lens", 0, 0, 1), (4, 33, "none", 1, 0, 1), (31, 33, "none", 0, 0, 1), (32, 33, "lens", 0, 0, 1), (4, 64, "lens", 0, 1, 1),
             (5, 65, "none", 0, 0, 1), (31, 100, "lens", 0, 1, 1), (25, 100, "dead", 0, 0, 1), (1, 255, "none", 0, 0, 1), (32, 256, "none", 0, 0, 1),
             (4, 257, "lens", 1, 0, 1), (5, 384, "none", 0, 0, 1), (5, 512, "none", 0, 0, 0), (32, 512, "lens", 1, 1, 0)]


def _seq_setup(dev, dk, Lq, Lk, mask, unit, spike):
    B, H = (4 if mask == "causal+lens" else 3), 3
    scale = 1.0 if unit else f32(dk ** -0.5)
    q, k, v, do = _seq_data(dk, B, H, Lq, Lk, 1000 * dk + 10 * Lk + Lq, spike, scale)
    causal = mask.startswith("causal")
    lens = _lens_for("dead" if mask.endswith("dead") else ("lens" if mask.endswith("lens") else "none"), B, Lk)
    prob = _Seq(dev, dk, B, H, Lq, Lk, q, k, v, do)
    h = lambda t, L_: _split(t, B, L_, H, dk)
    return prob, B, H, scale, causal, lens, (h(q, Lq), h(k, Lk), h(v, Lk), h(do, Lq)), _allow(B, Lq, Lk, causal, lens)


def _check_fwd(tag, out, lse, ref, B, Lq):
    dead = ref["dead"]                                                                   # [B, H, Lq]
    live = ~dead
    assert bool((lse[dead] == -INF).all()), (tag, "a fully masked row's lse is not -inf")
    r1 = _inside(tag + " lse", lse[live], ref["lse"][live], ref["b_lse"][live])
    H, dk = ref["out"].shape[1], ref["out"].shape[3]
    o = _split(out, B, Lq, H, dk)
    assert bool((o[dead] == 0).all()), (tag, "a fully masked row's output is not 0")
    r0 = _inside(tag + " out", o, ref["out"], ref["b_out"])
    return r0, r1


@pytest.mark.parametrize("dk", HEAD_DIMS)
def test_seq_attn_vs_fp64(abi_dev, dk):
    """dig_seq_attn_fwd_hd and dig_seq_attn_bwd_hd over SEQ_CASES against float64; the backward reads the fp32 lse the forward wrote.  At head dim
    64 the four entry points without a head-dim argument give the same bits."""
    dev, be = abi_dev, _backend(abi_dev)
    for Lq, Lk, mask, unit, spike, with_bwd in SEQ_CASES:
        prob, B, H, scale, causal, lens, (q, k, v, do), allow = _seq_setup(dev, dk, Lq, Lk, mask, unit, spike)
        adds = _attn_adds(be, "seq", dk, Lk)
        tag = f"seq_attn {be} dk {dk} {Lq} x {Lk} {mask} scale {scale:.3g}"
        out, lse = prob.fwd(scale, causal, lens)
        ref = _fwd_ref(q, k, v, scale, allow, adds)
        _check_fwd(tag, out, lse, ref, B, Lq)
        got = None
        if with_bwd:
            got = prob.bwd(scale, causal, lens, lse)
            want, bnd = _bwd_ref(q, k, v, do, scale, allow, lse.double(), adds[0], adds[1])
            for name, a, r, b, L_ in zip(("dq", "dk", "dv"), got, want, bnd, (Lq, Lk, Lk)):
                a = _split(a, B, L_, H, dk)
                _inside(f"{tag} {name}", a, r, b)
            if mask.endswith("dead"):                                                      # samples 0 and 2 are fully masked: exact zeros
                for a, L_ in zip(got, (Lq, Lk, Lk)):
                    a = a.reshape(B, L_, -1)
                    assert bool((a[0] == 0).all()) and bool((a[2] == 0).all()), tag
        if dk == 64:
            for form in ("", "_dropout"):
                o2, l2 = prob.fwd(scale, causal, lens, form=form)
                assert torch.equal(o2, out) and torch.equal(l2, lse), (tag, form)
                if with_bwd:
                    g2 = prob.bwd(scale, causal, lens, lse, form=form)
                    assert all(torch.equal(a, b) for a, b in zip(got, g2)), (tag, form)


@pytest.mark.parametrize("dk", HEAD_DIMS)
def test_seq_attn_fwd_then_bwd_vs_fp64_autograd(abi_dev, dk):
    """The composition: forward, then backward on the forward's lse, against float64 autograd of softmax attention; P's error carries the
    forward's lse bound.  The closed form of `_bwd_ref` on the float64 lse is autograd's gradient to 1e-12."""
    dev, be = abi_dev, _backend(abi_dev)
    for Lq, Lk, mask in ((25, 25, "causal+lens"), (25, 256, "none")):
        prob, B, H, scale, causal, lens, (q, k, v, do), allow = _seq_setup(dev, dk, Lq, Lk, mask, 0, 0)
        adds = _attn_adds(be, "seq", dk, Lk)
        out, lse = prob.fwd(scale, causal, lens)
        got = prob.bwd(scale, causal, lens, lse)
        ref = _fwd_ref(q, k, v, scale, allow, adds)
        qa, ka, va = (t.clone().requires_grad_(True) for t in (q, k, v))
        logits = ((qa @ ka.transpose(-1, -2)) * scale).masked_fill(~allow.expand(B, H, Lq, Lk), -INF)
        (logits.softmax(-1) @ va).backward(do)
        want, bnd = _bwd_ref(q, k, v, do, scale, allow, ref["lse"], adds[0], adds[1], extra=ref["b_lse"])
        for name, a, r, b, auto, L_ in zip(("dq", "dk", "dv"), got, want, bnd, (qa.grad, ka.grad, va.grad), (Lq, Lk, Lk)):
            assert float((r - auto).abs().max()) <= 1e-12 * (1 + float(auto.abs().max())), name
            _inside(f"seq_attn fwd+bwd {be} dk {dk} {Lq} x {Lk} {name}", _split(a, B, L_, H, dk), auto, b)


# ------------------------------------------------------------------------------------------------ exact arithmetic: routing and counting
def _codes(n, dk, nbits):
    """[n, dk] float: key j = the +-64 sign code of the bits of j over the first nbits channels, 0 behind."""
    j = torch.arange(n)[:, None]
    c = torch.arange(nbits)[None, :]
    out = torch.zeros(n, dk)
    out[:, :nbits] = torch.where(((j >> c) & 1) == 1, 64.0, -64.0)
    return out


def _pi(B, H, Lq, Lk, causal, lens, seed):
    """[B, H, Lq] target keys the mask allows."""
    g = torch.Generator().manual_seed(seed)
    r = torch.randint(0, 1 << 30, (B, H, Lq), generator=g)
    hi = torch.full((B, 1, 1), Lk, dtype=I64)
    if lens is not None:
        hi = torch.minimum(hi, lens.reshape(B, 1, 1))
    hi = hi.expand(B, H, Lq).clone()
    if causal:
        hi = torch.minimum(hi, (torch.arange(Lq) + 1).reshape(1, 1, Lq).expand(B, H, Lq))
    return r % hi


ROUTE_CASES = [(1, 1, "causal"), (8, 8, "causal+lens"), (32, 32, "causal+lens"), (5, 33, "none"), (32, 64, "lens"), (31, 65, "none"), (4, 257, "lens"),
               (32, 384, "none")]


@pytest.mark.parametrize("unit", [0, 1], ids=["scale_dk", "scale_1"])
@pytest.mark.parametrize("dk", HEAD_DIMS)
def test_seq_attn_routing_is_exact(abi_dev, dk, unit):
    """One-hot probabilities by construction (the docstring's routing): out == v[pi], lse the logit, dV the routed integer sums, dQ == dK == 0."""
    dev, be = abi_dev, _backend(abi_dev)
    scale = 1.0 if unit else f32(dk ** -0.5)
    nbits = 9
    for Lq, Lk, mask in ROUTE_CASES:
        B, H = (4 if mask == "causal+lens" else 3), 3
        causal = mask.startswith("causal")
        lens = _lens_for("lens" if mask.endswith("lens") else "none", B, Lk)
        pi = _pi(B, H, Lq, Lk, causal, lens, Lq + Lk + dk)
        g = torch.Generator().manual_seed(Lq * Lk + dk)
        kc = _codes(Lk, dk, nbits)                                                       # the same codes in every (sample, head)
        k4 = kc[None, None].expand(B, H, Lk, dk)
        q4 = kc[pi]                                                                      # [B, H, Lq, dk]
        v4 = torch.randn(B, H, Lk, dk, generator=g).bfloat16().float()
        do4 = torch.randint(-4, 5, (B, H, Lq, dk), generator=g).float()
        prob = _Seq(dev, dk, B, H, Lq, Lk, *(_merge(t).bfloat16() for t in (q4, k4, v4, do4)))
        tag = f"routing {be} dk {dk} {Lq} x {Lk} {mask} scale {scale:.3g}"
        out, lse = prob.fwd(scale, causal, lens)
        want_out = torch.gather(v4, 2, pi[..., None].expand(B, H, Lq, dk))
        assert torch.equal(_split(out, B, Lq, H, dk), want_out.double()), tag
        logit = torch.full((B, H, Lq), nbits * 4096.0, dtype=F64) * scale
        a_dot = _attn_adds(be, "seq", dk, Lk)[0]
        _inside(tag + " lse", lse, logit, torch.full_like(logit, (a_dot + 2) * U * nbits * 4096.0 * scale))
        lse_b = torch.full((B, H, Lq), float(np.float32(nbits * 4096.0) * np.float32(scale)), dtype=F32)      # fl(fl(q . k) scale): the backward's logit
        if unit or dk == 64:
            assert torch.equal(lse, lse_b), tag                                           # scale a power of two: nothing rounds
        dq, dk_, dv = prob.bwd(scale, causal, lens, lse_b)
        want_dv = torch.zeros(B, H, Lk, dk).scatter_add_(2, pi[..., None].expand(B, H, Lq, dk), do4)
        if unit or dk == 64:
            assert bool((dq == 0).all()) and bool((dk_ == 0).all()), tag
            assert torch.equal(_split(dv, B, Lk, H, dk), want_dv.double()), tag
        else:                                                                             # lse_b is a ROUNDED logit and fl(q . k) scale - lse may be contracted
            allow = _allow(B, Lq, Lk, causal, lens)
            want, bnd = _bwd_ref(q4.double(), k4.double(), v4.double(), do4.double(), scale, allow, lse_b.double(), a_dot, _attn_adds(be, "seq", dk, Lk)[1])
            for name, a, r, bb, L_ in zip(("dq", "dk", "dv"), (dq, dk_, dv), want, bnd, (Lq, Lk, Lk)):
                _inside(f"{tag} {name}", _split(a, B, L_, H, dk), r, bb)


COUNT_CASES = [(8, 8, "causal"), (32, 32, "causal"), (32, 32, "causal+lens"), (31, 31, "causal+lens"), (5, 33, "lens"), (4, 64, "none"), (5, 65, "lens"),
               (1, 255, "none"), (4, 256, "none"), (5, 257, "lens"), (32, 512, "lens"), (5, 512, "none")]


@pytest.mark.parametrize("dk", HEAD_DIMS)
def test_seq_attn_counting(abi_dev, dk):
    """q = 0: lse[i] = log(the number of keys the mask allows), out[i] = the mean of their v rows (the docstring's counting)."""
    dev, be = abi_dev, _backend(abi_dev)
    for Lq, Lk, mask in COUNT_CASES:
        B, H = (4 if mask == "causal+lens" else 3), 3
        causal = mask.startswith("causal")
        lens = _lens_for("lens" if mask.endswith("lens") else "none", B, Lk)
        g = torch.Generator().manual_seed(Lq + 3 * Lk + dk)
        hk = H * dk
        q = torch.zeros(B * Lq, hk).bfloat16()
        k = torch.randn(B * Lk, hk, generator=g).bfloat16()
        v = (torch.randint(-32, 33, (B * Lk, hk), generator=g).float() / 4).bfloat16()
        prob = _Seq(dev, dk, B, H, Lq, Lk, q, k, v)
        out, lse = prob.fwd(f32(dk ** -0.5), causal, lens)
        allow = _allow(B, Lq, Lk, causal, lens).expand(B, H, Lq, Lk)
        n = allow.sum(-1).double()
        a = _attn_adds(be, "seq", dk, Lk)[1]
        tag = f"counting {be} dk {dk} {Lq} x {Lk} {mask}"
        _inside(tag + " lse", lse, torch.log(n), torch.full_like(n, (a + 2) * U + E_FAST))
        mean = (allow.double() @ _split(v, B, Lk, H, dk)) / n[..., None]
        o = _split(out, B, Lq, H, dk)
        pow2 = (n == 2.0 ** torch.round(torch.log2(n)))[..., None].expand_as(o)
        assert torch.equal(o[pow2], mean.bfloat16().double()[pow2]), tag
        _inside(tag + " out", o, mean, (BF_ULP + 4 * U) * mean.abs())
        if mask == "none":
            assert bool(pow2.all()) == (Lk & (Lk - 1) == 0)


# ------------------------------------------------------------------------------------------------ dropout
def _keep_factors(sp, B, H, Lq, Lk):
    """[B, H, Lq, Lk] float64 factors 0 or fp32(1 / (1 - p)) by the hash of include/dig_hip.h on ((query << 16) | key, sample * heads + head)."""
    M = np.uint64(0xffffffff)
    a = (np.arange(Lq, dtype=np.uint64)[:, None] << np.uint64(16)) | np.arange(Lk, dtype=np.uint64)[None, :]
    b = np.arange(B * H, dtype=np.uint64)[:, None, None]
    x = (a[None] ^ np.uint64(sp.k0)) & M
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7feb352d)) & M
    x = (x + np.uint64(sp.k1) + ((b * np.uint64(0x9e3779b9)) & M)) & M
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846ca68b)) & M
    x = x ^ (x >> np.uint64(16))
    keep = torch.from_numpy((x >= np.uint64(sp.thr)).reshape(B, H, Lq, Lk))
    return keep.double() * float(np.float32(sp.scale))


@pytest.mark.parametrize("dk", HEAD_DIMS)
def test_seq_attn_dropout(abi_dev, dk):
    """Attention dropout p = 0.1 on both sides of the Lk <= 64 switch: the dropped probabilities are the normalised ones times 1 / (1 - p) (lse is
    the bits of the run without dropout, out and the gradients inside the bounds with the factors in), thr = 0 is the run without dropout."""
    from dig_amd import dropout as DR
    dev, be = abi_dev, _backend(abi_dev)
    plan = DR.DropPlan(5, 11)
    for Lq, Lk, mask, kind in ((25, 25, "causal+lens", 0), (25, 100, "none", 2)):
        prob, B, H, scale, causal, lens, (q, k, v, do), allow = _seq_setup(dev, dk, Lq, Lk, mask, 0, 0)
        adds = _attn_adds(be, "seq", dk, Lk)
        sp = plan.spec(DR.dec_site(1, kind), 0.1)
        keep = _keep_factors(sp, B, H, Lq, Lk)
        frac = float((keep == 0).double().mean())
        assert 0.05 < frac < 0.15, frac
        tag = f"dropout {be} dk {dk} {Lq} x {Lk}"
        out0, lse0 = prob.fwd(scale, causal, lens)
        out, lse = prob.fwd(scale, causal, lens, drop=sp)
        assert torch.equal(lse, lse0), tag
        assert not torch.equal(out, out0), tag
        ref = _fwd_ref(q, k, v, scale, allow, (adds[0], adds[1], adds[2] + 1), keep)
        _check_fwd(tag, out, lse, ref, B, Lq)
        got = prob.bwd(scale, causal, lens, lse, drop=sp)
        want, bnd = _bwd_ref(q, k, v, do, scale, allow, lse.double(), adds[0], adds[1], keep)
        for name, a, r, b, L_ in zip(("dq", "dk", "dv"), got, want, bnd, (Lq, Lk, Lk)):
            _inside(f"{tag} {name}", _split(a, B, L_, H, dk), r, b)
        off = DR.DropSpec()
        off.k0, off.k1, off.thr, off.scale = sp.k0, sp.k1, 0, sp.scale
        out1, lse1 = prob.fwd(scale, causal, lens, drop=off)
        assert torch.equal(out1, out0) and torch.equal(lse1, lse0), tag
        g0, g1 = prob.bwd(scale, causal, lens, lse0), prob.bwd(scale, causal, lens, lse0, drop=off)
        assert all(torch.equal(a, b) for a, b in zip(g0, g1)), tag
        if dk == 64:
            o2, l2 = prob.fwd(scale, causal, lens, drop=sp, form="_dropout")
            g2 = prob.bwd(scale, causal, lens, lse, drop=sp, form="_dropout")
            assert torch.equal(o2, out) and torch.equal(l2, lse) and all(torch.equal(a, b) for a, b in zip(got, g2)), tag


def test_seq_attn_refusals(abi_dev):
    """Every refusal returns before a launch and leaves the poisoned outputs untouched; a backward above 64 KiB of LDS still runs after them."""
    dev, be = abi_dev, _backend(abi_dev)
    L = _L()
    assert L.const("DIG_SEQ_ATTN_BWD_LDS_LIMIT") == 160 * 1024
    for dk in HEAD_DIMS:
        assert min(512, (160 * 1024 - 256 * dk) // (256 + 2 * dk)) == {64: 384, 48: 430, 24: 512}[dk]
    B, H, Lq, Lk = 3, 3, 5, 512
    for dk, over in ((64, 385), (48, 431), (24, None)):
        q, k, v, do = _seq_data(dk, B, H, Lq, Lk, dk)
        prob = _Seq(dev, dk, B, H, Lq, Lk, q, k, v, do)
        hk = H * dk
        out, lse, g = prob._mk("out", B * Lq, None), _buf(dev, B * H * Lq), prob.grads()
        lse_in = torch.zeros(B * H * Lq, device=dev)
        fa = lambda **kw: list(prob.fwd_args(out, lse, 0.125, 0, None, "_hd", None))
        ba = lambda Lk_=Lk: list(prob.bwd_args(g, lse_in, 0.125, 0, None, "_hd", None, Lk=Lk_))
        a = fa(); a[11] = 33
        _refused(ARG, "dig_seq_attn_fwd_hd", *a)
        a = fa(); a[12] = 513
        _refused(ARG, "dig_seq_attn_fwd_hd", *a)
        a = fa(); a[-2] = 32
        _refused(UNSUP, "dig_seq_attn_fwd_hd", *a)
        a = fa(); a[2] = prob.k.ptr(2)
        _refused(ALIGN, "dig_seq_attn_fwd_hd", *a)
        a = fa(); a[3] = hk + 4
        _refused(ALIGN, "dig_seq_attn_fwd_hd", *a)
        a = ba(64); a[17] = 33
        _refused(ARG, "dig_seq_attn_bwd_hd", *a)
        a = ba(513)
        _refused(ARG, "dig_seq_attn_bwd_hd", *a)
        a = ba(64); a[-2] = 32
        _refused(UNSUP, "dig_seq_attn_bwd_hd", *a)
        if over:
            _refused(UNSUP, "dig_seq_attn_bwd_hd", *ba(over))
            _refused(UNSUP, "dig_seq_attn_bwd_hd", *ba(512))
            if dk == 64:
                for form in ("", "_dropout"):
                    a = list(prob.bwd_args(g, lse_in, 0.125, 0, None, form, None, Lk=over))
                    _refused(UNSUP, _Seq.BWD[form], *a)
        for Lk_ in (64, 256):                                                              # both paths of the backward: 16-byte dK / dV stores
            a = ba(Lk_); a[4] = prob.v.ptr(2)
            _refused(ALIGN, "dig_seq_attn_bwd_hd", *a)
            a = ba(Lk_); a[11] = g[1].ptr(2)
            _refused(ALIGN, "dig_seq_attn_bwd_hd", *a)
            a = ba(Lk_); a[13] = g[2].ptr(2)
            _refused(ALIGN, "dig_seq_attn_bwd_hd", *a)
            a = ba(Lk_); a[12] = hk + 4
            _refused(ALIGN, "dig_seq_attn_bwd_hd", *a)
            a = ba(Lk_); a[14] = hk + 4
            _refused(ALIGN, "dig_seq_attn_bwd_hd", *a)
        _sync(dev)
        assert out.untouched() and _untouched(lse) and all(t.untouched() for t in g), dk
    # the high-water mark of the LDS limit is not moved by a refused shape: a legitimate backward above 64 KiB runs and is inside its bounds
    prob, B, H, scale, causal, lens, (q, k, v, do), allow = _seq_setup(dev, 64, 5, 256, "none", 0, 0)
    adds = _attn_adds(be, "seq", 64, 256)
    out, lse = prob.fwd(scale, causal, lens)
    got = prob.bwd(scale, causal, lens, lse)
    want, bnd = _bwd_ref(q, k, v, do, scale, allow, lse.double(), adds[0], adds[1])
    for name, a, r, b, L_ in zip(("dq", "dk", "dv"), got, want, bnd, (5, 256, 256)):
        _inside(f"after the refusals {be} {name}", _split(a, B, L_, H, 64), r, b)


# ================================================================================================ decode: self-attention
def _self_run(dev, qkv, B, T, H, dk, t, scale):
    L = _L()
    hk = H * dk
    cache = qkv.clone()
    cache[:, t + 1:] = math.nan                                                          # rows above t must not be read
    cd, out = _put(dev, cache), _buf(dev, B * hk, BF)
    L.call("dig_decode_self_attn", L.ptr(cd), L.ptr(out), B, T, H, dk, t, cf(scale), L.stream())
    _sync(dev)
    assert _guard_ok(out, B * hk)
    return _get(out, B * hk, B, hk)


def _self_operands(qkv, B, H, dk, t):
    hk = H * dk
    q = _split(qkv[:, t, :hk].reshape(B, hk), B, 1, H, dk)
    k = _split(qkv[:, :t + 1, hk:2 * hk].reshape(B * (t + 1), hk), B, t + 1, H, dk)
    v = _split(qkv[:, :t + 1, 2 * hk:].reshape(B * (t + 1), hk), B, t + 1, H, dk)
    return q, k, v


@pytest.mark.parametrize("dk", HEAD_DIMS)
def test_decode_self_attn_vs_fp64(abi_dev, dk):
    dev, be = abi_dev, _backend(abi_dev)
    B, H = 3, 3
    hk = H * dk
    for T, t in ((1, 0), (26, 0), (26, 1), (26, 25)):
        for unit in (0, 1):
            scale = 1.0 if unit else f32(dk ** -0.5)
            g = torch.Generator().manual_seed(dk + 31 * T + t)
            qkv = torch.randn(B, T, 3 * hk, generator=g).bfloat16()
            out = _self_run(dev, qkv, B, T, H, dk, t, scale)
            q, k, v = _self_operands(qkv, B, H, dk, t)
            adds = _attn_adds(be, "self", dk, t + 1)
            s = (q @ k.transpose(-1, -2)) * scale
            extra = 2 * (t * E_FAST + U * (s.amax(-1, keepdim=True) - s.amin(-1, keepdim=True))) if be == "hip" else 0.0
            ref = _fwd_ref(q, k, v, scale, torch.ones(B, 1, 1, t + 1, dtype=torch.bool), adds, extra=extra)
            _inside(f"decode_self {be} dk {dk} T {T} t {t} scale {scale:.3g}", _split(out, B, 1, H, dk), ref["out"], ref["b_out"])


@pytest.mark.parametrize("dk", HEAD_DIMS)
def test_decode_self_attn_routing_and_refusals(abi_dev, dk):
    """Row t's query is the code of one cached key: the output is that key's v row bit for bit, wherever the target sits among the t + 1 rows."""
    dev = abi_dev
    L = _L()
    B, H, T = 3, 3, 26
    hk = H * dk
    scale = f32(dk ** -0.5)
    g = torch.Generator().manual_seed(dk)
    for t in (0, 1, 12, 25):
        pi = _pi(B, H, 1, t + 1, False, None, dk + t)[..., 0]                            # [B, H]
        if t == 25:
            pi[0, 0], pi[0, 1] = 0, 25                                                   # the first and the last row
        kc = _codes(T, dk, 9)
        qkv = torch.zeros(B, T, 3, H, dk)
        qkv[:, :, 1] = kc[None, :, None, :]
        qkv[:, :, 2] = torch.randn(B, T, H, dk, generator=g)
        qkv[:, t, 0] = kc[pi]
        qkv = qkv.reshape(B, T, 3 * hk).bfloat16()
        out = _self_run(dev, qkv, B, T, H, dk, t, scale)
        v = qkv[:, :, 2 * hk:].reshape(B, T, H, dk)
        want = torch.gather(v, 1, pi[:, None, :, None].expand(B, 1, H, dk))[:, 0]
        assert torch.equal(out.reshape(B, H, dk), want), (dk, t)
    cd, out = _put(dev, qkv), _buf(dev, B * hk, BF)
    _refused(ARG, "dig_decode_self_attn", L.ptr(cd), L.ptr(out), B, T, H, dk, T, cf(scale), L.stream())
    _refused(ARG, "dig_decode_self_attn", L.ptr(cd), L.ptr(out), B, T, H, dk, -1, cf(scale), L.stream())
    _refused(UNSUP, "dig_decode_self_attn", L.ptr(cd), L.ptr(out), B, T, H, 32, 0, cf(scale), L.stream())
    _sync(dev)
    assert _untouched(out)


# ================================================================================================ decode: cross-attention
N_MEM = [1, 31, 32, 33, 255, 256, 257, 8192]


def _cross_run(dev, q, kv, B, Nm, H, dk, scale, spm, with_w):
    L = _L()
    hk = H * dk
    qd, kvd, out = _put(dev, q), _put(dev, kv), _buf(dev, B * hk, BF)
    w = _buf(dev, B * H * Nm) if with_w else None
    L.call("dig_decode_cross_attn", L.ptr(qd), L.ptr(kvd), L.ptr(out), L.ptr(w), B, Nm, H, dk, cf(scale), spm, L.stream())
    _sync(dev)
    assert _guard_ok(out, B * hk) and (w is None or _guard_ok(w, B * H * Nm))
    return _get(out, B * hk, B, hk), (_get(w, B * H * Nm, B, H, Nm) if with_w else None)


def _cross_operands(q, kv, B, Nm, H, dk, spm):
    """slots as queries: [G, H, spm, dk] against the G memories [G, H, Nm, dk]"""
    G, hk = B // spm, H * dk
    q4 = _split(q.reshape(B, hk), G, spm, H, dk)
    k4 = _split(kv[:, :, :hk].reshape(G * Nm, hk), G, Nm, H, dk)
    v4 = _split(kv[:, :, hk:].reshape(G * Nm, hk), G, Nm, H, dk)
    return q4, k4, v4


@pytest.mark.parametrize("dk", HEAD_DIMS)
def test_decode_cross_attn_vs_fp64(abi_dev, dk):
    dev, be = abi_dev, _backend(abi_dev)
    B, H = 10, 3
    hk = H * dk
    for Nm in N_MEM:
        for spm in ((5,) if Nm == 8192 else (1, 5)):
            G = B // spm
            scale = 1.0 if (Nm % 2 == 0 and spm == 1) else f32(dk ** -0.5)
            g = torch.Generator().manual_seed(dk + Nm + spm)
            q = torch.randn(B, hk, generator=g).bfloat16()
            kv = torch.randn(G, Nm, 2 * hk, generator=g).bfloat16()
            q4, k4, v4 = _cross_operands(q, kv, B, Nm, H, dk, spm)
            ref = _fwd_ref(q4, k4, v4, scale, torch.ones(G, 1, spm, Nm, dtype=torch.bool), _attn_adds(be, "cross", dk, Nm))
            tag = f"decode_cross {be} dk {dk} n_mem {Nm} slots {spm} scale {scale:.3g}"
            out, w = _cross_run(dev, q, kv, B, Nm, H, dk, scale, spm, True)
            _inside(tag + " out", _split(out, G, spm, H, dk), ref["out"], ref["b_out"])
            wg = w.reshape(G, spm, H, Nm).permute(0, 2, 1, 3)
            _inside(tag + " weights", wg, ref["p"], ref["b_p"])
            _inside(tag + " weight sums", wg.double().sum(-1), torch.ones(G, H, spm, dtype=F64), ref["b_p"].sum(-1))
            out2, _ = _cross_run(dev, q, kv, B, Nm, H, dk, scale, spm, False)
            assert torch.equal(out, out2), tag


@pytest.mark.parametrize("dk", HEAD_DIMS)
def test_decode_cross_attn_routing_and_refusals(abi_dev, dk):
    """One-hot `weights` and out == v[pi] bit for bit; the five beam slots of one memory are routed to different keys."""
    dev = abi_dev
    L = _L()
    B, H, spm = 10, 3, 5
    G, hk = B // spm, H * dk
    scale = f32(dk ** -0.5)
    for Nm in (5, 33, 257, 8192):
        g = torch.Generator().manual_seed(dk + Nm)
        pi = (torch.randint(0, Nm, (G, H, 1), generator=g) + torch.arange(spm)[None, None, :] * (Nm // spm)) % Nm       # [G, H, spm], distinct per slot
        kc = _codes(Nm, dk, 13)
        kv = torch.zeros(G, Nm, 2, H, dk)
        kv[:, :, 0] = kc[None, :, None, :]
        kv[:, :, 1] = torch.randn(G, Nm, H, dk, generator=g)
        kv = kv.reshape(G, Nm, 2 * hk).bfloat16()
        q = kc[pi].permute(0, 2, 1, 3).reshape(B, hk).bfloat16()                         # [G, H, spm, dk] -> [G * spm, H * dk]
        out, w = _cross_run(dev, q, kv, B, Nm, H, dk, scale, spm, True)
        v = kv[:, :, hk:].reshape(G, Nm, H, dk).permute(0, 2, 1, 3)                     # [G, H, Nm, dk]
        want = torch.gather(v, 2, pi[..., None].expand(G, H, spm, dk))
        assert torch.equal(out.reshape(G, spm, H, dk).permute(0, 2, 1, 3), want), (dk, Nm)
        onehot = torch.zeros(G, H, spm, Nm).scatter_(3, pi[..., None], 1.0)
        assert torch.equal(w.reshape(G, spm, H, Nm).permute(0, 2, 1, 3), onehot), (dk, Nm)
    Nm = 33
    q, kv = torch.zeros(B, hk).bfloat16(), torch.zeros(G, Nm + 1, 2 * hk).bfloat16()
    qd, kvd, out, w = _put(dev, q), _put(dev, kv), _buf(dev, B * hk, BF), _buf(dev, B * H * Nm)
    tail = lambda d=dk, s=spm: (d, cf(scale), s, L.stream())
    _refused(UNSUP, "dig_decode_cross_attn", L.ptr(qd), L.ptr(kvd), L.ptr(out), L.ptr(w), B, 8193, H, *tail())
    _refused(ARG, "dig_decode_cross_attn", L.ptr(qd), L.ptr(kvd), L.ptr(out), L.ptr(w), B, Nm, H, *tail(s=3))
    _refused(UNSUP, "dig_decode_cross_attn", L.ptr(qd), L.ptr(kvd), L.ptr(out), L.ptr(w), B, Nm, H, *tail(d=32))
    _refused(ALIGN, "dig_decode_cross_attn", L.ptr(qd), _off(kvd, 2), L.ptr(out), L.ptr(w), B, Nm, H, *tail())
    _refused(ALIGN, "dig_decode_cross_attn", _off(qd, 2), L.ptr(kvd), L.ptr(out), L.ptr(w), B, Nm, H, *tail())
    _sync(dev)
    assert _untouched(out) and _untouched(w)


# ================================================================================================ softmax + argmax
SM_C = [1, 63, 64, 65, 97, 200]


def _row_adds(be, C):
    return (-(-C // 64) - 1 + 6) if be == "hip" else max(C - 1, 0)


def _sm_rows(C, seed):
    """Logit rows: randn 3, then the tie and infinity rows that fit C."""
    g = torch.Generator().manual_seed(seed)
    rows = [torch.randn(C, generator=g) * 3 for _ in range(3)]
    def tie(*idx):
        r = torch.randn(C, generator=g).clamp_max(2.0)
        for i in idx:
            r[i] = 5.0
        return r
    rows.append(tie(0, C - 1))
    if C > 70:
        rows += [tie(6, 70), tie(3, 65), tie(65, 70)]
    if C > 134:
        rows += [tie(70, 134), tie(67, 131, 6 + 128)]
    if C > 3:
        r = tie(C - 2, C - 1)                                                            # -inf beside finite entries: the first of the finite maxima
        r[0::2] = -INF
        r[C - 2], r[C - 1] = 5.0, 5.0
        rows.append(r)
        r = torch.full((C,), -INF)
        r[C - 1] = -3.0                                                                  # one finite entry, last
        rows.append(r)
    r = torch.full((C,), -80.0)
    r[C // 2] = 80.0
    rows.append(r)
    rows.append(torch.full((C,), -INF))                                                  # no entry above -inf: token 0
    return torch.stack(rows)


@pytest.mark.parametrize("C", SM_C)
def test_softmax_argmax_vs_fp64(abi_dev, C):
    dev, be = abi_dev, _backend(abi_dev)
    L = _L()
    x = _sm_rows(C, C)
    B, ld = x.shape[0], C + 3
    xp = torch.full((B, ld), math.nan)
    xp[:, :C] = x
    xd, probs, tok = _put(dev, xp), _buf(dev, B * C), torch.full((B + GUARD,), -7, dtype=I64, device=dev)
    _refused(ARG, "dig_softmax_argmax", L.ptr(xd), C - 1, L.ptr(probs), L.ptr(tok), B, C, L.stream())
    _refused(ARG, "dig_softmax_argmax", L.ptr(xd), ld, L.ptr(probs), L.ptr(tok), 0, C, L.stream())
    _sync(dev)
    assert _untouched(probs) and bool((tok == -7).all())
    L.call("dig_softmax_argmax", L.ptr(xd), ld, L.ptr(probs), L.ptr(tok), B, C, L.stream())
    _sync(dev)
    assert _guard_ok(probs, B * C) and bool((tok[B:] == -7).all())
    x64 = x.double()
    want = torch.argmax(x64, 1)                                                         # the first index of the maximum
    want[-1] = 0
    assert torch.equal(tok[:B].cpu(), want), (C, tok[:B].cpu(), want)
    live = slice(0, B - 1)                                                              # (the row of -inf has NaN probabilities, as torch.softmax)
    m = x64[live].amax(1, keepdim=True)
    p = torch.softmax(x64[live], 1)
    d = torch.where(torch.isfinite(x64[live]), (x64[live] - m).abs(), torch.zeros_like(p))
    rho = U * d + (p * U * d).sum(1, keepdim=True) + 2 * E_FAST + (_row_adds(be, C) + 3) * U
    bnd = 1.01 * p * rho + TINY
    got = _get(probs, B * C, B, C)[live]
    _inside(f"softmax_argmax {be} C {C} probs", got, p, bnd)
    _inside(f"softmax_argmax {be} C {C} prob sums", got.double().sum(1), torch.ones(B - 1, dtype=F64), bnd.sum(1))


# ================================================================================================ embeddings
EMB_D = [1, 255, 256, 257, 640]


@pytest.mark.parametrize("d", EMB_D)
def test_embed_fwd_is_the_correctly_rounded_sum(abi_dev, d):
    """dig_seq_embed_fwd and dig_decode_embed: bf16(fp32(emb[clamp(token)] + pos)), no tolerance (the docstring: the float64 sum is exact)."""
    dev = abi_dev
    L = _L()
    vocab, B, T = 7, 3, 5
    g = torch.Generator().manual_seed(d)
    emb, pos = torch.randn(vocab, d, generator=g), torch.randn(T, d, generator=g)
    tok = torch.tensor([[0, 6, -1, 7, 3], [-3, 14, 2, 2, 5], [1, 4, 6, 0, vocab]], dtype=I64)
    tc = tok.clamp(0, vocab - 1)
    s64 = emb.double()[tc] + pos.double()[None]
    want = s64.float().bfloat16()
    ed, pd, td, x = _put(dev, emb), _put(dev, pos), _put(dev, tok), _buf(dev, B * T * d, BF)
    L.call("dig_seq_embed_fwd", L.ptr(td), L.ptr(ed), L.ptr(pd), L.ptr(x), B, T, d, vocab, L.stream())
    _sync(dev)
    assert _guard_ok(x, B * T * d)
    assert torch.equal(_get(x, B * T * d, B, T, d), want), d
    for t in (0, T - 1):
        x = _buf(dev, B * d, BF)
        td = _put(dev, tok[:, t])
        L.call("dig_decode_embed", L.ptr(td), L.ptr(ed), _off(pd, t * d * 4), L.ptr(x), B, d, vocab, L.stream())
        _sync(dev)
        assert _guard_ok(x, B * d) and torch.equal(_get(x, B * d, B, d), want[:, t]), (d, t)
    x = _buf(dev, B * T * d, BF)
    _refused(ARG, "dig_seq_embed_fwd", L.ptr(td), L.ptr(ed), L.ptr(pd), L.ptr(x), B, T, d, 0, L.stream())
    _refused(ARG, "dig_decode_embed", L.ptr(td), L.ptr(ed), L.ptr(pd), L.ptr(x), B, 0, vocab, L.stream())
    _sync(dev)
    assert _untouched(x)


EMB_BWD = [(1, 257, 1), (255, 257, 5), (256, 257, 8), (257, 257, 257), (257, 1, 257), (257, 256, 1), (257, 640, 257), (15360, 257, 30)]       # (n_tok, d, T)


@pytest.mark.parametrize("n_tok,d,T", EMB_BWD)
def test_embed_bwd_is_exact_on_dyadic_data(abi_dev, n_tok, d, T):
    """dx multiples of 1/4: demb == start + the float64 sums bit for bit for dig_seq_embed_bwd and dig_seq_embed_bwd_lens; the gradient of an
    out-of-range token goes to the row the forward read."""
    dev = abi_dev
    L = _L()
    vocab = 6
    g = torch.Generator().manual_seed(n_tok + d)
    dx = (torch.randint(-32, 33, (n_tok, d), generator=g).float() / 4).bfloat16()
    start = torch.randint(-32, 33, (vocab, d), generator=g).float() / 4
    nb = n_tok // T
    for kind in ("mixed", "equal"):
        if kind == "equal":
            tok = torch.full((n_tok,), 2, dtype=I64)
        else:
            tok = torch.randint(-2, vocab + 2, (n_tok,), generator=g)
            tok[tok == 4] = 3                                                            # token 4 has no hits
        tc = tok.clamp(0, vocab - 1)
        lens = torch.tensor([0, 1, T, T + 2, max(1, T // 2)], dtype=I64)[torch.arange(nb) % 5]
        if nb == 1:
            lens = torch.tensor([max(1, (2 * T) // 5)], dtype=I64)
        for use_lens in (False, True):
            live = torch.ones(n_tok, dtype=torch.bool)
            if use_lens:
                live = (torch.arange(n_tok) % T) < lens[torch.arange(n_tok) // T]
            want = start.double().index_add(0, tc[live], dx.double()[live])
            if kind == "mixed":
                assert torch.equal(want[4], start.double()[4])
            td, dxd, ld = _put(dev, tok), _put(dev, dx), _put(dev, lens)
            runs = []
            for rep in range(2):
                demb = _put(dev, start)
                if use_lens:
                    L.call("dig_seq_embed_bwd_lens", L.ptr(td), L.ptr(dxd), L.ptr(demb), n_tok, d, vocab, T, L.ptr(ld), L.stream())
                else:
                    L.call("dig_seq_embed_bwd", L.ptr(td), L.ptr(dxd), L.ptr(demb), n_tok, d, vocab, L.stream())
                _sync(dev)
                assert _guard_ok(demb, vocab * d) and _guard_ok(dxd, n_tok * d)
                runs.append(_get(demb, vocab * d, vocab, d))
            assert torch.equal(runs[0].double(), want), (n_tok, d, kind, use_lens, float((runs[0].double() - want).abs().max()))
            assert torch.equal(runs[0], runs[1])


def test_embed_bwd_refusals(abi_dev):
    dev = abi_dev
    L = _L()
    n, d, vocab = 15361, 8, 4
    td, dxd, demb = _put(dev, torch.zeros(n, dtype=I64)), _put(dev, torch.zeros(n, d).bfloat16()), _buf(dev, vocab * d)
    ld = _put(dev, torch.ones(n, dtype=I64))
    _refused(UNSUP, "dig_seq_embed_bwd", L.ptr(td), L.ptr(dxd), L.ptr(demb), n, d, vocab, L.stream())
    _refused(UNSUP, "dig_seq_embed_bwd_lens", L.ptr(td), L.ptr(dxd), L.ptr(demb), n, d, vocab, 1, L.ptr(ld), L.stream())
    _refused(ARG, "dig_seq_embed_bwd_lens", L.ptr(td), L.ptr(dxd), L.ptr(demb), 257, d, vocab, 5, L.ptr(ld), L.stream())
    _refused(ARG, "dig_seq_embed_bwd_lens", L.ptr(td), L.ptr(dxd), L.ptr(demb), 256, d, vocab, 0, L.ptr(ld), L.stream())
    _refused(ARG, "dig_seq_embed_bwd", L.ptr(td), L.ptr(dxd), L.ptr(demb), 0, d, vocab, L.stream())
    _sync(dev)
    assert _untouched(demb)


# ================================================================================================ sequence losses
LOSS_C = [1, 63, 64, 65, 97, 200]
LOSS_BT = [(1, 1), (7, 25), (4, 65), (70, 5)]
SMOOTH = [0.0, f32(0.1), 1.0]


def _term_adds(be, n):
    return (-(-n // 256) - 1 + 8) if be == "hip" else 0


def _loss_case(B, T, C, seed):
    g = torch.Generator().manual_seed(seed)
    n = B * T
    x = torch.randn(n, C, generator=g) * 3
    if n > 4:
        x[3] = -80.0
        x[3, C // 2] = 80.0
        if C > 1:
            x[4] = torch.where(torch.arange(C) % 2 == 0, 80.0, -80.0)
    tgt = torch.randint(0, C, (n,), generator=g)
    tgt[0::7] = -1
    tgt[1::11] = C + 5
    lens = torch.tensor([T, 0, T + 3, -2, max(1, T // 2)], dtype=I64)[torch.arange(B) % 5] if B > 1 else torch.tensor([T], dtype=I64)
    return x, tgt, lens


def _rows_ref(x, be):
    """Per row: float64 max, log-sum-exp, probabilities, and R_s, the relative bound of the row sum."""
    C = x.shape[1]
    a = _row_adds(be, C)
    x = x.double()
    m = x.amax(1, keepdim=True)
    e = torch.exp(x - m)
    s = e.sum(1, keepdim=True)
    p = e / s
    R = (a + 4) * U + 3 * U * (p * (x - m).abs()).sum(1, keepdim=True) + E_FAST
    e_log = E_FAST * (1 + torch.log(s).clamp_min(1.0))
    return m[:, 0], (m + torch.log(s))[:, 0], p, R[:, 0], e_log[:, 0]


def _ce_ref(x, tgt, lens, B, T, be):
    n, C = x.shape
    m, lse, p, R, e_log = _rows_ref(x, be)
    y = tgt.clamp(0, C - 1)
    xy = x.double()[torch.arange(n), y]
    mask = (torch.arange(n) % T) < lens[torch.arange(n) // T]
    term = torch.where(mask, lse - xy, torch.zeros_like(lse))
    r = torch.where(mask, R + e_log + 3 * U * (m.abs() + lse.abs() + xy.abs()), torch.zeros_like(lse))
    loss = term.sum() / B
    b_loss = (r.sum() + (_term_adds(be, n) + 1) * U * term.abs().sum()) / B + 3 * U * loss.abs()
    return dict(term=term, r=r, loss=loss, b_loss=b_loss, mask=mask, y=y, p=p, R=R, m=m, lse=lse, e_log=e_log)


def _pad_logits(x, ld):
    xp = torch.full((x.shape[0], ld), math.nan)
    xp[:, :x.shape[1]] = x
    return xp


def _grad_run(dev, name, xp, ld, tgt, lens, gs, B, T, C, ldd, smoothing=None):
    L = _L()
    n = B * T
    xd, td, lend = _put(dev, xp), _put(dev, tgt), _put(dev, lens)
    gd = _put(dev, torch.tensor([gs])) if gs is not None else None
    out = _buf(dev, n * ldd, BF)
    sm = () if smoothing is None else (cf(smoothing),)
    L.call(name, L.ptr(xd), ld, L.ptr(td), L.ptr(lend), L.ptr(gd), B, T, C, *sm, L.ptr(out), ldd, L.stream())
    _sync(dev)
    assert _guard_ok(out, n * ldd)
    return _get(out, n * ldd, n, ldd)


@pytest.mark.parametrize("B,T", LOSS_BT)
@pytest.mark.parametrize("C", LOSS_C)
def test_seq_cross_entropy_vs_fp64(abi_dev, C, B, T):
    dev, be = abi_dev, _backend(abi_dev)
    L = _L()
    n = B * T
    x, tgt, lens = _loss_case(B, T, C, 100 * C + n)
    ref = _ce_ref(x, tgt, lens, B, T, be)
    tag = f"seq_ce {be} C {C} B {B} T {T}"
    xd, td, lend = _put(dev, x), _put(dev, tgt), _put(dev, lens)
    runs = []
    for rep in range(2):
        ws, loss = _ws(dev, n), _buf(dev, 1)
        L.call("dig_seq_cross_entropy", L.ptr(xd), L.ptr(td), L.ptr(lend), B, T, C, L.ptr(ws), L.ptr(loss), L.stream())
        _sync(dev)
        assert _guard_ok(ws, n) and _guard_ok(loss, 1)
        runs.append((_get(ws, n), _get(loss, 1)))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), tag
    rows, loss = runs[0]
    assert bool((rows[~ref["mask"]] == 0).all()), tag
    _inside(tag + " row terms", rows, ref["term"], ref["r"] + U * ref["term"].abs())
    _inside(tag + " loss", loss, ref["loss"].reshape(1), ref["b_loss"].reshape(1))
    # the gradient
    ld, ldd = C + 3, C + 5
    one = torch.zeros(n, C, dtype=F64)
    one[torch.arange(n), ref["y"]] = 1
    z = (x.double() - ref["m"][:, None]).abs()
    for gs in (None, f32(0.37)):
        sc = (1.0 if gs is None else gs) / B
        live = ref["mask"][:, None].double()
        want = live * sc * (ref["p"] - one)
        bnd = live * (BF_ULP * want.abs() + 1.01 * sc * (ref["p"] * (ref["R"][:, None] + 3 * U * z + 4 * U + E_FAST) + 2 * U * (ref["p"] - one).abs() + TINY)
                      + 3 * U * want.abs())
        d = _grad_run(dev, "dig_seq_cross_entropy_bwd", _pad_logits(x, ld), ld, tgt, lens, gs, B, T, C, ldd)
        assert bool((d[:, C:] == 0).all()) and bool((d[~ref["mask"]] == 0).all()), tag
        _inside(f"{tag} g {gs} dlogits", d[:, :C], want, bnd)
        _inside(f"{tag} g {gs} dlogits row sums", d[:, :C].double().sum(1), torch.zeros(n, dtype=F64), bnd.sum(1))


def _ls_ref(x, tgt, lens, B, T, smoothing, be):
    n, C = x.shape
    ce = _ce_ref(x, tgt, lens, B, T, be)
    a, k = _row_adds(be, C), _term_adds(be, n)
    x64 = x.double()
    sj = ce["lse"] - x64.mean(1)
    e_sj = ce["R"] + ce["e_log"] + 2 * U * (ce["m"].abs() + ce["lse"].abs()) + (a + 2) * U * x64.abs().mean(1) + U * sj.abs()
    cnt = float(lens.clamp(0, T).sum())
    conf = 1.0 - smoothing
    t1, t2 = conf * n * ce["term"].sum() / B, smoothing * cnt * sj.sum() / B
    b = (conf * n * (ce["r"].sum() + (k + 1) * U * ce["term"].abs().sum()) + smoothing * cnt * (e_sj.sum() + (k + 1) * U * sj.abs().sum())) / B
    b = b + 8 * U * (abs(conf) * n * ce["term"].abs().sum() + smoothing * cnt * sj.abs().sum()) / B
    return ce, t1 + t2, b, cnt, sj, e_sj


@pytest.mark.parametrize("B,T", LOSS_BT)
@pytest.mark.parametrize("C", LOSS_C)
def test_seq_ls_cross_entropy_vs_fp64(abi_dev, C, B, T):
    dev, be = abi_dev, _backend(abi_dev)
    L = _L()
    n = B * T
    x, tgt, lens = _loss_case(B, T, C, 100 * C + n + 1)
    tag = f"seq_ls_ce {be} C {C} B {B} T {T}"
    xd, td, lend = _put(dev, x), _put(dev, tgt), _put(dev, lens)
    ld, ldd = C + 3, C + 5
    for sm in SMOOTH:
        ce, want, b_loss, cnt, sj, e_sj = _ls_ref(x, tgt, lens, B, T, sm, be)
        runs = []
        for rep in range(2):
            ws, loss = _ws(dev, 2 * n), _buf(dev, 1)
            L.call("dig_seq_ls_cross_entropy", L.ptr(xd), L.ptr(td), L.ptr(lend), B, T, C, cf(sm), L.ptr(ws), L.ptr(loss), L.stream())
            _sync(dev)
            assert _guard_ok(ws, 2 * n) and _guard_ok(loss, 1)
            runs.append((_get(ws, 2 * n), _get(loss, 1)))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), tag
        rows, loss = runs[0]
        _inside(f"{tag} sm {sm:.2g} nll rows", rows[:n], ce["term"], ce["r"] + U * ce["term"].abs())
        _inside(f"{tag} sm {sm:.2g} smooth rows", rows[n:], sj, e_sj)
        _inside(f"{tag} sm {sm:.2g} loss", loss, want.reshape(1), b_loss.reshape(1))
        if sm == 0.0:                                                                     # B T times the plain loss within the two bounds
            ws, plain = _ws(dev, n), _buf(dev, 1)
            L.call("dig_seq_cross_entropy", L.ptr(xd), L.ptr(td), L.ptr(lend), B, T, C, L.ptr(ws), L.ptr(plain), L.stream())
            _sync(dev)
            _inside(f"{tag} against B T times the plain loss", loss, n * _get(plain, 1).double(), (b_loss + n * ce["b_loss"]).reshape(1))
        one = torch.zeros(n, C, dtype=F64)
        one[torch.arange(n), ce["y"]] = 1
        z = (x.double() - ce["m"][:, None]).abs()
        p = ce["p"]
        eP = p * (ce["R"][:, None] + 3 * U * z + 4 * U + E_FAST) + TINY
        wn = ce["mask"][:, None].double() * (1.0 - sm) * n
        wsm = sm * cnt
        for gs in (None, f32(0.37)):
            sc = (1.0 if gs is None else gs) / B
            want_d = sc * (wn * (p - one) + wsm * (p - 1.0 / C))
            bnd = BF_ULP * want_d.abs() + 1.01 * sc * (wn + wsm) * eP + 8 * U * sc * (wn * (p - one).abs() + wsm * (p - 1.0 / C).abs() + wsm / C)
            d = _grad_run(dev, "dig_seq_ls_cross_entropy_bwd", _pad_logits(x, ld), ld, tgt, lens, gs, B, T, C, ldd, sm)
            assert bool((d[:, C:] == 0).all()), tag
            _inside(f"{tag} sm {sm:.2g} g {gs} dlogits", d[:, :C], want_d, bnd)
            _inside(f"{tag} sm {sm:.2g} g {gs} dlogits row sums", d[:, :C].double().sum(1), torch.zeros(n, dtype=F64), bnd.sum(1))


def test_seq_losses_are_exact_on_dominated_rows_and_refuse(abi_dev):
    """Integer logits in [-8, 8] with one class at 200: every row term is 0 or the integer gap, and the losses are exact (B a power of two;
    C = 64 and smoothing 1/4 for the label-smoothing form).  Refusals: smoothing -0.1 and 1.1, ld < C, B = 0."""
    dev = abi_dev
    L = _L()
    for B, T, C in ((4, 4, 64), (8, 33, 64), (2, 130, 64), (4, 5, 97)):
        n = B * T
        g = torch.Generator().manual_seed(n + C)
        x = torch.randint(-8, 9, (n, C), generator=g).float()
        dom = torch.randint(0, C, (n,), generator=g)
        x[torch.arange(n), dom] = 200.0
        tgt = torch.where(torch.arange(n) % 3 == 0, dom, torch.randint(0, C, (n,), generator=g))
        lens = torch.tensor([T, max(1, T // 2), 0, T + 1], dtype=I64)[torch.arange(B) % 4]
        mask = (torch.arange(n) % T) < lens[torch.arange(n) // T]
        gap = torch.where(mask, 200.0 - x[torch.arange(n), tgt], torch.zeros(n)).double()
        assert bool((gap[mask & (tgt == dom)] == 0).all()) and bool(((gap == 0) | (gap >= 192)).all())
        xd, td, lend = _put(dev, x), _put(dev, tgt), _put(dev, lens)
        both = []
        for rep in range(2):
            ws, loss = _ws(dev, n), _buf(dev, 1)
            L.call("dig_seq_cross_entropy", L.ptr(xd), L.ptr(td), L.ptr(lend), B, T, C, L.ptr(ws), L.ptr(loss), L.stream())
            _sync(dev)
            both.append((_get(ws, n), _get(loss, 1)))
        assert torch.equal(both[0][0].double(), gap), (B, T, C)
        assert float(both[0][1]) == float(gap.sum()) / B, (B, T, C)
        assert torch.equal(both[0][1], both[1][1])
        if C == 64 and n <= 16:
            sj = 200.0 - x.double().sum(1) / C
            cnt = float(lens.clamp(0, T).sum())
            want = (0.75 * n * gap.sum() + 0.25 * cnt * sj.sum()) / B
            ws, loss = _ws(dev, 2 * n), _buf(dev, 1)
            L.call("dig_seq_ls_cross_entropy", L.ptr(xd), L.ptr(td), L.ptr(lend), B, T, C, cf(0.25), L.ptr(ws), L.ptr(loss), L.stream())
            _sync(dev)
            assert torch.equal(_get(ws, 2 * n).double(), torch.cat([gap, sj])) and float(_get(loss, 1)) == float(want), (B, T, C)
    B, T, C = 4, 4, 64
    ws, loss, d = _ws(dev, 2 * n), _buf(dev, 1), _buf(dev, n * C, BF)
    for sm in (-0.1, 1.1):
        _refused(ARG, "dig_seq_ls_cross_entropy", L.ptr(xd), L.ptr(td), L.ptr(lend), B, T, C, cf(sm), L.ptr(ws), L.ptr(loss), L.stream())
        _refused(ARG, "dig_seq_ls_cross_entropy_bwd", L.ptr(xd), C, L.ptr(td), L.ptr(lend), None, B, T, C, cf(sm), L.ptr(d), C, L.stream())
    _refused(ARG, "dig_seq_ls_cross_entropy_bwd", L.ptr(xd), C - 1, L.ptr(td), L.ptr(lend), None, B, T, C, cf(0.1), L.ptr(d), C, L.stream())
    _refused(ARG, "dig_seq_cross_entropy_bwd", L.ptr(xd), C, L.ptr(td), L.ptr(lend), None, B, T, C, L.ptr(d), C - 1, L.stream())
    _refused(ARG, "dig_seq_cross_entropy", L.ptr(xd), L.ptr(td), L.ptr(lend), 0, T, C, L.ptr(ws), L.ptr(loss), L.stream())
    _sync(dev)
    assert _untouched(loss) and _untouched(d) and bool(torch.isnan(ws[:2 * n]).all())


# ================================================================================================ the bounds themselves
def test_fp32_restatement_is_inside_the_bounds():
    """Each formula in plain fp32 torch (no library) against the float64 reference, held to the bounds of the build with the longest summation
    chains.  The printed ratios are the docstring's."""
    be = "cpu_abi"
    worst = {}

    def note(name, r):
        worst[name] = max(worst.get(name, 0.0), r)

    for dk in HEAD_DIMS:
        for Lq, Lk, mask, unit, spike in ((25, 25, "causal+lens", 0, 0), (32, 100, "lens", 0, 1), (5, 384, "none", 1, 0)):
            B, H = (4 if mask == "causal+lens" else 3), 3
            scale = 1.0 if unit else f32(dk ** -0.5)
            qb, kb, vb, dob = _seq_data(dk, B, H, Lq, Lk, dk + Lk, spike, scale)
            causal = mask.startswith("causal")
            lens = _lens_for("lens" if mask.endswith("lens") else "none", B, Lk)
            allow = _allow(B, Lq, Lk, causal, lens)
            q, k, v, do = (_split(t, B, L_, H, dk) for t, L_ in ((qb, Lq), (kb, Lk), (vb, Lk), (dob, Lq)))
            adds = _attn_adds(be, "seq", dk, Lk)
            ref = _fwd_ref(q, k, v, scale, allow, adds)
            qf, kf, vf, dof = q.float(), k.float(), v.float(), do.float()
            ok = allow.expand(B, H, Lq, Lk)
            s = ((qf * f32(scale)) @ kf.transpose(-1, -2)).masked_fill(~ok, -INF)
            m = s.amax(-1, keepdim=True)
            e = torch.exp(s - m)
            sig = e.sum(-1, keepdim=True)
            out = ((e @ vf) * (1.0 / sig)).bfloat16()
            lse = (m + torch.log(sig))[..., 0]
            tag = f"restatement dk {dk} {Lq} x {Lk}"
            note("out", _inside(tag + " out", out, ref["out"], ref["b_out"]))
            note("lse", _inside(tag + " lse", lse, ref["lse"], ref["b_lse"]))
            want, bnd = _bwd_ref(q, k, v, do, scale, allow, lse.double(), adds[0], adds[1])
            P = torch.exp(((qf @ kf.transpose(-1, -2)) * f32(scale) - lse[..., None]).masked_fill(~ok, -INF))
            dP = (dof @ vf.transpose(-1, -2)).masked_fill(~ok, 0.0)
            dS = P * (dP - (P * dP).sum(-1, keepdim=True))
            got = ((dS @ kf) * f32(scale), (dS.transpose(-1, -2) @ qf) * f32(scale), P.transpose(-1, -2) @ dof)
            for name, a, r, b in zip(("dQ", "dK", "dV"), got, want, bnd):
                note(name, _inside(f"{tag} {name}", a.bfloat16(), r, b))
    for C in LOSS_C:
        B, T = 7, 25
        n = B * T
        x, tgt, lens = _loss_case(B, T, C, C)
        ce, ls_want, ls_b, cnt, sj, e_sj = _ls_ref(x, tgt, lens, B, T, f32(0.1), be)
        m = x.amax(1, keepdim=True)
        e = torch.exp(x - m)
        s = e.sum(1, keepdim=True)
        p = e / s
        rho = U * (x.double() - m.double()).abs()
        bp = 1.01 * ce["p"] * (rho + (ce["p"] * rho).sum(1, keepdim=True) + 2 * E_FAST + (_row_adds(be, C) + 3) * U) + TINY
        note("probs", _inside(f"restatement C {C} probs", p, ce["p"], bp))
        lse = (m + torch.log(s))[:, 0]
        term = torch.where(ce["mask"], lse - x[torch.arange(n), ce["y"]], torch.zeros(n))
        note("ce rows", _inside(f"restatement C {C} ce rows", term, ce["term"], ce["r"] + U * ce["term"].abs()))
        note("ce loss", _inside(f"restatement C {C} ce loss", (term.sum() / B).reshape(1), ce["loss"].reshape(1), ce["b_loss"].reshape(1)))
        one = torch.zeros(n, C)
        one[torch.arange(n), ce["y"]] = 1
        z = (x.double() - ce["m"][:, None]).abs()
        eP = ce["p"] * (ce["R"][:, None] + 3 * U * z + 4 * U + E_FAST) + TINY
        sc = f32(0.37) / B
        live = ce["mask"][:, None]
        d = (live.float() * f32(sc) * (p - one)).bfloat16()
        want = live.double() * sc * (ce["p"] - one.double())
        bnd = live.double() * (BF_ULP * want.abs() + 1.01 * sc * (eP + 2 * U * (ce["p"] - one.double()).abs()) + 3 * U * want.abs())
        note("ce gradient", _inside(f"restatement C {C} ce gradient", d, want, bnd))
        sm = f32(0.1)
        sjf = lse - x.sum(1) / C
        loss = ((1 - sm) * n * term.sum() + sm * cnt * sjf.sum()) / B
        note("ls loss", _inside(f"restatement C {C} ls loss", loss.reshape(1), ls_want.reshape(1), ls_b.reshape(1)))
        wn, wsm = live.double() * (1.0 - sm) * n, sm * cnt
        want = sc * (wn * (ce["p"] - one.double()) + wsm * (ce["p"] - 1.0 / C))
        bnd = BF_ULP * want.abs() + 1.01 * sc * (wn + wsm) * eP + 8 * U * sc * (wn * (ce["p"] - one.double()).abs() + wsm * (ce["p"] - 1.0 / C).abs() + wsm / C)
        d = (f32(sc) * (wn.float() * (p - one) + f32(wsm) * (p - f32(1.0 / C)))).bfloat16()
        note("ls gradient", _inside(f"restatement C {C} ls gradient", d, want, bnd))
    print("restatement, worst |err| / bound: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
