"""The argument rules of the C ABI are written once (dig_amd/csrc/abi_rules.h) and both builds call them.

1. Source pins: both builds include the one header of rules, and neither keeps a refusal of its own.
2. The rules a build gained when the two copies were merged, through the library, on both builds (`abi_dev`): the smallest arguments that
   reach the rule, every call describing memory that really is allocated, a pointer misaligned by stepping 2 or 4 bytes into a real buffer;
   every output is poisoned before the call and must come back untouched.  (Gained by the plain-C++ build unless noted: the bf16_shadow /
   tr_out alignment of the AdamW and EMA steps, the alignment rules of im2col / max-pool / the bf16 slab reduction / the attention block /
   the attention backward with the projection / the fused MLP, the GEMM forms that have no kernel, null entries of a transpose list,
   misaligned slabs of the grouped weight gradient.  Gained by both: BatchNorm with C <= 0.)
3. The magnitude rules (>= 2^32 offsets, LDS limits, B * max_len, the sequence attention backward's LDS bytes) through a stand-alone C++
   program (tests/abi_rules_main.cpp) that includes only the header, compiled with the address and undefined-behaviour sanitizers and run
   as a child process: nothing that large is ever described to a library.
"""
import ctypes
import glob
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
ARG, ALIGN, UNSUP = -1, -2, -4
POISON = 96.0                      # exact in bf16, fp32 and uint8
cf, cll = ctypes.c_float, ctypes.c_longlong
REFUSAL = re.compile(r"return\s+(\(int\))?DIG_ERR_(ARG|ALIGN|UNSUPPORTED)\b")
MARK = "unreachable: abi_rules.h"


# ------------------------------------------------------------------------------------------------ 1. source pins
def test_both_builds_include_the_one_header_of_rules():
    assert '#include "abi_rules.h"' in open(os.path.join(ROOT, "dig_amd", "csrc", "common.h")).read()
    assert '#include "../dig_amd/csrc/abi_rules.h"' in open(os.path.join(ROOT, "cpu_abi", "dig_cpu_common.h")).read()
    rules = open(os.path.join(ROOT, "dig_amd", "csrc", "abi_rules.h")).read()
    includes = re.findall(r"^#include\s+(\S+)", rules, re.M)
    assert includes == ["<cstddef>", "<cstdint>", '"../../include/dig_hip.h"'], includes
    assert "hip/hip_runtime" not in rules and "__global__" not in rules and "__device__" not in rules
    for helper in ("aligned16", "ranges_overlap"):                      # they live in the header of rules and nowhere else
        for other in ("dig_amd/csrc/common.h", "cpu_abi/dig_cpu_common.h"):
            assert not re.search(rf"bool {helper}\(", open(os.path.join(ROOT, other)).read()), (helper, other)
        assert re.search(rf"bool {helper}\(", rules), helper
    assert "abi_rules.h" in open(os.path.join(ROOT, "cpu_abi", "Makefile")).read()


def test_no_refusal_is_left_in_the_cpu_build():
    units = sorted(glob.glob(os.path.join(ROOT, "cpu_abi", "*.cpp")))
    assert len(units) >= 5
    left = [(os.path.basename(u), n + 1) for u in units for n, line in enumerate(open(u)) if REFUSAL.search(line)]
    assert not left, left
    assert sum(open(u).read().count("dig_rules::") for u in units) > 100


def test_every_refusal_left_in_the_hip_build_is_marked_unreachable():
    units = sorted(glob.glob(os.path.join(ROOT, "dig_amd", "csrc", "*.hip")))
    assert len(units) >= 20
    left = [(os.path.basename(u), n + 1) for u in units for n, line in enumerate(open(u)) if REFUSAL.search(line) and MARK not in line]
    assert not left, left
    assert sum(open(u).read().count("dig_rules::") for u in units) > 100


def test_the_shared_queries_are_defined_once():
    """The extern "C" definitions of the queries both builds answer alike are abi_queries.inc; no build defines one of them itself."""
    inc = open(os.path.join(ROOT, "dig_amd", "csrc", "abi_queries.inc")).read()
    names = re.findall(r'^extern "C" (?:int|long long) (dig_\w+)\(', inc, re.M)
    for q in ("dig_gemm_effective_splits", "dig_wgrad_group_effective_splits", "dig_layernorm_bwd_parts", "dig_layernorm_bwd_workspace_bytes",
              "dig_bn_fused_supported", "dig_attn_block_supported", "dig_mlp_chain_supported", "dig_mlp_chain_ln_parts",
              "dig_lexicon_search_workspace_bytes", "dig_ctc_lexicon_workspace_bytes", "dig_sumsq_workspace_bytes", "dig_mse_workspace_bytes",
              "dig_ce_rows_workspace_bytes", "dig_tcv_attn_bwd_workspace_bytes"):
        assert q in names, q
    units = glob.glob(os.path.join(ROOT, "dig_amd", "csrc", "*.hip")) + glob.glob(os.path.join(ROOT, "cpu_abi", "*.cpp"))
    for u in units:
        text = open(u).read()
        for q in names:
            assert not re.search(rf"^(?:extern \"C\" )?(?:int|long long) {q}\(", text, re.M), (os.path.basename(u), q)
    assert sum('#include "abi_queries.inc"' in open(u).read() or '#include "../dig_amd/csrc/abi_queries.inc"' in open(u).read() for u in units) == 2


# ------------------------------------------------------------------------------------------------ 2. gained rules, through the library
def _L():
    from dig_amd import _lib
    return _lib


def _buf(dev, n, dtype=F32):
    """n poisoned elements (64 more behind them, so that a pointer stepped a few bytes in still describes allocated memory)."""
    return torch.full((n + 64,), POISON, dtype=dtype, device=dev)


def _untouched(*bufs):
    return all(bool((b.float() == POISON).all()) for b in bufs)


def _off(t, nbytes):
    return ctypes.c_void_p(t.data_ptr() + nbytes)


def _refused(code, name, *args):
    L = _L()
    with pytest.raises(L.DigHipError) as e:
        L.call(name, *args)
    assert f"rc={code})" in str(e.value), (name, str(e.value))


@pytest.mark.parametrize("step_bytes", [2, 4])
def test_adamw_and_ema_refuse_a_misaligned_shadow(abi_dev, step_bytes):
    """bf16_shadow (and tr_out) are written with 8-byte stores: a shadow 2 or 4 bytes off is DIG_ERR_ALIGN on both builds (optim.hip)."""
    dev, L, P = abi_dev, _L(), _L().ptr
    n = 256
    p, g, m, v, sh = _buf(dev, n), _buf(dev, n), _buf(dev, n), _buf(dev, n), _buf(dev, n, BF)
    flags, tabs, s6 = torch.zeros(64, dtype=U8, device=dev), _buf(dev, 256), _buf(dev, 6)
    mats, tr_out = torch.zeros(64, dtype=U8, device=dev), _buf(dev, 64 * 64, BF)
    bad = _off(sh, step_bytes)
    head = (P(p), P(g), P(m), P(v), bad, cll(n))
    hyp = (cf(1e-3), cf(0.05), cf(1e-3), cf(0.0), cf(0.9), cf(0.999), cf(1e-8), 1, cf(1.0), None)
    _refused(ALIGN, "dig_adamw_step", *head, P(flags), *hyp, L.stream())
    _refused(ALIGN, "dig_adamw_step_tr", *head, P(flags), *hyp, P(mats), 1, 1, P(tr_out), L.stream())
    _refused(ALIGN, "dig_adamw_step_tr", P(p), P(g), P(m), P(v), P(sh), cll(n), P(flags), *hyp, P(mats), 1, 1, _off(tr_out, step_bytes), L.stream())
    _refused(ALIGN, "dig_adamw_step_dev", *head, P(flags), P(s6), cf(0.9), cf(0.999), cf(1e-8), cf(1.0), None, L.stream())
    _refused(ALIGN, "dig_adamw_step_groups", *head, P(flags), P(tabs), P(tabs), cf(0.9), cf(0.999), cf(1e-8), 1, cf(1.0), None, L.stream())
    n = 4
    _refused(ALIGN, "dig_ema_update", P(p), P(g), bad, cll(n), cf(0.99), L.stream())
    _refused(ALIGN, "dig_ema_update_dev", P(p), P(g), bad, cll(n), P(s6), L.stream())
    assert _untouched(p, g, m, v, sh, tr_out, s6, tabs)


def test_im2col_and_maxpool_refuse_misaligned_tensors(abi_dev):
    """16-byte loads and stores of the activations, 8-byte ones of the arg-max bytes (conv_patch.hip)."""
    dev, L, P = abi_dev, _L(), _L().ptr
    n_img, H, W, C = 1, 2, 2, 8
    x, col = _buf(dev, n_img * H * W * C, BF), _buf(dev, n_img * H * W * 9 * C, BF)
    y, idx = _buf(dev, n_img * C, BF), _buf(dev, n_img * C, U8)
    _refused(ALIGN, "dig_im2col3x3", _off(x, 2), P(col), n_img, H, W, C, 9 * C, L.stream())
    _refused(ALIGN, "dig_im2col3x3", P(x), _off(col, 4), n_img, H, W, C, 9 * C, L.stream())
    _refused(ALIGN, "dig_maxpool2x2_fwd", _off(x, 2), P(y), P(idx), n_img, H, W, C, L.stream())
    _refused(ALIGN, "dig_maxpool2x2_fwd", P(x), _off(y, 4), P(idx), n_img, H, W, C, L.stream())
    _refused(ALIGN, "dig_maxpool2x2_fwd", P(x), P(y), _off(idx, 4), n_img, H, W, C, L.stream())
    _refused(ALIGN, "dig_maxpool2x2_bwd", _off(y, 2), P(idx), P(x), n_img, H, W, C, L.stream())
    _refused(ALIGN, "dig_maxpool2x2_bwd", P(y), P(idx), _off(x, 4), n_img, H, W, C, L.stream())
    _refused(ALIGN, "dig_maxpool2x2_bwd", P(y), _off(idx, 4), P(x), n_img, H, W, C, L.stream())
    assert _untouched(x, col, y, idx)


def test_slab_reductions_refuse_misaligned_tensors(abi_dev):
    """dig_reduce_partials_bf16: 16-byte loads of the slabs, 8-byte stores of the bf16 sums; dig_reduce_partials_multi: each segment as
    dig_reduce_partials (gemm.hip)."""
    from dig_amd.ops import _ReduceSeg
    dev, L, P = abi_dev, _L(), _L().ptr
    part, out, outf = _buf(dev, 8), _buf(dev, 4, BF), _buf(dev, 8)
    _refused(ALIGN, "dig_reduce_partials_bf16", _off(part, 4), 1, cll(4), P(out), L.stream())
    _refused(ALIGN, "dig_reduce_partials_bf16", P(part), 1, cll(4), _off(out, 2), L.stream())
    _refused(ALIGN, "dig_reduce_partials_bf16", P(part), 1, cll(4), _off(out, 4), L.stream())
    segs = (_ReduceSeg * 2)(_ReduceSeg(part.data_ptr(), outf.data_ptr(), 4, 1, 0), _ReduceSeg(part.data_ptr() + 4, outf.data_ptr() + 16, 4, 1, 0))
    _refused(ALIGN, "dig_reduce_partials_multi", segs, 2, L.stream())       # refused as a whole: the first segment is not reduced either
    segs[1].partials, segs[1].n = part.data_ptr(), 6
    _refused(ARG, "dig_reduce_partials_multi", segs, 2, L.stream())
    assert _untouched(part, out, outf)


@pytest.mark.parametrize("C", [0, -8])
def test_batchnorm_refuses_a_width_that_is_not_positive(abi_dev, C):
    """C = 0 and C = -8 pass `C & 7`; both builds now refuse them with DIG_ERR_ARG before any launch (norm.hip)."""
    dev, L, P = abi_dev, _L(), _L().ptr
    rows = 2
    x, y, dy, dx = (_buf(dev, rows * 8, BF) for _ in range(4))
    sums, mean, rstd, gam, bet, ws, rm, rv, db, dg = (_buf(dev, 64) for _ in range(10))
    fwd = (P(x), P(sums), cf(rows), cf(1e-5), P(gam), P(bet), 1, P(y), P(mean), P(rstd))
    _refused(ARG, "dig_bn_fwd_apply", *fwd, rows, C, L.stream())
    _refused(ARG, "dig_bn_fwd_apply_running", *fwd, cf(0.1), P(rm), P(rv), rows, C, L.stream())
    bwd = (P(dy), P(x), P(mean), P(rstd), P(gam), P(bet), 1, P(sums))
    _refused(ARG, "dig_bn_bwd_stats", *bwd, P(ws), rows, C, L.stream())
    _refused(ARG, "dig_bn_bwd_stats_acc", *bwd, P(db), P(dg), P(ws), rows, C, L.stream())
    _refused(ARG, "dig_bn_bwd_apply", *bwd, cf(rows), P(dx), rows, C, L.stream())
    assert _untouched(x, y, dy, dx, sums, mean, rstd, gam, bet, ws, rm, rv, db, dg)


def test_gemm_refuses_the_forms_that_have_no_kernel(abi_dev):
    """dig_gemm_bf16: which (trans_a, trans_b, out_kind, tile) forms are instantiated is a rule of its own (gemm_form_ok); the column sums of
    the GELU backward exist for the 128x128 and 256x256 tiles only (gemm.hip)."""
    dev, L, P = abi_dev, _L(), _L().ptr
    I = J = 128
    R = 64
    A, B, C, Cf, res, cs = _buf(dev, I * R, BF), _buf(dev, J * R, BF), _buf(dev, I * J, BF), _buf(dev, I * J), _buf(dev, I * J, BF), _buf(dev, 2 * J)

    def gemm(ta, tb, kind, bk, out=C, act=0, resid=None, colsum=None):
        return ("dig_gemm_bf16", P(A), P(B), P(out), I, J, R, I if ta else R, J if not tb else R, J, ta, tb, kind, None, P(resid), J, None, 0, cf(1.0), 0,
                act, 1, 0, 0, bk, P(colsum), L.stream())
    _refused(UNSUP, *gemm(1, 0, 0, 0))
    _refused(UNSUP, *gemm(1, 0, 2, 64, out=Cf))
    _refused(UNSUP, *gemm(1, 1, 0, 32))
    _refused(UNSUP, *gemm(1, 1, 1, 0, out=Cf))
    _refused(UNSUP, *gemm(0, 0, 2, 64, out=Cf))           # split slabs of a forward layer: the wide tiles only
    _refused(UNSUP, *gemm(0, 1, 2, 32, out=Cf))
    _refused(UNSUP, *gemm(0, 1, 0, 264, act=2, resid=res, colsum=cs))
    _refused(UNSUP, *gemm(0, 1, 0, 212, act=2, resid=res, colsum=cs))
    assert _untouched(A, B, C, Cf, res, cs)


def test_fused_mlp_and_attention_block_refuse_misaligned_tensors(abi_dev):
    """Biases, side outputs and column-sum partials of the fused MLP, the activations of the one-launch attention block and of the attention
    backward with the projection are read and written 16 bytes at a time (mlp_chain.hip, attn_block.hip, attention.hip)."""
    dev, L, P = abi_dev, _L(), _L().ptr
    R, D, F = 2, 384, 128
    x, out, dx = _buf(dev, R * D, BF), _buf(dev, R * D, BF), _buf(dev, R * D, BF)
    w1, w2 = _buf(dev, F * D, BF), _buf(dev, D * F, BF)
    b1, b2, cs = _buf(dev, F), _buf(dev, D), _buf(dev, 4 * F)
    pre, act = _buf(dev, R * F, BF), _buf(dev, R * F, BF)
    _refused(ALIGN, "dig_mlp_chain_fwd", P(x), P(w1), _off(b1, 4), P(w2), P(b2), None, P(out), None, None, R, D, F, L.stream())
    _refused(ALIGN, "dig_mlp_chain_fwd", P(x), P(w1), P(b1), P(w2), P(b2), _off(x, 2), P(out), None, None, R, D, F, L.stream())
    _refused(ALIGN, "dig_mlp_chain_fwd", P(x), P(w1), P(b1), P(w2), P(b2), None, P(out), _off(pre, 2), P(act), R, D, F, L.stream())
    _refused(ALIGN, "dig_mlp_chain_bwd", P(x), P(w1), P(pre), P(w2), P(act), P(dx), _off(cs, 4), R, D, F, L.stream())
    n_img, E, heads = 1, 384, 6
    T = 256 * n_img
    ln1, xr, ctx, xmid, dy, dqkv = (_buf(dev, T * E, BF) for _ in range(6))
    qkv, lse = _buf(dev, T * 3 * E, BF), _buf(dev, n_img * heads * 256)
    wq, wp, qc, vc = _buf(dev, 3 * E * E, BF), _buf(dev, E * E, BF), _buf(dev, E), _buf(dev, E)
    blk = lambda a, b: ("dig_attn_block_fwd", a, P(xr), P(wq), None, P(wp), None, P(qkv), P(ctx), P(lse), b, n_img, heads, E, cf(0.125), L.stream())
    _refused(ALIGN, *blk(_off(ln1, 2), P(xmid)))
    _refused(ALIGN, *blk(P(ln1), _off(xmid, 4)))
    proj = lambda d, q, v: ("dig_attn_bwd_proj", P(qkv), P(ctx), d, P(wp), P(lse), P(dqkv), n_img, heads, E, cf(0.125), q, v, L.stream())
    _refused(ALIGN, *proj(_off(dy, 2), None, None))
    _refused(ARG, *proj(P(dy), P(qc), None))                # both column sums or none
    _refused(ARG, *proj(P(dy), None, P(vc)))
    assert _untouched(x, out, dx, w1, w2, b1, b2, cs, pre, act, ln1, xr, ctx, xmid, dy, dqkv, qkv, lse, wq, wp, qc, vc)


def test_table_entry_points_refuse_bad_entries(abi_dev):
    """A null matrix in a transpose list; misaligned slabs of the grouped weight gradient (mlp_chain.hip, wgrad.hip)."""
    from dig_amd.ops import _WgProb
    dev, L, P = abi_dev, _L(), _L().ptr
    a, b, ta, tb = (_buf(dev, 8 * 8, BF) for _ in range(4))
    srcs, dsts = (ctypes.c_void_p * 2)(a.data_ptr(), None), (ctypes.c_void_p * 2)(ta.data_ptr(), tb.data_ptr())
    _refused(ARG, "dig_transpose_bf16_multi", srcs, dsts, 2, 8, 8, L.stream())
    srcs[1], dsts[1] = b.data_ptr(), None
    _refused(ARG, "dig_transpose_bf16_multi", srcs, dsts, 2, 8, 8, L.stream())
    I, J, R = 128, 256, 64
    A, B, out, slabs = _buf(dev, R * I, BF), _buf(dev, R * J, BF), _buf(dev, I * J), _buf(dev, I * J)
    wmap = torch.zeros(8, dtype=torch.int32, device=dev)
    probs = (_WgProb * 1)(_WgProb(A.data_ptr(), B.data_ptr(), out.data_ptr(), I, J, J, I, J, 0))
    _refused(ALIGN, "dig_wgrad_group", probs, 1, None, 0, R, 1, P(wmap), 8, _off(slabs, 4), None, 1, 2, 1, L.stream())
    _refused(ALIGN, "dig_wgrad_group", None, 0, probs, 1, R, 1, None, 8, None, _off(slabs, 8), 1, 2, 1, L.stream())
    assert _untouched(a, b, ta, tb, A, B, out, slabs)


def test_the_loss_and_attention_backward_workspace_queries(abi_dev):
    """dig_mse_workspace_bytes, dig_ce_rows_workspace_bytes, dig_tcv_attn_bwd_workspace_bytes against the sizes include/dig_hip.h states in
    words: 257 floats; 1 + 3 n floats (one float at n = 0, nothing for n < 0); S Lq (2 d + heads) floats as a 64-bit product (nothing when an
    argument is not positive)."""
    q = _L().query
    assert q("dig_mse_workspace_bytes") == 257 * 4
    for n in (0, 1, 7, 4096, 2 ** 31 - 1):
        assert q("dig_ce_rows_workspace_bytes", n) == (1 + 3 * n) * 4, n
    assert q("dig_ce_rows_workspace_bytes", -1) == 0
    for S, Lq, heads, d in ((1, 1, 2, 128), (3, 5, 2, 128), (2, 25, 8, 512), (65535, 32, 8, 512), (2 ** 31 - 1, 32, 8, 512)):
        assert q("dig_tcv_attn_bwd_workspace_bytes", S, Lq, heads, d) == S * Lq * (2 * d + heads) * 4, (S, Lq, heads, d)
    assert 65535 * 32 * (2 * 512 + 8) * 4 > 2 ** 32 and 65535 * 32 * (2 * 512 + 8) > 2 ** 31         # neither the bytes nor the floats fit an int
    for bad in ((0, 5, 2, 128), (3, 0, 2, 128), (3, 5, 0, 128), (3, 5, 2, 0), (-1, 5, 2, 128), (3, 33, 2, 128), (3, 5, 8, 513), (3, 5, 129, 128)):
        assert q("dig_tcv_attn_bwd_workspace_bytes", *bad) == 0, bad


# ------------------------------------------------------------------------------------------------ 3. magnitude rules, stand-alone
def test_magnitude_rules_in_a_sanitized_stand_alone_program(tmp_path):
    """tests/abi_rules_main.cpp includes only abi_rules.h, passes dummy non-null pointers that are never dereferenced and asserts the code each
    magnitude rule returns just below, at and just above its limit and at INT_MAX arguments; built with the address and undefined-behaviour
    sanitizers (a signed overflow inside a rule's size arithmetic aborts the program) and run as a child process."""
    cxx = shutil.which("g++")
    assert cxx, "the stand-alone rule program needs g++"
    exe = str(tmp_path / "abi_rules_main")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            os.path.join(ROOT, "tests", "abi_rules_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    sys.stdout.write(run.stdout)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "abi_rules_main: all checks passed" in run.stdout
