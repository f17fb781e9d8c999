"""The scratch the op wrappers hand to the C ABI: one pool (dig_amd/scratch.py), every size from the library's own query.

1. Sizes and exact fit.  Each wrapper with scratch runs twice on the same inputs while scratch.get is wrapped: once through the pool as the
   product uses it, once with every floor ignored and a buffer of EXACTLY the requested elements, poison behind it (NaN; 0x7F bytes behind
   the zeroed areas of the loss reductions) and NaN in it (zero in the zeroed areas).  Both runs must ask for (tag, the owning query's
   floats) -- splits * I * J for slabs --, give the same bits, and leave the poison alone; a zeroed area's ticket word is zero again after
   two launches on one buffer.  Shapes: the smallest at which the partial-sum layouts differ -- rows 1, 63, 64, 65 and 16385 (past the
   1024 parts of the LayerNorm backward, and two 16384-row steps of the column sums' 512-block grid), C 8, 512 and 520 (one and two
   512-column blocks), 1 and 7 rows of logits, one and 256 workgroups of the MSE; the patch-embedding gradient (a weight-gradient GEMM,
   then the masked column sums in the layout dig_colsum has) at 64, 128 and 16640 tokens: one, two and 130 row blocks.
2. The pool: one buffer per (tag, stream) that only grows, tags never share storage, GradReduceBatch's pending slabs survive a wgrad.
3. The CPU test backend swaps nothing in ops and leaves no CPU tensor behind; the five old caches and their accessors are gone.
"""
import math

import pytest
import torch

BF, F32 = torch.bfloat16, torch.float32
GUARD = 64
ZEROED = ("mse", "ce")
ROWS = (1, 63, 64, 65, 16385)


def _mods():
    from dig_amd import _lib, ops, scratch
    return _lib, ops, scratch


def _rn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _q(name, *args):
    """The owning query's answer in floats, asked of the library directly (no memo)."""
    nbytes = _mods()[0].query(name, *args)
    assert nbytes > 0 and nbytes % 4 == 0, (name, args, nbytes)
    return nbytes // 4


# ------------------------------------------------------------------------------------------------ the wrappers: (outputs, expected requests)
def _colsum(dev, rows, C):
    _, ops, _ = _mods()
    x, out = _rn(1, rows, C).bfloat16().to(dev), torch.ones(C, device=dev)
    ops.colsum(x, out)
    return [out], [("partials", _q("dig_colsum_workspace_bytes", rows, C))]


def _layernorm_bwd(dev, rows, D=64):
    _, ops, _ = _mods()
    x, dy, dres = (_rn(s, rows, D).bfloat16().to(dev) for s in (2, 3, 4))
    g, b = (1 + 0.2 * _rn(5, D)).to(dev), (0.1 * _rn(6, D)).to(dev)
    _, mean, rstd = ops.layernorm_fwd(x, g, b, 1e-6)
    dg, db, dc = torch.zeros(D, device=dev), torch.ones(D, device=dev), torch.zeros(D, device=dev)
    dx = ops.layernorm_bwd(dy, x, g, b, mean, rstd, dres, dg, db, dres_colsum=dc)
    return [dx, dg, db, dc], [("partials", _q("dig_layernorm_bwd_workspace_bytes", rows, D))]


def _patch_embed_bwd(dev, n_img, gh, gw, D=64):
    _, ops, _ = _mods()
    n_tok = n_img * gh * gw
    img, dy = _rn(7, n_img, 3, 4 * gh, 4 * gw).to(dev), _rn(8, n_tok, D).bfloat16().to(dev)
    m8 = (_rn(9, n_img, gh * gw) > 0).to(torch.uint8).to(dev)
    dW, dbias, dmt = torch.zeros(D, 48, device=dev), torch.zeros(D, device=dev), torch.zeros(D, device=dev)
    ops.patch_embed_bwd_mfma(dy, img, m8, dW, dbias, dmt, D, gh, gw)
    sp = ops.wgrad_splits(n_tok, 1)[0]
    return [dW, dbias, dmt], [("slabs", sp * D * 48), ("partials", 2 * _q("dig_colsum_workspace_bytes", n_tok, D))]


def _batchnorm(dev, rows, C):
    _, ops, _ = _mods()
    x, dy = (2 * _rn(10, rows, C) + 0.5).bfloat16().to(dev), _rn(11, rows, C).bfloat16().to(dev)
    gamma, beta = (1 + 0.2 * _rn(12, C)).to(dev), (0.1 * _rn(13, C)).to(dev)
    mean, rstd = x.float().mean(0), torch.ones(C, device=dev)
    sums, s2 = torch.empty(2, C, device=dev), torch.empty(2, C, device=dev)
    db, dg = torch.full((C,), 0.5, device=dev), torch.full((C,), -0.25, device=dev)
    ops.bn_stats(x, sums)
    ops.bn_bwd_stats(dy, x, mean, rstd, gamma, beta, True, s2, db, dg)
    return [sums, s2, db, dg], [("partials", _q("dig_bn_stats_workspace_bytes", rows, C))] * 2


def _mse(dev, M, C, ld, ldd):
    _, ops, _ = _mods()
    pred, tgt = _rn(14, M, ld).to(dev), _rn(15, M, C).to(dev)
    out = []
    for _ in range(2):                                    # two launches on one buffer: the second finds the ticket word the first left
        loss, dpred = torch.zeros(1, device=dev), torch.empty(M, ldd, device=dev, dtype=BF)
        ops.mse_fwd_bwd(pred, ld, tgt, M, C, 0.7, loss, dpred, ldd)
        out += [loss, dpred]
    assert torch.equal(out[0], out[2]) and torch.equal(out[1], out[3])
    return out, [("mse", _q("dig_mse_workspace_bytes"))] * 2


def _ce_rows(dev, n, m=16):
    _, ops, _ = _mods()
    out = []
    for _ in range(2):
        logits, out3 = (3 * _rn(16, n, m)).to(dev), torch.zeros(3, device=dev)
        ops.ce_rows(logits, 2, 0.25, out3)
        out += [logits, out3]
    assert torch.equal(out[0], out[2]) and torch.equal(out[1], out[3])
    return out, [("ce", _q("dig_ce_rows_workspace_bytes", n))] * 2


def _tcv_attn_bwd(dev, S=3, Lq=5, N=32, H=2, d=128):
    _, ops, _ = _mods()
    R = S * Lq
    film, u, dc = _rn(17, R, 2 * d).bfloat16().to(dev), (_rn(18, R, H * d) * (1.5 / math.sqrt(2 * d))).bfloat16().to(dev), _rn(19, R, H * d).bfloat16().to(dev)
    vk, mem = _rn(20, S * N, d).bfloat16().to(dev), _rn(21, S * N, d).bfloat16().to(dev)
    lg, lb = (1 + 0.1 * _rn(22, d)).to(dev), (0.05 * _rn(23, d)).to(dev)
    c, lse = ops.tcv_attn_fwd(film, u, vk, mem, lg, lb, S, Lq, N, H)
    dlg, dlb = torch.ones(d, device=dev), torch.full((d,), -2.0, device=dev)
    du, dfilm, dvk, dmem = ops.tcv_attn_bwd(film, u, vk, mem, lg, lb, c, lse, dc, dlg, dlb, S, Lq, N, H)
    return [du, dfilm, dvk, dmem, dlg, dlb], [("slabs", _q("dig_tcv_attn_bwd_workspace_bytes", S, Lq, H, d))]


def _sgemm(dev, I=8, J=8, R=256):
    _, ops, _ = _mods()
    A, B, C = _rn(24, I, R).to(dev), _rn(25, J, R).to(dev), torch.empty(I, J, device=dev)
    ops.sgemm(A, B, C, I, J, R, False, 0.5)
    return [C], [("slabs", (R // 128) * I * J)]


def _wgrad(dev, I=128, J=128, rows=1024):
    _, ops, _ = _mods()
    dy, x, dw = _rn(26, rows, I).bfloat16().to(dev), _rn(27, rows, J).bfloat16().to(dev), torch.ones(I, J, device=dev)
    ops.wgrad(dy, x, dw, I, J, rows)
    sp = ops.wgrad_splits(rows, 1)[0]
    assert sp == 2
    return [dw], [("slabs", sp * I * J)]


def _split_gemm(dev, I=64, J=128, R=2048):
    _, ops, _ = _mods()
    x, w = _rn(28, I, R).bfloat16().to(dev), (_rn(29, J, R) / 32).bfloat16().to(dev)
    sp = ops.narrow_splits(I, J, R)
    assert sp == 4
    return [ops._split_gemm_bf16(x, w, I, J, R, False, 212, sp, None)], [("slabs", sp * I * J)]


CASES = ([("colsum", _colsum, (r, C)) for r in ROWS for C in (8, 512, 520)] + [("layernorm_bwd", _layernorm_bwd, (r,)) for r in ROWS] +
         [("patch_embed_bwd_mfma", _patch_embed_bwd, a) for a in ((1, 8, 8), (2, 8, 8), (65, 8, 32))] +
         [("batchnorm", _batchnorm, (r, 8)) for r in ROWS] + [("batchnorm", _batchnorm, (65, 520))] +
         [("mse_fwd_bwd", _mse, (1, 1, 1, 8)), ("mse_fwd_bwd", _mse, (300, 48, 48, 56)), ("mse_fwd_bwd", _mse, (2000, 48, 48, 48))] +
         [("ce_rows", _ce_rows, (1,)), ("ce_rows", _ce_rows, (7,))] + [("tcv_attn_bwd", _tcv_attn_bwd, ()), ("sgemm", _sgemm, ()),
                                                                         ("wgrad", _wgrad, ()), ("split_gemm_bf16", _split_gemm, ())])


class _ExactFit:
    """scratch.get's stand-in: a buffer of exactly `numel` elements with GUARD poisoned ones behind it, kept per (tag, numel) so that a second
    launch finds what the first one left."""

    def __init__(self):
        self.bufs, self.asked = {}, []

    def __call__(self, tag, dev, numel, dtype=F32, *, zero=False, floor=0):
        assert dtype == F32 and zero == (tag in ZEROED)
        self.asked.append((tag, numel))
        if (tag, numel) not in self.bufs:
            full = torch.full((numel + GUARD,), math.nan, device=dev)
            if zero:
                full.view(torch.uint8).fill_(0x7F)
                full[:numel] = 0
            self.bufs[tag, numel] = full
        return self.bufs[tag, numel][:numel]

    def check(self):
        for (tag, numel), full in self.bufs.items():
            guard = full[numel:]
            assert bool((guard.view(torch.uint8) == 0x7F).all()) if tag in ZEROED else bool(guard.isnan().all()), (tag, numel)
            if tag in ZEROED:
                assert float(full[0]) == 0.0, (tag, "ticket word")


@pytest.mark.parametrize("name,fn,args", CASES, ids=[f"{n}-{'x'.join(map(str, a))}" for n, _, a in CASES])
def test_every_wrapper_asks_for_its_query_and_fits_it_exactly(abi_dev, monkeypatch, name, fn, args):
    _, _, scratch = _mods()
    real, asked = scratch.get, []

    def recording(tag, dev, numel, *a, **kw):
        asked.append((tag, numel))
        return real(tag, dev, numel, *a, **kw)
    monkeypatch.setattr(scratch, "get", recording)
    out_pool, want = fn(abi_dev, *args)
    assert asked == want, (asked, want)
    exact = _ExactFit()
    monkeypatch.setattr(scratch, "get", exact)
    out_exact, _ = fn(abi_dev, *args)
    assert exact.asked == want, (exact.asked, want)
    for a, b in zip(out_pool, out_exact):
        assert bool(a.float().isfinite().all()) and torch.equal(a, b), name
    exact.check()


# ------------------------------------------------------------------------------------------------ 2. the pool
@pytest.fixture
def pool():
    """dig_amd.scratch with this module's tags (test_*) forgotten again afterwards."""
    scratch = _mods()[2]
    yield scratch
    for key in [k for k in scratch._pool if k[0].startswith("test_")]:
        del scratch._pool[key]


def test_one_buffer_per_tag_that_only_grows(abi_dev, pool):
    a = pool.get("test_a", abi_dev, 10)
    assert a.numel() == 10 and a.dtype == F32 and a.device.type == abi_dev.type
    assert pool.get("test_a", abi_dev, 10) is a and pool.get("test_a", abi_dev, 3) is a
    b = pool.get("test_a", abi_dev, 11, floor=4)
    assert b is not a and b.numel() == 11 and pool.get("test_a", abi_dev, 10) is b
    f = pool.get("test_f", abi_dev, 3, floor=16)
    assert f.numel() == 16 and pool.get("test_f", abi_dev, 16, floor=16) is f
    z = pool.get("test_z", abi_dev, 5, zero=True, floor=8)
    assert z.numel() == 8 and not bool(z.any())
    spans = sorted((t.data_ptr(), t.data_ptr() + 4 * t.numel()) for t in (b, f, z))
    assert all(spans[k][1] <= spans[k + 1][0] for k in range(2)), spans              # two tags never share storage
    h = pool.get("test_h", abi_dev, 6, torch.int32)
    assert h.dtype == torch.int32


@pytest.mark.gpu
def test_two_streams_get_two_buffers(pool):
    dev = torch.device("cuda:0")
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    with torch.cuda.stream(s1):
        a = pool.get("test_s", dev, 8)
    with torch.cuda.stream(s2):
        b = pool.get("test_s", dev, 8)
    with torch.cuda.stream(s1):
        assert pool.get("test_s", dev, 8) is a
    assert a.data_ptr() != b.data_ptr()


def test_pending_batch_slabs_survive_a_wgrad(abi_dev):
    """GradReduceBatch's slabs wait in their own tag until flush(): a plain wgrad on the same stream in between (the "slabs" tag) must not
    touch them.  The flushed gradient has the bits of the unbatched one."""
    _, ops, _ = _mods()
    I = J = 128
    rows = 1024
    dy, x = _rn(30, rows, I).bfloat16().to(abi_dev), _rn(31, rows, J).bfloat16().to(abi_dev)
    dy2, x2 = _rn(32, rows, I).bfloat16().to(abi_dev), _rn(33, rows, J).bfloat16().to(abi_dev)
    want, want2 = torch.ones(I, J, device=abi_dev), torch.zeros(I, J, device=abi_dev)
    ops.wgrad(dy, x, want, I, J, rows)
    ops.wgrad(dy2, x2, want2, I, J, rows)
    assert ops.BATCH_SLABS
    batch, got, got2 = ops.GradReduceBatch(), torch.ones(I, J, device=abi_dev), torch.zeros(I, J, device=abi_dev)
    batch.wgrad(dy, x, got)
    assert len(batch.slabs) == 1
    ops.wgrad(dy2, x2, got2, I, J, rows)
    batch.flush()
    assert torch.equal(got, want) and torch.equal(got2, want2) and not torch.equal(want, want2)


def test_the_grouped_weight_gradient_sets_alternate_and_never_alias(abi_dev):
    _, ops, scratch = _mods()
    for key in [k for k in scratch._pool if k[0].startswith("wgrad_group") and k[1] == abi_dev]:
        del scratch._pool[key]                                     # (earlier tests of this process may have grown them past the floor)
    grp = ops.WgradGroup(abi_dev)
    a, b, c = grp.next_slabs(1024), grp.next_slabs(1024), grp.next_slabs(1024)
    assert c is a and a is not b and a.numel() == b.numel() == ops.GROUP_FLOOR == (1 << 26) // 4
    assert not (a.data_ptr() < b.data_ptr() + 4 * b.numel() and b.data_ptr() < a.data_ptr() + 4 * a.numel())
    assert ops.GradReduceBatch.SLAB_FLOATS == 1 << 25 and (ops.SLAB_FLOOR, ops.PARTIAL_FLOOR, ops.LOSS_FLOOR) == (1 << 22, 1 << 20, 4096)


# ------------------------------------------------------------------------------------------------ 3. the CPU backend, the old names
def test_the_cpu_backend_leaves_no_cpu_tensor_in_the_pool():
    from cpu_abi_util import cpu_abi_backend
    _lib, ops, scratch = _mods()
    stream, stream_key = _lib.stream, _lib.stream_key
    with cpu_abi_backend() as dev:
        assert _lib.stream is not stream and _lib.stream_key is not stream_key
        ops.colsum(torch.ones(3, 8, dtype=BF), torch.zeros(8))
        assert any(t.device.type == "cpu" for t in scratch._pool.values())
    assert _lib.stream is stream and _lib.stream_key is stream_key
    assert not any(t.device.type == "cpu" for t in scratch._pool.values()) and not any(k[1] == dev for k in scratch._pool)


def test_ops_keeps_none_of_the_five_caches():
    _, ops, _ = _mods()
    for name in ("_batch_workspace", "_loss_workspace", "_stream_id", "_ws", "_ws2", "_ws3", "_loss_ws", "_wg_slabs"):
        assert not hasattr(ops, name), name
    # (the two names that earlier revisions of cpu_abi_util save and restore stay readable, and are neither a cache nor a function)
    assert getattr(ops, "_workspace", None) is None and getattr(ops, "_workspace2", None) is None
    assert not hasattr(ops.WgradGroup, "_slabs")
    src = open(ops.__file__).read()
    for call in ("_workspace(", "_workspace2(", "_batch_workspace(", "_loss_workspace(", "_stream_id(", "dev.type"):
        assert call not in src, call


def test_the_pool_serves_a_cpu_device_with_nothing_swapped():
    """stream_key gives a device without streams the key 0 itself: the host code above the ABI reaches its scratch on torch.device("cpu")
    whether or not a test backend swapped stream_key."""
    _lib, _, scratch = _mods()
    dev = torch.device("cpu")
    assert _lib.stream_key(dev) == 0
    try:
        a = scratch.get("test_cpu", dev, 4)
        assert a.device.type == "cpu" and scratch.get("test_cpu", dev, 4) is a
    finally:
        scratch._pool.pop(("test_cpu", dev, 0), None)
