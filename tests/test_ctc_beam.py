"""CTC prefix beam search (`--ctc_beam_width`, dig_ctc_beam_decode in csrc/ctc.hip and cpu_abi/dig_cpu_rec.cpp) against its specification
tests/ctc_beam_model.py: exact strings on samples that the specification itself selects, an exhaustive case against the CTC likelihood of every
labeling, agreement with the greedy rule on peaked frames, the host-side checks on both builds, the wiring through `CTCRecModelTrain.decode`
and `evaluate`, and the driver flag.  Operator tests run on both builds (`abi_dev`).

Which samples are asserted is decided by the specification alone.  A fixed-seed generator draws 2n candidates per case (frames as
tests/test_ctc.py draws them: 40 % blank, every odd frame repeats its predecessor half the time; logits = randn + `peak` at the frame's class
+ `bump` at one random class; pad columns NaN).  With e32 = the largest |logp32 - logp64| of the specification over the candidates and
G = 64 * max(e32, 2^-20 * max |logp64|), a candidate is kept when its smallest float64 selection gap is at least G: below that an fp32 search
may legitimately pick another prefix.  The first n kept candidates are the case; fewer than n kept fails on the CPU."""
import ctypes
import itertools
import math
import os
import types

import numpy as np
import pytest
import torch

import ctc_beam_model as BM
import ctc_model as S
import dig_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _draw(T, C, n, seed, peak, bump):
    """(x fp32 [n, T, ld] with NaN pad columns, frames [n, T])."""
    g = torch.Generator().manual_seed(seed)
    blank = C - 1
    frames = torch.randint(0, C, (n, T), generator=g)
    frames[torch.rand(frames.shape, generator=g) < 0.4] = blank
    k = T // 2
    frames[:, 1::2] = torch.where(torch.rand((n, k), generator=g) < 0.5, frames[:, 0:2 * k:2], frames[:, 1::2])      # runs
    v = torch.randn(n, T, C, generator=g)
    v.scatter_add_(2, frames.unsqueeze(-1), torch.full((n, T, 1), float(peak)))
    v.scatter_add_(2, torch.randint(0, C, (n, T, 1), generator=g), torch.full((n, T, 1), float(bump)))
    ld = 128 if C <= 128 else C
    x = torch.full((n, T, ld), float("nan"))
    x[:, :, :C] = v
    return x, frames


def _symbols(C):
    """(blank, eos, padding) of a case: the last class; a class that can occur in a prefix; any other int."""
    return (C - 1, C - 4, C - 3) if C >= 5 else (C - 1, 0, 7)


# (T, C, W, B, peak, bump).  peak 5 / bump 4 except at the grid edge, whose flatter frames make the search differ from the greedy collapse.
# Kept of drawn with these values: T32_W8 10 of 16, T32_W1 8 of 8, T64_W4 5 of 8 (a longer row meets more near-ties), C256_W32 4 of 4,
# grid_edge 126 of 130, never_full 6 of 6, T5 2 of 2, wiring 16 of 16
CASES = {
    "T32_W8": (32, 98, 8, 8, 5.0, 4.0),
    "T32_W1": (32, 98, 1, 4, 5.0, 4.0),
    "T64_W4": (64, 98, 4, 4, 5.0, 4.0),
    "C256_W32": (8, 256, 32, 2, 5.0, 4.0),
    "grid_edge": (12, 6, 4, 65, 2.5, 2.0),
    "never_full": (1, 3, 8, 3, 5.0, 4.0),
    "T5": (5, 4, 3, 1, 5.0, 4.0),
    "wiring": (32, 98, 4, 8, 5.0, 4.0),                                       # (the batch of the evaluate() test below)
}
_REF = {}


def _select(logp64, logp32, gap64, n):
    """The kept candidates' indices (the first n) and e32, from the specification's figures alone."""
    e32 = float((logp32 - logp64).abs().max())
    G = 64 * max(e32, 2.0 ** -20 * float(logp64.abs().max()))
    keep = torch.nonzero(gap64 >= G).reshape(-1)
    return keep, e32, G


def _reference(name):
    """Computed once per case and shared: x [B, T, ld], ids64, logp64, n64, e32 of the kept samples."""
    if name not in _REF:
        T, C, W, B, peak, bump = CASES[name]
        blank, eos, pad = _symbols(C)
        x, frames = _draw(T, C, 2 * B, seed=1000 * T + 10 * C + W, peak=peak, bump=bump)
        ids64, logp64, n64, kept64, gap64 = BM.beam_decode(x[:, :, :C], blank, eos, pad, W, np.float64)
        _, logp32, _, _, _ = BM.beam_decode(x[:, :, :C], blank, eos, pad, W, np.float32)
        keep, e32, G = _select(logp64, logp32, gap64, B)
        print(f"{name}: kept {len(keep)} of {2 * B} candidates, e32 {e32:.3e}, G {G:.3e}")
        assert len(keep) >= B, (name, len(keep), 2 * B, e32, G)
        keep = keep[:B]
        assert all(len(k) == T and all(len(f) <= W for f in k) for k in kept64)
        _REF[name] = dict(x=x[keep].contiguous(), frames=frames[keep], ids=ids64[keep], logp=logp64[keep], n=n64[keep], e32=e32)
    return _REF[name]


def _check_rows(ids, score, logp, n, want_ids, want_logp, want_n, e32, eos, pad):
    ids, score, logp, n = ids.cpu(), score.cpu(), logp.cpu().double(), n.cpu().long()
    assert torch.equal(n, want_n) and torch.equal(ids, want_ids), (ids, want_ids)
    err = (logp - want_logp).abs()
    bound = 4 * e32 + 2.0 ** -20 * want_logp.abs()
    print(f"logp err {float(err.max()):.3e} (e32 {e32:.3e}, |logp| max {float(want_logp.abs().max()):.2f})")
    assert (err <= bound).all(), (err, bound)
    want_s0 = torch.exp(logp)
    assert ((score[:, 0].double() - want_s0).abs() <= 1e-6 * want_s0).all()
    assert bool((score[:, 1:] == 1.0).all())
    for b in range(ids.shape[0]):                                            # cells past n: EOS, then PADDING
        k = int(n[b])
        assert int(ids[b, k]) == eos and bool((ids[b, k + 1:] == pad).all())


# ---------------------------------------------------------------------------------------------- 1. the operator against the specification
@pytest.mark.parametrize("name", [c for c in CASES if c != "wiring"])
def test_ctc_beam_decode_equals_the_specification(abi_dev, name):
    """Device figures (MI355X): DESIGN.md section 1, row N1 CTC head."""
    from dig_amd.ctc_recognizer import ctc_beam_decode
    T, C, W, B, _, _ = CASES[name]
    blank, eos, pad = _symbols(C)
    r = _reference(name)
    assert r["x"].shape[0] == B and bool(torch.isnan(r["x"][:, :, C:]).all())
    xd = r["x"].to(abi_dev)
    ids, score, logp, n = ctc_beam_decode(xd, C, blank, eos, pad, W)
    assert ids.dtype == torch.int64 and tuple(ids.shape) == (B, T + 1) and tuple(score.shape) == (B, T + 1) and tuple(logp.shape) == (B,)
    _check_rows(ids, score, logp, n, r["ids"], r["logp"], r["n"], r["e32"], eos, pad)
    again = ctc_beam_decode(xd, C, blank, eos, pad, W)                        # a second launch: equal bits
    for a, b_ in zip((ids, score, logp, n), again):
        assert torch.equal(a.cpu().view(torch.uint8), b_.cpu().view(torch.uint8))
    if name == "grid_edge":                                                   # the search is not the greedy collapse (the prototype: 22 of 32)
        greedy_ids, _, _ = S.greedy_decode(r["x"][:, :, :C], blank, eos, pad)
        differ = int((greedy_ids != r["ids"]).any(1).sum())
        print(f"{name}: the specification differs from the greedy collapse in {differ} of {B} samples")
        assert differ >= 1
    if name == "never_full":
        assert int(r["n"].max()) <= 1


def test_ctc_beam_decode_finds_the_most_likely_labeling(abi_dev):
    """T = 4, labels {0, 1}, blank 2, W = 32: the 31 labelings of length <= 4 all fit in the beam, so nothing is ever pruned and the result
    must be the arg-max of the float64 CTC likelihood (tests/ctc_model.py::ctc_nll) over all of them, with that likelihood as logp.  Samples
    are kept by the gap rule applied to the two best likelihoods (peak 2.5, bump 2.0)."""
    from dig_amd.ctc_recognizer import ctc_beam_decode
    T, C, W, n_keep, blank, eos, pad = 4, 3, 32, 8, 2, -1, 9
    labelings = [list(l) for k in range(T + 1) for l in itertools.product((0, 1), repeat=k)]
    assert len(labelings) == 31
    feasible = torch.tensor([len(l) + sum(l[i] == l[i - 1] for i in range(1, len(l))) <= T for l in labelings])
    target = torch.zeros((31, T), dtype=torch.int64)
    for i, l in enumerate(labelings):
        target[i, :len(l)] = torch.tensor(l, dtype=torch.int64)
    lens = torch.tensor([len(l) for l in labelings])
    x, _ = _draw(T, C, 2 * n_keep, seed=4343, peak=2.5, bump=2.0)
    ll = torch.stack([torch.where(feasible, -S.ctc_nll(x[b:b + 1, :, :C].double().expand(31, T, C), target, lens, blank),
                                  torch.full((31,), float("-inf"), dtype=torch.float64)) for b in range(x.shape[0])])
    top = ll.sort(dim=1, descending=True)
    ids64, logp64, n64, _, _ = BM.beam_decode(x[:, :, :C], blank, eos, pad, W, np.float64)
    _, logp32, _, _, _ = BM.beam_decode(x[:, :, :C], blank, eos, pad, W, np.float32)
    keep, e32, G = _select(logp64, logp32, top.values[:, 0] - top.values[:, 1], n_keep)
    assert len(keep) >= n_keep, (len(keep), e32, G)
    keep = keep[:n_keep]
    want_ids = torch.full((n_keep, T + 1), pad, dtype=torch.int64)
    want_n = torch.zeros(n_keep, dtype=torch.int64)
    for j, b in enumerate(keep.tolist()):
        l = labelings[int(top.indices[b, 0])]
        want_ids[j, :len(l)] = torch.tensor(l, dtype=torch.int64)
        want_ids[j, len(l)] = eos
        want_n[j] = len(l)
    want_logp = top.values[keep, 0]
    assert torch.equal(ids64[keep], want_ids) and float((logp64[keep] - want_logp).abs().max()) <= 1e-12      # the specification, on the CPU first
    ids, score, logp, n = ctc_beam_decode(x[keep].contiguous().to(abi_dev), C, blank, eos, pad, W)
    _check_rows(ids, score, logp, n, want_ids, want_logp, want_n, e32, eos, pad)


def test_ctc_beam_decode_agrees_with_greedy_on_peaked_frames(abi_dev, golden_dir):
    """The six hand-made rows of the fixture (runs, repeats, EOS inside, UNKNOWN, all blank, 32 distinct) as logits with a peak of 30 over unit
    noise: one alignment carries all the probability, so the search returns the greedy collapse, EOS removed the same way."""
    from dig_amd.ctc_recognizer import ctc_beam_decode, ctc_greedy_decode
    z = np.load(os.path.join(golden_dir, "ctc_tiny.npz"), allow_pickle=False)
    voc = [str(v) for v in z["voc"]]
    C, blank, eos, pad, W = len(voc) + 1, len(voc), voc.index("EOS"), voc.index("PADDING"), 8
    hand = torch.from_numpy(z["hand_frames"]).long()
    assert bool((hand == eos).any())                                           # the row with EOS inside is among them
    g = torch.Generator().manual_seed(30)
    x = torch.full((6, 32, 128), float("nan"))
    x[:, :, :C] = torch.randn(6, 32, C, generator=g).scatter_add_(2, hand.unsqueeze(-1), torch.full((6, 32, 1), 30.0))
    greedy_ids, _, greedy_n = S.greedy_decode(x[:, :, :C], blank, eos, pad)
    ids64, logp64, n64, _, _ = BM.beam_decode(x[:, :, :C], blank, eos, pad, W, np.float64)
    assert torch.equal(ids64, greedy_ids) and torch.equal(n64, greedy_n)       # the specification, on the CPU first
    ids, score, logp, n = ctc_beam_decode(x.to(abi_dev), C, blank, eos, pad, W)
    assert torch.equal(ids.cpu(), greedy_ids) and torch.equal(n.cpu().long(), greedy_n)
    assert torch.equal(ids, ctc_greedy_decode(x.to(abi_dev), C, blank, eos, pad)[0])


# ---------------------------------------------------------------------------------------------- 2. host-side validation (no GPU)
@pytest.mark.parametrize("build", ["hip", "cpu_abi"])
def test_ctc_beam_entry_point_validates_on_the_host(build):
    """Every error code of dig_ctc_beam_decode, before any launch, on both builds; a refused call writes nothing."""
    from cpu_abi_util import build as build_cpu
    from dig_amd import _lib as L
    lib = ctypes.CDLL(L.LIB_PATH if build == "hip" else build_cpu())
    f = lib.dig_ctc_beam_decode
    f.restype, f.argtypes = ctypes.c_int, L._prototypes()["dig_ctc_beam_decode"]
    ARG, UNS, OK = L.const("DIG_ERR_ARG"), L.const("DIG_ERR_UNSUPPORTED"), L.const("DIG_OK")
    poison = 0x5A
    bufs = {k: (ctypes.c_ubyte * 4096)(*([poison] * 4096)) for k in ("x", "ids", "score", "logp", "n")}
    p = {k: ctypes.cast(v, ctypes.c_void_p) for k, v in bufs.items()}

    def dec(**kw):
        a = dict(x=p["x"], ld=128, B=4, T=32, C=98, blank=97, eos=94, pad=95, W=8, ids=p["ids"], score=p["score"], logp=p["logp"], n=p["n"])
        a.update(kw)
        return f(a["x"], a["ld"], a["B"], a["T"], a["C"], a["blank"], a["eos"], a["pad"], a["W"], a["ids"], a["score"], a["logp"], a["n"], None)

    for k in ("x", "ids", "score", "logp", "n"):
        assert dec(**{k: None}) == ARG, k
    for kw in ({"B": -1}, {"T": 0}, {"T": -3}, {"C": 0}, {"C": -1}, {"ld": 97}, {"ld": 0}, {"blank": 98}, {"blank": -1}, {"W": 0}, {"W": -2}):
        assert dec(**kw) == ARG, kw
    for kw in ({"T": 65}, {"C": 257, "ld": 257}, {"C": 1, "blank": 0, "ld": 1}, {"W": 33}):
        assert dec(**kw) == UNS, kw
    assert dec(B=0) == OK and dec(B=0, T=64, C=256, ld=256, blank=255, W=32) == OK
    assert dec(B=0, eos=-1, pad=10 ** 6) == OK                                 # (eos and padding are any ints)
    assert all(all(v == poison for v in b) for b in bufs.values())


# ---------------------------------------------------------------------------------------------- 3. wiring: the model's decode and evaluate()
class _StubCTC:
    """What evaluate() and decode read of a CTC model, with fixed logits per batch and `decode` the real method."""
    is_ctc, beam_width = True, 0

    def __init__(self, logits, C, eos, pad, width):
        from dig_amd.ctc_recognizer import CTCRecModelTrain
        self.batches, self.i = logits, 0
        self.blank, self.eos, self.padding, self.ctc_beam_width, self.training = C - 1, eos, pad, width, True
        self.decode = types.MethodType(CTCRecModelTrain.decode, self)

    def eval(self):
        self.training = False
        return self

    def __call__(self, batch):
        out = self.batches[self.i].to(batch[0].device)
        self.i += 1
        return out, None, None, None


def test_ctc_beam_width_reaches_evaluate_and_decode(abi_dev):
    from dig_amd import recognizer
    from dig_amd.datasets import find_classes
    from dig_amd.ctc_recognizer import ctc_greedy_decode
    from dig_amd.engine_for_finetuning import evaluate
    T, C, W, B, _, _ = CASES["wiring"]
    r = _reference("wiring")
    voc = find_classes("ALLCASES_SYMBOLS")                                    # 94 characters, EOS, PADDING, UNKNOWN: nb_classes 97
    assert len(voc) + 1 == C
    blank, eos, pad = C - 1, voc.index("EOS"), voc.index("PADDING")
    assert (blank, eos, pad) == _symbols(C)
    x = r["x"][:, :, :C].contiguous()
    # targets: the specification's own rows for the even samples, a neighbour's for the odd ones
    target, lens = r["ids"].clone(), r["n"] + 1
    target[1::2], lens[1::2] = r["ids"][0::2], (r["n"] + 1)[0::2]
    split = ((0, 3), (3, B))
    batches = [(torch.zeros(hi - lo, 3, 32, 128), target[lo:hi], lens[lo:hi]) for lo, hi in split]
    loader = type("Loader", (list,), {})(batches)
    loader.dataset = types.SimpleNamespace(idx_to_class={i: c for i, c in enumerate(voc)})
    logits = [x[lo:hi] for lo, hi in split]
    args = types.SimpleNamespace(beam_width=0)
    beam = evaluate(loader, _StubCTC(logits, C, eos, pad, W), abi_dev, args)
    greedy = evaluate(loader, _StubCTC(logits, C, eos, pad, 0), abi_dev, args)
    want = sum(float(recognizer.accuracy(r["ids"][lo:hi].to(abi_dev), target[lo:hi].to(abi_dev), voc)) * (hi - lo) for lo, hi in split) / B
    assert 0.0 < want < 1.0 and beam["acc"] == want
    assert sorted(beam) == sorted(greedy) == ["acc", "loss", "recognition_fmeasure"]
    assert beam["loss"] == greedy["loss"] and math.isfinite(beam["loss"])
    # ---- decode: 0 is the greedy launch bit for bit; a model in training mode decodes greedily whatever its width
    xd = x.to(abi_dev)
    m = _StubCTC(logits, C, eos, pad, W)
    want_greedy = ctc_greedy_decode(xd, C, blank, eos, pad)
    for got in (m.decode(xd, beam_width=0), m.decode(xd)):
        assert len(got) == 3 and all(torch.equal(a.cpu().view(torch.uint8), b_.cpu().view(torch.uint8)) for a, b_ in zip(got, want_greedy))
    ids, score, n = m.eval().decode(xd)
    assert torch.equal(ids.cpu(), r["ids"]) and torch.equal(n.cpu().long(), r["n"]) and bool((score[:, 1:] == 1.0).all())
    ids1, _, _ = m.decode(xd, beam_width=1)
    assert tuple(ids1.shape) == (B, T + 1)


def test_ctc_model_takes_its_beam_width_from_the_arguments():
    from dig_amd.ctc_recognizer import CTCRecModelTrain
    ecfg = O.DiGConfig(**O.TINY)
    kw = dict(embed_dim=ecfg.embed_dim, depth=ecfg.depth, num_heads=ecfg.heads, nb_classes=97, max_len=25)
    assert CTCRecModelTrain(**kw).ctc_beam_width == 0 and CTCRecModelTrain(ctc_beam_width=32, **kw).ctc_beam_width == 32
    for bad in (-1, 33):
        with pytest.raises(ValueError, match="ctc_beam_width"):
            CTCRecModelTrain(ctc_beam_width=bad, **kw)
    args = dict(model="simmim_vit_tiny_patch4_32x128", nb_classes=97, max_len=25, drop=0.0, attn_drop_rate=0.0, drop_path=0.0)
    assert CTCRecModelTrain(types.SimpleNamespace(ctc_beam_width=4, **args)).ctc_beam_width == 4
    assert CTCRecModelTrain(types.SimpleNamespace(**args)).ctc_beam_width == 0
    with pytest.raises(ValueError, match="ctc_beam_width"):
        CTCRecModelTrain(types.SimpleNamespace(ctc_beam_width=40, **args))


# ---------------------------------------------------------------------------------------------- 4. the driver
from test_finetune_driver import COMMON, _driver  # noqa: E402

CTC = COMMON + " --decoder_type ctc"


def test_driver_ctc_beam_width_flag():
    drv = _driver()
    assert drv.get_args(CTC.split()).ctc_beam_width == 0 and drv.get_args(COMMON.split()).ctc_beam_width == 0
    args = drv.get_args((CTC + " --ctc_beam_width 4").split())
    assert args.ctc_beam_width == 4 and args.decoder_type == "ctc" and args.beam_width == 0
    assert drv.get_args((CTC + " --ctc_beam_width 32").split()).ctc_beam_width == 32
    with pytest.raises(SystemExit, match="--decoder_type ctc"):
        drv.get_args((COMMON + " --ctc_beam_width 4").split())
    with pytest.raises(SystemExit, match="--decoder_type ctc"):
        drv.get_args((COMMON + " --decoder_type attention --ctc_beam_width 4").split())
    for bad in ("33", "-1"):
        with pytest.raises(SystemExit, match="1..32"):
            drv.get_args((CTC + " --ctc_beam_width " + bad).split())
    with pytest.raises(SystemExit, match="decodes greedily.*--ctc_beam_width"):
        drv.get_args((CTC + " --beam_width 5").split())
    with pytest.raises(SystemExit, match="decodes greedily"):
        drv.get_args((CTC + " --beam_width 5 --ctc_beam_width 4").split())
    assert "--ctc_beam_width" in drv.__doc__


@pytest.mark.gpu
def test_ctc_driver_evaluates_with_the_beam(tmp_path):
    """One epoch of the synthetic CTC recipe, then --eval --resume with width 0 and width 4: the same four finite meters, an equal loss (it is
    taken on the frames' logits, whatever decodes them), and the line naming the beam decoder printed once, by the run that uses it."""
    import contextlib
    import io
    drv = _driver()
    out = str(tmp_path)
    with contextlib.redirect_stdout(io.StringIO()):
        drv.main(drv.get_args((CTC + " --epochs 1 --save_ckpt --output_dir " + out).split()))
    ck = os.path.join(out, "checkpoint-0.pth")
    assert os.path.exists(ck)
    got = {}
    for width in (0, 4):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            res = drv.main(drv.get_args((CTC + f" --epochs 1 --eval --resume {ck} --ctc_beam_width {width}").split()))
        got[width] = res["test_stats"]
        assert buf.getvalue().count("CTC prefix beam search") == (1 if width else 0)
        assert ("width 4" in buf.getvalue()) == bool(width)
    for width in (0, 4):
        assert set(got[width]) == {"loss", "acc", "recognition_fmeasure", "edit_distance"} and all(math.isfinite(v) for v in got[width].values())
    assert got[0]["loss"] == got[4]["loss"]


# ---------------------------------------------------------------------------------------------- 5. the build
def test_ctc_beam_kernel_uses_no_scratch():
    from dig_amd import build
    build.build(verbose=False)
    rows = [r for r in build.kernel_resources() if r["name"].startswith("ctc_beam_kernel")]
    assert len(rows) == 1 and rows[0]["scratch"] == 0 and rows[0]["hot"], rows
