"""CTC forced alignment (`--ctc_align_out`, dig_ctc_align in csrc/ctc.hip and cpu_abi/dig_cpu_rec.cpp) against its specification
tests/ctc_align_model.py: the device's path is valid, optimal to the specification's fp32 error and equal to the specification's wherever
the specification's own gap to the second-best path allows an fp32 run no other choice; its figures are those of its own path; the edge
cases of the rule; an exhaustive case over all frame strings; agreement with the greedy decode; the host-side checks on both builds; the
wiring through `CTCRecModelTrain.align`, `evaluate` and the driver.  Operator tests run on both builds (`abi_dev`).

Frames are drawn by `_draw` of tests/test_ctc_beam.py (peak 5 / bump 4; 2.5 / 2 for the small grid).  The labels of sample b cycle through
four forms: the frames' collapse, one substitution, one deletion, one insertion (positions and classes from a fixed-seed generator), so that
most alignments are not the frame-wise arg-max.  With e32 = max |s32 - s64| of the specification over the samples of a call and
G = 64 * max(e32, 2^-20 * max |s64|), a sample whose `second_best_gap` is at least G must come back with the specification's path.  Every
sample of every case has such a gap (asserted on the CPU, from the specification alone)."""
import ctypes
import itertools
import json
import os

import numpy as np
import pytest
import torch

import ctc_align_model as AM
from test_ctc_beam import _draw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON_I, POISON_F = -77, 12345.0


# ---------------------------------------------------------------------------------------------- the call, on poisoned outputs
def _align(dev, x, C, target, lens, blank, len_offset, frames=True):
    """dig_ctc_align through the library on outputs filled with a poison: (start, end, char_logp, path_logp, frame_label) on the host."""
    from dig_amd import _lib as L
    B, T, ld = x.shape
    ldt = target.shape[1]
    xd, tg, ln = x.to(dev).contiguous(), target.to(dev).contiguous(), lens.to(dev).contiguous()
    start = torch.full((B, ldt), POISON_I, dtype=torch.int32, device=dev)
    end = torch.full((B, ldt), POISON_I, dtype=torch.int32, device=dev)
    clp = torch.full((B, ldt), POISON_F, dtype=torch.float32, device=dev)
    plp = torch.full((B,), POISON_F, dtype=torch.float32, device=dev)
    fl = torch.full((B, T), POISON_I, dtype=torch.int32, device=dev) if frames else None
    L.call("dig_ctc_align", L.ptr(xd), ld, L.ptr(tg), ldt, L.ptr(ln), len_offset, B, T, C, blank, L.ptr(start), L.ptr(end), L.ptr(clp), L.ptr(plp),
           L.ptr(fl), L.stream())
    return start.cpu(), end.cpu(), clp.cpu(), plp.cpu(), (fl.cpu() if frames else None)


def _rows(labelings, ldt, fill=-1):
    target = torch.full((len(labelings), ldt), fill, dtype=torch.int64)
    for i, l in enumerate(labelings):
        assert len(l) <= ldt
        target[i, :len(l)] = torch.tensor(l, dtype=torch.int64)
    return target, torch.tensor([len(l) for l in labelings], dtype=torch.int64)


def _tables(x, C):
    """The specification's two tables of a call: log_softmax in float64 and in float32, [B, T, C] numpy."""
    v = x[:, :, :C]
    return torch.log_softmax(v.double(), -1).numpy(), torch.log_softmax(v.float(), -1).numpy()


def _bound(e32, value):
    return 4 * e32 + 2.0 ** -20 * abs(float(value))


# ---------------------------------------------------------------------------------------------- the cases
# (T, C, B, ldt, peak, bump): the recipe shape; the longest row with the widest target; more than one wave of samples on the small flat grid;
# every class count; two frames; one frame (labels of length 0 and 1 align, length 2 has no alignment)
CASES = {
    "T32_C98": (32, 98, 8, 33, 5.0, 4.0),
    "T64_ldt63": (64, 98, 4, 63, 5.0, 4.0),
    "small_grid": (12, 6, 65, 13, 2.5, 2.0),
    "C256": (8, 256, 2, 9, 5.0, 4.0),
    "T2": (2, 4, 8, 3, 5.0, 4.0),
    "T1": (1, 3, 6, 2, 5.0, 4.0),
}
SEEDS = {"T1": 7114}                                                          # (a draw whose fourth frame is no blank: the insertion gives two labels)
_REF = {}


def _collapse(row, blank):
    return [c for j, c in enumerate(row) if c != blank and not (j > 0 and row[j - 1] == c)]


def _forms(frames, C, seed):
    """The labels of sample b: form b % 4 of the collapse of its frames."""
    blank, rng, out = C - 1, np.random.RandomState(seed), []
    for b, row in enumerate(frames.tolist()):
        l, form = _collapse(row, blank), b % 4
        if form == 1 and l:                                                  # one substitution, by another class that is not the blank
            p = rng.randint(len(l))
            l[p] = (l[p] + 1 + rng.randint(C - 2)) % (C - 1)
        elif form == 2 and l:                                                # one deletion
            del l[rng.randint(len(l))]
        elif form == 3:                                                      # one insertion
            l.insert(rng.randint(len(l) + 1), int(rng.randint(C - 1)))
        out.append(l)
    return out


def _specify(x, C, labelings, blank):
    """Per sample the specification's figures: s64, states64, s32, gap; then e32 and G of the call."""
    lp64, lp32 = _tables(x, C)
    T = x.shape[1]
    rows = []
    for b, l in enumerate(labelings):
        if not AM.feasible(l, blank, T, C):
            rows.append(None)
            continue
        s64, st64 = AM.viterbi(lp64[b], l, blank)
        s32, _ = AM.viterbi(lp32[b], l, blank)
        rows.append(dict(s64=float(s64), states=st64.tolist(), s32=float(s32), gap=AM.second_best_gap(lp64[b], l, blank)))
    fin = [r for r in rows if r is not None]
    e32 = max(abs(r["s32"] - r["s64"]) for r in fin)
    G = 64 * max(e32, 2.0 ** -20 * max(abs(r["s64"]) for r in fin))
    return lp64, rows, e32, G


def _reference(name):
    if name not in _REF:
        T, C, B, ldt, peak, bump = CASES[name]
        x, frames = _draw(T, C, B, seed=SEEDS.get(name, 7100 + 100 * T + C), peak=peak, bump=bump)
        labelings = _forms(frames, C, seed=T + C)
        lp64, rows, e32, G = _specify(x, C, labelings, C - 1)
        fin = [r for r in rows if r is not None]
        kept = sum(r["gap"] >= G for r in fin)
        print(f"{name}: {len(fin)} of {B} samples align, {kept} kept, smallest gap {min(r['gap'] for r in fin):.3e}, e32 {e32:.3e}, G {G:.3e}")
        assert kept == len(fin), (name, kept, len(fin), sorted(r["gap"] for r in fin)[:3], G)
        _REF[name] = dict(x=x, labelings=labelings, lp64=lp64, rows=rows, e32=e32, G=G)
    return _REF[name]


def _check_sample(b, l, blank, lp64, spec, e32, G, start, end, clp, plp, fl, ldt):
    """Everything the rule says of one aligned sample, from the device's own path."""
    n, T = len(l), lp64.shape[0]
    states = AM.states_of_frame_labels(fl[b].tolist())
    assert AM.validity(states, l), (b, states, l)
    want_start, want_end, want_clp = AM.spans(lp64, l, blank, states)
    assert start[b, :n].tolist() == want_start and end[b, :n].tolist() == want_end, (b, start[b], end[b], states)
    assert all(e > s_ >= 0 for s_, e in zip(want_start, want_end))
    assert bool((start[b, n:] == -1).all()) and bool((end[b, n:] == -1).all()) and bool((clp[b, n:] == 0).all())
    own = float(AM.path_score(lp64, l, blank, states))
    assert own >= spec["s64"] - _bound(e32, spec["s64"]), (b, own, spec["s64"])
    assert abs(float(plp[b]) - own) <= _bound(e32, own), (b, float(plp[b]), own)
    for k in range(n):
        assert abs(float(clp[b, k]) - float(want_clp[k])) <= _bound(e32, want_clp[k]), (b, k, float(clp[b, k]), want_clp[k])
    blanks = sum(float(lp64[t, blank]) for t in range(T) if not states[t] & 1)
    total = float(clp[b, :n].double().sum()) + blanks
    assert abs(float(plp[b]) - total) <= _bound(e32, total), (b, float(plp[b]), total)
    if spec["gap"] >= G:
        assert states == spec["states"], (b, states, spec["states"])
    return abs(float(plp[b]) - own)


def _check_no_alignment(b, start, end, clp, plp, fl):
    assert float(plp[b]) == float("-inf") and bool((start[b] == -1).all()) and bool((end[b] == -1).all()) and bool((clp[b] == 0).all())
    assert fl is None or bool((fl[b] == -2).all())


# ---------------------------------------------------------------------------------------------- 1. the operator against the specification
@pytest.mark.parametrize("name", list(CASES))
def test_ctc_align_against_the_specification(abi_dev, name):
    """Device figures (MI355X): DESIGN.md section 1, row N1 CTC head."""
    from dig_amd.ctc_recognizer import ctc_align
    T, C, B, ldt, _, _ = CASES[name]
    blank = C - 1
    r = _reference(name)
    x, labelings = r["x"], r["labelings"]
    assert bool(torch.isnan(x[:, :, C:]).all()) and (x.shape[2] > C or C == 256)
    target, n = _rows(labelings, ldt)
    got = _align(abi_dev, x, C, target, n + 1, blank, 1)
    start, end, clp, plp, fl = got
    aligned, worst = 0, 0.0
    for b, l in enumerate(labelings):
        if r["rows"][b] is None:
            _check_no_alignment(b, start, end, clp, plp, fl)
        else:
            worst = max(worst, _check_sample(b, l, blank, r["lp64"][b], r["rows"][b], r["e32"], r["G"], start, end, clp, plp, fl, ldt))
            aligned += 1
    print(f"{name}: {aligned} aligned samples, path_logp err {worst:.3e} (e32 {r['e32']:.3e})")
    if name == "T1":                                                          # lengths 0 and 1 align, length 2 has no alignment
        lens = [len(l) for l in labelings]
        assert {0, 1, 2} <= set(lens) and all((r["rows"][b] is None) == (lens[b] == 2) for b in range(B))
    else:
        assert aligned >= B - B // 8, (aligned, B)                            # (an insertion can leave a short row without an alignment)
    again = _align(abi_dev, x, C, target, n + 1, blank, 1)                    # a second launch: equal bits
    for a, b_ in zip(got, again):
        assert torch.equal(a.view(torch.uint8), b_.view(torch.uint8))
    off0 = _align(abi_dev, x, C, target, n, blank, 0, frames=False)           # len_offset 0 and 1 agree on shifted lengths; no frame_label
    for a, b_ in zip(got[:4], off0[:4]):
        assert torch.equal(a.view(torch.uint8), b_.view(torch.uint8))
    pub = ctc_align(x.to(abi_dev), C, target.to(abi_dev), (n + 1).to(abi_dev), blank, want_frames=True)     # the Python surface: the same call
    assert len(pub) == 5 and len(ctc_align(x.to(abi_dev), C, target.to(abi_dev), (n + 1).to(abi_dev), blank)) == 4
    for a, b_ in zip(got, pub):
        assert a.dtype == b_.dtype and torch.equal(a.view(torch.uint8), b_.cpu().view(torch.uint8))


def test_ctc_align_edge_cases(abi_dev):
    """n = 0; "aa" at T = 3; rows without an alignment (n + repeats > T, the blank as a label, a label >= C, a negative label), whose NaN pad
    columns prove that nothing is indexed by such a label; target_len beyond ldt."""
    T, C, ldt, blank = 3, 5, 4, 4
    x, _ = _draw(T, C, 9, seed=31, peak=2.5, bump=2.0)
    assert x.shape[2] == 128 and bool(torch.isnan(x[:, :, C:]).all())
    labelings = [[], [1, 1], [0, 1, 2], [1, 1, 2], [1, blank], [2, C], [2, 127], [-1], [3, 0, 3, 0]]
    lens = torch.tensor([1, 3, 4, 4, 3, 3, 3, 2, 9])                           # (with EOS; the last one beyond ldt: clamped to 4 labels > T)
    target, n = _rows(labelings, ldt)
    start, end, clp, plp, fl = _align(abi_dev, x, C, target, lens, blank, 1)
    lp64, lp32 = _tables(x, C)
    e32 = max(abs(float(AM.viterbi(lp32[b], labelings[b], blank)[0]) - float(AM.viterbi(lp64[b], labelings[b], blank)[0])) for b in (0, 1, 2))
    # n = 0: the all-blank path
    want = float(lp64[0, :, blank].sum())
    assert abs(float(plp[0]) - want) <= _bound(e32, want) and fl[0].tolist() == [-1] * T
    assert bool((start[0] == -1).all()) and bool((end[0] == -1).all()) and bool((clp[0] == 0).all())
    # "aa" at T = 3: a, blank, a
    assert fl[1].tolist() == [0, -1, 1] and start[1].tolist() == [0, 2, -1, -1] and end[1].tolist() == [1, 3, -1, -1]
    want = float(lp64[1, 0, 1] + lp64[1, 1, blank] + lp64[1, 2, 1])
    assert abs(float(plp[1]) - want) <= _bound(e32, want)
    assert abs(float(clp[1, 0]) - lp64[1, 0, 1]) <= _bound(e32, lp64[1, 0, 1]) and abs(float(clp[1, 1]) - lp64[1, 2, 1]) <= _bound(e32, lp64[1, 2, 1])
    # three distinct labels on three frames: one path
    assert fl[2].tolist() == [0, 1, 2] and start[2].tolist() == [0, 1, 2, -1] and end[2].tolist() == [1, 2, 3, -1]
    for b in range(3, 9):
        _check_no_alignment(b, start, end, clp, plp, fl)
    # target_len far beyond ldt is clamped to ldt: the same row as the exact length
    long_rows = [[0, 1], [2, 0]]
    t2, _ = _rows(long_rows, 2)
    a = _align(abi_dev, x[:2], C, t2, torch.tensor([3, 3]), blank, 1)
    b_ = _align(abi_dev, x[:2], C, t2, torch.tensor([50, 2 ** 40]), blank, 1)
    for u, v in zip(a, b_):
        assert torch.equal(u.view(torch.uint8), v.view(torch.uint8))
    assert bool((a[3] > float("-inf")).all()) and bool((a[0] >= 0).all())
    # a negative length is no label at all
    c = _align(abi_dev, x[:2], C, t2, torch.tensor([0, -5]), blank, 1)
    assert c[4].tolist() == [[-1] * T] * 2 and bool((c[0] == -1).all())


def test_ctc_align_finds_the_best_member_of_every_labeling(abi_dev):
    """T = 5, C = 4: all 4^5 frame strings grouped by their collapse.  The best member of a group is the best alignment of its labeling; the
    device must return it wherever the group's two best members are at least G apart (the specification does, checked first)."""
    T, C, blank, ldt = 5, 4, 3, 5
    x, _ = _draw(T, C, 2, seed=5454, peak=2.5, bump=2.0)
    lp64, lp32 = _tables(x, C)
    strings = list(itertools.product(range(C), repeat=T))
    groups = {}
    for f in strings:
        groups.setdefault(tuple(_collapse(list(f), blank)), []).append(f)
    labelings = sorted(groups, key=lambda l: (len(l), l))
    every = [l for k in range(T + 1) for l in itertools.product(range(C - 1), repeat=k)]
    assert sorted(l for l in every if AM.feasible(l, blank, T, C)) == sorted(labelings) and len(labelings) < len(every)
    target, n = _rows([list(l) for l in labelings], ldt)
    total_kept = 0
    for s in range(2):
        _, rows, e32, G = _specify(x[s:s + 1].expand(len(labelings), T, x.shape[2]), C, [list(l) for l in labelings], blank)
        xs = x[s:s + 1].expand(len(labelings), T, x.shape[2]).contiguous()
        start, end, clp, plp, fl = _align(abi_dev, xs, C, target, n, blank, 0)
        kept = 0
        for b, l in enumerate(labelings):
            scored = sorted(((float(sum(lp64[s, t, f[t]] for t in range(T))), f) for f in groups[l]), reverse=True)
            gap = scored[0][0] - scored[1][0] if len(scored) > 1 else float("inf")
            best = list(scored[0][1])
            want = [-1 if c == blank else None for c in best]                 # the member as a frame_label row
            k = -1
            for t, c in enumerate(best):
                if c != blank:
                    k += 0 if (t > 0 and best[t - 1] == c) else 1
                    want[t] = k
            if gap >= G:
                kept += 1
                assert AM.states_of_frame_labels(want) == rows[b]["states"], (s, l, want, rows[b]["states"])    # the specification
                assert abs(rows[b]["s64"] - scored[0][0]) <= 1e-12
                assert fl[b].tolist() == want, (s, l, fl[b].tolist(), want)
                assert abs(float(plp[b]) - scored[0][0]) <= _bound(e32, scored[0][0])
            _check_sample(b, list(l), blank, lp64[s], rows[b], e32, G, start, end, clp, plp, fl, ldt)
        print(f"sample {s}: {kept} of {len(labelings)} labelings kept (G {G:.3e})")
        total_kept += kept
    assert total_kept >= len(labelings)                                       # (at least half of the groups of the two samples)


def test_ctc_align_of_the_greedy_rows_is_the_frame_argmax(abi_dev):
    """Aligning the rows of dig_ctc_greedy_decode (eos outside [0, C): nothing is removed) gives the arg-max path: path_logp = sum_t max_c lp,
    the spans are the runs of the frame arg-max."""
    from dig_amd.ctc_recognizer import ctc_align, ctc_greedy_decode
    T, C, B = 32, 98, 8
    blank, eos, pad = C - 1, -1, C + 5
    x, _ = _draw(T, C, B, seed=808, peak=5.0, bump=4.0)
    lp64, lp32 = _tables(x, C)
    xd = x.to(abi_dev)
    ids, _, n = ctc_greedy_decode(xd, C, blank, eos, pad)
    assert tuple(ids.shape) == (B, T + 1)
    start, end, clp, plp, fl = (t.cpu() for t in ctc_align(xd, C, ids, n.long(), blank, len_offset=0, want_frames=True))
    am = torch.from_numpy(lp64).argmax(-1)
    e32 = float(np.abs(lp32.max(-1).astype(np.float64).sum(-1) - lp64.max(-1).sum(-1)).max())
    for b in range(B):
        want = float(lp64[b].max(-1).sum())
        assert abs(float(plp[b]) - want) <= _bound(e32, want), (b, float(plp[b]), want)
        row = am[b].tolist()
        runs = [(t, c) for t, c in enumerate(row) if c != blank and not (t > 0 and row[t - 1] == c)]
        assert int(n[b]) == len(runs) and ids[b, :len(runs)].tolist() == [c for _, c in runs]
        for k, (t0, c) in enumerate(runs):
            t1 = t0
            while t1 < T and row[t1] == c:
                t1 += 1
            assert (int(start[b, k]), int(end[b, k])) == (t0, t1), (b, k)
        assert [(-1 if c == blank else 0) for c in row] == [min(v, 0) for v in fl[b].tolist()]


# ---------------------------------------------------------------------------------------------- 2. host-side validation (no GPU)
@pytest.mark.parametrize("build", ["hip", "cpu_abi"])
def test_ctc_align_entry_point_validates_on_the_host(build):
    """Each smallest refused call of dig_ctc_align before any launch, on both builds; a refused call leaves poisoned outputs untouched; B = 0
    returns OK without a launch."""
    from cpu_abi_util import build as build_cpu
    from dig_amd import _lib as L
    lib = ctypes.CDLL(L.LIB_PATH if build == "hip" else build_cpu())
    f = lib.dig_ctc_align
    f.restype, f.argtypes = ctypes.c_int, L._prototypes()["dig_ctc_align"]
    assert len(f.argtypes) == 16
    ARG, UNS, OK = L.const("DIG_ERR_ARG"), L.const("DIG_ERR_UNSUPPORTED"), L.const("DIG_OK")
    poison = 0x5A
    names = ("x", "target", "lens", "start", "end", "clp", "plp", "fl")
    bufs = {k: (ctypes.c_ubyte * 4096)(*([poison] * 4096)) for k in names}
    p = {k: ctypes.cast(v, ctypes.c_void_p) for k, v in bufs.items()}

    def call(**kw):
        a = dict(p, ld=128, ldt=25, off=1, B=4, T=32, C=98, blank=97)
        a.update(kw)
        return f(a["x"], a["ld"], a["target"], a["ldt"], a["lens"], a["off"], a["B"], a["T"], a["C"], a["blank"], a["start"], a["end"], a["clp"],
                 a["plp"], a["fl"], None)

    for k in names[:-1]:
        assert call(**{k: None}) == ARG, k
    for kw in ({"B": -1}, {"T": 0}, {"C": 0}, {"ldt": 0}, {"ld": 97}, {"blank": 98}, {"blank": -1}):
        assert call(**kw) == ARG, kw
    for kw in ({"T": 65}, {"C": 257, "ld": 257, "blank": 0}, {"C": 1, "ld": 1, "blank": 0}, {"ldt": 64}):
        assert call(**kw) == UNS, kw
    assert call(B=0) == OK and call(B=0, fl=None) == OK and call(B=0, T=64, C=256, ld=256, blank=255, ldt=63) == OK
    assert all(all(v == poison for v in b) for b in bufs.values())


def test_both_builds_export_the_entry_point():
    import subprocess
    from cpu_abi_util import exported
    from dig_amd import _lib as L
    assert "dig_ctc_align" in exported()
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert any(line.split()[-1] == "dig_ctc_align" for line in out.splitlines())


# ---------------------------------------------------------------------------------------------- 3. wiring: the model, evaluate(), the records
def test_alignment_records_of_a_batch(abi_dev):
    """`CTCAlignment` on the alignment of a batch through a stub of the model: characters by the vocabulary, boxes = spans * frame_columns, the
    record of a row without an alignment; and `evaluate` with args.ctc_align_out writes these records, index and ground truth added, in
    evaluation order, with the meters it returns without the flag."""
    import tempfile
    import types
    from dig_amd.ctc_recognizer import CTCRecModelTrain
    from dig_amd.datasets import find_classes
    from dig_amd.engine_for_finetuning import evaluate
    from dig_amd.evaluation_metric import CTCAlignment
    from test_ctc_beam import _StubCTC
    T, C, B = 32, 98, 8
    voc = find_classes("ALLCASES_SYMBOLS")
    assert len(voc) + 1 == C and CTCRecModelTrain.frame_columns == 4
    blank, eos, pad = C - 1, voc.index("EOS"), voc.index("PADDING")
    x, frames = _draw(T, C, B, seed=7100 + 100 * T + C, peak=5.0, bump=4.0)
    x = x[:, :, :C].contiguous()
    words = _forms(frames, C, seed=T + C)
    words[5] = [voc.index("a")] * 20                                           # 20 + 19 repeats > 32 frames: no alignment
    words[6] = [voc.index("Q"), voc.index("UNKNOWN"), voc.index("!")]
    target = torch.full((B, 40), pad, dtype=torch.int64)
    for b, l in enumerate(words):
        target[b, :len(l)] = torch.tensor(l, dtype=torch.int64)
        target[b, len(l)] = eos
    lens = torch.tensor([len(l) + 1 for l in words])
    dataset = types.SimpleNamespace(idx_to_class={i: c for i, c in enumerate(voc)})

    def stub(batches):
        m = _StubCTC(batches, C, eos, pad, 0)
        m.align = types.MethodType(CTCRecModelTrain.align, m)
        m.frame_columns = CTCRecModelTrain.frame_columns
        return m

    m = stub([x])
    spans = m.align(x.to(abi_dev), target, lens)
    recs = CTCAlignment(dataset, m.frame_columns)(target, lens - 1, *spans)
    start, end, clp, plp = (t.cpu() for t in spans)
    assert len(recs) == B and tuple(start.shape) == (B, 40)
    for b, (rec, l) in enumerate(zip(recs, words)):
        text = "".join(voc[c] if len(voc[c]) == 1 else "\ufffd" for c in l)
        assert rec["text"] == text
        if b == 5:
            assert rec == {"text": "a" * 20, "path_logp": None, "chars": []} and float(plp[b]) == float("-inf")
            continue
        assert rec["path_logp"] == float(plp[b]) and "".join(c[0] for c in rec["chars"]) == text and len(rec["chars"]) == len(l)
        for k, (ch, x0, x1, logp) in enumerate(rec["chars"]):
            assert (x0, x1, logp) == (4 * int(start[b, k]), 4 * int(end[b, k]), float(clp[b, k])) and 0 <= x0 < x1 <= 128
        assert [c[1] for c in rec["chars"]] == sorted(c[1] for c in rec["chars"])
    assert recs[6]["text"] == "Q\ufffd!"
    # ---- evaluate(): two batches, targets and predictions
    split = ((0, 3), (3, B))
    batches = [(torch.zeros(hi - lo, 3, 32, 128), target[lo:hi], lens[lo:hi]) for lo, hi in split]
    loader = type("Loader", (list,), {})(batches)
    loader.dataset = dataset
    logits = [x[lo:hi] for lo, hi in split]
    plain = evaluate(loader, stub(logits), abi_dev, types.SimpleNamespace(beam_width=0))
    with tempfile.TemporaryDirectory() as tmp:
        for of in ("target", "prediction"):
            path = os.path.join(tmp, of + ".jsonl")
            args = types.SimpleNamespace(beam_width=0, ctc_align_out=path, ctc_align_of=of)
            assert evaluate(loader, stub(logits), abi_dev, args) == plain
            lines = [json.loads(s) for s in open(path, encoding="utf-8")]
            assert [r["index"] for r in lines] == list(range(B))
            assert [r["word"] for r in lines] == [r["text"] for r in recs]
            if of == "target":
                assert [{k: v for k, v in r.items() if k not in ("index", "word")} for r in lines] == recs
            else:
                ids, _, n = stub(logits).decode(x.to(abi_dev))
                want = CTCAlignment(dataset, 4)(ids, n, *m.align(x.to(abi_dev), ids, n, len_offset=0))
                assert [{k: v for k, v in r.items() if k not in ("index", "word")} for r in lines] == want
                assert all("".join(c[0] for c in r["chars"]) == r["text"] for r in lines)


_TINY = {}


def _tiny(golden_dir):
    """The tiny model of tests/test_ctc.py on the device, its evaluation logits (the classifier scaled as the fixture scales it), and their
    two specification tables."""
    if not _TINY:
        from test_ctc import _device_model, _fixture, _scaled
        f = _fixture(golden_dir)
        m = _device_model(f, _scaled(f["P"], float(f["z"]["cls_scale"]))).eval()
        with torch.no_grad():
            logits = m.logits(f["images"].to("cuda:0"))
        _TINY.update(f=f, m=m, logits=logits)
    return _TINY


@pytest.mark.gpu
@pytest.mark.parametrize("rows_of", ["target", "greedy", "beam", "lexicon"])
def test_ctc_model_align_against_the_specification(golden_dir, rows_of):
    """`CTCRecModelTrain.align` on the tiny model's own logits: the fixture's targets (len_offset 1) and the rows of its three decoders
    (len_offset 0), each against the specification on the logits the device produced."""
    from dig_amd.ctc_recognizer import ctc_lexicon_decode
    t = _tiny(golden_dir)
    f, m, logits = t["f"], t["m"], t["logits"]
    voc = f["voc"]
    blank = len(voc)
    B, T, C = logits.shape
    assert (T, C, m.blank) == (32, blank + 1, blank)
    if rows_of == "target":
        rows, lens, off = f["targets"], f["lens"], 1
    elif rows_of == "lexicon":                                                # (the fixture's 37 classes are no named vocabulary: a pool of label rows)
        g = torch.Generator().manual_seed(9)
        pool = torch.randint(0, voc.index("EOS"), (12, 6), generator=g).to(torch.int32)
        pool_len = torch.randint(0, 7, (12,), generator=g).to(torch.int32)
        _, _, ids, _, n = ctc_lexicon_decode(logits, C, blank, m.eos, m.padding, (pool.to("cuda:0"), pool_len.to("cuda:0")), [0] * B, [12] * B)
        rows, lens, off = ids.cpu(), n.cpu().long(), 0
    else:
        ids, _, n = m.decode(logits, beam_width=4 if rows_of == "beam" else 0)
        rows, lens, off = ids.cpu(), n.cpu().long(), 0
    start, end, clp, plp = (v.cpu() for v in m.align(logits, rows, lens, len_offset=off))
    ldt = min(rows.shape[1], 63)
    assert tuple(start.shape) == (B, ldt) and start.dtype == torch.int32 and clp.dtype == torch.float32
    labelings = [rows[b, :max(int(lens[b]) - off, 0)].tolist() for b in range(B)]
    lp64, spec, e32, G = _specify(logits.cpu(), C, labelings, blank)
    aligned = 0
    for b, l in enumerate(labelings):
        if spec[b] is None:
            _check_no_alignment(b, start, end, clp, plp, None)
            continue
        aligned += 1
        n = len(l)
        own_start, own_end = start[b, :n].tolist(), end[b, :n].tolist()
        assert all(0 <= s_ < e for s_, e in zip(own_start, own_end)) and all(e <= s_ for e, s_ in zip(own_end, own_start[1:]))
        assert bool((start[b, n:] == -1).all()) and bool((clp[b, n:] == 0).all())
        if spec[b]["gap"] >= G:
            want_start, want_end, want_clp = AM.spans(lp64[b], l, blank, spec[b]["states"])
            assert own_start == want_start and own_end == want_end, (b, own_start, want_start)
            assert abs(float(plp[b]) - spec[b]["s64"]) <= _bound(e32, spec[b]["s64"])
            for k in range(n):
                assert abs(float(clp[b, k]) - float(want_clp[k])) <= _bound(e32, want_clp[k])
    print(f"{rows_of}: {aligned} of {B} rows aligned, e32 {e32:.3e}, G {G:.3e}")
    assert aligned >= 1


# ---------------------------------------------------------------------------------------------- 4. the driver
from test_finetune_driver import COMMON, _driver  # noqa: E402

CTC16 = COMMON.replace("--synthetic 32", "--synthetic 16") + " --decoder_type ctc"


def test_driver_ctc_align_flags(tmp_path):
    drv = _driver()
    out = str(tmp_path / "align.jsonl")
    args = drv.get_args(CTC16.split())
    assert args.ctc_align_out is None and args.ctc_align_of == "prediction"
    args = drv.get_args((CTC16 + f" --ctc_align_out {out} --ctc_align_of target").split())
    assert (args.ctc_align_out, args.ctc_align_of) == (out, "target")
    assert drv.get_args((CTC16 + f" --ctc_align_out {out} --ctc_beam_width 4").split()).ctc_beam_width == 4
    for head in ("tf_decoder", "attention"):
        with pytest.raises(SystemExit, match="--ctc_align_out.*--decoder_type ctc"):
            drv.get_args((COMMON + f" --decoder_type {head} --ctc_align_out {out}").split())
    with pytest.raises(SystemExit, match="--ctc_align_out"):
        drv.get_args((COMMON + f" --ctc_align_out {out}").split())
    with pytest.raises(SystemExit, match="--ctc_align_out.*does not exist"):
        drv.get_args((CTC16 + f" --ctc_align_out {tmp_path / 'missing' / 'align.jsonl'}").split())
    with pytest.raises(SystemExit, match="--ctc_align_of"):
        drv.get_args((CTC16 + " --ctc_align_of target").split())
    assert "--ctc_align_out" in drv.__doc__ and "--ctc_align_of" in drv.__doc__
    assert not os.path.exists(out)                                            # (parsing the flag creates nothing)


@pytest.mark.gpu
def test_ctc_driver_writes_the_alignment(tmp_path, monkeypatch):
    """--eval on 16 synthetic images with --ctc_align_out: 16 lines whose characters concatenate to the text, boxes that are increasing multiples
    of 4 inside [0, 128] and repeat what `model.align` returned for the batch; the meters of the run without the flag; the flag is named once."""
    import contextlib
    import io
    from dig_amd.ctc_recognizer import CTCRecModelTrain
    drv = _driver()
    base = CTC16 + f" --epochs 1 --eval --output_dir {tmp_path}"
    seen = []
    real = CTCRecModelTrain.align

    def recording(self, logits, rows, lengths, len_offset=1):
        out = real(self, logits, rows, lengths, len_offset)
        seen.append((rows.cpu(), lengths.cpu().long() - len_offset, [t.cpu() for t in out]))
        return out
    monkeypatch.setattr(CTCRecModelTrain, "align", recording)
    with contextlib.redirect_stdout(io.StringIO()) as quiet:
        plain = drv.main(drv.get_args(base.split()))["test_stats"]
    assert not seen and "--ctc_align_out" not in quiet.getvalue()
    for of in ("prediction", "target"):
        path = str(tmp_path / (of + ".jsonl"))
        with open(path, "w") as fh:
            fh.write("stale\n")                                               # (the run starts the file afresh)
        del seen[:]
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            stats = drv.main(drv.get_args((base + f" --ctc_align_out {path} --ctc_align_of {of}").split()))["test_stats"]
        assert stats == plain and buf.getvalue().count("--ctc_align_out") == 1
        lines = [json.loads(s) for s in open(path, encoding="utf-8")]
        assert len(lines) == 16 and [r["index"] for r in lines] == list(range(16))
        assert sum(len(rows) for rows, _, _ in seen) == 16
        i = 0
        for rows, n, (start, end, clp, plp) in seen:
            for b in range(rows.shape[0]):
                r, k = lines[i], int(n[b])
                i += 1
                if r["path_logp"] is None:
                    assert float(plp[b]) == float("-inf") and r["chars"] == []
                    continue
                assert "".join(c[0] for c in r["chars"]) == r["text"] and len(r["chars"]) == k and r["path_logp"] == float(plp[b])
                edges = [v for c in r["chars"] for v in (c[1], c[2])]
                assert edges == sorted(edges) and all(v % 4 == 0 and 0 <= v <= 128 for v in edges) and all(c[1] < c[2] for c in r["chars"])
                assert [(c[1], c[2], c[3]) for c in r["chars"]] == [(4 * int(start[b, j]), 4 * int(end[b, j]), float(clp[b, j])) for j in range(k)]
                if of == "target":
                    assert r["text"] == r["word"] and k >= 1
        assert all(isinstance(r["word"], str) and r["word"] for r in lines)


# ---------------------------------------------------------------------------------------------- 5. the build
def test_ctc_align_kernel_uses_no_scratch():
    from dig_amd import build
    build.build(verbose=False)
    rows = [r for r in build.kernel_resources() if r["name"].startswith("ctc_align_kernel")]
    assert len(rows) == 1 and rows[0]["scratch"] == 0 and rows[0]["hot"], rows
