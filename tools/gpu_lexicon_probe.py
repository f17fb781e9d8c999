"""Throughput of the lexicon search (dig_lexicon_search): B = 256 predictions, T = 25, against synthetic lexicons of 50 words per image
(disjoint ranges), 1 000 words per image (disjoint ranges) and one shared lexicon of 90 000 words.  Prints (query, word) pairs per second.

    python tools/gpu_lexicon_probe.py [--len LO HI]     # lengths of queries and words, drawn uniformly; default 25 25 = 625 cells per pair
"""
import os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dig_amd import evaluation_metric as EM
dev = torch.device("cuda:0")
lo, hi = (int(sys.argv[sys.argv.index("--len") + 1]), int(sys.argv[sys.argv.index("--len") + 2])) if "--len" in sys.argv else (25, 25)
B, T = 256, 25
rng = np.random.RandomState(0)


def strings(n, ld):
    lens = rng.randint(lo, hi + 1, size=n).astype(np.int32)
    rows = rng.randint(ord("a"), ord("z") + 1, size=(n, ld)).astype(np.int32)
    rows[np.arange(ld)[None, :] >= lens[:, None]] = 0
    return torch.from_numpy(rows).to(dev), torch.from_numpy(lens).to(dev)


q, ql = strings(B, T)
for name, per_query, shared in (("50 per image", 50, False), ("1 000 per image", 1000, False), ("90 000 shared", 90000, True)):
    W = per_query if shared else per_query * B
    w, wl = strings(W, max(hi, 1))
    begin = [0] * B if shared else [b * per_query for b in range(B)]
    count = [per_query] * B
    for _ in range(3):
        best = EM.lexicon_search(q, ql, w, wl, begin, count)
    n = 10
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        best = EM.lexicon_search(q, ql, w, wl, begin, count)
    e1.record()
    torch.cuda.synchronize()
    dt = e0.elapsed_time(e1) * 1e-3 / n
    pairs = B * per_query
    print(f"lexicon search B={B} T={T} lengths {lo}-{hi}, {name}: {dt * 1e3:.3f} ms per batch = {pairs / dt:.3e} pairs/s "
          f"(mean distance {best[1].float().mean().item():.2f})")
