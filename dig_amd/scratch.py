"""The caller-owned scratch of the C ABI, one pool for every wrapper: a buffer per (tag, device, stream) that only grows.  Launches on one
stream are ordered, so wrappers that share a tag share memory; what must survive other launches (slabs pending until a flush, the zeroed
areas of the loss reductions) has a tag of its own.  Sizes come from the library's *_workspace_bytes queries (floats())."""
import functools

import torch

from . import _lib as L

_pool = {}


def get(tag, dev, numel, dtype=torch.float32, *, zero=False, floor=0):
    """At least `numel` elements, allocated at first use; a larger request replaces the buffer by one of max(numel, floor) elements
    (zero=True: zero-filled, for kernels that need and leave a zero ticket word)."""
    key = (tag, dev, L.stream_key(dev))
    w = _pool.get(key)
    if w is None or w.numel() < numel:
        w = _pool[key] = (torch.zeros if zero else torch.empty)(max(numel, floor), device=dev, dtype=dtype)
    return w


@functools.lru_cache(maxsize=None)
def _floats(lib_path, query, args):
    return (L.query(query, *args) + 3) // 4


def floats(query, *args):
    """fp32 elements of the scratch that `query` (a *_workspace_bytes of include/dig_hip.h) asks for; one FFI crossing per library and
    argument tuple (two builds answer the per-build queries differently)."""
    return _floats(L.lib()._name, query, args)


def drop(dev):
    """Forget every buffer of `dev`."""
    for key in [k for k in _pool if k[1] == dev]:
        del _pool[key]
