"""The layout rules of the flat parameter arenas, written once for the pre-training model (MoCo_ViT) and the recognition models (RecModel):
where a tensor starts, how the q / v biases of a block form the fused-QKV bias vector, the encoder's parameter names, and the views the
kernels read.  The AdamW granule tables, the EMA over mirrored offsets and the fused projections all rest on these rules.  No GPU needed."""
import math
from collections import OrderedDict
from typing import NamedTuple

import numpy as np
import torch

ALIGN = 256  # arena granule (elements): every parameter starts on a 1 KiB boundary

# per encoder block, under the key names encoder_blocks reads: fp32 parameters, bf16 GEMM operands, and the gradients ("g") of both
ENC_F32 = ("norm1.weight", "norm1.bias", "attn.proj.bias", "norm2.weight", "norm2.bias", "mlp.fc1.bias", "mlp.fc2.bias")
ENC_W16 = ("attn.qkv.weight", "attn.proj.weight", "mlp.fc1.weight", "mlp.fc2.weight")
ENC_GRAD = ENC_F32 + ENC_W16


class Slot(NamedTuple):
    """One parameter's place: elements [offset, offset + numel) of its arena.  group: the optimizer's granule group, arena: which arena
    (None where a model has one arena and no group table)."""
    offset: int
    numel: int
    shape: tuple
    group: object = None
    arena: object = None


def round_up(n):
    return (n + ALIGN - 1) // ALIGN * ALIGN


def _slot(v):
    return v if isinstance(v, Slot) else Slot(None, math.prod(v), tuple(v))


def place(shapes, start=0, groups=None):
    """Lay the tensors of `shapes` (ordered name -> shape, or name -> Slot still without an offset) out from element `start`, in that order,
    each on an ALIGN boundary; every value becomes its placed Slot (the order of the mapping is kept: state dicts and optimizer indices follow
    it).  `attn.q_bias` and `attn.v_bias` of a block share one bundle q_bias | zeros | v_bias = the [3D] bias vector of the fused QKV GEMM (K has
    no bias; the gap belongs to no slot and stays zero).  groups: a list that receives the slot's group once per granule.  Returns the end."""
    off = start
    for name in list(shapes):
        s, size = _slot(shapes[name]), None
        if name.endswith("attn.v_bias") and name[:-6] + "q_bias" in shapes:
            continue                                                        # placed with its q_bias
        if name.endswith("attn.q_bias") and name[:-6] + "v_bias" in shapes:
            shapes[name[:-6] + "v_bias"] = _slot(shapes[name[:-6] + "v_bias"])._replace(offset=off + 2 * s.numel)
            size = 3 * s.numel
        shapes[name] = s._replace(offset=off)
        padded = round_up(size or s.numel)
        if groups is not None:
            groups.extend([s.group] * (padded // ALIGN))
        off += padded
    return off


def encoder_shapes(prefix, D, F, depth, final_norm):
    """The ViT encoder's parameters in registration order (modeling_pretrain_vit.py:27-111, blocks modeling_finetune.py:43-170)."""
    o = OrderedDict()
    o[prefix + "mask_token"] = (1, 1, D)
    o[prefix + "patch_embed.proj.weight"] = (D, 3, 4, 4); o[prefix + "patch_embed.proj.bias"] = (D,)
    for i in range(depth):
        b = f"{prefix}blocks.{i}."
        o[b + "norm1.weight"] = (D,); o[b + "norm1.bias"] = (D,)
        o[b + "attn.q_bias"] = (D,); o[b + "attn.v_bias"] = (D,)
        o[b + "attn.qkv.weight"] = (3 * D, D); o[b + "attn.proj.weight"] = (D, D); o[b + "attn.proj.bias"] = (D,)
        o[b + "norm2.weight"] = (D,); o[b + "norm2.bias"] = (D,)
        o[b + "mlp.fc1.weight"] = (F, D); o[b + "mlp.fc1.bias"] = (F,); o[b + "mlp.fc2.weight"] = (D, F); o[b + "mlp.fc2.bias"] = (D,)
    if final_norm:
        o[prefix + "norm.weight"] = (D,); o[prefix + "norm.bias"] = (D,)
    return o


def view(flat, slot):
    return flat[slot.offset:slot.offset + slot.numel].view(slot.shape)


def split(flats, slots, names, skip=()):
    """{index in `names`: {key: the name's view of flats[key]}}: flat arenas (Adam moments) in torch.optim's per-parameter state layout."""
    return {i: {k: view(f, slots[n]) for k, f in flats.items()} for i, n in enumerate(names) if n not in skip}


def join(flats, slots, names, state):
    """Write a split() layout back into the flat arenas: zeroed, then every listed tensor copied to its slot (shapes checked)."""
    for f in flats.values():
        f.zero_()
    for i, st in state.items():
        slot = slots[names[int(i)]]
        for k, f in flats.items():
            if tuple(st[k].shape) != slot.shape:
                raise ValueError(f"optimizer state {i} ({names[int(i)]}): shape {tuple(st[k].shape)} != {slot.shape}")
            view(f, slot).copy_(st[k])


def group_names(groups):
    """The parameter names of an optimizer's groups, group by group: position = torch.optim's parameter index."""
    return [n for g in groups for n in g["names"]]


def optimizer_state_dict(moments, slots, groups, step, stateless=()):
    """A fused optimizer's checkpoint in torch.optim's per-parameter layout (what the reference's checkpoints hold, custom_optim/optimizer.py
    state_dict): {'state': {i: {'step', moment views}}, 'param_groups': [{..., 'params': [i, ...]}]} with i enumerating the groups' "names" group
    by group.  moments: {key: flat arena}; step: the one step counter (0: no state yet); stateless: names that hold an index but no state."""
    state = split(moments, slots, group_names(groups), stateless) if step > 0 else {}
    for st in state.values():
        st["step"] = step
    out, k = [], 0
    for g in groups:
        d = {key: v for key, v in g.items() if key not in ("params", "names")}
        d.setdefault("amsgrad", False)
        d["params"] = list(range(k, k + len(g["names"])))
        k += len(g["names"])
        out.append(d)
    return {"state": state, "param_groups": out}


def load_optimizer_state(moments, slots, groups, sd):
    """The reverse of optimizer_state_dict: checks the group shapes, writes the moments back (join) and returns the step counter."""
    if [len(g["params"]) for g in sd["param_groups"]] != [len(g["names"]) for g in groups]:
        raise ValueError("loaded state dict has different parameter groups")
    join(moments, slots, group_names(groups), sd["state"])
    steps = {int(st["step"]) for st in sd["state"].values()}
    if len(steps) > 1:
        raise ValueError("per-parameter step counts differ; the fused optimizer keeps one step counter")
    return steps.pop() if steps else 0


def fused(flat, slots, first, count):
    """`count` [out, in] weights registered from `first` on as one [count * out, in] matrix (q|k|v, k|v): they must lie back to back."""
    names = list(slots)
    i = names.index(first)
    o, n, s = slots[first][:3]
    run = names[i:i + count]
    assert len(run) == count and all(slots[m][:3] == (o + j * n, n, s) for j, m in enumerate(run)), (first, run)
    return flat[o:o + count * n].view(count * s[0], s[1])


def qkv_bias(flat, slots, block_prefix, D):
    """The [3D] vector q_bias | zeros | v_bias of one block (see place)."""
    o = slots[block_prefix + "attn.q_bias"].offset
    assert slots[block_prefix + "attn.v_bias"].offset == o + 2 * D
    return flat[o:o + 3 * D]


def enc_block_views(slots, prefix, depth, D, f32, w16, grads=None):
    """One dict per encoder block for encoder_blocks: ENC_F32 names and "qkv_bias" as views of the arena `f32`, ENC_W16 names of its bf16
    shadow `w16`; with `grads`, "g": ENC_GRAD names and "qkv_bias" in the gradient arena."""
    blocks = []
    for i in range(depth):
        b = f"{prefix}blocks.{i}."
        blk = {k: view(f32, slots[b + k]) for k in ENC_F32}
        blk.update({k: view(w16, slots[b + k]) for k in ENC_W16})
        blk["qkv_bias"] = qkv_bias(f32, slots, b, D)
        if grads is not None:
            blk["g"] = {k: view(grads, slots[b + k]) for k in ENC_GRAD}
            blk["g"]["qkv_bias"] = qkv_bias(grads, slots, b, D)
        blocks.append(blk)
    return blocks


def encoder_pos_table(n_pos, d):
    """The encoder's fixed position table, fp32 [n_pos, d]: get_sinusoid_encoding_table (modeling_finetune.py:200-210; float64 math, then cast)."""
    ang = np.arange(n_pos, dtype=np.float64)[:, None] / np.power(10000.0, 2.0 * (np.arange(d) // 2) / d)[None, :]
    ang[:, 0::2] = np.sin(ang[:, 0::2])
    ang[:, 1::2] = np.cos(ang[:, 1::2])
    return torch.from_numpy(ang).to(torch.float32)
