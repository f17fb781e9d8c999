#!/usr/bin/env python
"""Record the parameter-arena layout of every model family, one line per fact, for a parent / child comparison of a change to the layout code
(CPU only; prints to stdout).  Per model: a sha256 over the ordered (name, offset, numel, shape, group, arena) list, the arena sizes, the
granule group bytes, the gradient buckets, the granule index table FineTuneAdamW builds and the state_dict() key order.

    python tools/arena_layout_dump.py > layout.txt          # at both commits, then diff the two files
"""
import hashlib
import os
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from dig_amd.finetune import LayerDecayValueAssigner, RecModelTrain, create_optimizer  # noqa: E402
from dig_amd.recognizer import ENCODERS, RecModel  # noqa: E402
from dig_amd.registry import create_model  # noqa: E402

KW = dict(pretrained=False, drop_path_rate=0.0, mlp_dim=4096, dim=256, T=0.2, num_windows=5, queue_size=65536)


def sha(obj):
    return hashlib.sha256(obj if isinstance(obj, bytes) else repr(obj).encode()).hexdigest()[:32]


def slot_rows(slots):
    """(name, offset, numel, shape, group, arena) of a name -> slot mapping whose values are objects with those fields or plain
    (offset, numel, shape[, group, arena]) tuples."""
    rows = []
    for n, s in slots.items():
        if hasattr(s, "offset"):
            rows.append((n, int(s.offset), int(s.numel), tuple(s.shape), getattr(s, "group", None), getattr(s, "arena", None)))
        else:
            rows.append((n, int(s[0]), int(s[1]), tuple(s[2])) + (tuple(s[3:5]) if len(s) >= 5 else (None, None)))
    return rows


def dump_pretrain(tag, m):
    print(f"{tag} slots={len(m.specs)} layout={sha(slot_rows(m.specs))}")
    print(f"{tag} n_online={m.n_online} n_ema={m.n_ema} momentum_numel={m._flat['momentum'].numel()}")
    print(f"{tag} flat_groups={sha(m.flat_groups.numpy().tobytes())} granules={m.flat_groups.numel()}")
    print(f"{tag} bucket_ranges={[(k,) + tuple(m.bucket_range(k)) for k in m.bucket_names]}")
    print(f"{tag} bucket_groups={sorted(m.bucket_groups().items())}")
    print(f"{tag} state_dict_keys={sha(list(m.state_dict().keys()))} n={len(m.state_dict())}")


def dump_rec(tag, m, opt=None):
    print(f"{tag} slots={len(m._offsets)} layout={sha(slot_rows(m._offsets))}")
    print(f"{tag} n_flat={m.n_flat}")
    print(f"{tag} state_dict_keys={sha(list(m.state_dict().keys()))} n={len(m.state_dict())}")
    if opt is not None:
        opt._tables()
        print(f"{tag} adamw_granule_table={sha(opt._idx.numpy().tobytes())} granules={opt._idx.numel()} groups={len(opt.param_groups)}")


def main():
    torch.manual_seed(0)
    for size in ("tiny", "small", "base"):
        dump_pretrain(f"simmim_moco_{size}", create_model(f"pretrain_simmim_moco_ori_vit_{size}_patch4_32x128", patchnet_name="no_patchtrans", **KW))
    dump_pretrain("dis_only_small", create_model("pretrain_moco_ori_vit_small_patch4_32x128", patchnet_name="no_patchtrans", **KW))
    dump_pretrain("gen_only_small", create_model("pretrain_simmim_ori_vit_small_patch4_32x128", patchnet_name="no_patchtrans", **KW))
    for pn in ("regular", "conv", "no_patchtrans"):
        dump_pretrain(f"simmim_moco_small_{pn}", create_model("pretrain_simmim_moco_ori_vit_small_patch4_32x128", patchnet_name=pn, **KW))
    oargs = dict(opt="adamw", lr=1e-4, weight_decay=0.05, opt_eps=1e-8, opt_betas=[0.9, 0.999])
    for enc in ENCODERS:
        size = enc.split("_")[2]
        for dec, one_d in (("tf_decoder", False), ("small_tf_decoder", False), ("tf_decoder", True)):
            args = types.SimpleNamespace(model=enc, decoder_name=dec, nb_classes=97, max_len=25, use_1d_attdec=one_d, **oargs)
            tag = f"{size}_{dec}{'_1d' if one_d else ''}"
            dump_rec(f"rec_{tag}", RecModel(args))
            for fixed in (0, 3):
                m = RecModelTrain(args)
                m.fix_encoder_layers(fixed)
                nl = m.get_num_layers()
                asg = LayerDecayValueAssigner([0.75 ** (nl + 1 - i) for i in range(nl + 2)])
                dump_rec(f"rec_train_{tag}_fixed{fixed}", m, create_optimizer(args, m, get_num_layer=asg.get_layer_id, get_layer_scale=asg.get_scale))


if __name__ == "__main__":
    main()
