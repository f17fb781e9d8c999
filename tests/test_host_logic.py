"""Host-side logic of the product package on CPU: model surface (state_dict layout), flat-arena invariants, param
groups, schedules, checkpoint round trip, and the no-fallback rule.  No kernels run here."""
import os
import types

import numpy as np
import pytest
import torch

import dig_oracle as O
from dig_amd import utils as U
from dig_amd import arena
from dig_amd.arena import ALIGN
from dig_amd.modeling_pretrain_moco_mim_ori import MoCo_ViT
from dig_amd.optim_factory import create_optimizer, get_parameter_groups
from dig_amd.registry import create_model

KW = dict(pretrained=False, drop_path_rate=0.0, drop_block_rate=None, mlp_dim=4096, dim=256, T=0.2, num_windows=4,
          encoder_type='vit', queue_size=65536, patchnet_name='no_patchtrans')


@pytest.fixture(scope="module")
def small():
    torch.manual_seed(0)
    return create_model("pretrain_simmim_moco_ori_vit_small_patch4_32x128", **KW)


def tiny_model():
    cfg = O.DiGConfig(**O.TINY)
    return cfg, MoCo_ViT(encoder_embed_dim=cfg.embed_dim, encoder_depth=cfg.depth, encoder_num_heads=cfg.heads,
                         decoder_embed_dim=cfg.dec_dim, mlp_dim=cfg.moco_mlp_dim, dim=cfg.moco_dim, T=cfg.T, num_windows=4,
                         use_pixel_target=True, patchnet_name='no_patchtrans')


def test_state_dict_layout_matches_reference_inventory(small):
    cfg = O.make_config("pretrain_simmim_moco_ori_vit_small_patch4_32x128")
    ref_p, ref_b = O.param_shapes(cfg), O.buffer_shapes(cfg)
    named = list(small.named_parameters())
    assert [n for n, _ in named] == list(ref_p.keys())                       # names AND order
    assert all(tuple(p.shape) == ref_p[n] for n, p in named)
    sd = small.state_dict()
    assert len(sd) == 398
    for n, shp in ref_b.items():
        assert tuple(sd[n].shape) == shp, n
    assert sd["encoder_projection_layer.1.num_batches_tracked"].dtype == torch.int64
    assert [n for n, p in named if not p.requires_grad] == [n for n in ref_p if not O.is_trainable(n)]
    assert sum(p.numel() for _, p in named if p.requires_grad) == 43606192
    assert "pos_embed" not in " ".join(sd.keys()) and small.encoder.pos_embed.shape == (1, 256, 384)
    assert small.encoder.patch_embed.patch_size == (4, 4) and small.no_weight_decay() == {'pos_embed', 'cls_token'}


def test_pos_embed_equals_reference_formula(small):
    assert torch.equal(small.encoder.pos_embed[0], O.sinusoid_table(256, 384))


def test_arena_layout_invariants(small):
    m = small
    offs = sorted((s.offset, s.numel, n) for n, s in m.specs.items() if s.arena == "online")
    for (o1, n1, a), (o2, n2, b) in zip(offs, offs[1:]):
        assert o1 + n1 <= o2, (a, b)                                          # no overlap
    for n, s in m.specs.items():
        if not n.endswith("attn.v_bias"):
            assert s.offset % ALIGN == 0, n                                   # 1 KiB granules (AdamW group table, 16-B GEMM alignment)
        p = dict(m.named_parameters())[n]
        assert p.data_ptr() == m._flat[s.arena].data_ptr() + 4 * s.offset     # parameters are views of the arena
        if s.arena == "online":
            assert p.grad is not None and p.grad.data_ptr() == m._flat["grad"].data_ptr() + 4 * s.offset
    # q_bias | zeros | v_bias bundle = the fused-QKV bias vector
    D = m.D
    for i in range(m.depth):
        q, v = m.specs[f"encoder.blocks.{i}.attn.q_bias"], m.specs[f"encoder.blocks.{i}.attn.v_bias"]
        assert v.offset == q.offset + 2 * D
        assert torch.count_nonzero(m._flat["online"][q.offset + D:q.offset + 2 * D]) == 0
    # momentum arena mirrors the EMA-source prefix of the online arena
    for src, dst in O.ema_pairs([n for n in m.specs if m.specs[n].arena == "online"]):
        assert m.specs[src].offset == m.specs[dst].offset and m.specs[src].offset + m.specs[src].numel <= m.n_ema
    # gradient buckets tile the online arena exactly, in backward order
    rng = sorted(m.bucket_range(k) for k in m.bucket_names)
    assert rng[0][0] == 0 and rng[-1][1] == m.n_online
    assert all(a[1] == b[0] for a, b in zip(rng, rng[1:]))


def test_param_groups_follow_reference_rule(small):
    decay, no_decay = get_parameter_groups(small, 0.1, small.no_weight_decay())
    od, ond = O.param_groups(OrderedDictLike(small), 0.1)
    assert decay == od and no_decay == ond
    groups = small.flat_groups
    for n in decay + no_decay:
        s = small.specs[n]
        g = groups[s.offset // ALIGN:(s.offset + s.numel + ALIGN - 1) // ALIGN]
        assert bool((g == (0 if n in decay else 1)).all()), n
    assert "encoder.mask_token" in decay                                      # [1,1,D] is not 1-D: it decays in the reference


class OrderedDictLike(dict):
    def __init__(self, model):
        super().__init__((n, p) for n, p in model.named_parameters())


def test_optimizer_surface(small):
    args = types.SimpleNamespace(opt="adamw", lr=3e-4, weight_decay=0.1, opt_eps=1e-8, opt_betas=[0.9, 0.999])
    opt = create_optimizer(args, small)
    assert len(opt.param_groups) == 2
    g0, g1 = opt.param_groups
    assert g0["weight_decay"] == 0.1 and g1["weight_decay"] == 0.0 and g0["lr_scale"] == g1["lr_scale"] == 1.0
    assert g0["lr"] == 3e-4 and tuple(g0["betas"]) == (0.9, 0.999) and g0["eps"] == 1e-8
    assert sum(p.numel() for g in opt.param_groups for p in g["params"]) == 43606192
    with pytest.raises(NotImplementedError):
        create_optimizer(types.SimpleNamespace(opt="sgd", lr=1.0, weight_decay=0.0), small)


def test_schedules_bit_exact(golden_dir):
    g = np.load(os.path.join(golden_dir, "masks_schedules.npz"))
    assert np.array_equal(g["sched/lr"], U.cosine_scheduler(1.5e-4 * 4, 1e-5, 10, 50, warmup_epochs=1))
    assert np.array_equal(g["sched/lr_ws"], U.cosine_scheduler(6e-4, 1e-5, 10, 50, warmup_epochs=1, warmup_steps=20))
    assert np.array_equal(g["sched/wd"], U.cosine_scheduler(0.1, 0.1, 10, 50))
    a = types.SimpleNamespace(epochs=10, moco_m=0.99)
    assert np.array_equal(g["sched/moco_m"], np.array([U.adjust_moco_momentum(e / 7.0, a) for e in range(70)]))
    with pytest.raises(AssertionError):                                       # the reference's quirk is kept
        U.cosine_scheduler(6e-4, 1e-5, 10, 50, warmup_epochs=0, warmup_steps=20)


def test_state_dict_roundtrip_and_checkpoint(tmp_path):
    cfg, m = tiny_model()
    P, S = O.det_state(cfg, 9)
    m.load_state_dict({**P, **S})
    sd = m.state_dict()
    for k, v in {**P, **S}.items():
        assert torch.equal(sd[k], v), k
    args = types.SimpleNamespace(opt="adamw", lr=1e-3, weight_decay=0.1, opt_eps=1e-8, opt_betas=None, output_dir=str(tmp_path),
                                 auto_resume=True, resume="", start_epoch=0)
    opt = create_optimizer(args, m)
    scaler = U.NativeScalerWithGradNormCount()
    U.save_model(args, 3, m, m, opt, scaler)
    U.save_model(args, 12, m, m, opt, scaler)
    _, m2 = tiny_model()
    opt2 = create_optimizer(args, m2)
    U.auto_load_model(args, m2, m2, opt2, scaler)
    assert args.resume.endswith("checkpoint-12.pth") and args.start_epoch == 13
    for (n, a), (_, b) in zip(m.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), n
    ck = torch.load(args.resume, map_location="cpu", weights_only=False)
    assert set(ck.keys()) == {"model", "optimizer", "epoch", "scaler", "args"} and ck["scaler"]["scale"] == 1.0


def test_to_device_keeps_views_bound():
    _, m = tiny_model()
    m2 = m.to(torch.device("cpu"))
    assert m2 is m
    p = dict(m.named_parameters())["pix_decoder.4.bias"]
    with torch.no_grad():
        m.flat_params.fill_(0.25)
    assert float(p[0]) == 0.25 and p.grad.data_ptr() == m.flat_grads.data_ptr() + 4 * m.specs["pix_decoder.4.bias"].offset


def test_no_cpu_fallback():
    cfg, m = tiny_model()
    im, au, mk = O.synthetic_batch(2, cfg, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(im, au, mk.bool(), 0.99, True)


def test_unsupported_variants_fail_loudly():
    """What is NOT built raises at construction (never a silent fallback): a patch extractor the reference does not know either
    (modeling_pretrain_moco_mim_ori.py:371-382 raises for anything but regular / no_patchtrans / conv), dropout rates no flag of the
    pre-training driver sets, an objective-less model."""
    with pytest.raises(NotImplementedError):
        MoCo_ViT(use_pixel_target=True, patchnet_name='deformable')
    with pytest.raises(NotImplementedError):
        MoCo_ViT(use_pixel_target=True, patchnet_name='no_patchtrans', drop_rate=0.1)
    with pytest.raises(ValueError):
        MoCo_ViT(use_pixel_target=False, use_moco_target=False, patchnet_name='no_patchtrans')
    with pytest.raises(RuntimeError):
        create_model("no_such_model")


def test_every_reference_factory_and_cli_default_constructs():
    """All nine factories of modeling_pretrain_moco_mim_ori.py (:627-871) with the reference driver's ARGPARSE defaults
    (run_mae_pretraining_moco.py:87,143-145: --num_windows 5, --patchnet_name regular, --drop_path 0), with the README flags and with the third
    value --patchnet_name takes (conv): parameter AND buffer names and order are the reference's (oracle.param_shapes / buffer_shapes, pinned by
    the fixtures written from the unmodified reference)."""
    import dataclasses
    for fam, kind in (("pretrain_simmim_moco_ori", "simmim_moco"), ("pretrain_moco_ori", "moco"), ("pretrain_simmim_ori", "simmim")):
        for size in ("tiny", "small", "base"):
            name = f"{fam}_vit_{size}_patch4_32x128"
            for nw, pn in ((5, "regular"), (4, "no_patchtrans"), (5, "conv")):
                m = create_model(name, **dict(KW, num_windows=nw, patchnet_name=pn))
                cfg = dataclasses.replace(O.make_config(name), num_windows=nw, patchnet=pn if kind != "simmim" else "no_patchtrans")
                assert [k for k, _ in m.named_parameters()] == list(O.param_shapes(cfg).keys()), (name, pn)
                assert {k: tuple(v.shape) for k, v in m.named_parameters()} == {k: tuple(v) for k, v in O.param_shapes(cfg).items()}, (name, pn)
                assert sorted(k for k, _ in m.named_buffers()) == sorted(O.buffer_shapes(cfg).keys()), (name, pn)
                assert m.use_moco_target == cfg.use_moco and m.use_pixel_target == cfg.use_pixel


def test_product_package_never_imports_the_oracle():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for dirpath, _, files in os.walk(os.path.join(root, "dig_amd")):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert "dig_oracle" not in src and "oracle" + "/" not in src, f


def test_optimizer_state_dict_interchanges_with_reference_layout(golden_dir, tmp_path):
    """N2: the fused optimizer's state_dict has the reference optimizer's structure (fixture produced by the
    reference's own custom_optim.AdamW after one step: parameter index order, group sizes / keys, per-index shapes)."""
    g = np.load(os.path.join(golden_dir, "optimizer_state_structure.npz"))
    cfg, m = tiny_model()
    args = types.SimpleNamespace(opt="adamw", lr=1e-3, weight_decay=0.1, opt_eps=1e-8, opt_betas=None)
    opt = create_optimizer(args, m)
    assert opt.state_dict()["state"] == {}                                   # like torch: empty before the first step
    opt._step = 1
    opt.exp_avg.normal_()
    opt.exp_avg_sq.uniform_()
    sd = opt.state_dict()
    idx_names = g["idx_names"].tolist()
    assert len(sd["state"]) == int(g["n_state"]) and [len(x["params"]) for x in sd["param_groups"]] == g["group_sizes"].tolist()
    assert [x["weight_decay"] for x in sd["param_groups"]] == g["group_wd"].tolist()
    assert set(g["group_keys"].tolist()) <= set(sd["param_groups"][0].keys())
    assert opt._named_specs() == idx_names                                    # same parameter <-> index mapping
    named = dict(m.named_parameters())
    for i, n in enumerate(idx_names):
        assert tuple(sd["state"][i]["exp_avg"].shape) == tuple(named[n].shape) and sd["state"][i]["step"] == 1
    # round trip through a torch.save'd checkpoint into a fresh optimizer
    torch.save({"optimizer": U._to_cpu(sd)}, tmp_path / "o.pth")
    _, m2 = tiny_model()
    opt2 = create_optimizer(args, m2)
    opt2.load_state_dict(torch.load(tmp_path / "o.pth", weights_only=False)["optimizer"])
    used = torch.zeros(m.n_online, dtype=torch.bool)
    for n in idx_names:
        sp = m.specs[n]
        used[sp.offset:sp.offset + sp.numel] = True
    assert opt2._step == 1 and torch.equal(opt2.exp_avg[used], opt.exp_avg[used]) and torch.equal(opt2.exp_avg_sq[used], opt.exp_avg_sq[used])
    # pads of the flat moment buffers are not part of any parameter: a load leaves them zero
    assert float(opt2.exp_avg[~used].abs().max()) == 0.0


def test_finetune_model_init_and_pretrained_encoder_handoff():
    """RecModelTrain initialises like the reference (xavier encoder, PyTorch-default decoder) and `load_pretrained` takes the encoder
    of a pre-training checkpoint the way run_class_finetuning.py:362-440 does: `encoder.*` loaded, momentum encoder / heads reported
    as unused, decoder / linear_norm reported as not initialised and left at their init."""
    import types
    from dig_amd.finetune import RecModelTrain
    from dig_amd.modeling_pretrain_moco_mim_ori import MoCo_ViT
    cfg = O.DiGConfig(**O.TINY)
    torch.manual_seed(3)
    pre = MoCo_ViT(encoder_embed_dim=cfg.embed_dim, encoder_depth=cfg.depth, encoder_num_heads=cfg.heads, decoder_embed_dim=cfg.dec_dim,
                   mlp_dim=cfg.moco_mlp_dim, dim=cfg.moco_dim, T=cfg.T, num_windows=4, use_pixel_target=True, patchnet_name='no_patchtrans')
    ck = {"model": pre.state_dict(), "epoch": 3}
    m = RecModelTrain(embed_dim=cfg.embed_dim, depth=cfg.depth, num_heads=cfg.heads, n_layers=2, d_model=128, n_head=2, d_k=64, d_inner=64,
                      nb_classes=97, max_len=8)
    sd0 = m.state_dict()
    D = cfg.embed_dim
    w = sd0["encoder.blocks.0.attn.qkv.weight"]
    assert abs(w.abs().max().item() - (6.0 / (D + 3 * D)) ** 0.5) < 2e-3 and sd0["encoder.blocks.0.mlp.fc1.bias"].abs().max() == 0
    assert torch.equal(sd0["decoder.layer_stack.1.norm3.weight"], torch.ones(128)) and abs(sd0["decoder.trg_word_emb.weight"].std().item() - 1) < 0.05
    assert abs(sd0["decoder.layer_stack.0.mlp.w_1.weight"].abs().max().item() - 128 ** -0.5) < 2e-3
    assert 0 < sd0["linear_norm.0.bias"].abs().max().item() <= D ** -0.5
    missing, unexpected = m.load_pretrained(ck)
    sd1 = m.state_dict()
    for k, v in ck["model"].items():
        if k.startswith("encoder.") and k in sd1:
            assert torch.equal(sd1[k], v.float()), k
    # (encoder.norm is Identity in the pre-training model, modeling_pretrain_moco_mim_ori.py:362-363: the fine-tune model's stays at init)
    assert all(k.startswith(("decoder.", "linear_norm.", "encoder.norm.")) for k in missing) and "decoder.classifier.weight" in missing
    assert "encoder.norm.weight" in missing
    assert any(k.startswith("momentum_encoder.") for k in unexpected) and not any(k.startswith("encoder.blocks") for k in unexpected)
    for k in missing:
        assert torch.equal(sd1[k], sd0[k]), k
    bad = dict(ck["model"])
    bad["encoder.norm.weight"] = torch.zeros(D + 1)
    with pytest.raises(RuntimeError):
        m.load_pretrained({"model": bad})
    with pytest.raises(ValueError):
        RecModelTrain(embed_dim=cfg.embed_dim, depth=cfg.depth, num_heads=cfg.heads, n_layers=2, d_model=128, n_head=2, d_k=64, d_inner=64,
                      drop_rate=1.0)


def test_pretrain_driver_parses_the_readme_command_and_shards_image_folders(tmp_path):
    """run_mae_pretraining_moco.py (repo root): the reference's README flag set (README.md:53-78) parses as is; the image-folder source
    shards a directory tree over ranks like DistributedSampler(shuffle=True, drop_last=True) -- disjoint per rank, reshuffled per epoch."""
    import importlib.util
    from PIL import Image
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("dig_driver", os.path.join(root, "run_mae_pretraining_moco.py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    readme = ("--image_alone_path DATA --mask_ratio 0.7 --batch_size 128 --opt adamw --output_dir OUT --epochs 10 --warmup_steps 5000 --max_len 25 "
              "--num_view 2 --moco_dim 256 --moco_mlp_dim 4096 --moco_m 0.99 --moco_m_cos --moco_t 0.2 --num_windows 4 --contrast_warmup_steps 0 "
              "--contrast_start_epoch 0 --loss_weight_pixel 1. --loss_weight_contrast 0.1 --only_mim_on_ori_img --weight_decay 0.1 "
              "--opt_betas 0.9 0.999 --model pretrain_simmim_moco_ori_vit_small_patch4_32x128 --patchnet_name no_patchtrans --encoder_type vit")
    a = drv.get_args(readme.split())
    assert a.batch_size == 128 and a.num_view == 2 and a.moco_t == 0.2 and a.only_mim_on_ori_img and a.opt_betas == [0.9, 0.999]
    assert a.use_moco_m_cos == 1 and a.normlize_target is False and a.image_alone_path == ["DATA"] and a.warmup_epochs == 40
    rng = np.random.RandomState(0)
    for i in range(23):
        d = tmp_path / f"d{i % 3}"
        d.mkdir(exist_ok=True)
        Image.fromarray(rng.randint(0, 255, size=(20 + i, 50 + 2 * i, 3), dtype=np.uint8)).save(d / f"im{i}.png")
    seen = []
    tf = lambda crops, aug: (len(crops), [c.shape for c in crops], None)
    for rank in range(2):
        ld = drv.ImageFolderCrops([str(tmp_path)], 4, rank, 2, tf, None, 2)
        assert len(ld) == 23 // 4 // 2
        ld.set_epoch(0)
        e0 = [b[0][1] for b in ld]
        ld.set_epoch(1)
        e1 = [b[0][1] for b in ld]
        assert all(len(b) == 4 for b in e0) and e0 != e1
        seen.append({sh for b in e0 for sh in b})
    assert not (seen[0] & seen[1])                                          # every crop has a distinct shape here: shards are disjoint
    # --num_samples / --aloneimage_num_samples: the first N samples, as the reference's datasets cap theirs
    assert len(drv.ImageFolderCrops([str(tmp_path)], 4, 0, 1, tf, None, 2, cap=9).files) == 9


def test_pretrain_driver_accepts_every_flag_of_the_reference(capsys):
    """Every flag name of the reference's get_args (run_mae_pretraining_moco.py:30-277; names only -- a list of interface facts) parses here: the
    ones its pre-training path never reads are accepted and reported, --use_ema (teacher-student mode) and an LMDB --data_path say what they
    are and stop."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("dig_driver2", os.path.join(root, "run_mae_pretraining_moco.py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    p = argparse_names(drv)
    for n in REFERENCE_FLAGS.split():
        assert n in p, n
    a = drv.get_args("--data_path synthetic --batch_size 8 --voc_type ALLCASES_SYMBOLS --pin_mem --use_abi_aug --mask_scales 1 --world_size 8 "
                     "--local_rank 0 --momentum 0.9 --train_url X --imagenet_default_mean_and_std".split())
    assert a.data_path == ["synthetic"] and a.batch_size == 8
    out = capsys.readouterr().out
    assert "--voc_type" in out and "--use_abi_aug" in out and "accepted, not used" in out
    with pytest.raises(SystemExit):
        drv.get_args(["--use_ema"])
    with pytest.raises(SystemExit):
        drv.get_args(["--no_such_flag", "1"])


def argparse_names(drv):
    import argparse
    names = set()
    orig = argparse.ArgumentParser.add_argument

    def rec(self, *a, **k):
        names.update(x for x in a if isinstance(x, str) and x.startswith("--"))
        return orig(self, *a, **k)
    argparse.ArgumentParser.add_argument = rec
    try:
        drv.get_args([])
    finally:
        argparse.ArgumentParser.add_argument = orig
    return names


REFERENCE_FLAGS = """--aloneimage_num_samples --alternately_epoch_training --alternately_training --attn_map_type --aug_ratio --auto_resume --batch_size
--clip_grad --cluster_update_interval --color_jitter --contrast_start_epoch --contrast_temperature --contrast_warmup_steps --corner_prob --corner_ratio
--corrupt_ops_ratios --ctx_max_len --ctx_min_len --ctx_nb_classes --ctx_num_samples --ctx_path --data_path --device --dist_on_itp --dist_url
--distill_start_epoch --drop_path --encoder_type --epochs --eval_freq --first_train_mim --fix_mask_token --image_alone_path --image_to_ctx_ratio
--imagenet_default_mean_and_std --input_h --input_size --input_w --local_rank --log_dir --loss_feat_beta --loss_feat_type --loss_weight_consist
--loss_weight_contrast --loss_weight_distill --loss_weight_feat_align --loss_weight_pixel --loss_weight_pos --loss_weight_semgroup --loss_win_size --lr
--mask_ratio --mask_ratios --mask_scales --max_len --min_lr --mix_train_with_aloneimage --mix_train_with_ctx --moco_dim --moco_m --moco_m_cos
--moco_mlp_dim --moco_t --model --momentum --momentum_teacher --momentum_teacher_end --no_auto_resume --no_pin_mem --normlize_target --num_distribution
--num_mem_slots --num_relation_heads --num_samples --num_target_layers --num_view --num_windows --num_workers --only_mim_on_ori_img
--only_real_data_for_pretrain --opt --opt_betas --opt_eps --output_dir --patchnet_name --pin_mem --queue_size --recon_patch_scales --relation_T
--relation_window_size --resume --save_ckpt_freq --seed --soft_label_type --start_epoch --text_loss_weight --text_mask_ratio --train_interpolation
--train_url --use_abi_aug --use_color_aug --use_corner_mask --use_ema --use_hard_sample --use_image_slice --use_loss_weight --use_mem_in_decoder --use_mim
--use_moco --use_moco_m_cos --use_multiscale_mask --use_patch_transformer --vis_loss_weight --voc_type --warmup_epochs --warmup_lr --warmup_steps
--weight_decay --weight_decay_end --world_size"""


def test_tensorboard_logger_surface(tmp_path):
    """utils.TensorboardLogger (reference utils/utils.py:285-306): update(head=..., **scalars) / set_step() / flush(), as train_one_epoch
    and the driver call them; without tensorboardX / tensorboard the scalars land in scalars.jsonl with the reference's tags and steps."""
    import json
    import torch
    from dig_amd import utils
    lw = utils.TensorboardLogger(log_dir=str(tmp_path))
    lw.set_step(40)
    lw.update(loss=1.5, head="loss")
    lw.update(lr=torch.tensor(2e-4), min_lr=None, head="opt")
    lw.set_step()
    lw.update(grad_norm=3, head="opt")
    lw.flush()
    assert lw.step == 41
    with pytest.raises(TypeError):
        lw.update(loss="x", head="loss")
    if isinstance(lw.writer, utils._JsonlScalarWriter):
        rows = [json.loads(l) for l in open(tmp_path / "scalars.jsonl")]
        assert [(r["tag"], r["step"]) for r in rows] == [("loss/loss", 40), ("opt/lr", 40), ("opt/grad_norm", 41)]
        assert rows[0]["value"] == 1.5 and abs(rows[1]["value"] - 2e-4) < 1e-9


def test_recognizer_state_dict_round_trip_on_cpu():
    """RecModel / RecModelTrain keep their weights in one fp32 arena: state_dict() -> load_state_dict() is bit-exact on the CPU and keeps the
    registration order; strict loading still refuses a missing key, an unexpected key and a wrong shape (and ignores the reference's buffer
    and `patch_embed.*` aliases)."""
    import decode_oracle as D
    from dig_amd.recognizer import RecModel
    from dig_amd.finetune import RecModelTrain
    c, ecfg = D.DecoderConfig(**D.TINY), O.DiGConfig(**O.TINY)
    P = {**D.det_encoder_state(ecfg, 3), **D.det_decoder_state(c, 4)}
    kw = dict(embed_dim=ecfg.embed_dim, depth=ecfg.depth, num_heads=ecfg.heads, n_layers=c.n_layers, d_model=c.d_model, n_head=c.n_head,
              d_k=c.d_k, d_inner=c.d_inner, nb_classes=c.num_classes, max_len=c.max_seq_len)
    for cls in (RecModel, RecModelTrain):
        m = cls(**kw)
        m.load_state_dict({**P, "decoder.position_enc.position_table": torch.zeros(1, 200, c.d_model),
                           "patch_embed.proj.bias": P["encoder.patch_embed.proj.bias"]})
        sd = m.state_dict()
        assert list(sd) == list(m.param_shapes()) and set(sd) == set(P)
        assert all(v.dtype == torch.float32 and v.device.type == "cpu" and torch.equal(v, P[k]) for k, v in sd.items())
        m2 = cls(**kw)
        m2.load_state_dict(sd)
        sd2 = m2.state_dict()
        assert list(sd2) == list(sd) and all(torch.equal(sd2[k], sd[k]) for k in sd)
        sd["encoder.norm.weight"].add_(1.0)                                    # clones: the model is not written through them
        assert torch.equal(m.state_dict()["encoder.norm.weight"], P["encoder.norm.weight"])
        first = next(iter(P))
        with pytest.raises(KeyError, match="missing"):
            m2.load_state_dict({k: v for k, v in P.items() if k != first})
        with pytest.raises(KeyError, match="unexpected"):
            m2.load_state_dict({**P, "decoder.no_such.weight": torch.zeros(1)})
        with pytest.raises(ValueError, match="shape"):
            m2.load_state_dict({**P, "decoder.classifier.bias": torch.zeros(c.num_classes + 1)})
        m2.load_state_dict({"encoder.norm.bias": torch.full_like(P["encoder.norm.bias"], 2.0)}, strict=False)
        assert float(m2.state_dict()["encoder.norm.bias"].min()) == 2.0
    with pytest.raises(RuntimeError, match="cuda"):
        RecModel(**kw).eval()(torch.zeros(1, 3, 32, 128))


def test_decoder_cross_attention_form_is_chosen_once_from_the_shape_facts():
    """RecModel picks its decoder cross-attention form (dig_amd/decoder_cross.py) from text_cond_vis, the number of memory tokens and the head
    dim; the text-conditional form adds its eight parameters per layer directly behind that layer's enc_attn.fc.weight and moves no other name."""
    import types
    from dig_amd import decoder_cross as DC
    from dig_amd.recognizer import RecModel

    def model(decoder_name, **flags):
        return RecModel(types.SimpleNamespace(model="simmim_vit_tiny_patch4_32x128", decoder_name=decoder_name, nb_classes=97, max_len=25, **flags))
    for decoder_name, flags, n_mem, d_k, form in (("tf_decoder", {}, 256, 64, DC.MfmaFewQuery),
                                                  ("tf_decoder", dict(use_1d_attdec=True), 32, 64, DC.SequenceKernel),
                                                  ("corres_tiny_tf_decoder", {}, 256, 24, DC.SequenceKernel),
                                                  ("corres_small_tf_decoder", {}, 256, 48, DC.SequenceKernel),
                                                  ("tf_decoder", dict(text_cond_vis=True), 256, 64, DC.TextConditional),
                                                  ("tf_decoder", dict(text_cond_vis=True, use_1d_attdec=True), 32, 64, DC.TextConditional)):
        m = model(decoder_name, **flags)
        assert (m.n_mem, m.dk) == (n_mem, d_k) and type(m.cross) is form, (decoder_name, flags, type(m.cross))
    plain, tcv = list(model("tf_decoder").param_shapes()), list(model("tf_decoder", text_cond_vis=True).param_shapes())
    extra = ("gamma_decode.weight", "gamma_decode.bias", "vis_proj.weight", "vis_proj.bias", "vis_norm.weight", "vis_norm.bias",
             "vis_cond_norm.weight", "vis_cond_norm.bias")
    want = []
    for n in plain:
        want.append(n)
        if n.endswith("enc_attn.fc.weight"):
            want += [n[:-len("fc.weight")] + e for e in extra]
    assert tcv == want and len(tcv) == len(plain) + 8 * 6


@pytest.mark.parametrize("D", [192, 64])
def test_place_bundles_q_and_v_bias(D):
    """arena.place at the smallest shapes where the q_bias | zeros | v_bias bundle can go wrong: D = 192 (576 elements padded to 768, v_bias at
    +384 inside a granule, not on a boundary) and D = 64 (the whole bundle inside one granule)."""
    def shapes():
        return arena.encoder_shapes("encoder.", D, 4 * D, 1, True)

    def check(slots, end, start, groups):
        q, v = slots["encoder.blocks.0.attn.q_bias"], slots["encoder.blocks.0.attn.v_bias"]
        assert list(slots) == list(shapes())                                   # registration order kept
        assert q.offset % ALIGN == 0 and v.offset == q.offset + 2 * D
        spans = sorted((s.offset, s.offset + s.numel) for s in slots.values())
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))            # no two slots overlap
        assert all(hi <= q.offset + D or lo >= q.offset + 2 * D for lo, hi in spans)      # the gap belongs to no slot
        assert all(s.offset % ALIGN == 0 for n, s in slots.items() if not n.endswith("attn.v_bias"))
        assert spans[0][0] == start and end % ALIGN == 0 and end >= spans[-1][1]
        assert len(groups) == (end - start) // ALIGN                           # one entry per granule
        assert all(s.numel == int(np.prod(s.shape)) and s.shape == tuple(shapes()[n]) for n, s in slots.items())
    a, ga = shapes(), []
    end_a = arena.place(a, groups=ga)
    check(a, end_a, 0, ga)
    b, gb = shapes(), []
    start = 5 * ALIGN
    end_b = arena.place(b, start, gb)
    check(b, end_b, start, gb)
    assert end_b == end_a + start and ga == gb
    assert all(b[n].offset == a[n].offset + start and b[n][1:] == a[n][1:] for n in a)     # every offset shifts by exactly `start`
    # the group of a slot fills its granules: a bundle's are its q_bias's
    g, gs = {n: arena.Slot(None, int(np.prod(s)), tuple(s), 0 if len(s) >= 2 else 1, "x") for n, s in shapes().items()}, []
    arena.place(g, groups=gs)
    for n, s in g.items():
        if not n.endswith("attn.v_bias"):
            assert gs[s.offset // ALIGN] == s.group and s.arena == "x", n
    assert [s.offset for s in g.values()] == [s.offset for s in a.values()]
    # without its sibling a q_bias is an ordinary tensor
    alone = {"blocks.0.attn.q_bias": (D,), "w": (D, D)}
    arena.place(alone)
    assert alone["w"].offset == ALIGN * ((D + ALIGN - 1) // ALIGN)


def test_fused_needs_adjacent_weights():
    slots = {"a.linear_q.weight": (16, 16), "a.linear_k.weight": (16, 16), "a.linear_v.weight": (16, 16), "a.bias": (16,), "b.weight": (16, 16),
             "c.weight": (8, 8), "d.weight": (8, 8)}
    n = arena.place(slots)
    flat = torch.arange(n, dtype=torch.float32)
    kv = arena.fused(flat, slots, "a.linear_k.weight", 2)
    assert kv.shape == (32, 16) and kv.data_ptr() == arena.view(flat, slots["a.linear_k.weight"]).data_ptr()
    assert torch.equal(kv[16:], arena.view(flat, slots["a.linear_v.weight"]))
    kv[16, 0] = -1.0                                                           # shares storage with the arena
    assert float(flat[slots["a.linear_v.weight"].offset]) == -1.0
    assert arena.fused(flat, slots, "a.linear_q.weight", 3).shape == (48, 16)
    for first, count in (("a.linear_v.weight", 2),        # another shape follows
                         ("a.bias", 2),
                         ("c.weight", 2),                  # same shape, but 64 elements are padded to a granule: not back to back
                         ("d.weight", 2)):                 # nothing follows
        with pytest.raises(AssertionError):
            arena.fused(flat, slots, first, count)


def test_encoder_names_agree_between_pretraining_and_recognition():
    """What lets a pre-training checkpoint load into the recognizer: a Gen-only MoCo_ViT (it keeps encoder.norm) and a RecModel of the same
    width and depth have the same encoder.* names, shapes and relative offsets."""
    from dig_amd.recognizer import RecModel
    m = MoCo_ViT(encoder_embed_dim=192, encoder_depth=2, encoder_num_heads=3, use_pixel_target=True, use_moco_target=False)
    r = RecModel(embed_dim=192, depth=2, num_heads=3, n_layers=1, d_model=64, n_head=1, d_inner=64)
    enc_m = [(n, s.shape, s.offset - m.specs["encoder.mask_token"].offset) for n, s in m.specs.items() if n.startswith("encoder.")]
    enc_r = [(n, s.shape, s.offset - r._offsets["encoder.mask_token"].offset) for n, s in r._offsets.items() if n.startswith("encoder.")]
    assert enc_m == enc_r and len(enc_m) == 3 + 13 * 2 + 2
    assert torch.equal(m.encoder.pos_embed[0], arena.encoder_pos_table(256, 192))


def test_enc_block_views_point_at_their_slots():
    D, depth = 64, 2
    slots = arena.encoder_shapes("encoder.", D, 4 * D, depth, False)
    n = arena.place(slots)
    f32, grads, w16 = torch.zeros(n), torch.zeros(n), torch.zeros(n, dtype=torch.bfloat16)
    plain = arena.enc_block_views(slots, "encoder.", depth, D, f32, w16)
    train = arena.enc_block_views(slots, "encoder.", depth, D, f32, w16, grads)
    assert len(plain) == len(train) == depth
    for i in range(depth):
        b = f"encoder.blocks.{i}."
        assert "g" not in plain[i] and set(plain[i]) == set(arena.ENC_F32 + arena.ENC_W16 + ("qkv_bias",)) == set(train[i]) - {"g"}
        assert set(train[i]["g"]) == set(arena.ENC_GRAD + ("qkv_bias",))
        for blk in (plain[i], train[i]):
            for k in arena.ENC_F32:
                assert blk[k].data_ptr() == arena.view(f32, slots[b + k]).data_ptr() and blk[k].shape == slots[b + k].shape
            for k in arena.ENC_W16:
                assert blk[k].data_ptr() == arena.view(w16, slots[b + k]).data_ptr() and blk[k].dtype == torch.bfloat16
            assert blk["qkv_bias"].data_ptr() == arena.qkv_bias(f32, slots, b, D).data_ptr() and blk["qkv_bias"].shape == (3 * D,)
        for k in arena.ENC_GRAD:
            assert train[i]["g"][k].data_ptr() == arena.view(grads, slots[b + k]).data_ptr() and train[i]["g"][k].shape == slots[b + k].shape
        assert train[i]["g"]["qkv_bias"].data_ptr() == arena.qkv_bias(grads, slots, b, D).data_ptr()
        assert arena.qkv_bias(f32, slots, b, D).data_ptr() == f32.data_ptr() + 4 * slots[b + "attn.q_bias"].offset


def test_split_and_join_round_trip_moment_arenas():
    slots = {"a.weight": (4, 8), "a.bias": (8,), "b.weight": (3, 3)}
    n = arena.place(slots)
    flats = {"exp_avg": torch.arange(n, dtype=torch.float32), "exp_avg_sq": -torch.arange(n, dtype=torch.float32)}
    names = ["b.weight", "a.weight", "a.bias"]                                  # the optimizer's order, not the arena's
    state = arena.split(flats, slots, names, skip={"a.bias"})
    assert sorted(state) == [0, 1] and state[0]["exp_avg"].shape == (3, 3)
    assert state[1]["exp_avg_sq"].data_ptr() == arena.view(flats["exp_avg_sq"], slots["a.weight"]).data_ptr()
    saved = {i: {k: v.clone() for k, v in st.items()} for i, st in state.items()}
    arena.join(flats, slots, names, {str(i): st for i, st in saved.items()})    # (keys may come back as strings)
    assert all(torch.equal(arena.view(flats[k], slots[names[i]]), saved[i][k]) for i in saved for k in flats)
    assert float(arena.view(flats["exp_avg"], slots["a.bias"]).abs().sum()) == 0.0       # what is not listed is zero
    with pytest.raises(ValueError, match="shape"):
        arena.join(flats, slots, names, {0: {"exp_avg": torch.zeros(9), "exp_avg_sq": torch.zeros(3, 3)}})
