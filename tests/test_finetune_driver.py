"""run_class_finetuning.py (the fine-tune / evaluation driver) and dig_amd/rec_datasets.py (labelled data sources, the device-side batch
loader).  Host tests: flags, datasets, schedules.  GPU tests: the driver against the same pieces driven by hand, resume, --eval, and one short
run per other head / view.  Nothing here asserts an accuracy: the checks are equalities between two ways of driving the same kernels."""
import importlib.util
import json
import math
import os
import random
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _driver():
    spec = importlib.util.spec_from_file_location("dig_finetune_driver", os.path.join(ROOT, "run_class_finetuning.py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    return drv


# every flag name of the reference's get_args (run_class_finetuning.py:43-255; names only -- a list of interface facts)
REFERENCE_FLAGS = """--batch_size --epochs --update_freq --save_ckpt_freq --eval_freq --model --decoder_name --decoder_type --insert_sem --text_cond_vis
--input_size --input_h --input_w --drop --attn_drop_rate --drop_path --use_seq_cls_token --disable_eval_during_finetuning --model_ema --model_ema_decay
--model_ema_force_cpu --num_mem_slots --use_mem_in_decoder --use_1d_attdec --opt --opt_eps --opt_betas --clip_grad --momentum --weight_decay
--weight_decay_end --lr --layer_decay --warmup_lr --min_lr --warmup_epochs --warmup_steps --use_contrastive_center_loss --use_multi_label_loss
--color_jitter --aa --smoothing --train_interpolation --crop_pct --beam_width --reprob --remode --recount --resplit --mixup --cutmix --cutmix_minmax
--mixup_prob --mixup_switch_prob --mixup_mode --finetune --model_key --model_prefix --init_scale --use_mean_pooling --use_cls --fixed_encoder_layers
--data_path --eval_data_path --other_test_data_folders --nb_classes --imagenet_default_mean_and_std --data_set --output_dir --train_url --log_dir
--device --seed --resume --auto_resume --no_auto_resume --save_ckpt --no_save_ckpt --start_epoch --eval --dist_eval --num_workers --pin_mem
--no_pin_mem --voc_type --max_len --num_samples --w2v_path --num_parts --num_view --use_abi_aug --world_size --local_rank --dist_on_itp --dist_url
--enable_deepspeed"""
# ... and the defaults it gives them (the same kind of fact)
REFERENCE_DEFAULTS = dict(batch_size=64, epochs=30, update_freq=1, save_ckpt_freq=1, eval_freq=1000, decoder_name="tf_decoder", decoder_type="tf_decoder",
                          insert_sem=False, text_cond_vis=False, input_size=224, input_h=32, input_w=128, drop=0.0, attn_drop_rate=0.0, drop_path=0.1,
                          use_seq_cls_token=False, disable_eval_during_finetuning=False, model_ema=False, model_ema_decay=0.9999,
                          model_ema_force_cpu=False, num_mem_slots=0, use_mem_in_decoder=False, use_1d_attdec=False, opt="adamw", opt_eps=1e-8,
                          opt_betas=None, clip_grad=None, momentum=0.9, weight_decay=0.05, weight_decay_end=None, lr=1e-3, layer_decay=0.75,
                          warmup_lr=1e-6, min_lr=1e-6, warmup_epochs=5, warmup_steps=-1, use_contrastive_center_loss=False,
                          use_multi_label_loss=False, color_jitter=0.4, aa="rand-m9-mstd0.5-inc1", smoothing=0.1, train_interpolation="bicubic",
                          crop_pct=None, beam_width=0, reprob=0.25, remode="pixel", recount=1, resplit=False, mixup=0.8, cutmix=1.0,
                          cutmix_minmax=None, mixup_prob=1.0, mixup_switch_prob=0.5, mixup_mode="batch", finetune="", model_key="model|module",
                          model_prefix="", init_scale=0.001, use_mean_pooling=False, fixed_encoder_layers=0, eval_data_path=None, nb_classes=1000,
                          imagenet_default_mean_and_std=True, data_set="IMNET", output_dir="", train_url="/home/ma-user/modelarts/outputs/train_url_0/",
                          log_dir=None, device="cuda", seed=0, resume="", auto_resume=True, save_ckpt=True, start_epoch=0, eval=False, dist_eval=False,
                          num_workers=5, pin_mem=True, voc_type="ALLCASES_SYMBOLS", max_len=100, num_samples=math.inf, w2v_path=None, num_parts=1,
                          num_view=1, use_abi_aug=False, world_size=1, local_rank=-1, dist_on_itp=False, dist_url="env://", enable_deepspeed=False)
MODEL = "--model simmim_vit_small_patch4_32x128"
SYN = MODEL + " --data_path synthetic --synthetic 32"


def argparse_names(drv, argv):
    import argparse
    names = set()
    orig = argparse.ArgumentParser.add_argument

    def rec(self, *a, **k):
        names.update(x for x in a if isinstance(x, str) and x.startswith("--"))
        return orig(self, *a, **k)
    argparse.ArgumentParser.add_argument = rec
    try:
        drv.get_args(argv)
    finally:
        argparse.ArgumentParser.add_argument = orig
    return names


# ---------------------------------------------------------------------------------------------- flags
def test_driver_accepts_every_flag_of_the_reference(capsys):
    drv = _driver()
    names = argparse_names(drv, SYN.split())
    for n in REFERENCE_FLAGS.split():
        assert n in names, n
    for own in ("--synthetic", "--eval_edit_distance"):
        assert own in names
    a = drv.get_args(SYN.split())
    for k, v in REFERENCE_DEFAULTS.items():
        assert getattr(a, k) == v, k
    assert a.other_test_data_folders is None and a.data_path == ["synthetic"] and a.synthetic == 32 and a.eval_edit_distance is False
    assert "accepted, not used" not in capsys.readouterr().out
    a = drv.get_args((SYN + " --mixup 0.5 --cutmix_minmax 0.2 0.8 --aa v0 --reprob 0.1 --resplit --use_cls --num_mem_slots 4 --momentum 0.8 "
                      "--train_url X --imagenet_default_mean_and_std --model_ema_force_cpu --no_pin_mem --local_rank 3").split())
    out = capsys.readouterr().out
    assert "accepted, not used" in out
    for n in ("--mixup", "--cutmix_minmax", "--aa", "--reprob", "--resplit", "--use_cls", "--num_mem_slots", "--momentum", "--train_url",
              "--imagenet_default_mean_and_std", "--model_ema_force_cpu", "--no_pin_mem", "--local_rank"):
        assert n in out, n
    assert "--cutmix " not in out and a.mixup == 0.5 and a.pin_mem is False and a.use_mean_pooling is False
    # the README's two command lines, as written
    ft = drv.get_args((MODEL + " --data_path DATA --eval_data_path DATA --finetune M.pth --output_dir OUT --batch_size 256 --opt adamw --opt_betas 0.9 0.999 "
                       "--weight_decay 0.05 --data_set image_lmdb --nb_classes 97 --smoothing 0. --max_len 25 --epochs 10 --warmup_epochs 1 --drop 0.1 "
                       "--attn_drop_rate 0.1 --drop_path 0.1 --dist_eval --lr 1e-4 --num_samples 1 --fixed_encoder_layers 0 --decoder_name tf_decoder "
                       "--use_abi_aug --num_view 2").split())
    assert ft.data_path == ["DATA"] and ft.num_view == 2 and ft.use_abi_aug and ft.opt_betas == [0.9, 0.999] and ft.num_samples == 1.0
    ev = drv.get_args((MODEL + " --data_path DATA --eval_data_path DATA --output_dir OUT --batch_size 512 --opt adamw --opt_betas 0.9 0.999 --weight_decay 0.05 "
                       "--data_set image_lmdb --nb_classes 97 --smoothing 0. --max_len 25 --resume M.pth --eval --epochs 20 --warmup_epochs 2 --drop 0.1 "
                       "--attn_drop_rate 0.1 --dist_eval --num_samples 1000000 --fixed_encoder_layers 0 --decoder_name tf_decoder --beam_width 0").split())
    assert ev.eval and ev.resume == "M.pth" and ev.beam_width == 0


@pytest.mark.parametrize("flags, says", [("--enable_deepspeed", "deepspeed"), ("--use_seq_cls_token 1", "--use_seq_cls_token"),
                                         ("--insert_sem", "--insert_sem"), ("--w2v_path 1", "--w2v_path"),
                                         ("--use_contrastive_center_loss", "never imports"),
                                         ("--decoder_name decoupled_tf_decoder", "decoupled"), ("--input_h 64", "32 x 128"),
                                         ("--input_w 256", "32 x 128"), ("--finetune https://host/m.pth", "download")])
def test_driver_stops_at_what_is_not_built(flags, says):
    drv = _driver()
    with pytest.raises(SystemExit) as e:
        drv.get_args((SYN + " " + flags).split())
    assert says in str(e.value)


@pytest.mark.parametrize("data_set", ["CIFAR", "IMNET", "image_folder"])
def test_driver_stops_at_the_classification_datasets(data_set):
    drv = _driver()
    with pytest.raises(SystemExit) as e:
        drv.get_args((MODEL + " --data_path DATA --data_set " + data_set).split())
    assert data_set in str(e.value)
    with pytest.raises(SystemExit) as e:
        drv.get_args(["--data_path", "synthetic"])                    # the reference's default --model is not a recognition encoder
    assert "deit_base_patch16_224" in str(e.value)


def test_driver_refuses_an_unknown_flag():
    drv = _driver()
    with pytest.raises(SystemExit):
        drv.get_args((SYN + " --no_such_flag 1").split())


def test_lr_scaling_schedules_and_checkpoint_frequency():
    drv = _driver()
    a = drv.get_args((SYN + " --batch_size 8 --update_freq 2 --epochs 3 --warmup_epochs 1 --lr 1e-3 --min_lr 1e-5 --weight_decay 0.05 "
                      "--weight_decay_end 0.1 --save_ckpt_freq 3").split())
    plan = drv.plan_schedule(a, n_train=100, world=2)
    assert plan["total_batch_size"] == 32 and plan["steps_per_epoch"] == 3 and plan["lr"] == 1e-3 * 32 / 256
    lr, wd = plan["lr_schedule_values"], plan["wd_schedule_values"]
    assert len(lr) == 9 and len(wd) == 9
    assert lr[0] == 0.0 and lr[2] == plan["lr"] and lr[3] == plan["lr"] and lr[-1] > 1e-5 and all(x >= y for x, y in zip(lr[3:], lr[4:]))
    assert wd[0] == 0.05 and all(x <= y for x, y in zip(wd, wd[1:])) and wd[-1] < 0.1
    assert drv.plan_schedule(drv.get_args(SYN.split()), 640, 1)["weight_decay_end"] == 0.05       # unset: constant weight decay
    assert drv.save_ckpt_freq(a) == 3
    a.epochs = 101
    assert drv.save_ckpt_freq(a) == 20                                # above 100 epochs (:600-601)
    a.epochs = 100
    assert drv.save_ckpt_freq(a) == 3


# ---------------------------------------------------------------------------------------------- datasets
def _png(path, rng, h=40, w=100):
    from PIL import Image
    Image.fromarray(rng.randint(0, 255, size=(h, w, 3), dtype=np.uint8)).save(path)


def _three_samples(tmp_path, max_len):
    """[a word too long for max_len, a good sample, a truncated file]."""
    rng = np.random.RandomState(3)
    names = ["long.png", "good.png", "cut.png"]
    for i, n in enumerate(names):
        _png(str(tmp_path / n), rng, 30 + i, 90 + i)
    raw = (tmp_path / "cut.png").read_bytes()
    (tmp_path / "cut.png").write_bytes(raw[:len(raw) // 2])
    words = ["x" * (max_len - 1), "Good", "cut"]
    return names, words


def test_image_list_substitutes_the_next_sample(tmp_path):
    from dig_amd.rec_datasets import ImageList
    names, words = _three_samples(tmp_path, 25)
    (tmp_path / "gt.txt").write_text("".join(f"{n}\t{w}\n" for n, w in zip(names, words)), encoding="utf-8")
    ds = ImageList(str(tmp_path), "ALLCASES_SYMBOLS", 25)
    assert len(ds) == 3 and ds.classes[94] == "EOS" and ds.class_to_idx["PADDING"] == 95 and ds.idx_to_class[96] == "UNKNOWN"
    crop, word = ds[1]
    assert word == "Good" and crop.dtype == np.uint8 and crop.shape == (31, 91, 3)
    for i in (0, 2):                                                  # too long -> the next sample; truncated -> the next one (wrapping)
        c, w = ds[i]
        assert w == "Good" and np.array_equal(c, crop)
    assert ImageList(str(tmp_path), "LOWERCASE", 25)[1][1] == "good"
    assert len(ImageList(str(tmp_path), "ALLCASES", 25, num_samples=2)) == 2
    with pytest.raises(FileNotFoundError):
        ImageList(str(tmp_path / "nowhere"), "ALLCASES", 25)


def _lmdb_stub(dbs):
    class Txn:
        def __init__(self, d):
            self.d = d

        def get(self, key):
            return self.d.get(key)

    class Env:
        def __init__(self, d):
            self.d = d

        def begin(self, **kw):
            return Txn(self.d)
    mod = types.ModuleType("lmdb")
    mod.open = lambda root, **kw: Env(dbs[root])
    return mod


def test_image_lmdb_through_a_stub_module(tmp_path, monkeypatch):
    from dig_amd import rec_datasets as RD
    names, words = _three_samples(tmp_path, 25)
    db = {b"num-samples": b"3"}
    for i, (n, w) in enumerate(zip(names, words)):
        db[b"image-%09d" % (i + 1)] = (tmp_path / n).read_bytes()
        db[b"label-%09d" % (i + 1)] = w.encode()
    db2 = {b"num-samples": b"1", b"image-000000001": db[b"image-000000002"], b"label-000000001": b"two"}
    monkeypatch.setitem(sys.modules, "lmdb", _lmdb_stub({"ROOT": db, "ROOT2": db2}))
    ds = RD.ImageLmdb("ROOT", "ALLCASES_SYMBOLS", 25)
    assert len(ds) == 3
    crop, word = ds[1]
    assert word == "Good" and crop.shape == (31, 91, 3)
    for i in (0, 2):
        c, w = ds[i]
        assert w == "Good" and np.array_equal(c, crop)
    assert len(RD.ImageLmdb("ROOT", "ALLCASES_SYMBOLS", 25, num_samples=0.5)) == 1          # a value <= 1 is a fraction (:27-28)
    assert len(RD.ImageLmdb("ROOT", "ALLCASES_SYMBOLS", 25, num_samples=2)) == 2
    # several roots -> ConcatDataset, as build_dataset does
    args = types.SimpleNamespace(data_path=["ROOT", "ROOT2"], eval_data_path="ROOT2", data_set="image_lmdb", voc_type="ALLCASES_SYMBOLS", max_len=25,
                                 num_samples=math.inf, nb_classes=97, seed=0, synthetic=0)
    both, nb = RD.build_dataset(True, args)
    assert nb == 97 and len(both) == 4 and both[3][1] == "two" and both.class_to_idx["EOS"] == 94
    assert len(RD.build_dataset(False, args)[0]) == 1
    args.nb_classes = 1000
    with pytest.raises(SystemExit):
        RD.build_dataset(True, args)


def test_image_lmdb_without_the_module_says_what_to_do(monkeypatch):
    from dig_amd import rec_datasets as RD
    monkeypatch.setitem(sys.modules, "lmdb", None)
    with pytest.raises(ImportError) as e:
        RD.ImageLmdb("ROOT", "ALLCASES_SYMBOLS", 25)
    assert "lmdb" in str(e.value) and "image_list" in str(e.value) and "synthetic" in str(e.value)


@pytest.mark.parametrize("voc_type, max_len", [("ALLCASES_SYMBOLS", 25), ("LOWERCASE", 8)])
def test_synthetic_words_are_deterministic_and_bounded(voc_type, max_len):
    from dig_amd.rec_datasets import SyntheticWords
    a, b = SyntheticWords(24, voc_type, max_len, seed=5), SyntheticWords(40, voc_type, max_len, seed=5)
    other = SyntheticWords(24, voc_type, max_len, seed=6)
    assert len(a) == 24 and len(SyntheticWords(24, voc_type, max_len, seed=5, num_samples=0.5)) == 12
    lengths = set()
    for i in range(24):
        (ca, wa), (cb, wb) = a[i], b[i]
        assert wa == wb and np.array_equal(ca, cb)                    # index -> sample depends on (seed, index) alone
        assert 1 <= len(wa) <= max_len - 2 and all(c in a.class_to_idx for c in wa)
        assert ca.dtype == np.uint8 and ca.ndim == 3 and ca.shape[2] == 3 and 24 <= ca.shape[0] <= 64 and 60 <= ca.shape[1] <= 320
        assert ca.std() > 0                                           # something was drawn
        lengths.add(len(wa))
    assert len(lengths) > 1 and [w for _, w in (a[i] for i in range(24))] != [w for _, w in (other[i] for i in range(24))]
    if voc_type == "LOWERCASE":
        assert all(w == w.lower() for _, w in a.samples)


def test_loaders_follow_the_reference_samplers():
    from dig_amd.rec_datasets import SyntheticWords, make_loader
    ds = SyntheticWords(21, "ALLCASES_SYMBOLS", 25, seed=1)
    args = types.SimpleNamespace(batch_size=4, num_workers=0, dist_eval=False)
    train = make_loader(ds, args, True)
    assert isinstance(train.sampler, torch.utils.data.DistributedSampler) and train.sampler.shuffle and len(train) == 5     # drop_last
    train.sampler.set_epoch(0)
    e0 = [w for _, ws in train for w in ws]
    train.sampler.set_epoch(1)
    e1 = [w for _, ws in train for w in ws]
    assert len(e0) == 20 and e0 != e1
    shards = [make_loader(ds, args, True, rank=r, world=2) for r in range(2)]
    assert all(len(s) == 2 for s in shards)
    val = make_loader(ds, args, False)
    assert isinstance(val.sampler, torch.utils.data.SequentialSampler) and val.batch_size == 6 and len(val) == 4            # int(1.5 * 4), last batch kept
    batches = list(val)
    assert [len(ws) for _, ws in batches] == [6, 6, 6, 3] and [w for _, ws in batches for w in ws] == [ds[i][1] for i in range(21)]
    assert isinstance(batches[0][0], list) and batches[0][0][0].dtype == np.uint8
    args.dist_eval = True
    assert isinstance(make_loader(ds, args, False, rank=1, world=2).sampler, torch.utils.data.DistributedSampler)


def test_device_batches_yield_the_engine_triple(abi_dev):
    from dig_amd.datasets import LabelEncoder
    from dig_amd.rec_datasets import SyntheticWords, device_loader
    ds = SyntheticWords(7, "ALLCASES_SYMBOLS", 25, seed=2)
    args = types.SimpleNamespace(batch_size=2, num_workers=0, dist_eval=False, input_h=32, input_w=128, num_view=1, use_abi_aug=False,
                                 voc_type="ALLCASES_SYMBOLS", max_len=25)
    loader = device_loader(ds, args, False, abi_dev)
    assert loader.dataset is ds and isinstance(loader.sampler, torch.utils.data.SequentialSampler) and len(loader) == 3
    seen = 0
    enc = LabelEncoder("ALLCASES_SYMBOLS", 25, abi_dev)
    for images, targets, lens in loader:
        n = images.shape[0]
        assert tuple(images.shape) == (n, 3, 32, 128) and images.dtype == torch.float32 and images.device.type == abi_dev.type
        want, want_lens = enc([ds[seen + i][1] for i in range(n)])
        assert torch.equal(targets, want) and torch.equal(lens, want_lens) and float(images.abs().max()) <= 1.0
        seen += n
    assert seen == 7


# ---------------------------------------------------------------------------------------------- GPU: the driver end to end
COMMON = (SYN + " --eval_data_path synthetic --data_set image_lmdb --nb_classes 97 --batch_size 8 --decoder_name small_tf_decoder --max_len 25 "
          "--epochs 2 --warmup_epochs 0 --drop 0.1 --attn_drop_rate 0.1 --drop_path 0.1 --num_workers 0 --smoothing 0. --eval_edit_distance")


def _load(path):
    return torch.load(path, map_location="cpu", weights_only=False)


@pytest.fixture(scope="module")
def straight_run(tmp_path_factory):
    """Two epochs straight through into directory A (shared, read-only, by the tests below)."""
    drv = _driver()
    out = str(tmp_path_factory.mktemp("straight"))
    res = drv.main(drv.get_args((COMMON + " --save_ckpt --output_dir " + out).split()))
    return out, res


@pytest.mark.gpu
def test_driver_equals_the_api(straight_run):
    """main(args) against a loop written here from the package's own pieces with the same seeds: every tensor of the final state_dict agrees."""
    import dig_amd.utils as U
    from dig_amd.engine_for_finetuning import train_one_epoch
    from dig_amd.finetune import LayerDecayValueAssigner, RecModelTrain, SeqCrossEntropyLoss, create_optimizer
    from dig_amd.rec_datasets import build_dataset, device_loader
    out, res = straight_run
    assert math.isfinite(res["train_stats"]["loss"]) and set(res) >= {"train_stats", "test_stats", "max_accuracy"}
    drv = _driver()
    args = drv.get_args(COMMON.split())
    dev = torch.device("cuda", 0)
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    random.seed(args.seed)
    train, _ = build_dataset(True, args)
    loader = device_loader(train, args, True, dev, seed=args.seed)
    model = RecModelTrain(args)
    args.window_size, args.patch_size = (8, 32), (4, 4)
    model.to(dev)
    steps = len(train) // args.batch_size
    assert steps == 4 == len(loader)
    args.lr = args.lr * args.batch_size / 256
    nl = model.get_num_layers()
    asg = LayerDecayValueAssigner([args.layer_decay ** (nl + 1 - i) for i in range(nl + 2)])
    opt = create_optimizer(args, model, skip_list=model.no_weight_decay(), get_num_layer=asg.get_layer_id, get_layer_scale=asg.get_scale)
    scaler, crit = U.NativeScalerWithGradNormCount(), SeqCrossEntropyLoss()
    lrs = U.cosine_scheduler(args.lr, args.min_lr, args.epochs, steps, warmup_epochs=0, warmup_steps=-1)
    wds = U.cosine_scheduler(args.weight_decay, args.weight_decay, args.epochs, steps)
    for epoch in range(args.epochs):
        stats = train_one_epoch(model, crit, loader, opt, dev, epoch, scaler, None, None, None, start_steps=epoch * steps, lr_schedule_values=lrs,
                                wd_schedule_values=wds, num_training_steps_per_epoch=steps, update_freq=1, args=args)
    want = model.state_dict()
    got = _load(os.path.join(out, "checkpoint-1.pth"))["model"]
    assert set(got) == set(want)
    assert all(torch.equal(got[k], want[k]) for k in want), [k for k in want if not torch.equal(got[k], want[k])][:5]
    assert stats["loss"] == res["train_stats"]["loss"]


@pytest.mark.gpu
def test_resume_continues_bit_for_bit(straight_run, tmp_path, monkeypatch):
    """One epoch into directory B, the run interrupted at the start of the second (as a killed job is), a second invocation that
    auto-resumes: checkpoint-1.pth of B equals the straight run's in model, optimizer moments, step count and dropout key counter."""
    import dig_amd.engine_for_finetuning as E
    out_a, _ = straight_run
    drv = _driver()
    argv = (COMMON + " --save_ckpt --auto_resume --output_dir " + str(tmp_path)).split()
    real = E.train_one_epoch

    class Interrupted(Exception):
        pass

    def one_epoch_only(model, criterion, data_loader, optimizer, device, epoch, *a, **k):
        if epoch == 1:
            raise Interrupted
        return real(model, criterion, data_loader, optimizer, device, epoch, *a, **k)
    monkeypatch.setattr(E, "train_one_epoch", one_epoch_only)
    with pytest.raises(Interrupted):
        drv.main(drv.get_args(argv))
    monkeypatch.setattr(E, "train_one_epoch", real)
    assert os.path.exists(tmp_path / "checkpoint-0.pth") and not os.path.exists(tmp_path / "checkpoint-1.pth")
    args = drv.get_args(argv)
    drv.main(args)
    assert args.start_epoch == 1
    a, b = _load(os.path.join(out_a, "checkpoint-1.pth")), _load(str(tmp_path / "checkpoint-1.pth"))
    assert all(torch.equal(a["model"][k], b["model"][k]) for k in a["model"]), [k for k in a["model"] if not torch.equal(a["model"][k], b["model"][k])][:5]
    sa, sb = a["optimizer"]["state"], b["optimizer"]["state"]
    assert sa.keys() == sb.keys() and len(sa) > 0
    for i in sa:
        assert torch.equal(sa[i]["exp_avg"], sb[i]["exp_avg"]) and torch.equal(sa[i]["exp_avg_sq"], sb[i]["exp_avg_sq"])
        assert int(sa[i]["step"]) == int(sb[i]["step"]) == 8
    assert a["dig_amd"] == b["dig_amd"] and a["dig_amd"]["drop_step"] == 8
    lines = [json.loads(l) for l in (tmp_path / "log.txt").read_text().splitlines()]
    assert [l["epoch"] for l in lines] == [0, 1]
    last_a = [json.loads(l) for l in open(os.path.join(out_a, "log.txt"))][-1]
    assert {k: v for k, v in lines[-1].items() if k.startswith("test_")} == {k: v for k, v in last_a.items() if k.startswith("test_")}


@pytest.mark.gpu
def test_eval_reproduces_the_logged_metrics(straight_run, tmp_path):
    from PIL import Image
    from dig_amd.rec_datasets import SyntheticWords
    out, res = straight_run
    extra = tmp_path / "extra_set"                                    # one more evaluation set, in the project's image_list format
    extra.mkdir()
    src = SyntheticWords(5, "ALLCASES_SYMBOLS", 25, seed=11)
    with open(extra / "gt.txt", "w", encoding="utf-8") as f:
        for i in range(5):
            Image.fromarray(src[i][0]).save(extra / f"w{i}.png")
            f.write(f"w{i}.png\t{src[i][1]}\n")
    drv = _driver()
    got = drv.main(drv.get_args((COMMON + " --eval --resume " + os.path.join(out, "checkpoint-1.pth") + " --other_test_data_folders " + str(extra)).split()))
    last = [json.loads(l) for l in open(os.path.join(out, "log.txt"))][-1]
    assert set(got["test_stats"]) == {"loss", "acc", "recognition_fmeasure", "edit_distance"}
    for k in ("acc", "loss", "recognition_fmeasure", "edit_distance"):
        assert got["test_stats"][k] == last["test_" + k] == res["test_stats"][k], k
    assert list(got["eval"]) == ["synthetic", str(extra)]
    other = got["eval"][str(extra)]
    assert set(other) == set(got["test_stats"]) and all(math.isfinite(v) for v in other.values()) and 0.0 <= other["acc"] <= 1.0


VARIANTS = {"attention": "--decoder_type attention", "abi_views": "--num_view 2 --use_abi_aug", "ema": "--model_ema --model_ema_decay 0.9",
            "frozen": "--fixed_encoder_layers 3"}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(VARIANTS))
def test_other_heads_and_views_construct_and_step(name, tmp_path):
    """One short run each: finite loss, a checkpoint; no accuracy is asserted."""
    from dig_amd.finetune import RecModelTrain
    drv = _driver()
    argv = (COMMON.replace("--epochs 2", "--epochs 1").replace("--smoothing 0.", "--smoothing 0.1") + " --save_ckpt --output_dir " + str(tmp_path) + " "
            + VARIANTS[name]).split()
    res = drv.main(drv.get_args(argv))
    assert math.isfinite(res["train_stats"]["loss"]) and math.isfinite(res["test_stats"]["loss"])
    ck = _load(str(tmp_path / "checkpoint-0.pth"))
    if name == "ema":
        assert set(ck["model_ema"]) == set(ck["model"])
        moved = [k for k in ck["model"] if not torch.equal(ck["model"][k], ck["model_ema"][k])]
        assert moved and all(torch.isfinite(v).all() for v in ck["model_ema"].values())
    else:
        assert "model_ema" not in ck
    if name == "frozen":
        args = drv.get_args(argv)
        torch.manual_seed(args.seed)
        first = RecModelTrain(args).state_dict()                      # the initial values: the driver seeds torch the same way before it builds
        frozen = [k for k in first if "encoder.patch_embed" in k or (k.startswith("encoder.blocks.") and int(k.split(".")[2]) < 2)]
        assert len(frozen) > 20
        assert all(torch.equal(ck["model"][k], first[k]) for k in frozen), [k for k in frozen if not torch.equal(ck["model"][k], first[k])][:5]
        assert any(not torch.equal(ck["model"][k], first[k]) for k in first if k.startswith("encoder.blocks.2."))
