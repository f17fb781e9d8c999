"""Fine-tune and evaluation driver for the MI355X engine: the two README commands of the reference (README.md:91-116, 129-152) run against
this file, with `--data_path` / `--eval_data_path` pointed at `synthetic` or a directory with `gt.txt` where there is no LMDB reader.

    python run_class_finetuning.py --model simmim_vit_small_patch4_32x128 --data_path DATA --eval_data_path DATA --finetune PRETRAIN.pth \
        --output_dir OUT --batch_size 256 --opt adamw --opt_betas 0.9 0.999 --weight_decay 0.05 --data_set image_lmdb --nb_classes 97 \
        --smoothing 0. --max_len 25 --epochs 10 --warmup_epochs 1 --drop 0.1 --attn_drop_rate 0.1 --drop_path 0.1 --dist_eval --lr 1e-4 \
        --num_samples 1 --fixed_encoder_layers 0 --decoder_name tf_decoder --use_abi_aug --num_view 2
    python run_class_finetuning.py ... --resume OUT/checkpoint-9.pth --eval --beam_width 0

What it keeps of run_class_finetuning.py:258-640 (`main`): distributed init from the launcher's environment, per-rank seeding (:271-274),
the train / evaluation datasets, samplers and loaders (:285-334: DistributedSampler(shuffle=True) + drop_last for training, batches of
int(1.5 * batch_size) in order or sharded by --dist_eval for evaluation), `RecModel`, `AttnRecModel` or `CTCRecModel` by --decoder_type (:350-355),
args.window_size / args.patch_size (:357-360), the --finetune load (:362-440: --model_key search, `head.*` removal, `backbone.` strip,
non-strict load under --model_prefix with the missing / unexpected report), --model_ema (:446-454), lr = lr * total batch / 256 (:462-464),
layer-wise lr decay, the no-weight-decay list and --fixed_encoder_layers (:471-521), the step-level cosine lr / weight-decay schedules
(:524-533), the criterion by --smoothing (:535-544), auto-resume (:553), --eval with --other_test_data_folders relative to the parent of
--eval_data_path (:557-580), and the epoch loop (:585-635): `train_one_epoch` with the validation loader and --eval_freq, `save_model` every
--save_ckpt_freq epochs (20 above 100 epochs), the per-epoch `evaluate`, the `best` checkpoint, the TensorboardLogger scalars and one JSON
line per epoch in `log.txt` with the reference's keys.

What is different, on purpose:
  * the input pipeline.  A dataset hands over `(uint8 crop, word)`; resize / ABINet / seqCLR views and the label encoding run on the MI355X
    on whole batches (dig_amd/rec_datasets.py).  Beside `image_lmdb` (through the `lmdb` module, where it is installed) there are
    `--data_set image_list` (a directory with `gt.txt`: `relative/path<TAB>word` per line) and `--data_path synthetic --synthetic N` (rendered
    random words); a substituted sample is the one right behind the refused one (see rec_datasets.py);
  * data parallelism is one all-reduce of the flat gradient arena (`FlatGradComm`) instead of DistributedDataParallel;
  * the `pos_embed` interpolation of :403-424 has nothing to act on (the encoders here carry sinusoid tables, not a learned `pos_embed`) and is
    left out, as are the `pvt` / `ladder` key rewrites of models that are not built;
  * --other_test_data_folders defaults to no folders (the reference's default names twelve benchmark directories beside the evaluation set);
  * `ignore_index` of the label-smoothing criterion is stored and never read by the reference's forward; here it is an attribute of the criterion;
  * --eval returns instead of calling exit(0); `main(args)` returns {"train_stats", "test_stats", "max_accuracy"} for in-process callers;
  * the `screen.txt` tee of utils/logging.py is not reproduced: redirect stdout;
  * flags whose code path the reference never reaches are accepted and reported; flags that select what is not built (deepspeed, the
    sequential cls token, semantic insertion, w2v targets, the contrastive centre loss, the decoupled decoder, the ImageNet / CIFAR / folder
    datasets, inputs other than 32 x 128) say so and stop;
  * `--decoder_type ctc`: the reference's help text promises it and models/model_builder.py has `CTCRecModel`, but its `main` raises for it and
    has no criterion.  Here it builds `CTCRecModelTrain` under `SeqCTCLoss` whatever --smoothing says (reported once when --smoothing > 0 is
    ignored); --beam_width > 0 (the autoregressive beam), --text_cond_vis and --use_1d_attdec stop with it (dig_amd/ctc_recognizer.py says
    what is mirrored and what is this project's own definition);
  * `--decoder_type attention --beam_width K` (K <= 8): the reference's `AttnRecModel.forward` ignores the flag and samples greedily although its
    head carries `beam_search`; here `evaluate` decodes by that method (said once), with its `predecessors` an integer division;
  * own flags: --data_set image_list, --synthetic N, --eval_edit_distance (adds the EditDistance meter to `evaluate`), --ctc_beam_width K
    (with --decoder_type ctc: `evaluate` decodes by CTC prefix beam search of width K <= 32, said once; 0, the default, is the greedy collapse;
    the training loop's class accuracy stays greedy), --ctc_lexicon FILE (with --decoder_type ctc: a UTF-8 file, one word per line;
    `evaluate` decodes each image to the word of FILE with the highest CTC likelihood, said once; not together with --ctc_beam_width),
    --ctc_align_out FILE (with --decoder_type ctc: `evaluate` makes one more device call per batch, the forced alignment of the rows it just
    decoded through the frames, and appends one JSON line per image to FILE in evaluation order, `FILE.rankN` with more than one rank:
    {"index", "word" (the ground truth), "text", "path_logp", "chars": [[char, x0, x1, logp], ...]} with the character boxes in crop columns;
    FILE is emptied when the run starts; said once; meters and return values stay as they are), --ctc_align_of {prediction,target} (what
    --ctc_align_out aligns: the decoded rows, the default, or the ground-truth targets).

Multi-rank runs are wired (samplers, FlatGradComm, the meters' all-reduce) but only the single-rank path is tested."""
import argparse
import datetime
import json
import math
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# Flags of the reference's get_args (run_class_finetuning.py:43-255) whose code path its `main` never reaches -- the mixup family sits behind
# `if False:` (:340), the timm augmentation / pooling / head-init options belong to the classification script this one was derived from, ranks
# come from the launcher's environment, pinning is the device transform's business.  name -> (type, the reference's default).  Parsed,
# reported once when given, not used.
REFERENCE_ONLY_VALUES = {
    "--mixup": (float, 0.8), "--cutmix": (float, 1.0), "--mixup_prob": (float, 1.0), "--mixup_switch_prob": (float, 0.5), "--mixup_mode": (str, "batch"),
    "--aa": (str, "rand-m9-mstd0.5-inc1"), "--color_jitter": (float, 0.4), "--reprob": (float, 0.25), "--remode": (str, "pixel"), "--recount": (int, 1),
    "--train_interpolation": (str, "bicubic"), "--crop_pct": (float, None), "--input_size": (int, 224), "--init_scale": (float, 0.001),
    "--num_mem_slots": (int, 0), "--num_parts": (int, 1), "--train_url": (str, "/home/ma-user/modelarts/outputs/train_url_0/"),
    "--momentum": (float, 0.9), "--warmup_lr": (float, 1e-6), "--world_size": (int, 1), "--local_rank": (int, -1)}
REFERENCE_ONLY_SWITCHES = ("--resplit", "--use_mem_in_decoder", "--use_multi_label_loss", "--model_ema_force_cpu", "--dist_on_itp")
MODELS = ("simmim_vit_tiny_patch4_32x128", "simmim_vit_small_patch4_32x128", "simmim_vit_base_patch4_32x128")


def get_args(argv=None):
    p = argparse.ArgumentParser("DiG fine-tuning and evaluation on MI355X (dig_amd)", add_help=True)
    a = p.add_argument
    a("--batch_size", default=64, type=int, help="samples per GPU")
    a("--epochs", default=30, type=int)
    a("--update_freq", default=1, type=int)
    a("--save_ckpt_freq", default=1, type=int)
    a("--eval_freq", default=1000, type=int)
    # model
    a("--model", default="deit_base_patch16_224", type=str, help="one of " + ", ".join(MODELS))
    a("--decoder_name", default="tf_decoder", type=str)
    a("--decoder_type", default="tf_decoder", type=str, help="tf_decoder (RecModel), attention (AttnRecModel) or ctc (CTCRecModel)")
    a("--insert_sem", action="store_true", default=False)
    a("--text_cond_vis", action="store_true", default=False)
    a("--input_h", default=32, type=int)
    a("--input_w", default=128, type=int)
    a("--drop", type=float, default=0.0)
    a("--attn_drop_rate", type=float, default=0.0)
    a("--drop_path", type=float, default=0.1)
    a("--use_seq_cls_token", type=bool, default=False)
    a("--disable_eval_during_finetuning", action="store_true", default=False)
    a("--model_ema", action="store_true", default=False)
    a("--model_ema_decay", type=float, default=0.9999)
    a("--use_1d_attdec", action="store_true", default=False)
    # optimizer
    a("--opt", default="adamw", type=str)
    a("--opt_eps", default=1e-8, type=float)
    a("--opt_betas", default=None, type=float, nargs="+")
    a("--clip_grad", type=float, default=None)
    a("--weight_decay", type=float, default=0.05)
    a("--weight_decay_end", type=float, default=None)
    a("--lr", type=float, default=1e-3)
    a("--layer_decay", type=float, default=0.75)
    a("--min_lr", type=float, default=1e-6)
    a("--warmup_epochs", type=int, default=5)
    a("--warmup_steps", type=int, default=-1)
    a("--use_contrastive_center_loss", action="store_true", default=False)
    a("--smoothing", type=float, default=0.1)
    a("--beam_width", type=int, default=0)
    a("--ctc_beam_width", type=int, default=0, help="with --decoder_type ctc: evaluate with a CTC prefix beam search of this width (1..32); 0 = greedy")
    a("--ctc_lexicon", type=str, default=None, metavar="FILE",
      help="with --decoder_type ctc: evaluate by decoding each image to the most probable word of FILE (UTF-8, one word per line)")
    a("--ctc_align_out", type=str, default=None, metavar="FILE",
      help="with --decoder_type ctc: evaluate also aligns every image's string to its frames and writes one JSON line per image to FILE")
    a("--ctc_align_of", type=str, default="prediction", choices=("prediction", "target"),
      help="what --ctc_align_out aligns: the rows the evaluation decoded (default) or the ground-truth targets")
    # fine-tuning
    a("--finetune", default="", help="pre-training checkpoint to start from")
    a("--model_key", default="model|module", type=str)
    a("--model_prefix", default="", type=str)
    a("--fixed_encoder_layers", type=int, default=0)
    # data
    a("--data_path", default="/datasets01/imagenet_full_size/061417/train", nargs="+", type=str,
      help="LMDB root(s), image_list directories (gt.txt), or `synthetic` (with --synthetic N)")
    a("--eval_data_path", default=None, type=str)
    a("--other_test_data_folders", type=str, nargs="+", default=None, help="with --eval: further evaluation sets beside --eval_data_path")
    a("--nb_classes", default=1000, type=int)
    a("--data_set", default="IMNET", choices=["CIFAR", "IMNET", "image_folder", "image_lmdb", "image_list"], type=str)
    a("--synthetic", type=int, default=0, help="N rendered random words for a `synthetic` data path")
    a("--voc_type", type=str, default="ALLCASES_SYMBOLS", choices=["LOWERCASE", "ALLCASES", "ALLCASES_SYMBOLS"])
    a("--max_len", type=int, default=100)
    a("--num_samples", type=float, default=math.inf, help="cap on the training samples per root; a value <= 1 is a fraction")
    a("--w2v_path", type=int, default=None)
    a("--num_view", default=1, type=int)
    a("--use_abi_aug", action="store_true", default=False)
    a("--num_workers", default=5, type=int)
    # run
    a("--output_dir", default="")
    a("--log_dir", default=None)
    a("--device", default="cuda")
    a("--seed", default=0, type=int)
    a("--resume", default="")
    a("--auto_resume", action="store_true", default=True)
    a("--no_auto_resume", action="store_false", dest="auto_resume")
    a("--save_ckpt", action="store_true", default=True)
    a("--no_save_ckpt", action="store_false", dest="save_ckpt")
    a("--start_epoch", default=0, type=int)
    a("--eval", action="store_true", help="evaluation only")
    a("--eval_edit_distance", action="store_true", default=False, help="evaluate() also reports the mean edit distance")
    a("--dist_eval", action="store_true", default=False)
    a("--dist_url", default="env://")
    a("--enable_deepspeed", action="store_true", default=False)
    # accepted, not used
    for name, (ty, _) in REFERENCE_ONLY_VALUES.items():
        a(name, type=ty, default=None, help=argparse.SUPPRESS)
    a("--cutmix_minmax", type=float, nargs="+", default=None, help=argparse.SUPPRESS)
    for name in REFERENCE_ONLY_SWITCHES:
        a(name, action="store_true", default=False, help=argparse.SUPPRESS)
    a("--use_mean_pooling", action="store_true", default=None, help=argparse.SUPPRESS)
    a("--use_cls", action="store_false", dest="use_mean_pooling", default=None, help=argparse.SUPPRESS)
    a("--imagenet_default_mean_and_std", action="store_true", default=None, help=argparse.SUPPRESS)
    a("--pin_mem", action="store_true", default=None, help=argparse.SUPPRESS)
    a("--no_pin_mem", action="store_false", dest="pin_mem", default=None, help=argparse.SUPPRESS)
    args = p.parse_args(argv)

    given = [n for n in REFERENCE_ONLY_VALUES if getattr(args, n[2:]) is not None] + [n for n in REFERENCE_ONLY_SWITCHES if getattr(args, n[2:])]
    given += ["--cutmix_minmax"] if args.cutmix_minmax is not None else []
    given += ["--use_mean_pooling / --use_cls"] if args.use_mean_pooling is not None else []
    given += ["--imagenet_default_mean_and_std"] if args.imagenet_default_mean_and_std is not None else []
    given += ["--pin_mem / --no_pin_mem"] if args.pin_mem is not None else []
    if given:
        print("flags of the reference that its fine-tune path does not read either (accepted, not used): " + " ".join(given))
    for name, (_, default) in REFERENCE_ONLY_VALUES.items():                     # (every flag carries the reference's default)
        if getattr(args, name[2:]) is None:
            setattr(args, name[2:], default)
    args.use_mean_pooling = bool(args.use_mean_pooling)
    args.imagenet_default_mean_and_std = True
    args.pin_mem = True if args.pin_mem is None else args.pin_mem
    refuse_unbuilt(args)
    return args


def refuse_unbuilt(args):
    """Flags that select something this repository does not build: say what it is and stop."""
    if args.enable_deepspeed:
        raise SystemExit("--enable_deepspeed: the deepspeed engine (run_class_finetuning.py:483-494) is not built; the step runs in bf16 without it")
    if args.use_seq_cls_token:
        raise SystemExit("--use_seq_cls_token: the encoder-only model with a sequential cls token (create_encoder, :347-348) is not built")
    if args.insert_sem:
        raise SystemExit("--insert_sem: the decoder with inserted semantics (models/decoder.py) is not built")
    if args.w2v_path is not None:
        raise SystemExit("--w2v_path: word2vec targets (engine_for_finetuning.py) are not built")
    if args.use_contrastive_center_loss:
        raise SystemExit("--use_contrastive_center_loss: the reference names a class ContrastiveCenterLoss (:547) that it never imports; not built")
    if args.decoder_name == "decoupled_tf_decoder":
        raise SystemExit("--decoder_name decoupled_tf_decoder: the decoupled decoder (models/decoder.py) is not built")
    if args.decoder_type not in ("tf_decoder", "attention", "ctc"):
        raise SystemExit(f"--decoder_type {args.decoder_type}: tf_decoder, attention or ctc (the reference raises NotImplementedError, :355)")
    if args.decoder_type == "ctc":
        if args.beam_width > 0:
            raise SystemExit("--beam_width with --decoder_type ctc: the CTC head decodes greedily (frame arg-max, collapsed) unless --ctc_beam_width K asks "
                             "for its prefix beam search; --beam_width is the autoregressive beam, built for tf_decoder")
        if args.text_cond_vis:
            raise SystemExit("--text_cond_vis with --decoder_type ctc: the text-conditional cross-attention belongs to the transformer decoder; the CTC head has none")
        if args.use_1d_attdec:
            raise SystemExit("--use_1d_attdec with --decoder_type ctc: the CTC head always classifies the 32 column means of the token grid; the flag selects "
                             "the attention decoders' memory")
    if args.decoder_type == "attention" and not 0 <= args.beam_width <= 8:
        raise SystemExit(f"--beam_width {args.beam_width} with --decoder_type attention: 0 (greedy sample) or a beam search of width 1..8")
    if args.ctc_beam_width != 0 and args.decoder_type != "ctc":
        raise SystemExit(f"--ctc_beam_width with --decoder_type {args.decoder_type}: the prefix beam search decodes the CTC head's frames "
                         "(--decoder_type ctc); the transformer decoder's beam is --beam_width")
    if not 0 <= args.ctc_beam_width <= 32:
        raise SystemExit(f"--ctc_beam_width {args.ctc_beam_width}: 0 (greedy) or a width of 1..32")
    if args.ctc_lexicon is not None:
        if args.decoder_type != "ctc":
            raise SystemExit(f"--ctc_lexicon with --decoder_type {args.decoder_type}: the lexicon decode scores every word by the CTC head's frames "
                             "(--decoder_type ctc); the other heads have no likelihood of a whole word built")
        if args.ctc_beam_width > 0:
            raise SystemExit("--ctc_lexicon with --ctc_beam_width: an evaluation decodes by one rule, the most probable lexicon word or the prefix "
                             "beam search; give one of the two")
        if not os.path.isfile(args.ctc_lexicon):
            raise SystemExit(f"--ctc_lexicon {args.ctc_lexicon}: no such file (UTF-8, one word per line)")
        from dig_amd.ctc_recognizer import read_lexicon_file
        if not read_lexicon_file(args.ctc_lexicon):
            raise SystemExit(f"--ctc_lexicon {args.ctc_lexicon}: the file holds no word (one per line; empty lines are skipped)")
    if args.ctc_align_out is not None:
        if args.decoder_type != "ctc":
            raise SystemExit(f"--ctc_align_out with --decoder_type {args.decoder_type}: the forced alignment places a string on the CTC head's frames "
                             "(--decoder_type ctc); the autoregressive heads have no frames to align to")
        if not os.path.isdir(os.path.dirname(os.path.abspath(args.ctc_align_out))):
            raise SystemExit(f"--ctc_align_out {args.ctc_align_out}: the directory {os.path.dirname(os.path.abspath(args.ctc_align_out))} does not exist")
        if os.path.isdir(args.ctc_align_out):
            raise SystemExit(f"--ctc_align_out {args.ctc_align_out}: a directory, not a file")
    elif args.ctc_align_of != "prediction":
        raise SystemExit(f"--ctc_align_of {args.ctc_align_of} without --ctc_align_out FILE: there is no alignment to choose the rows of")
    if (args.input_h, args.input_w) != (32, 128):
        raise SystemExit(f"--input_h {args.input_h} --input_w {args.input_w}: the encoders are built for 32 x 128 crops")
    paths = [args.data_path] if isinstance(args.data_path, str) else list(args.data_path)
    if args.data_set in ("CIFAR", "IMNET", "image_folder") and paths != ["synthetic"]:
        raise SystemExit(f"--data_set {args.data_set}: the image-classification datasets of the script this driver descends from are not built; "
                         "use image_lmdb, image_list, or --data_path synthetic")
    if args.model not in MODELS:
        raise SystemExit(f"--model {args.model}: the recognition encoders built here are {', '.join(MODELS)}")
    if args.finetune.startswith("https"):
        raise SystemExit("--finetune takes a file here: download the checkpoint first")


def plan_schedule(args, n_train, world):
    """run_class_finetuning.py:462-469,524-533: the global batch, steps per epoch, the scaled lr and the two step-level schedules."""
    import dig_amd.utils as utils
    total_batch_size = args.batch_size * args.update_freq * world
    steps = n_train // total_batch_size
    lr = args.lr * total_batch_size / 256
    lr_values = utils.cosine_scheduler(lr, args.min_lr, args.epochs, steps, warmup_epochs=args.warmup_epochs, warmup_steps=args.warmup_steps)
    wd_end = args.weight_decay if args.weight_decay_end is None else args.weight_decay_end
    wd_values = utils.cosine_scheduler(args.weight_decay, wd_end, args.epochs, steps)
    return {"total_batch_size": total_batch_size, "steps_per_epoch": steps, "lr": lr, "weight_decay_end": wd_end,
            "lr_schedule_values": lr_values, "wd_schedule_values": wd_values}


def save_ckpt_freq(args):
    """:600-601: above 100 epochs a checkpoint every 20."""
    return 20 if args.epochs > 100 else args.save_ckpt_freq


def build_model(args):
    from dig_amd.attn_recognizer import AttnRecModelTrain
    from dig_amd.ctc_recognizer import CTCRecModelTrain
    from dig_amd.finetune import RecModelTrain
    return {"tf_decoder": RecModelTrain, "attention": AttnRecModelTrain, "ctc": CTCRecModelTrain}[args.decoder_type](args)


def load_finetune_checkpoint(model, args):
    """:362-440: --model_key search, `head.*` of another shape removed, `backbone.` stripped, non-strict load under --model_prefix."""
    checkpoint = torch.load(args.finetune, map_location="cpu", weights_only=False)
    print("Load ckpt from %s" % args.finetune)
    picked = checkpoint
    for model_key in args.model_key.split("|"):
        if model_key in checkpoint:
            picked = checkpoint[model_key]
            print("Load state_dict by model_key = %s" % model_key)
            break
    shapes = model.param_shapes()
    for k in ("head.weight", "head.bias"):
        if k in picked and tuple(picked[k].shape) != tuple(shapes.get(k, ())):
            print(f"Removing key {k} from pretrained checkpoint")
            del picked[k]
    return model.load_pretrained(checkpoint, model_key=args.model_key, prefix=args.model_prefix)


def main(args):
    import dig_amd.utils as utils
    from dig_amd.engine_for_finetuning import evaluate, train_one_epoch
    from dig_amd.finetune import (FlatGradComm, LayerDecayValueAssigner, ModelEma, SeqCrossEntropyLoss, SeqLabelSmoothingCrossEntropyLoss,
                                  create_optimizer)
    from dig_amd.rec_datasets import build_dataset, device_loader

    utils.init_distributed_mode(args)
    print(args)
    device = torch.device(args.device, getattr(args, "gpu", 0)) if args.device == "cuda" else torch.device(args.device)
    if device.type == "cuda":
        torch.cuda.set_device(device)
    seed = args.seed + utils.get_rank()
    torch.manual_seed(seed)
    np.random.seed(seed)
    random.seed(seed)

    # evaluation only: the training path is not read (the reference points it at the evaluation set, :282-283)
    if args.eval:
        args.data_path = [args.eval_data_path]
    world, rank = utils.get_world_size(), utils.get_rank()
    dataset_train, args.nb_classes = build_dataset(is_train=True, args=args)
    dataset_val = None if args.disable_eval_during_finetuning else build_dataset(is_train=False, args=args)[0]
    data_loader_train = device_loader(dataset_train, args, True, device, seed=seed, rank=rank, world=world)
    print("Sampler_train = %s" % str(data_loader_train.sampler))
    data_loader_val = None if dataset_val is None else device_loader(dataset_val, args, False, device, seed=seed, rank=rank, world=world)

    log_writer = None
    if rank == 0 and args.log_dir is not None:
        os.makedirs(args.log_dir, exist_ok=True)
        log_writer = utils.TensorboardLogger(log_dir=args.log_dir)

    model = build_model(args)
    patch_size = (4, 4)
    print("Patch size = %s" % str(patch_size))
    args.window_size = (args.input_h // patch_size[0], args.input_w // patch_size[1])
    args.patch_size = patch_size
    if args.finetune:
        load_finetune_checkpoint(model, args)
    model.to(device)

    model_ema = None
    if args.model_ema:
        model_ema = ModelEma(model, decay=args.model_ema_decay)
        print("Using EMA with decay = %.8f" % args.model_ema_decay)

    n_parameters = sum(p.numel() for p in model.parameters())          # (counted before --fixed_encoder_layers freezes any, as at :457)
    print("Model = %s" % model.__class__.__name__)
    print("number of params:", n_parameters)

    plan = plan_schedule(args, len(dataset_train), world)
    num_training_steps_per_epoch = plan["steps_per_epoch"]
    args.lr, args.weight_decay_end = plan["lr"], plan["weight_decay_end"]
    print("LR = %.8f" % args.lr)
    print("Batch size = %d" % plan["total_batch_size"])
    print("Update frequent = %d" % args.update_freq)
    print("Number of training examples = %d" % len(dataset_train))
    print("Number of training training per epoch = %d" % num_training_steps_per_epoch)
    if num_training_steps_per_epoch == 0 and not args.eval:
        raise SystemExit("fewer training samples than one global batch")

    num_layers = model.get_num_layers()
    assigner = None
    if args.layer_decay < 1.0:
        assigner = LayerDecayValueAssigner(list(args.layer_decay ** (num_layers + 1 - i) for i in range(num_layers + 2)))
        print("Assigned values = %s" % str(assigner.values))
    skip_weight_decay_list = model.no_weight_decay()
    print("Skip weight decay list: ", skip_weight_decay_list)

    if world > 1:
        model.comm = FlatGradComm(model)                       # parameters broadcast from rank 0, gradient arena all-reduced per step
    if args.fixed_encoder_layers > 0:
        print("these layers are fixed during training: ", model.fix_encoder_layers(args.fixed_encoder_layers))
    optimizer = create_optimizer(args, model, skip_list=skip_weight_decay_list,
                                 get_num_layer=assigner.get_layer_id if assigner is not None else None,
                                 get_layer_scale=assigner.get_scale if assigner is not None else None)
    loss_scaler = utils.NativeScalerWithGradNormCount()

    print("Use step level LR scheduler!")
    lr_schedule_values, wd_schedule_values = plan["lr_schedule_values"], plan["wd_schedule_values"]
    print("Max WD = %.7f, Min WD = %.7f" % (max(wd_schedule_values, default=args.weight_decay), min(wd_schedule_values, default=args.weight_decay)))

    if args.decoder_type == "ctc":
        from dig_amd.ctc_recognizer import SeqCTCLoss
        if args.smoothing > 0.:
            print(f"--smoothing {args.smoothing} is ignored with --decoder_type ctc: the criterion is the CTC loss")
        criterion = SeqCTCLoss(blank=model.blank)
        if model.ctc_beam_width > 0:
            print(f"evaluation decoder = CTC prefix beam search, width {model.ctc_beam_width} (--ctc_beam_width); the training loop's accuracy decodes greedily")
        if model.ctc_lexicon is not None:
            print(f"evaluation decoder = the most probable of the {len(model.ctc_lexicon.words)} words of {args.ctc_lexicon} by CTC likelihood "
                  f"({model.ctc_lexicon.n_rows} label rows; --ctc_lexicon); the training loop's accuracy decodes greedily")
        if args.ctc_align_out is not None:
            mine = args.ctc_align_out + (f".rank{utils.get_rank()}" if utils.get_world_size() > 1 else "")
            open(mine, "w").close()                                            # (every evaluate() of the run appends)
            print(f"evaluation also writes the CTC forced alignment of the {'targets' if args.ctc_align_of == 'target' else 'decoded rows'} to {mine}: "
                  f"one JSON line per image, character boxes in crop columns ({model.frame_columns} per frame; --ctc_align_out)")
    elif args.smoothing > 0.:
        criterion = SeqLabelSmoothingCrossEntropyLoss(smoothing=args.smoothing)
        criterion.ignore_index = dataset_train.class_to_idx["PADDING"]
    else:
        criterion = SeqCrossEntropyLoss()
    if args.decoder_type == "attention" and model.beam_width > 0:
        print(f"evaluation decoder = beam search of the GRU attention head, width {model.beam_width} (--beam_width); the training loop's accuracy "
              "is the teacher-forced arg-max")
    print("criterion = %s" % str(criterion))

    utils.auto_load_model(args=args, model=model, model_without_ddp=model, optimizer=optimizer, loss_scaler=loss_scaler, model_ema=model_ema)

    if args.eval:
        results = {}
        test_stats = evaluate(data_loader_val, model, device, args=args)
        print(f"Accuracy of the network on the {len(dataset_val)} test images: {test_stats['acc']:.4f}%")
        results[args.eval_data_path] = test_stats
        eval_data_dir = os.path.dirname(args.eval_data_path)
        for folder in args.other_test_data_folders or []:
            args.eval_data_path = os.path.join(eval_data_dir, folder)
            other = build_dataset(is_train=False, args=args)[0]
            loader = device_loader(other, args, False, device, seed=seed)          # (in order on every rank, :569)
            stats = evaluate(loader, model, device, args=args)
            print(f"Accuracy of the network on the {len(other)} test images: {stats['acc']:.4f}%")
            results[args.eval_data_path] = stats
        return {"train_stats": None, "test_stats": test_stats, "max_accuracy": test_stats["acc"], "eval": results}

    print(f"Start training for {args.epochs} epochs")
    start_time = time.time()
    max_accuracy = 0.0
    train_stats = test_stats = None
    for epoch in range(args.start_epoch, args.epochs):
        if args.distributed:
            data_loader_train.sampler.set_epoch(epoch)
        if log_writer is not None:
            log_writer.set_step(epoch * num_training_steps_per_epoch * args.update_freq)
        train_stats = train_one_epoch(model, criterion, data_loader_train, optimizer, device, epoch, loss_scaler, args.clip_grad, model_ema, None,
                                      log_writer=log_writer, start_steps=epoch * num_training_steps_per_epoch,
                                      lr_schedule_values=lr_schedule_values, wd_schedule_values=wd_schedule_values,
                                      num_training_steps_per_epoch=num_training_steps_per_epoch, update_freq=args.update_freq, args=args,
                                      data_loader_val=data_loader_val, max_accuracy=max_accuracy, criterion_aux=None)
        max_accuracy = train_stats["max_accuracy"]
        if args.output_dir and args.save_ckpt:
            args.save_ckpt_freq = save_ckpt_freq(args)
            if (epoch + 1) % args.save_ckpt_freq == 0 or epoch + 1 == args.epochs:
                utils.save_model(args=args, model=model, model_without_ddp=model, optimizer=optimizer, loss_scaler=loss_scaler, epoch=epoch,
                                 model_ema=model_ema)
        log_stats = {**{f"train_{k}": v for k, v in train_stats.items()}}
        if data_loader_val is not None:
            test_stats = evaluate(data_loader_val, model, device, args=args)
            print(f"Accuracy of the network on the {len(dataset_val)} test images: {test_stats['acc']:.4f}%")
            if max_accuracy < test_stats["acc"]:
                max_accuracy = test_stats["acc"]
                if args.output_dir and args.save_ckpt:
                    utils.save_model(args=args, model=model, model_without_ddp=model, optimizer=optimizer, loss_scaler=loss_scaler, epoch="best",
                                     model_ema=model_ema)
            print(f"Max accuracy: {max_accuracy:.2f}%")
            if log_writer is not None:
                log_writer.update(test_acc=test_stats["acc"], head="perf", step=epoch)
                log_writer.update(test_loss=test_stats["loss"], head="perf", step=epoch)
            log_stats.update({f"test_{k}": v for k, v in test_stats.items()})
        log_stats.update({"epoch": epoch, "n_parameters": n_parameters})
        if args.output_dir and utils.is_main_process():
            if log_writer is not None:
                log_writer.flush()
            with open(os.path.join(args.output_dir, "log.txt"), mode="a", encoding="utf-8") as f:
                f.write(json.dumps(log_stats) + "\n")
    print("Training time {}".format(str(datetime.timedelta(seconds=int(time.time() - start_time)))))
    return {"train_stats": train_stats, "test_stats": test_stats, "max_accuracy": max_accuracy}


if __name__ == "__main__":
    opts = get_args()
    if opts.output_dir:
        os.makedirs(opts.output_dir, exist_ok=True)
    main(opts)
