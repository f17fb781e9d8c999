"""The text-conditional decoder cross-attention (`--text_cond_vis`) at the README configuration (README.md:92-118: simmim_vit_small_patch4_32x128 +
tf_decoder, 97 classes, max_len 25, batch 256, README drop rates, AdamW with layer decay 0.75; random weights and labels): the fine-tune
training step and the greedy evaluation with and without the flag, and the new launches alone at the decoder's shapes (S = 256, Lq = 25,
N = 256, d = 512, 8 heads), event-timed.  The forward's arithmetic is 2 sweeps x (LayerNorm of a row + heads x d multiply-adds) per (query, key)
pair; the fraction of the fp32 vector peak counts the heads x d multiply-adds of both sweeps only (2 FLOP each) against 157 TFLOP/s."""
import os, sys, time, types
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dig_amd import build, ops
from dig_amd.finetune import RecModelTrain, SeqCrossEntropyLoss, LayerDecayValueAssigner, create_optimizer
from dig_amd.utils import NativeScalerWithGradNormCount
dev = torch.device("cuda:0")
B, T = 256, 25
print("kernel sources", build.source_hash())


def model(flag):
    args = types.SimpleNamespace(model="simmim_vit_small_patch4_32x128", decoder_name="tf_decoder", nb_classes=97, max_len=T, drop=0.1, attn_drop_rate=0.1,
                                 drop_path=0.1, opt="adamw", lr=1e-4, weight_decay=0.05, opt_eps=1e-8, opt_betas=[0.9, 0.999], text_cond_vis=flag)
    torch.manual_seed(0)
    m = RecModelTrain(args, decoder_dropout=0.1)
    m.to(dev); m.train()
    nl = m.get_num_layers()
    asg = LayerDecayValueAssigner([0.75 ** (nl + 1 - i) for i in range(nl + 2)])
    opt = create_optimizer(args, m, get_num_layer=asg.get_layer_id, get_layer_scale=asg.get_scale)
    for grp in opt.param_groups: grp["lr"] = args.lr * grp["lr_scale"]
    return m, opt


g = torch.Generator().manual_seed(0)
images = (torch.rand(B, 3, 32, 128, generator=g) * 2 - 1).to(dev)
rng = np.random.RandomState(0)
lens = torch.from_numpy(rng.randint(3, 26, size=B)); tg = torch.from_numpy(rng.randint(0, 94, size=(B, T)))
for b in range(B): tg[b, int(lens[b]) - 1] = 94; tg[b, int(lens[b]):] = 95
tg, lens = tg.to(dev), lens.to(dev)
crit, scaler = SeqCrossEntropyLoss(), NativeScalerWithGradNormCount()


def timed(fn, warm, n):
    for _ in range(warm): fn()
    torch.cuda.synchronize(); t = time.perf_counter()
    for _ in range(n): fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / n


res = {}
for flag in (False, True):
    m, opt = model(flag)

    def step():
        opt.zero_grad()
        scaler(crit(m((images, tg, lens))[0], tg, lens), opt, clip_grad=None, parameters=None)
    res["train", flag] = timed(step, 3, 8)
    m.eval()
    res["eval", flag] = timed(lambda: m((images, None, None)), 2, 5)
    print(f"text_cond_vis={flag}: fine-tune step {res['train', flag] * 1e3:.1f} ms = {B / res['train', flag]:.0f} images/s; greedy evaluation "
          f"{res['eval', flag] * 1e3:.1f} ms = {B / res['eval', flag]:.0f} images/s", flush=True)
    del m, opt
print(f"ratio with / without the flag: training {res['train', True] / res['train', False]:.2f}, evaluation {res['eval', True] / res['eval', False]:.2f}")

S, Lq, N, H, d = B, T, 256, 8, 512
rn = lambda *s: torch.randn(*s, generator=g).to(dev)
film, u = rn(S * Lq, 2 * d).bfloat16(), (rn(S * Lq, H * d) * (1.5 / (2 * d) ** 0.5)).bfloat16()
vk, mem, dc = rn(S * N, d).bfloat16(), rn(S * N, d).bfloat16(), rn(S * Lq, H * d).bfloat16()
lg, lb, dlg, dlb = torch.ones(d, device=dev), torch.zeros(d, device=dev), torch.zeros(d, device=dev), torch.zeros(d, device=dev)
c, lse = ops.tcv_attn_fwd(film, u, vk, mem, lg, lb, S, Lq, N, H)


def ev(fn, n=5):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


tf = ev(lambda: ops.tcv_attn_fwd(film, u, vk, mem, lg, lb, S, Lq, N, H))
tb = ev(lambda: ops.tcv_attn_bwd(film, u, vk, mem, lg, lb, c, lse, dc, dlg, dlb, S, Lq, N, H))
t1 = ev(lambda: ops.tcv_attn_fwd(film[:S], u[:S], vk, mem, lg, lb, S, 1, N, H))
flop = 2 * 2 * S * Lq * N * H * d
print(f"dig_tcv_attn_fwd S={S} Lq={Lq} N={N} d={d}: {tf:.3f} ms = {flop / tf / 1e9:.1f} TFLOP/s of the two contractions = {flop / tf / 1e9 / 157 * 100:.1f} % of the "
      f"fp32 vector peak; dig_tcv_attn_bwd (3 launches): {tb:.3f} ms; forward with Lq=1 (one decode step): {t1:.3f} ms")
