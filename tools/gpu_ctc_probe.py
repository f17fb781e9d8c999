"""Throughput of the CTCRecModel training step and evaluation (`--decoder_type ctc`) beside the tf_decoder's in the same run on the same box:
simmim_vit_small_patch4_32x128 encoder, 97 classes, max_len 25, batch 256, README drop rates (--drop 0.1 --attn_drop_rate 0.1 --drop_path 0.1;
the tf_decoder's own dropout 0.1), AdamW with layer decay 0.75; random weights and labels.  Training: forward + criterion + backward + AdamW.
Evaluation: the eval forward and, for the CTC head, `decode` (for the tf_decoder the forward IS the greedy decode, replayed from its HIP graph);
for the CTC head also with the prefix beam search of widths 4, 8, 16 and 32 (`--ctc_beam_width`) in place of the greedy decode, beside the
decode launch alone on the same logits and the share of rows that the search decodes differently (random weights: flat frames).
Lexicon decode (`--ctc_lexicon`, dig_ctc_lexicon_decode): the evaluation forward + decode and the decode launch alone against 50 words per
image (disjoint ranges), 1 000 per image (disjoint ranges) and one shared list of 90 000 words, word lengths 3 to 12 (rows sorted by length
within a range, as `LabelLexicon` lays them out) and every word at 25 labels, as (image, word) scores per second; beside each, on the same
lexicons, dig_lexicon_search on the greedy strings (the setup of tools/gpu_lexicon_probe.py) and the ratio of the two times.
Prints the figures stamped with build.source_hash().  No time gate: there is no earlier CTC path to compare with.

    python tools/gpu_ctc_probe.py [--lexicon]    # --lexicon: the lexicon lines only
"""
import os, sys, time, types
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dig_amd import build
LEXICON_ONLY = "--lexicon" in sys.argv
from dig_amd.ctc_recognizer import CTCRecModelTrain, SeqCTCLoss
from dig_amd.finetune import RecModelTrain, SeqCrossEntropyLoss, LayerDecayValueAssigner, create_optimizer
from dig_amd.utils import NativeScalerWithGradNormCount
dev = torch.device("cuda:0")
B = 256
g = torch.Generator().manual_seed(0)
images = (torch.rand(B, 3, 32, 128, generator=g) * 2 - 1).to(dev)
rng = np.random.RandomState(0)
lens = torch.from_numpy(rng.randint(3, 26, size=B)); tg = torch.from_numpy(rng.randint(0, 94, size=(B, 25)))
for b in range(B): tg[b, int(lens[b]) - 1] = 94; tg[b, int(lens[b]):] = 95


def timed(fn, n=10):
    for _ in range(2): fn()
    torch.cuda.synchronize(); t = time.perf_counter()
    for _ in range(n): fn()
    torch.cuda.synchronize(); return (time.perf_counter() - t) / n


def lexicon_lines(m, evaluate, ev):
    """The lexicon decode of model m (eval mode) on the probe's images, and dig_lexicon_search on the greedy strings of the same logits."""
    from dig_amd import evaluation_metric as EM
    from dig_amd.ctc_recognizer import ctc_lexicon_decode
    out = m((images, None, None))[0]
    x = out.detach().float().contiguous()
    T, C = x.shape[1], x.shape[2]
    q, ql = EM.tokens_to_text(m.decode(out, beam_width=0)[0], [chr(ord("a") + i % 26) for i in range(94)] + ["EOS", "PADDING", "UNKNOWN"])
    lrng = np.random.RandomState(1)
    for lo, hi in ((3, 12), (25, 25)):
        for name, per, shared in (("50 per image", 50, False), ("1 000 per image", 1000, False), ("90 000 shared", 90000, True)):
            W = per if shared else per * B
            lens = lrng.randint(lo, hi + 1, size=W).astype(np.int32)
            lens = np.sort(lens.reshape(-1, per), axis=1).reshape(-1)         # (a range's rows by length)
            rows = lrng.randint(0, 94, size=(W, hi)).astype(np.int32)
            rows[np.arange(hi)[None, :] >= lens[:, None]] = 0
            pool = (torch.from_numpy(rows).to(dev), torch.from_numpy(lens).to(dev))
            text = (torch.from_numpy(rows + ord("a") * (rows > 0)).to(dev), pool[1])
            begin, count = ([0] * B if shared else [b * per for b in range(B)]), [per] * B
            dec = timed(lambda: ctc_lexicon_decode(x, C, m.blank, m.eos, m.padding, pool, begin, count))
            full = timed(lambda: ctc_lexicon_decode(m((images, None, None))[0].detach().float().contiguous(), C, m.blank, m.eos, m.padding, pool, begin, count), 5)
            srch = timed(lambda: EM.lexicon_search(q, ql, text[0], text[1], begin, count))
            best = ctc_lexicon_decode(x, C, m.blank, m.eos, m.padding, pool, begin, count)[0]
            print(f"ctc lexicon decode B={B} T={T} C={C} lengths {lo}-{hi}, {name}: forward + decode {full*1e3:.2f} ms ({full/ev:.2f}x the greedy "
                  f"evaluation); decode alone {dec*1e3:.3f} ms = {B*per/dec:.3e} (image, word) scores/s ({int((best >= 0).sum())} of {B} images got a "
                  f"word); dig_lexicon_search on the greedy strings {srch*1e3:.3f} ms: the likelihood decode takes {dec/srch:.2f}x its time", flush=True)


def measure(name):
    args = types.SimpleNamespace(model="simmim_vit_small_patch4_32x128", decoder_name="tf_decoder", nb_classes=97, max_len=25, drop=0.1, attn_drop_rate=0.1,
                                 drop_path=0.1, opt="adamw", lr=1e-4, weight_decay=0.05, opt_eps=1e-8, opt_betas=[0.9, 0.999])
    torch.manual_seed(0)
    m = CTCRecModelTrain(args) if name == "ctc" else RecModelTrain(args, decoder_dropout=0.1)
    m.to(dev); m.train()
    nl = m.get_num_layers()
    asg = LayerDecayValueAssigner([0.75 ** (nl + 1 - i) for i in range(nl + 2)])
    opt = create_optimizer(args, m, get_num_layer=asg.get_layer_id, get_layer_scale=asg.get_scale)
    for grp in opt.param_groups: grp["lr"] = args.lr * grp["lr_scale"]
    crit, scaler = (SeqCTCLoss(m.blank) if name == "ctc" else SeqCrossEntropyLoss()), NativeScalerWithGradNormCount()
    def step():
        opt.zero_grad()
        loss = crit(m((images, tg, lens))[0], tg, lens)
        return loss, scaler(loss, opt, clip_grad=None, parameters=None)
    train = float("nan")
    if not LEXICON_ONLY:
        for _ in range(3): loss, gn = step()
        torch.cuda.synchronize(); t = time.perf_counter(); n = 10
        for _ in range(n): loss, gn = step()
        torch.cuda.synchronize(); train = (time.perf_counter() - t) / n
    m.eval()
    def evaluate():
        out = m((images, None, None))[0]
        return m.decode(out)[0] if name == "ctc" else out.argmax(-1)
    for _ in range(3): ids = evaluate()
    torch.cuda.synchronize(); t = time.perf_counter(); n = 10
    for _ in range(n): ids = evaluate()
    torch.cuda.synchronize(); ev = (time.perf_counter() - t) / n
    if not LEXICON_ONLY:
        print(f"{name}: training step B={B}: {train*1e3:.2f} ms = {B/train:.0f} images/s (loss {loss.item():.3f}, grad norm {gn.item():.3f}); "
              f"evaluation forward + decode: {ev*1e3:.2f} ms = {B/ev:.0f} images/s (ids {tuple(ids.shape)})", flush=True)
    if name == "ctc" and LEXICON_ONLY:
        print(f"ctc: greedy evaluation forward + decode: {ev*1e3:.2f} ms = {B/ev:.0f} images/s", flush=True)
        lexicon_lines(m, evaluate, ev)
    elif name == "ctc":
        def timed(fn, n=20):
            for _ in range(3): fn()
            torch.cuda.synchronize(); t = time.perf_counter()
            for _ in range(n): fn()
            torch.cuda.synchronize(); return (time.perf_counter() - t) / n
        out = m((images, None, None))[0]
        greedy_ids, dec0 = m.decode(out, beam_width=0)[0], timed(lambda: m.decode(out, beam_width=0))
        print(f"ctc: greedy decode alone {dec0*1e3:.3f} ms", flush=True)
        for width in (4, 8, 16, 32):
            m.ctc_beam_width = width
            evw, decw = timed(evaluate, 10), timed(lambda: m.decode(out))
            differ = int((m.decode(out)[0] != greedy_ids).any(1).sum())
            print(f"ctc: --ctc_beam_width {width}: evaluation forward + decode: {evw*1e3:.2f} ms = {B/evw:.0f} images/s ({evw/ev:.3f}x the greedy "
                  f"evaluation); beam decode alone {decw*1e3:.3f} ms; {differ} of {B} rows differ from the greedy ones", flush=True)
        m.ctc_beam_width = 0
        lexicon_lines(m, evaluate, ev)
    return train, ev


print(f"source hash {build.source_hash()}, {torch.cuda.get_device_name(0)}")
ctc = measure("ctc")
if LEXICON_ONLY:
    sys.exit(0)
tfd = measure("tf_decoder")
print(f"ctc / tf_decoder: training step {ctc[0] / tfd[0]:.3f}x the time, evaluation {ctc[1] / tfd[1]:.3f}x the time")
