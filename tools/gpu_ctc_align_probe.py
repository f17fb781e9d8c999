"""Cost of the CTC forced alignment (`--ctc_align_out`, dig_ctc_align) on the CTCRecModel of tools/gpu_ctc_probe.py: simmim_vit_small_patch4_32x128
encoder, 97 classes + blank (C = 98), T = 32 frames, batch 256, random weights; target words of 3 to 12 letters.  From one run:

  * the align launch alone, of the target words and of the greedy rows, on the model's evaluation logits;
  * the evaluation forward + greedy decode, without and with the alignment of the rows just decoded (what `evaluate` adds per batch);
  * the greedy decode launch and the loss launch alone on the same logits, as the yardsticks (one wave per sample each).

Prints the figures stamped with build.source_hash().  No time gate: there is no earlier alignment path to compare with.

    python tools/gpu_ctc_align_probe.py
"""
import os, sys, time, types
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dig_amd import build
from dig_amd.ctc_recognizer import CTCRecModelTrain, ctc_align, ctc_greedy_decode, ctc_loss
dev = torch.device("cuda:0")
B = 256
g = torch.Generator().manual_seed(0)
images = (torch.rand(B, 3, 32, 128, generator=g) * 2 - 1).to(dev)
rng = np.random.RandomState(0)
lens = torch.from_numpy(rng.randint(4, 14, size=B)); tg = torch.from_numpy(rng.randint(0, 94, size=(B, 25)))     # 3 to 12 letters, then EOS
for b in range(B): tg[b, int(lens[b]) - 1] = 94; tg[b, int(lens[b]):] = 95
tg, lens = tg.to(dev), lens.to(dev)


def timed(fn, n=50):
    for _ in range(5): fn()
    torch.cuda.synchronize(); t = time.perf_counter()
    for _ in range(n): fn()
    torch.cuda.synchronize(); return (time.perf_counter() - t) / n


args = types.SimpleNamespace(model="simmim_vit_small_patch4_32x128", decoder_name="tf_decoder", nb_classes=97, max_len=25, drop=0.1, attn_drop_rate=0.1,
                             drop_path=0.1)
torch.manual_seed(0)
m = CTCRecModelTrain(args)
m.to(dev); m.eval()
out = m((images, None, None))[0]
x = out.detach().float().contiguous()
T, C = x.shape[1], x.shape[2]
ids, _, n = m.decode(out, beam_width=0)


def evaluate(align):
    o = m((images, None, None))[0]
    rows, _, cnt = m.decode(o, beam_width=0)
    return m.align(o, rows, cnt, len_offset=0) if align else rows


print(f"source hash {build.source_hash()}, {torch.cuda.get_device_name(0)}")
plp_t, plp_g = ctc_align(x, C, tg, lens, m.blank)[3], m.align(out, ids, n, len_offset=0)[3]
print(f"ctc align B={B} T={T} C={C}: {int(torch.isfinite(plp_t).sum())} of {B} target words (3 to 12 letters) and {int(torch.isfinite(plp_g).sum())} of {B} "
      f"greedy rows (mean length {float(n.float().mean()):.1f}) have an alignment")
al_t = timed(lambda: ctc_align(x, C, tg, lens, m.blank))
al_f = timed(lambda: ctc_align(x, C, tg, lens, m.blank, want_frames=True))
al_g = timed(lambda: ctc_align(x, C, ids, n.long(), m.blank, len_offset=0))
gr = timed(lambda: ctc_greedy_decode(x, C, m.blank, m.eos, m.padding))
ls = timed(lambda: ctc_loss(x, C, tg, lens, m.blank))
print(f"align launch alone (with its five output allocations): target words {al_t*1e6:.1f} us, with frame_label {al_f*1e6:.1f} us, greedy rows {al_g*1e6:.1f} us; "
      f"greedy decode launch alone {gr*1e6:.1f} us; loss launches alone {ls*1e6:.1f} us: align = {al_t/gr:.2f}x the greedy decode, {al_t/ls:.2f}x the loss")
# alternating, three rounds: the difference of two 10 ms figures is read against their spread
ev0, ev1 = [], []
for _ in range(3):
    ev0.append(timed(lambda: evaluate(False), 20)); ev1.append(timed(lambda: evaluate(True), 20))
print(f"evaluation forward + greedy decode: {min(ev0)*1e3:.3f} ms (rounds {', '.join(f'{v*1e3:.3f}' for v in ev0)}) = {B/min(ev0):.0f} images/s; "
      f"with the alignment of the decoded rows: {min(ev1)*1e3:.3f} ms (rounds {', '.join(f'{v*1e3:.3f}' for v in ev1)}) = {B/min(ev1):.0f} images/s, "
      f"{min(ev1)/min(ev0):.4f}x")
