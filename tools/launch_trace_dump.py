#!/usr/bin/env python
"""Record what the Python side launches, for a parent / child comparison of a change that must not move a launch (CPU only; prints to stdout).

Every step of the package is a list of C-ABI calls (dig_amd._lib.call).  This tool runs the tiny configurations of the test fixtures against the
plain-C++ build of the ABI (cpu_abi/libdig_cpu.so) with `_lib.call` hooked, torch's HIP streams replaced by named stand-ins, and prints per case
  * the number of calls and a sha256 over the trace: one line per call -- the stream it was issued on, the entry point, its scalar arguments
    (pointers shown as p / 0) -- and one per stream hand-over (wait_stream, event record / wait, record_stream);
  * a sha256 of every result tensor (losses, logits, gradient arenas, parameters, optimizer moments).
`--full` prints the trace lines themselves as well.

    python tools/launch_trace_dump.py > trace.txt          # at both commits, then diff the two files
"""
import contextlib
import ctypes
import hashlib
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, _p)

import torch  # noqa: E402

from cpu_abi_util import cpu_abi_backend  # noqa: E402
from dig_amd import _lib, ops  # noqa: E402

TRACE = []
FULL = "--full" in sys.argv


def sha(t):
    if torch.is_tensor(t):
        t = t.detach().contiguous().reshape(-1)
        raw = t.view(torch.uint8).numpy().tobytes() if t.numel() else b""
        return hashlib.sha256(repr((str(t.dtype), tuple(t.shape))).encode() + raw).hexdigest()[:24]
    return hashlib.sha256(repr(t).encode()).hexdigest()[:24]


# ---- stand-ins for torch's streams and events: a name, the hand-overs written into the trace
class Stream:
    count = 0
    cuda_stream = 0

    def __init__(self, device=None, priority=0, name=None):
        Stream.count += 1
        self.device, self.name = torch.device(device if device is not None else "cpu"), name or f"s{Stream.count}(prio {priority})"

    @staticmethod
    def priority_range():
        return (0, -1)

    def wait_stream(self, other):
        if other is not self:
            TRACE.append(f"{self.name}: wait_stream {other.name}")

    def wait_event(self, ev):
        TRACE.append(f"{self.name}: wait_event of {ev.on}")


class Event:
    def __init__(self, enable_timing=False):
        self.on = None

    def record(self, stream=None):
        self.on = (stream or _stack[-1]).name
        TRACE.append(f"{self.on}: event record")


MAIN = Stream(name="main")
_stack = [MAIN]


@contextlib.contextmanager
def _stream_ctx(st):
    _stack.append(st)
    try:
        yield
    finally:
        _stack.pop()


def _record_stream(t, st):
    TRACE.append(f"{_stack[-1].name}: record_stream {st.name}")


def _scalar(a):
    if a is None:
        return "0"
    if isinstance(a, ctypes.c_void_p):
        return "p" if a.value else "0"
    if isinstance(a, (ctypes.c_float, ctypes.c_double)):
        return repr(float(a.value))
    if hasattr(a, "value"):
        return repr(a.value)
    if isinstance(a, (int, float)):
        return repr(a)
    return "ref"                                                        # ctypes.byref(struct)


@contextlib.contextmanager
def backend():
    """The CPU build of the ABI with `_lib.call` hooked and torch.cuda's stream surface replaced."""
    with cpu_abi_backend() as dev:
        real_call = _lib.call

        def call(name, *args):
            TRACE.append(f"{_stack[-1].name}: {name}(" + ", ".join(_scalar(a) for a in args) + ")")
            return real_call(name, *args)
        saved = (torch.cuda.Stream, torch.cuda.Event, torch.cuda.current_stream, torch.cuda.stream, torch.cuda.is_current_stream_capturing)
        _lib.call = call
        torch.cuda.Stream, torch.cuda.Event = Stream, Event
        torch.cuda.current_stream = lambda device=None: _stack[-1]
        torch.cuda.stream = _stream_ctx
        torch.cuda.is_current_stream_capturing = lambda: False
        torch.Tensor.record_stream = _record_stream
        try:
            yield dev
        finally:
            _lib.call = real_call
            torch.cuda.Stream, torch.cuda.Event, torch.cuda.current_stream, torch.cuda.stream, torch.cuda.is_current_stream_capturing = saved
            del torch.Tensor.record_stream


def case(name, fn):
    """Run fn() -> {result name: tensor or value}; print the case's trace digest and result hashes."""
    del TRACE[:]
    Stream.count = 1
    torch.manual_seed(0)
    results = fn()
    print(f"{name} calls={sum(': dig_' in l for l in TRACE)} lines={len(TRACE)} trace={sha(TRACE)}")
    for k, v in results.items():
        print(f"{name} {k}={sha(v) if torch.is_tensor(v) else v}")
    if FULL:
        for l in TRACE:
            print(f"{name} | {l}")


# ---- pre-training --------------------------------------------------------------------------------------------------------------------------
class StubComm:
    """A process group of one that the step takes for a real one: identity collectives, the process-group plan of forward and backward."""
    world, rank, world_override = 1, 0, True

    def all_reduce_(self, t):
        TRACE.append(f"{_stack[-1].name}: all_reduce {tuple(t.shape)}")
        return t

    def all_gather_cat(self, t):
        TRACE.append(f"{_stack[-1].name}: all_gather {tuple(t.shape)}")
        return t

    def grad_ready(self, model, key):
        TRACE.append(f"{_stack[-1].name}: grad_ready {key}")


def pretrain(pixel=True, moco=True, comm=None, patchnet="no_patchtrans", steps=1, optimizer=False, fwd_mode=None):
    from dig_amd import engine_core as EC
    from dig_amd.modeling_pretrain_moco_mim_ori import MoCo_ViT
    from dig_amd.optim_factory import create_optimizer

    def run():
        m = MoCo_ViT(encoder_embed_dim=128, encoder_depth=2, encoder_num_heads=2, decoder_embed_dim=64, mlp_dim=256, dim=64, T=0.2, num_windows=4,
                     use_pixel_target=pixel, use_moco_target=moco, patchnet_name=patchnet)
        m.comm = comm
        m.train()
        if fwd_mode is not None:
            saved_mode, EC.FWD_MODE = EC.FWD_MODE, fwd_mode
        g = torch.Generator().manual_seed(77)
        B = 4
        images, aug = torch.rand((B, 3, 32, 128), generator=g) * 2 - 1, torch.rand((B, 3, 32, 128), generator=g) * 2 - 1
        mask = torch.zeros(B, 2, m.N, dtype=torch.bool)
        for b in range(B):
            for v in range(2):
                mask[b, v, torch.randperm(m.N, generator=g)[:179]] = True
        opt = None
        if optimizer:
            args = types.SimpleNamespace(opt="adamw", lr=1e-3, weight_decay=0.05, opt_eps=1e-8, opt_betas=None)
            with contextlib.redirect_stdout(sys.stderr):
                opt = create_optimizer(args, m)
        out = {}
        for i in range(steps):
            if opt is not None:
                opt.zero_grad()
            st = EC._Step(m)
            contra, accs, vis = st.forward(images, aug, mask, 0.99, 1, training=True)
            st.backward(torch.tensor(1.0) if moco else None, torch.full_like(vis, 1e-3) if pixel else None)
            if opt is not None:
                opt.step()
            out.update({f"step{i}.contra": contra, f"step{i}.accs": accs, f"step{i}.vis_out": vis, f"step{i}.grads": m.flat_grads.clone(),
                        f"step{i}.momentum": m._flat["momentum"].clone(), f"step{i}.bn_stats": m._flat["bn_stats"].clone()})
        if fwd_mode is not None:
            EC.FWD_MODE = saved_mode
        if opt is not None:
            out["params"] = m.flat_params
            sd = opt.state_dict()
            with contextlib.redirect_stdout(sys.stderr):
                opt2 = create_optimizer(args, m)
            opt2.load_state_dict(sd)
            out.update({"state_dict.layout": sha([(k, sorted(v)) for k, v in sd["state"].items()] + [sorted(g_.items()) for g_ in sd["param_groups"]]),
                        "reloaded.step": opt2._step, "reloaded.exp_avg": opt2.exp_avg, "reloaded.exp_avg_sq": opt2.exp_avg_sq,
                        "reloaded.groups": sha([sorted((k, v) for k, v in g_.items() if k not in ("params",)) for g_ in opt2.param_groups])})
        return out
    return run


# ---- fine-tuning ---------------------------------------------------------------------------------------------------------------------------
def _batch(B, T, lens):
    g = torch.Generator().manual_seed(5)
    images = torch.rand((B, 3, 32, 128), generator=g) * 2 - 1
    targets = torch.randint(0, 94, (B, T), generator=g)
    lens = torch.tensor(lens)
    for b in range(B):
        targets[b, lens[b] - 1] = 94
        targets[b, lens[b]:] = 95
    return images, targets, lens


def _tf_model(dev, cls=None, **kw):
    from dig_amd.finetune import RecModelTrain
    kw = {**dict(embed_dim=128, depth=2, num_heads=2, n_layers=2, d_model=128, n_head=2, d_k=64, d_inner=64, nb_classes=97, max_len=8), **kw}
    m = (cls or RecModelTrain)(**kw)
    m._loaded = True
    m._bind(dev)
    return m


def _gru_model(dev, **kw):
    from dig_amd.attn_recognizer import AttnRecModelTrain
    m = AttnRecModelTrain(embed_dim=128, depth=2, num_heads=2, nb_classes=97, max_len=8, sDim=128, attDim=64, **kw)
    m._bind(dev)
    return m


def _ctc_model(dev, **kw):
    from dig_amd.ctc_recognizer import CTCRecModelTrain
    m = CTCRecModelTrain(embed_dim=128, depth=2, num_heads=2, nb_classes=97, max_len=8, **kw)
    m._bind(dev)
    return m


def _train_step(m, images, targets, lens, crit):
    """One forward / loss / backward through the step object (what RecModelTrain.forward's autograd node runs)."""
    st = m._step_cls(m)
    logits = st.forward(images, targets, lens)
    lg = logits.detach().clone().requires_grad_(True)
    loss = crit(lg, targets, lens)
    loss.backward()
    st.backward(lg.grad.contiguous().float())
    return logits, loss.detach(), lg.grad


def finetune(dev, make, lens_on_host=None, smoothing=None, steps=1, optimizer=False, ctc=False):
    from dig_amd import finetune as FT
    from dig_amd.ctc_recognizer import SeqCTCLoss

    def run():
        m = make(dev).train()
        images, targets, lens = _batch(3, m.max_len, [8, 3, 5])
        crit = SeqCTCLoss() if ctc else FT.SeqCrossEntropyLoss() if smoothing is None else FT.SeqLabelSmoothingCrossEntropyLoss(smoothing)
        opt = None
        if optimizer:
            nl = m.get_num_layers()
            asg = FT.LayerDecayValueAssigner([0.75 ** (nl + 1 - i) for i in range(nl + 2)])
            args = types.SimpleNamespace(opt="adamw", lr=1e-2, weight_decay=0.05, opt_eps=1e-8, opt_betas=None)
            make_opt = lambda: FT.create_optimizer(args, m, get_num_layer=asg.get_layer_id, get_layer_scale=asg.get_scale)
            opt = make_opt()
        out = {}
        for i in range(steps):
            if opt is not None:
                opt.zero_grad()
            if lens_on_host is not None:                                # the GRU head: max(lengths) from the host copy, or read back
                m._steps_hint = int(lens.max()) if lens_on_host else None
            logits, loss, dl = _train_step(m, images, targets, lens, crit)
            if opt is not None:
                opt.step()
            out.update({f"step{i}.logits": logits, f"step{i}.loss": loss, f"step{i}.dlogits": dl, f"step{i}.grads": m.flat_grads.clone()})
        out["drop_step"] = m.drop_step
        if opt is not None:
            out["params"] = m.flat_params
            sd = opt.state_dict()
            opt2 = make_opt()
            opt2.load_state_dict(sd)
            out.update({"state_dict.layout": sha([(k, sorted(v)) for k, v in sd["state"].items()] + [sorted(g_.items()) for g_ in sd["param_groups"]]),
                        "reloaded.step": opt2._step, "reloaded.exp_avg": opt2.exp_avg, "reloaded.exp_avg_sq": opt2.exp_avg_sq,
                        "reloaded.groups": sha([sorted((k, v) for k, v in g_.items() if k not in ("params", "names")) for g_ in opt2.param_groups])})
        return out
    return run


def decode(dev, beam, **kw):
    def run():
        m = _tf_model(dev, **kw).eval()
        m._prepare(dev)
        images = _batch(3, m.max_len, [8, 3, 5])[0]
        with torch.no_grad():
            mem = m.memory(m.encoder_features(images))
            if beam:
                return {"memory": mem, "ids": m.beam_search(mem, m.n_mem, beam)}
            probs, maps, toks = m.greedy_decode(mem, m.n_mem)
            return {"memory": mem, "probs": probs, "maps": maps, "tokens": toks}
    return run


def sample(dev):
    def run():
        m = _gru_model(dev, drop_rate=0.1, attn_drop_rate=0.1, drop_path_rate=0.1, drop_seed=3).eval()
        m.drop_step = 7
        images = _batch(3, m.max_len, [8, 3, 5])[0]
        before = (m.drop_rate, m.attn_drop_rate, m.dpr, list(m.dpr), m.drop_step)

        def unchanged():
            return (m.drop_rate is before[0] and m.attn_drop_rate is before[1] and m.dpr is before[2] and list(m.dpr) == before[3]
                    and m.drop_step == before[4])
        probs = m.sample(images)
        out = {"probs": probs, "model_state_unchanged": unchanged()}
        real = ops.patch_embed_fwd

        def boom(*a, **k):
            raise RuntimeError("patch embedding refused")
        ops.patch_embed_fwd = boom
        try:
            m.sample(images)
        except RuntimeError:
            out["model_state_unchanged_after_raise"] = unchanged()
        finally:
            ops.patch_embed_fwd = real
        return out
    return run


def ctc_eval(dev):
    def run():
        m = _ctc_model(dev).eval()
        logits = m.logits(_batch(3, m.max_len, [8, 3, 5])[0])
        out = {"logits": logits}
        for tag, bw in (("greedy", None), ("beam4", 4)):
            out.update({f"{tag}.{k}": v for k, v in zip(("ids", "score", "n"), m.decode(logits, bw))})
        return out
    return run


def layout(dev):
    """Arena offsets and seeded initial weights of the three models: per model one hash over [(name, offset, shape)] and n_flat, one over the
    hashes of every tensor of the initial state_dict() (`--full`: each of them)."""
    from dig_amd.attn_recognizer import AttnRecModelTrain
    from dig_amd.ctc_recognizer import CTCRecModelTrain
    from dig_amd.finetune import RecModelTrain
    small = dict(model="simmim_vit_small_patch4_32x128", nb_classes=97, max_len=25, drop=0.1, attn_drop_rate=0.0, drop_path=0.1)
    ns = lambda **kw: types.SimpleNamespace(**{**small, **kw})
    builds = {"tiny_tf": lambda: _tf_model(dev), "tiny_gru": lambda: _gru_model(dev), "tiny_ctc": lambda: _ctc_model(dev),
              "small_tf_decoder": lambda: RecModelTrain(ns(decoder_name="tf_decoder")),
              "small_corres_small_tf_decoder": lambda: RecModelTrain(ns(decoder_name="corres_small_tf_decoder")),
              "small_tf_decoder_text_cond_vis": lambda: RecModelTrain(ns(decoder_name="tf_decoder", text_cond_vis=True)),
              "small_gru_args": lambda: AttnRecModelTrain(ns()), "small_ctc_args": lambda: CTCRecModelTrain(ns(ctc_beam_width=4))}

    def run():
        out = {}
        for tag, build in builds.items():
            torch.manual_seed(0)
            m = build()
            out[tag + ".offsets"] = sha([(k, s.offset, s.shape) for k, s in m._offsets.items()] + [m.n_flat])
            each = [(k, sha(v)) for k, v in m.state_dict().items()]
            out[tag + ".init"] = sha(each)
            out[tag + ".config"] = sha((m.D, m.H, m.depth, m.F, m.nb_classes, m.max_len, m.drop_rate, m.attn_drop_rate, m.dpr, m.beam_width,
                                        getattr(m, "ctc_beam_width", None)))
            if FULL:
                out.update({f"{tag}.init.{k}": h for k, h in each})
        return out
    return run


def losses(dev):
    def run():
        from dig_amd import finetune as FT
        from dig_amd import recognizer as R
        _, targets, lens = _batch(3, 8, [8, 3, 5])
        g = torch.Generator().manual_seed(9)
        x = torch.randn((3, 8, 97), generator=g) * 2
        out = {"eval.ce": R.SeqCrossEntropyLoss()(x, targets, lens)}
        for tag, crit in (("ce", FT.SeqCrossEntropyLoss()), ("ls0.1", FT.SeqLabelSmoothingCrossEntropyLoss(0.1)), ("ls0", FT.SeqLabelSmoothingCrossEntropyLoss(0.0))):
            xi = x.clone().requires_grad_(True)
            loss = crit(xi, targets, lens)
            (loss * 0.5).backward()
            out.update({f"{tag}.loss": loss.detach(), f"{tag}.grad": xi.grad})
        return out
    return run


HD24, HD48 = dict(d_model=192, n_head=8, d_k=24), dict(d_model=192, n_head=4, d_k=48)      # (the GEMM refuses width 128 with d_k = 24)


def main():
    with backend() as dev:
        case("pretrain_single", pretrain())
        case("pretrain_process_group", pretrain(comm=StubComm()))
        case("pretrain_single_side_plan", pretrain(fwd_mode="side"))
        case("pretrain_single_serial_plan", pretrain(fwd_mode="serial"))
        case("pretrain_single_regular_patchnet", pretrain(patchnet="regular"))
        case("pretrain_process_group_regular_patchnet", pretrain(patchnet="regular", comm=StubComm()))
        case("pretrain_single_conv_patchnet", pretrain(patchnet="conv"))
        case("pretrain_process_group_conv_patchnet", pretrain(patchnet="conv", comm=StubComm()))
        case("pretrain_dis_only", pretrain(pixel=False))
        case("pretrain_dis_only_process_group", pretrain(pixel=False, comm=StubComm()))
        case("pretrain_gen_only", pretrain(moco=False))
        case("pretrain_adamw_two_steps_reload", pretrain(steps=2, optimizer=True))
        case("finetune_tf_2d", finetune(dev, _tf_model))
        case("finetune_tf_1d", finetune(dev, lambda d: _tf_model(d, use_1d_attdec=True)))
        case("finetune_tf_frozen_prefix", finetune(dev, lambda d: (lambda m: (m.fix_encoder_layers(2), m)[1])(_tf_model(d))))
        case("finetune_gru_lens_host", finetune(dev, _gru_model, lens_on_host=True))
        case("finetune_gru_lens_device", finetune(dev, _gru_model, lens_on_host=False))
        case("finetune_tf_drop", finetune(dev, lambda d: _tf_model(d, drop_rate=0.1, attn_drop_rate=0.1, drop_path_rate=0.1, decoder_dropout=0.1, drop_seed=3)))
        case("finetune_gru_drop", finetune(dev, lambda d: _gru_model(d, drop_rate=0.1, attn_drop_rate=0.1, drop_path_rate=0.1, drop_seed=3), lens_on_host=True))
        case("finetune_tf_smoothing", finetune(dev, _tf_model, smoothing=0.1))
        case("finetune_adamw_two_steps_reload", finetune(dev, _tf_model, steps=2, optimizer=True))
        case("finetune_tf_tcv", finetune(dev, lambda d: _tf_model(d, text_cond_vis=True)))
        case("finetune_tf_tcv_nodrop", finetune(dev, lambda d: _tf_model(d, text_cond_vis=True, decoder_dropout=0.0)))
        case("finetune_tf_tcv_1d", finetune(dev, lambda d: _tf_model(d, text_cond_vis=True, use_1d_attdec=True)))
        case("finetune_tf_hd24", finetune(dev, lambda d: _tf_model(d, **HD24)))
        case("finetune_tf_hd48", finetune(dev, lambda d: _tf_model(d, **HD48)))
        case("finetune_ctc", finetune(dev, _ctc_model, ctc=True))
        case("finetune_ctc_drop", finetune(dev, lambda d: _ctc_model(d, drop_rate=0.1, attn_drop_rate=0.1, drop_path_rate=0.1, drop_seed=3), ctc=True))
        case("finetune_ctc_adamw_two_steps_reload", finetune(dev, _ctc_model, steps=2, optimizer=True, ctc=True))
        case("eval_greedy", decode(dev, 0))
        case("eval_beam3", decode(dev, 3))
        case("eval_greedy_tcv", decode(dev, 0, text_cond_vis=True))
        case("eval_beam3_tcv", decode(dev, 3, text_cond_vis=True))
        case("eval_greedy_hd24", decode(dev, 0, **HD24))
        case("gru_sample", sample(dev))
        case("ctc_eval", ctc_eval(dev))
        case("layout", layout(dev))
        case("losses", losses(dev))


if __name__ == "__main__":
    main()
