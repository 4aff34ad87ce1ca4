#!/usr/bin/env python3
"""Time the Adam-only part of a training step on the GPU: n3dt.FlatAdam (one libn3dt launch over the arenas) against
torch.optim.Adam(fused=True) on the same parameters, in one process.  Two parameter sets: (a) a config-3 HeadNeRFNet (lr 1e-4),
(b) the Audio2style FlatBucket stand-in (21.5 M floats, lr 1e-7, betas (0.5, 0.999)).  Each optimizer is timed eagerly (hipEvents
around every step() call: host enqueue cost included, as a training loop pays it) and inside a captured graph (events around
replay()); the figure is the MEDIAN of `--iters` steps after `--warmup`.  GB/s counts the 4 reads + 3 writes of 4 bytes per element
the update needs.  Then one config-3 training step (B = 2, bf16 renderer, FlatBucket stand-in, two optimizers) with torch's fused
Adam and with FlatAdam, alternating.  Prints one JSON object.

The guarded step (FlatAdam(max_grad_norm=1.0, skip_nonfinite=True): the norm kernel + the Adam kernel, 32 bytes per element) is a
row of its own next to the unguarded one, and "guard_pairs" times the two ALTERNATELY in this run -- `--pairs` times eager, then
`--pairs` times as graph replays -- which is the comparison to quote: guarded / unguarded of the same build, same process.
--against-lib PATH: also time the UNGUARDED n3dt_flat_adam_step of another build of libn3dt.so (e.g. the parent commit's) against
this build's on the same tables, alternating pairs, eager and graph ("lib_pairs").

--trace-steps N: nothing is timed; N eager steps of each optimizer on each set and nothing else, for a
`rocprofv3 --kernel-trace --stats -- python tools/adam_time.py --trace-steps N` run (launches per step = Calls / N).

Run each invocation under a time limit, e.g.  timeout -k 10 300 python tools/adam_time.py
"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "nerf-3dtalker-code_amd"))

from n3dt import BaseOptions, FlatAdam, HeadNeRFNet, parallel, synthetic as syn  # noqa: E402
from n3dt.train import fused_data_losses, disk_mask  # noqa: E402

CONFIG3 = {"featmap_size": 64, "featmap_nc": 256, "pred_img_size": 512, "num_sample_coarse": 64}
SETS = {"headnerf_config3": dict(lr=1e-4, betas=(0.9, 0.999)), "audio2style_flatbucket": dict(lr=1e-7, betas=(0.5, 0.999))}


def make_module(name, dev):
    if name == "headnerf_config3":
        net = HeadNeRFNet(BaseOptions(CONFIG3), False, False, train_precision="bf16").to(dev)
        net.load_state_dict(syn.make_state_dict(BaseOptions(CONFIG3), seed=0, bg_noise=0.1), strict=True)
        return net
    return parallel.FlatBucket().to(dev)


GUARD = dict(max_grad_norm=1.0, skip_nonfinite=True)


def make_optimizer(kind, name, mod, capturable=False):
    if kind == "flat":
        return FlatAdam(mod.parameters(), modules=[mod], **SETS[name])
    if kind == "flat_guarded":
        return FlatAdam(mod.parameters(), modules=[mod], **GUARD, **SETS[name])
    return torch.optim.Adam(mod.parameters(), fused=True, capturable=capturable, **SETS[name])


def fill_grads(mod, kind):
    """Gradients where each optimizer expects them: the arena slices for FlatAdam, ordinary tensors for torch."""
    gen = torch.Generator(device="cuda").manual_seed(1)
    for p in mod.parameters():
        p.grad = torch.randn(p.shape, device=p.device, generator=gen) * 1e-3
    if kind.startswith("flat"):
        arena = mod.grad_arena() if hasattr(mod, "grad_arena") else parallel._arena_for(list(mod.parameters()))
        arena.adopt()


def median_us(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev) * 1e3


def time_set(name, dev, warmup, iters):
    out = {}
    for kind in ("flat", "flat_guarded", "torch_fused"):
        mod = make_module(name, dev)
        numel = sum(p.numel() for p in mod.parameters() if p.requires_grad)
        fill_grads(mod, kind)
        opt = make_optimizer(kind, name, mod)
        eager = median_us(opt.step, warmup, iters)
        mod = make_module(name, dev)
        fill_grads(mod, kind)
        opt = make_optimizer(kind, name, mod, capturable=True)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                opt.step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            opt.step()
        graphed = median_us(graph.replay, warmup, iters)
        nbytes = (32.0 if kind == "flat_guarded" else 28.0) * numel
        out[kind] = {"eager_us": round(eager, 2), "graph_us": round(graphed, 2), "eager_GBps": round(nbytes / eager / 1e3, 1),
                     "graph_GBps": round(nbytes / graphed / 1e3, 1)}
        out["numel"], out["tensors"] = numel, sum(1 for p in mod.parameters() if p.requires_grad)
    return out


def _graph_of(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph


def _alternate(fns, warmup, iters, pairs):
    """{label: [median us] * pairs}, the labels taken in turn inside every pair."""
    out = {k: [] for k in fns}
    for _ in range(pairs):
        for k, fn in fns.items():
            out[k].append(round(median_us(fn, warmup, iters), 2))
    return out


def _ratio(d, num, den):
    return round(statistics.median(d[num]) / statistics.median(d[den]), 4)


def guard_pairs(name, dev, warmup, iters, pairs):
    """The guarded step against the unguarded one of this build, alternating, eager and as graph replays."""
    opts = {}
    for kind in ("flat", "flat_guarded"):
        mod = make_module(name, dev)
        fill_grads(mod, kind)
        opts[kind] = (make_optimizer(kind, name, mod), mod)
    eager = _alternate({k: o.step for k, (o, _) in opts.items()}, warmup, iters, pairs)
    graphs = {k: _graph_of(o.step) for k, (o, _) in opts.items()}
    graph = _alternate({k: g.replay for k, g in graphs.items()}, warmup, iters, pairs)
    skipped = int(opts["flat_guarded"][0].skipped_steps)
    assert skipped == 0, "the timed guarded steps must be real steps, %d were skipped" % skipped
    return {"eager_us": eager, "graph_us": graph, "eager_guarded_over_unguarded": _ratio(eager, "flat_guarded", "flat"),
            "graph_guarded_over_unguarded": _ratio(graph, "flat_guarded", "flat")}


def lib_pairs(name, dev, other_path, warmup, iters, pairs):
    """n3dt_flat_adam_step (unguarded) of this build and of the libn3dt.so at `other_path`, on one optimizer's tables."""
    import ctypes
    from n3dt import _lib
    mod = make_module(name, dev)
    fill_grads(mod, "flat")
    opt = make_optimizer("flat", name, mod)
    opt.step()
    vp, ci = ctypes.c_void_p, ctypes.c_int
    other = ctypes.CDLL(other_path)
    other.n3dt_flat_adam_step.restype = ci
    other.n3dt_flat_adam_step.argtypes = [vp, vp, ci, vp, ci, vp, vp]

    def call(L):
        def fn():
            s = vp(torch.cuda.current_stream(dev).cuda_stream)
            rc = L.n3dt_flat_adam_step(opt._tensor_dev.data_ptr(), opt._chunk_dev.data_ptr(), opt._n_chunks, opt._group_dev.data_ptr(),
                                       len(opt.param_groups), opt._counter.data_ptr(), s)
            assert rc == 0
        return fn
    fns = {"this": call(_lib.lib()), "other": call(other)}
    eager = _alternate(fns, warmup, iters, pairs)
    graphs = {k: _graph_of(f) for k, f in fns.items()}
    graph = _alternate({k: g.replay for k, g in graphs.items()}, warmup, iters, pairs)
    return {"eager_us": eager, "graph_us": graph, "eager_this_over_other": _ratio(eager, "this", "other"),
            "graph_this_over_other": _ratio(graph, "this", "other")}


def train_step_ms(dev, kind, warmup, iters):
    opt = BaseOptions(CONFIG3)
    B = 2
    d = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in syn.frame_inputs(opt, B).items()}
    net = make_module("headnerf_config3", dev)
    enc = make_module("audio2style_flatbucket", dev)
    o1 = make_optimizer(kind, "headnerf_config3", net)
    o2 = make_optimizer(kind, "audio2style_flatbucket", enc)
    gt = torch.full((B, 3, 512, 512), 0.5, device=dev)
    mask = disk_mask(B, 512).to(dev)
    # the stand-in's gradient: one fill per step either way -- into its arena slice for FlatAdam (where Audio2style's backward
    # leaves it), into a tensor of its own for torch
    arena = parallel._arena_for(list(enc.parameters())) if kind == "flat" else None

    def fill_enc():
        if arena is None:
            return enc.fill_grad(1e-3)
        enc.flat.grad = arena.view(0)
        enc.flat.grad.fill_(1e-3)

    def step():
        out = net("train", d["batch_xy"], d["batch_uv"], d["audiostyle"], None, d["shape_code"], d["appea_code"], d["batch_Rmats"],
                  d["batch_Tvecs"], d["batch_inv_inmats"])
        t = fused_data_losses(out["coarse_dict"], gt, mask)
        o1.zero_grad()
        o2.zero_grad()
        t["total_loss"].backward()
        fill_enc()
        o1.step()
        o2.step()
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        step()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def trace(dev, steps):
    for name in SETS:
        for kind in ("flat", "flat_guarded", "torch_fused"):
            mod = make_module(name, dev)
            fill_grads(mod, kind)
            opt = make_optimizer(kind, name, mod)
            for _ in range(steps):
                opt.step()
    torch.cuda.synchronize()
    print(json.dumps({"trace_steps": steps, "sets": list(SETS), "optimizers": ["flat", "flat_guarded", "torch_fused"]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--step-iters", type=int, default=20)
    ap.add_argument("--trace-steps", type=int, default=0)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--against-lib", default=None)
    ap.add_argument("--skip-train-step", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    if args.trace_steps:
        return trace(dev, args.trace_steps)
    out = {"iters": args.iters, "warmup": args.warmup, "pairs": args.pairs, "bytes_per_element": 28, "bytes_per_element_guarded": 32}
    for name in SETS:
        out[name] = time_set(name, dev, args.warmup, args.iters)
        out[name]["guard_pairs"] = guard_pairs(name, dev, args.warmup, args.iters, args.pairs)
        if args.against_lib:
            out[name]["lib_pairs"] = lib_pairs(name, dev, args.against_lib, args.warmup, args.iters, args.pairs)
    if args.skip_train_step:
        print(json.dumps(out, sort_keys=True))
        return
    runs = {"torch_fused": [], "flat": []}
    for _ in range(2):
        for kind in ("torch_fused", "flat"):
            runs[kind].append(round(train_step_ms(dev, kind, 3, args.step_iters), 4))
    out["config3_train_step_ms"] = runs
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
