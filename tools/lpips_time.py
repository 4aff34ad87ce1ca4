#!/usr/bin/env python3
"""Time n3dt.LPIPS on the GPU against the same arithmetic in torch ops on the device, in one process.

The torch side quantises with tensor ops, performs the reference's reshape of the HWC bytes on the device, scales, and runs
AlexNet's five convolutions and two pools with fp32 F.conv2d / F.max_pool2d (MIOpen) and the distance with element-wise kernels
in fp32 (libn3dt's distance stage is float64, so the two are the same computation, not the same arithmetic) -- what a user would
write without libn3dt.  Both sides are checked against each other before anything is timed.  Each
figure is the median of `--iters` calls (hipEvents around every call, host enqueue cost included) after `--warmup`; the two are
taken ALTERNATELY, `--pairs` times, and the ratio is formed from the medians over the pairs.  The achieved fraction of the bf16
MFMA peak is the convolutions' multiply-accumulates (counted from the shapes, times the three products of the operand split) over
the WHOLE call's time, so it is an end-to-end figure, not a kernel's.
With --validate it also times train.validate() per batch with and without lpips= at the default geometry (32 -> 256 x 256).
Prints one JSON object.

Run under a time limit, e.g.  timeout -k 10 300 python tools/lpips_time.py
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "nerf-3dtalker-code_amd"))

from n3dt import LPIPS, synthetic as syn  # noqa: E402
from n3dt.eval_utils import ALEXNET_CONVS as CONVS  # noqa: E402

BF16_PEAK_FLOPS = 2.5e15  # dense bf16 MFMA, the device's specification


def conv_macs(size):
    """multiply-accumulates of the five convolutions for ONE image of size x size"""
    total, n = 0, size
    for layer, (_, cin, cout, k, stride, pad) in enumerate(CONVS):
        if layer in (1, 2):
            n = (n - 3) // 2 + 1
        n = (n + 2 * pad - k) // stride + 1
        total += n * n * cout * cin * k * k
    return total


def torch_lpips(sd, pred, gt):
    B, _, H, W = pred.shape
    x = torch.cat([pred, gt])
    q = torch.nan_to_num(x * 255.0, nan=0.0).clamp(0.0, 255.0).to(torch.uint8)
    x = q.permute(0, 2, 3, 1).contiguous().reshape(2 * B, 3, H, W).float()  # the reference's reshape, not a transpose
    shift = torch.tensor([-0.030, -0.088, -0.188], device=x.device).view(1, 3, 1, 1)
    scale = torch.tensor([0.458, 0.448, 0.450], device=x.device).view(1, 3, 1, 1)
    x = (x - shift) / scale
    total = 0.0
    for layer, (idx, _, _, _, stride, pad) in enumerate(CONVS):
        if layer in (1, 2):
            x = F.max_pool2d(x, 3, 2)
        x = torch.relu(F.conv2d(x, sd["features.%d.weight" % idx], sd["features.%d.bias" % idx], stride=stride, padding=pad))
        n = x / (x.square().sum(dim=1, keepdim=True).sqrt() + 1e-10)
        d = ((n[:B] - n[B:]).square() * sd["lin%d.model.1.weight" % layer]).sum(dim=1)
        total = total + d.mean(dim=(1, 2))
    return total


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


def time_validate(lp, dev, batches_n, repeats):
    from n3dt import BaseOptions, HeadNeRFNet, validate
    opt = BaseOptions()
    net = HeadNeRFNet(opt, include_vd=False, hier_sampling=False).to(dev)
    net.load_state_dict(syn.make_state_dict(opt, seed=0, bg_noise=0.1), strict=True)
    batches = []
    for i in range(batches_n):
        b = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in syn.frame_inputs(opt, 1, first_frame=i).items()}
        gt, mask = syn.sharp_target(1, opt.pred_img_size, seed=4321 + i)
        b["gt_rgb"], b["mask"] = gt.to(dev), mask.to(dev)
        batches.append(b)
    ms = {"without": [], "with_lpips": []}
    for r in range(repeats + 2):
        for key, kw in (("without", {}), ("with_lpips", {"lpips": lp})):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = validate(net, batches, **kw)  # ends in its one synchronisation
            if r >= 2:  # two warm-up rounds
                ms[key].append((time.perf_counter() - t0) * 1e3 / batches_n)
    return {"pred_img_size": opt.pred_img_size, "batches": batches_n, "images_per_batch": 1, "repeats": repeats, "LPIPS": res["LPIPS"],
            "ms_per_batch": {k: round(statistics.median(v), 4) for k, v in ms.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--validate", action="store_true")
    args = ap.parse_args()
    assert args.iters >= 20 and args.warmup >= 5, "at least 20 timed calls after 5 warm-ups"
    dev = torch.device("cuda:0")
    sd = syn.lpips_alex_state_dict(5)
    lp = LPIPS(sd)
    dsd = {k: v.to(dev) for k, v in sd.items()}
    rows = []
    for batch in args.batches:
        gen = torch.Generator(device=dev).manual_seed(batch)
        pred = torch.rand(batch, 3, args.size, args.size, device=dev, generator=gen)
        gt = (pred.flip(-1) * 0.7 + 0.15 + 0.05 * torch.randn(pred.shape, device=dev, generator=gen)).clamp(0.0, 1.0)
        a, b = lp(pred, gt), torch_lpips(dsd, pred, gt)
        rel = float(((a - b.double()) / a).abs().max())
        assert rel <= 1e-4, rel  # fp32 torch ops against the split-bf16 kernels
        fns = {"n3dt": lambda: lp(pred, gt), "torch": lambda: torch_lpips(dsd, pred, gt)}
        us = {k: [] for k in fns}
        for _ in range(args.pairs):
            for k, fn in fns.items():
                us[k].append(round(median_us(fn, args.warmup, args.iters), 2))
        row = {"batch": batch, "size": args.size, "max_relative_difference": rel, "us": us,
               "n3dt_us": statistics.median(us["n3dt"]), "torch_us": statistics.median(us["torch"])}
        row["torch_over_n3dt"] = round(row["torch_us"] / row["n3dt_us"], 3)
        macs = conv_macs(args.size) * 2 * batch
        row["conv_gmac_algorithmic"] = round(macs / 1e9, 3)
        row["fraction_of_bf16_peak_end_to_end"] = round(3 * 2 * macs / (row["n3dt_us"] * 1e-6) / BF16_PEAK_FLOPS, 5)
        rows.append(row)
    out = {"iters": args.iters, "warmup": args.warmup, "pairs": args.pairs, "rows": rows}
    if args.validate:
        out["validate"] = time_validate(lp, dev, 4, 10)
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
