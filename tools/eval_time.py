#!/usr/bin/env python3
"""Time n3dt.image_metrics on the GPU against a torch-on-device formulation of the same arithmetic, in one process.

The torch side quantises and grey-converts with integer tensor ops, forms the five maps X, Y, X^2, Y^2, XY in float64, takes
their 7x7 window means with avg_pool2d (stride 1, no padding: exactly the valid windows) and evaluates S, its mean and the PSNR
with element-wise kernels -- what a user would write without libn3dt.  Both sides are checked against each other before anything
is timed.  Each figure is the median of `--iters` calls (hipEvents around every call, host enqueue cost included) after
`--warmup`; the two are taken ALTERNATELY, `--pairs` times, and the ratio is formed from the medians over the pairs.
Prints one JSON object.

Run under a time limit, e.g.  timeout -k 10 300 python tools/eval_time.py
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "nerf-3dtalker-code_amd"))

from n3dt import image_metrics  # noqa: E402

C1, C2 = (0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2


def torch_metrics(pred, gt):
    def u8(x):
        return torch.nan_to_num(x * 255.0, nan=0.0).clamp(0.0, 255.0).to(torch.uint8).to(torch.int32)

    def grey(q):
        return ((q[:, 0] * 3735 + q[:, 1] * 19235 + q[:, 2] * 9798 + 16384) >> 15).to(torch.float64).unsqueeze(1)
    qa, qb = u8(pred), u8(gt)
    x, y = grey(qa), grey(qb)
    ux, uy, uxx, uyy, uxy = (F.avg_pool2d(m, 7, stride=1) for m in (x, y, x * x, y * y, x * y))
    k = 49.0 / 48.0
    vx, vy, vxy = k * (uxx - ux * ux), k * (uyy - uy * uy), k * (uxy - ux * uy)
    s = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
    d = (qa - qb).to(torch.float64)
    mse = (d * d).mean(dim=(1, 2, 3))
    return {"SSIM": s.mean(dim=(1, 2, 3)), "PSNR": 20.0 * torch.log10(255.0 / (mse.sqrt() + 2.220446049250313e-16))}


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=5)
    args = ap.parse_args()
    assert args.iters >= 20 and args.warmup >= 5, "at least 20 timed calls after 5 warm-ups"
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    pred = torch.rand(args.batch, 3, args.size, args.size, device=dev, generator=gen)
    gt = (pred + 0.05 * torch.randn(pred.shape, device=dev, generator=gen)).clamp(0.0, 1.0)
    a, b = image_metrics(pred, gt), torch_metrics(pred, gt)
    diff = {k: float((a[k] - b[k]).abs().max()) for k in a}
    assert max(diff.values()) <= 1e-9, diff
    fns = {"n3dt": lambda: image_metrics(pred, gt), "torch": lambda: torch_metrics(pred, gt)}
    us = {k: [] for k in fns}
    for _ in range(args.pairs):
        for k, fn in fns.items():
            us[k].append(round(median_us(fn, args.warmup, args.iters), 2))
    out = {"batch": args.batch, "size": args.size, "iters": args.iters, "warmup": args.warmup, "pairs": args.pairs,
           "max_abs_difference": diff, "us": us, "n3dt_us": statistics.median(us["n3dt"]), "torch_us": statistics.median(us["torch"])}
    out["torch_over_n3dt"] = round(out["torch_us"] / out["n3dt_us"], 3)
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
