#!/usr/bin/env python3
"""Time the VGG16 perceptual term, forward + backward, on the GPU: libn3dt's kernels (n3dt.perceptual) in both precisions, and the
same computation composed of torch.nn.functional ops (conv2d on MIOpen) in bf16 and fp32, in one process.  hipEvents over `--iters`
iterations after `--warmup`; prints one JSON object (ms per forward + backward, GFLOP of the convolutions, % of the dense bf16 peak).

Run each invocation under a time limit, e.g.  timeout -k 10 300 python tools/vgg_time.py
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "nerf-3dtalker-code_amd"))

from n3dt import synthetic as syn  # noqa: E402
from n3dt.perceptual import VGGPerceptualLoss, load_vgg16_features, VGG_CONV_CHANNELS  # noqa: E402

BF16_PEAK_TFLOPS = 2500.0  # MI355X dense bf16 MFMA
HS = (224, 224, 112, 112, 56, 56, 56, 28, 28, 28)


def gflop(B):
    mac = sum(9 * ci * co * h * h for (ci, co), h in zip(VGG_CONV_CHANNELS, HS))
    return 2.0 * mac * (2 * B + B) / 1e9  # forward on 2B images, input gradient (same work as a forward) on the B predictions


def torch_term(weights, x, y, dtype):
    mean = torch.tensor([0.485, 0.456, 0.406], device=x.device).view(1, 3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225], device=x.device).view(1, 3, 1, 1)
    x = F.interpolate((torch.nan_to_num(x) - mean) / std, size=(224, 224), mode="bilinear", align_corners=False).to(dtype)
    y = F.interpolate((y - mean) / std, size=(224, 224), mode="bilinear", align_corners=False).to(dtype)
    it = iter(weights)
    loss = 0.0
    for ops in (("c", "c"), ("p", "c", "c"), ("p", "c", "c", "c"), ("p", "c", "c", "c")):
        for op in ops:
            if op == "p":
                x, y = F.max_pool2d(x, 2), F.max_pool2d(y, 2)
            else:
                w, b = next(it)
                x, y = F.relu(F.conv2d(x, w, b, padding=1)), F.relu(F.conv2d(y, w, b, padding=1))
        loss = loss + F.l1_loss(x.float(), y.float())
    return loss


def time_it(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    sd = syn.vgg16_features_state_dict(0)
    weights = load_vgg16_features(sd)
    out = {"bf16_peak_tflops": BF16_PEAK_TFLOPS, "iters": args.iters, "configs": {}}
    for name, B, P in (("config3", 2, 512), ("config4", 4, 256)):
        g = torch.Generator().manual_seed(0)
        merge = torch.rand(B, 3, P, P, generator=g).to(dev)
        gt = torch.rand(B, 3, P, P, generator=g).to(dev)
        mask = torch.ones(B, 1, P, P, device=dev)
        res = {"batch": B, "img_size": P, "gflop": gflop(B)}
        for prec in ("bf16", "fp32"):
            f = VGGPerceptualLoss(sd, precision=prec)
            x = merge.clone().requires_grad_(True)

            def step():
                x.grad = None
                f.masked(x, gt, mask, 1.0).backward()
            ms = time_it(step, args.warmup, args.iters)
            res["n3dt_" + prec] = {"ms": ms, "pct_bf16_peak": 100.0 * res["gflop"] / (ms * 1e-3) / (BF16_PEAK_TFLOPS * 1e3)}
        for dname, dt in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
            wd = [(w.to(dev, dt), b.to(dev, dt)) for w, b in weights]
            x = merge.clone().requires_grad_(True)

            def step_t():
                x.grad = None
                torch_term(wd, x, gt, dt).backward()
            ms = time_it(step_t, args.warmup, args.iters)
            res["miopen_" + dname] = {"ms": ms, "pct_bf16_peak": 100.0 * res["gflop"] / (ms * 1e-3) / (BF16_PEAK_TFLOPS * 1e3)}
        out["configs"][name] = res
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
