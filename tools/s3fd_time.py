#!/usr/bin/env python3
"""Time n3dt.S3FD on the GPU against the same network assembled from torch fp32 modules (MIOpen), in one process.

The torch side is what a user would write without libn3dt: nn.Conv2d modules built from the same state dict and the layer table
(n3dt.s3fd.CONVS), F.relu, F.max_pool2d, the L2Norm formula, the twelve head convolutions and the max-out, under torch.no_grad();
it stops at the twelve head maps (the reference's tail runs in numpy on the host and is not timed).  `detect` goes on through
scores, decode and NMS, `boxes` through pads and smoothing as well.  Both sides' head maps are checked against each other before
anything is timed.  Each figure is the median of `--iters` calls (hipEvents around every call, host enqueue cost included) after
`--warmup`; the sides are taken ALTERNATELY, `--pairs` times, and the ratio is formed from the medians over the pairs.  The
achieved fraction of the bf16 MFMA peak is the convolutions' multiply-accumulates (counted from the table, heads included, times
the three products of the operand split) over the WHOLE detect call's time, so it is an end-to-end figure, not a kernel's.
Prints one JSON object.

Run under a time limit, e.g.  timeout -k 10 300 python tools/s3fd_time.py
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

from n3dt import S3FD, synthetic as syn  # noqa: E402
from n3dt.s3fd import CONVS, LEVEL_C, LEVEL_CONF, LEVEL_SOURCES, MEANS, NORMS, conv_out  # noqa: E402

BF16_PEAK_FLOPS = 2.5e15  # dense bf16 MFMA, the device's specification


def conv_macs(H, W):
    """multiply-accumulates of the 19 convolutions and 12 heads for ONE H x W frame (true channel counts)"""
    total, level = 0.0, 0
    for _, cin, cout, k, s, p, pool, lv in CONVS:
        H, W = conv_out(H, k, s, p), conv_out(W, k, s, p)
        total += H * W * cout * cin * k * k
        if lv:
            total += H * W * (LEVEL_CONF[level] + 4) * LEVEL_C[level] * 9
            level += 1
        if pool:
            H, W = H // 2, W // 2
    return total


class TorchS3FD(torch.nn.Module):
    def __init__(self, sd):
        super().__init__()
        self.convs = torch.nn.ModuleList()
        for name, cin, cout, k, s, p, _, _ in CONVS:
            conv = torch.nn.Conv2d(cin, cout, k, s, p)
            conv.load_state_dict({"weight": sd[name + ".weight"], "bias": sd[name + ".bias"]})
            self.convs.append(conv)
        self.heads = torch.nn.ModuleList()
        for src, c, conf in zip(LEVEL_SOURCES, LEVEL_C, LEVEL_CONF):
            for part, n in (("conf", conf), ("loc", 4)):
                conv = torch.nn.Conv2d(c, n, 3, 1, 1)
                conv.load_state_dict({"weight": sd["%s_mbox_%s.weight" % (src, part)], "bias": sd["%s_mbox_%s.bias" % (src, part)]})
                self.heads.append(conv)
        self.norm_weights = torch.nn.ParameterList([torch.nn.Parameter(sd[n + ".weight"].clone()) for n in NORMS])

    def forward(self, x):
        out = []
        for c, conv in enumerate(self.convs):
            x = F.relu(conv(x))
            level = CONVS[c][7]
            if level:
                src = x
                if level <= 3:
                    src = x / (x.pow(2).sum(dim=1, keepdim=True).sqrt() + 1e-10) * self.norm_weights[level - 1].view(1, -1, 1, 1)
                out += [self.heads[2 * level - 2](src), self.heads[2 * level - 1](src)]
            if CONVS[c][6]:
                x = F.max_pool2d(x, 2, 2)
        chunk = torch.chunk(out[0], 4, 1)
        out[0] = torch.cat([torch.max(torch.max(chunk[0], chunk[1]), chunk[2]), chunk[3]], dim=1)
        return out


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
    ap.add_argument("--shapes", type=int, nargs="+", default=[1, 256, 1, 512, 16, 512], help="pairs: frames, side")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=5)
    args = ap.parse_args()
    assert args.iters >= 20 and args.warmup >= 5, "at least 20 timed calls after 5 warm-ups"
    dev = torch.device("cuda:0")
    sd = syn.s3fd_state_dict(5)
    det = S3FD(sd)
    ref = TorchS3FD(sd).to(dev).eval()
    mean = torch.tensor(MEANS, device=dev)[None, :, None, None]
    rows = []
    with torch.no_grad():
        for n, side in zip(args.shapes[0::2], args.shapes[1::2]):
            gen = torch.Generator(device=dev).manual_seed(n + side)
            frames = torch.rand(n, 3, side, side, device=dev, generator=gen)
            x = 255.0 * frames - mean
            diff = max(float((a.double() - b.double()).abs().max()) for a, b in zip(det.forward(x), ref(x)))
            assert diff <= 1e-2, diff  # fp32 torch modules against the split-bf16 kernels, logits of O(10)
            fns = {"detect": lambda: det.detect(frames), "boxes": lambda: det.boxes(frames, strict=False), "heads": lambda: det.forward(x),
                   "torch": lambda: ref(x)}
            us = {k: [] for k in fns}
            for _ in range(args.pairs):
                for k, fn in fns.items():
                    us[k].append(round(median_us(fn, args.warmup, args.iters), 2))
            row = {"frames": n, "side": side, "max_abs_difference_heads": diff, "us": us}
            for k in fns:
                row[k + "_us"] = statistics.median(us[k])
            row["torch_over_detect"] = round(row["torch_us"] / row["detect_us"], 3)
            macs = conv_macs(side, side) * n
            row["conv_gflop_algorithmic"] = round(2 * macs / 1e9, 3)
            row["fraction_of_bf16_peak_end_to_end"] = round(3 * 2 * macs / (row["detect_us"] * 1e-6) / BF16_PEAK_FLOPS, 5)
            rows.append(row)
    print(json.dumps({"iters": args.iters, "warmup": args.warmup, "pairs": args.pairs, "rows": rows}, sort_keys=True))


if __name__ == "__main__":
    main()
