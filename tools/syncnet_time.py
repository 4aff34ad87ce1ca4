#!/usr/bin/env python3
"""Time n3dt.SyncNet on the GPU against the same network assembled from torch fp32 modules (MIOpen), in one process.

The torch side is what a user would write without libn3dt: per block nn.Conv2d + nn.BatchNorm2d (eval mode) + the residual + ReLU
built from the same state dict and the layer table (n3dt.syncnet.BLOCKS), then F.normalize and the dot product, under
torch.no_grad().  Both sides are checked against each other before anything is timed.  Each figure is the median of `--iters`
calls (hipEvents around every call, host enqueue cost included) after `--warmup`; the two are taken ALTERNATELY, `--pairs`
times, and the ratio is formed from the medians over the pairs.  The achieved fraction of the bf16 MFMA peak is the
convolutions' multiply-accumulates (counted from the table, times the three products of the operand split) over the WHOLE
call's time, so it is an end-to-end figure, not a kernel's.
Prints one JSON object.

Run under a time limit, e.g.  timeout -k 10 300 python tools/syncnet_time.py
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

from n3dt import SyncNet, synthetic as syn  # noqa: E402
from n3dt.syncnet import BLOCKS, FACE_BLOCKS, block_names, block_shapes  # noqa: E402

BF16_PEAK_FLOPS = 2.5e15  # dense bf16 MFMA, the device's specification


def conv_macs():
    """multiply-accumulates of the 31 convolutions for ONE window (true C_in, without the channel padding)"""
    total = 0
    for (cin, cout, (kh, kw), _, _, _), (_, (_, ho, wo)) in zip(BLOCKS, block_shapes()):
        total += ho * wo * cout * cin * kh * kw
    return total


class TorchSyncNet(torch.nn.Module):
    def __init__(self, sd):
        super().__init__()
        self.convs, self.norms = torch.nn.ModuleList(), torch.nn.ModuleList()
        for name, (cin, cout, k, stride, pad, _) in zip(block_names(), BLOCKS):
            conv, bn = torch.nn.Conv2d(cin, cout, k, stride, pad), torch.nn.BatchNorm2d(cout)
            conv.load_state_dict({"weight": sd[name + ".conv_block.0.weight"], "bias": sd[name + ".conv_block.0.bias"]})
            bn.load_state_dict({k2: sd["%s.conv_block.1.%s" % (name, k2)] for k2 in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")})
            self.convs.append(conv)
            self.norms.append(bn)

    def forward(self, mel, faces):
        x = faces
        for b, (conv, bn) in enumerate(zip(self.convs, self.norms)):
            if b == len(FACE_BLOCKS):
                face, x = x, mel
            y = bn(conv(x))
            x = torch.relu(y + x if BLOCKS[b][5] else y)
        a, f = F.normalize(x.flatten(1), p=2, dim=1), F.normalize(face.flatten(1), p=2, dim=1)
        return a, f, (a * f).sum(dim=1)


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
    ap.add_argument("--windows", type=int, nargs="+", default=[1, 16, 128])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=5)
    args = ap.parse_args()
    assert args.iters >= 20 and args.warmup >= 5, "at least 20 timed calls after 5 warm-ups"
    dev = torch.device("cuda:0")
    sd = syn.syncnet_state_dict(5)
    net = SyncNet(sd)
    ref = TorchSyncNet(sd).to(dev).eval()
    rows = []
    with torch.no_grad():
        for n in args.windows:
            gen = torch.Generator(device=dev).manual_seed(n)
            faces = torch.rand(n, 15, 48, 96, device=dev, generator=gen)
            mel = torch.rand(n, 1, 80, 16, device=dev, generator=gen) * 8.0 - 4.0
            got, want = net._run(mel, faces), ref(mel, faces)
            diff = max(float((g.double() - w.double()).abs().max()) for g, w in zip(got, want))
            assert diff <= 1e-4, diff  # fp32 torch modules against the split-bf16 kernels, unit-norm embeddings
            fns = {"n3dt": lambda: net._run(mel, faces), "torch": lambda: ref(mel, faces)}
            us = {k: [] for k in fns}
            for _ in range(args.pairs):
                for k, fn in fns.items():
                    us[k].append(round(median_us(fn, args.warmup, args.iters), 2))
            row = {"windows": n, "max_abs_difference": diff, "us": us, "n3dt_us": statistics.median(us["n3dt"]), "torch_us": statistics.median(us["torch"])}
            row["torch_over_n3dt"] = round(row["torch_us"] / row["n3dt_us"], 3)
            macs = conv_macs() * n
            row["conv_gflop_algorithmic"] = round(2 * macs / 1e9, 3)
            row["fraction_of_bf16_peak_end_to_end"] = round(3 * 2 * macs / (row["n3dt_us"] * 1e-6) / BF16_PEAK_FLOPS, 5)
            rows.append(row)
    print(json.dumps({"iters": args.iters, "warmup": args.warmup, "pairs": args.pairs, "gflop_per_window": round(2 * conv_macs() / 1e9, 3), "rows": rows},
                     sort_keys=True))


if __name__ == "__main__":
    main()
