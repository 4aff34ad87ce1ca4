#!/usr/bin/env python3
"""Time n3dt.FAN on the GPU against the same network assembled from torch fp32 modules (MIOpen), in one process.

The torch side is what a user would write without libn3dt: nn.Conv2d and nn.BatchNorm2d modules (eval mode) built from the same
state dict under the reference's names, F.relu, F.avg_pool2d, F.interpolate and the coordinate channels concatenated as
AddCoordsTh does, under torch.no_grad().  `forward` is timed at 1, 16 and 128 images; `landmarks` -- the crop in front, the decode
and the tail behind the network -- at 1 and 16 frames of 256 x 256, where the torch side is the network alone on the crops (the
reference's crop, decode and glue run in cv2 / numpy on the host and are not timed).  Both sides' last heat maps are checked
against each other before anything is timed.  Each figure is the median of `--iters` calls (hipEvents around every call, host
enqueue cost included) after `--warmup`; the sides are taken ALTERNATELY, `--pairs` times, and the ratio is formed from the
medians over the pairs.  The achieved fraction of the bf16 MFMA peak is the convolutions' multiply-accumulates (counted from the
table, times the three products of the operand split) over the WHOLE call's time: an end-to-end figure, not a kernel's.  Prints one
JSON object; --out writes it to that file too, --readme README.md rewrites the measured sentence of the README's row.

Run under a time limit, e.g.  timeout -k 10 300 python tools/fan_time.py --out profiles/fan_time.json --readme README.md
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

from n3dt import FAN, synthetic as syn  # noqa: E402
from n3dt.fan import BN_PARTS, HG_BLOCKS, conv_table, coords  # noqa: E402

BF16_PEAK_FLOPS = 2.5e15  # dense bf16 MFMA, the device's specification


def conv_macs(M, N):
    """multiply-accumulates of every convolution for ONE image (true channel counts, the coordinate channels included)"""
    total = 0.0
    for j, row in enumerate(conv_table(M, N)):
        if row is None:
            continue
        name, _, cin, cout, k, _, wc = row
        hw = 128 * 128 if j < 5 else 64 * 64  # the stem's output and conv2 at 128^2
        if j >= 12:
            t = (j - 12) % 47
            if 1 <= t <= 39:  # the hourglass's ConvBlocks: b1_l at 2^(l+2), b2 / b3 / b2_plus at half that
                b = HG_BLOCKS[(t - 1) // 3]
                level = int(b[-1])
                side = (4 << level) if b.startswith("b1_") else (2 << level)
                hw = side * side
        total += hw * cout * (wc if k != 7 else 6) * k * k
    return total


class TorchFAN(torch.nn.Module):
    def __init__(self, sd, M, N):
        super().__init__()
        self.M = M
        self.mods = torch.nn.ModuleDict()
        for key in sd:
            name, part = key.rsplit(".", 1)
            mod = name.replace(".", "/")
            if part != "weight" or mod in self.mods:
                continue
            w = sd[key]
            if w.dim() == 4:
                m = torch.nn.Conv2d(w.shape[1], w.shape[0], w.shape[2], 2 if w.shape[2] == 7 else 1, w.shape[2] // 2, bias=name + ".bias" in sd)
                m.load_state_dict({p: sd["%s.%s" % (name, p)] for p in ("weight", "bias") if "%s.%s" % (name, p) in sd})
            else:
                m = torch.nn.BatchNorm2d(w.shape[0])
                m.load_state_dict({p: sd["%s.%s" % (name, p)] for p in BN_PARTS + ("num_batches_tracked",)})
            self.mods[mod] = m
        self.register_buffer("c256", coords(256)[None])
        self.register_buffer("c64", coords(64)[None])

    def m(self, name):
        return self.mods[name.replace(".", "/")]

    def cb(self, name, x):
        o1 = self.m(name + ".conv1")(F.relu(self.m(name + ".bn1")(x)))
        o2 = self.m(name + ".conv2")(F.relu(self.m(name + ".bn2")(o1)))
        o3 = self.m(name + ".conv3")(F.relu(self.m(name + ".bn3")(o2)))
        if (name + ".downsample.2").replace(".", "/") in self.mods:
            x = self.m(name + ".downsample.2")(F.relu(self.m(name + ".downsample.0")(x)))
        return torch.cat((o1, o2, o3), 1) + x

    def hourglass(self, s, level, x):
        up1 = self.cb("m%d.b1_%d" % (s, level), x)
        low = self.cb("m%d.b2_%d" % (s, level), F.avg_pool2d(x, 2, 2))
        low = self.hourglass(s, level - 1, low) if level > 1 else self.cb("m%d.b2_plus_1" % s, low)
        low = self.cb("m%d.b3_%d" % (s, level), low)
        return up1 + F.interpolate(low, scale_factor=2, mode="nearest")

    def forward(self, x):
        n = x.shape[0]
        x = F.relu(self.m("bn1")(self.m("conv1.conv")(torch.cat((x, self.c256.expand(n, -1, -1, -1)), 1))))
        previous = self.cb("conv4", self.cb("conv3", F.avg_pool2d(self.cb("conv2", x), 2, 2)))
        outs, tmp = [], None
        c64 = self.c64.expand(n, -1, -1, -1)
        for s in range(self.M):
            t = torch.cat((previous, c64), 1)
            if s > 0:
                gate = (torch.clamp(tmp[:, -1:], 0.0, 1.0) > 0.05).float()
                t = torch.cat((t, gate * c64[:, :2]), 1)
            ll = self.cb("top_m_%d" % s, self.hourglass(s, 4, self.m("m%d.coordconv.conv" % s)(t)))
            ll = F.relu(self.m("bn_end%d" % s)(self.m("conv_last%d" % s)(ll)))
            tmp = self.m("l%d" % s)(ll)
            outs.append(tmp)
            if s < self.M - 1:
                previous = previous + self.m("bl%d" % s)(ll) + self.m("al%d" % s)(tmp)
        return outs


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


def readme_fragment(rows):
    """the measured sentence of the README row: one clause per timed call, in bold where n3dt is the slower side"""
    parts = []
    for r in rows:
        text = "`%s` %d x 256^2: %.2f ms vs torch fp32 %.2f ms (%.2fx, %.1f %% of the bf16 MFMA peak end to end)" % (
            r["call"], r["images"], r["n3dt_us"] / 1e3, r["torch_us"] / 1e3, r["torch_over_n3dt"], 100 * r["fraction_of_bf16_peak_end_to_end"])
        parts.append("**%s: slower**" % text if r["torch_over_n3dt"] < 1.0 else text)
    return "; ".join(parts)


README_BEGIN, README_END = "<!-- fan_time -->", "<!-- /fan_time -->"


def write_readme(path, rows):
    """replace what stands between the two markers of the README's row with the sentence measured now"""
    text = open(path).read()
    a, b = text.index(README_BEGIN) + len(README_BEGIN), text.index(README_END)
    with open(path, "w") as f:
        f.write(text[:a] + readme_fragment(rows) + text[b:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--forward", type=int, nargs="+", default=[1, 16, 128], help="images of 256 x 256")
    ap.add_argument("--landmarks", type=int, nargs="+", default=[1, 16], help="frames of 256 x 256")
    ap.add_argument("--modules", type=int, default=4)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--readme", default=None, help="a README file: the measured sentence between its %s markers is replaced" % README_BEGIN)
    args = ap.parse_args()
    assert args.iters >= 20 and args.warmup >= 5, "at least 20 timed calls after 5 warm-ups"
    dev = torch.device("cuda:0")
    M, N = args.modules, 98
    sd = syn.fan_state_dict(5, M, N)
    net = FAN(sd, num_modules=M, num_landmarks=N)
    ref = TorchFAN(sd, M, N).to(dev).eval()
    rows = []
    with torch.no_grad():
        for what, counts in (("forward", args.forward), ("landmarks", args.landmarks)):
            for n in counts:
                gen = torch.Generator(device=dev).manual_seed(n)
                x = torch.rand(n, 3, 256, 256, device=dev, generator=gen)
                if what == "forward":
                    mine = lambda: net.forward(x)  # noqa: E731
                    crops = x
                else:
                    mine = lambda: net.landmarks(x)  # noqa: E731
                    crops = net.crops(x)[0]
                a, b = net.forward(crops)[-1].double(), ref(crops)[-1].double()
                # a gate cell on the threshold may fall differently on the two sides; the median is not moved by it
                diff = float((a - b).abs().median())
                assert diff <= 1e-3, diff
                fns = {what: mine, "torch": lambda: ref(crops)}
                us = {k: [] for k in fns}
                for _ in range(args.pairs):
                    for k, fn in fns.items():
                        us[k].append(round(median_us(fn, args.warmup, args.iters), 2))
                row = {"call": what, "images": n, "num_modules": M, "median_abs_difference_heat": diff, "us": us}
                row["n3dt_us"], row["torch_us"] = statistics.median(us[what]), statistics.median(us["torch"])
                row["torch_over_n3dt"] = round(row["torch_us"] / row["n3dt_us"], 3)
                macs = conv_macs(M, N) * n
                row["conv_gflop_algorithmic"] = round(2 * macs / 1e9, 3)
                row["fraction_of_bf16_peak_end_to_end"] = round(3 * 2 * macs / (row["n3dt_us"] * 1e-6) / BF16_PEAK_FLOPS, 5)
                rows.append(row)
    result = {"iters": args.iters, "warmup": args.warmup, "pairs": args.pairs, "device": torch.cuda.get_device_name(0),
              "torch_side": "the network alone in torch fp32 modules; for `landmarks` on the crops, the crop, decode and tail untimed", "rows": rows}
    text = json.dumps(result, sort_keys=True)
    print(text)
    if args.readme:
        write_readme(args.readme, rows)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
