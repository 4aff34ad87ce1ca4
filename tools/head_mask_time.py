#!/usr/bin/env python3
"""Time n3dt.HeadMask on the GPU against the same network assembled from torch fp32 modules (MIOpen), in one process.

The torch side is what a user would write without libn3dt: nn.Conv2d and nn.BatchNorm2d modules (eval mode) built from the same
state dict under the class's keys, F.relu, F.max_pool2d, F.interpolate and torch.sigmoid, under torch.no_grad(), restricted -- as
the library's mask path is -- to the 26 convolutions the selected output (pred_res[2]) needs.  `logits` is timed against that
network; `masks` (frames -> head and eye masks: normalisation, network, labels, post-process, all on the device) against the torch
network followed by F.interpolate(bilinear, align_corners=True) and argmax -- the reference's post-process runs in OpenCV on the
host and is not part of the torch side.  `postprocess` alone is timed against tests/head_mask_restatement.postprocess, numpy on
the host, on the device's own labels of the first image.  Both sides' logits are checked against each other before anything is
timed.  Each figure is the median of `--iters` calls (hipEvents around every call, host enqueue cost included) after `--warmup`;
the sides are taken ALTERNATELY, `--pairs` times, and the ratio is formed from the medians over the pairs.  The achieved fraction
of the bf16 MFMA peak is the convolutions' multiply-accumulates (counted from the table, times the three products of the operand
split) over the WHOLE call's time: an end-to-end figure, not a kernel's.  Prints one JSON object; --out writes it to that file too,
--readme README.md rewrites the measured sentence of the README's row.

Run under a time limit, e.g.  timeout -k 10 540 python tools/head_mask_time.py --out profiles/head_mask_time.json --readme README.md
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
sys.path.insert(0, os.path.join(REPO, "tests"))

from n3dt import HeadMask, synthetic as syn  # noqa: E402
from n3dt import head_mask as nh  # noqa: E402

BF16_PEAK_FLOPS = 2.5e15  # dense bf16 MFMA, the device's specification
OUTPUT = 2


def conv_macs(H, W):
    """multiply-accumulates of the 26 convolutions output 2 needs, for ONE image"""
    z = nh.feature_sizes(H, W)
    total = 0.0
    for b, (name, _, cin, cout, k, s, p, kind, _) in enumerate(nh.CONVS):
        if b >= 20 and b not in (nh.AVG, nh.ARM32, nh.ARM32_ATT, nh.HEAD32, nh.OUT32, nh.OUT32 + 1):
            continue
        if kind == nh.SMALL:
            hw = 1
        elif b == 0:
            hw = z[0][0] * z[0][1]
        elif b < 20:
            layer = int(name.split("layer")[1][0])
            hw = z[layer][0] * z[layer][1]
        elif b == nh.ARM32:
            hw = z[4][0] * z[4][1]
        else:
            hw = z[3][0] * z[3][1]
        total += hw * (cout or 19) * cin * k * k
    return total


class TorchParser(torch.nn.Module):
    """the context path up to feat_cp16 and the out32 head, as torch modules under the class's keys"""

    def __init__(self, sd):
        super().__init__()
        self.mods = torch.nn.ModuleDict()
        for conv, bn, cin, cout, k, s, p, _, _ in nh.CONVS:
            m = torch.nn.Conv2d(cin, cout or 19, k, s, p, bias=False)
            m.load_state_dict({"weight": sd[conv + ".weight"]})
            self.mods[conv.replace(".", "/")] = m
            if bn is not None:
                m = torch.nn.BatchNorm2d(cout)
                m.load_state_dict({part: sd["%s.%s" % (bn, part)] for part in nh.BN_PARTS + ("num_batches_tracked",)})
                self.mods[bn.replace(".", "/")] = m

    def m(self, name):
        return self.mods[name.replace(".", "/")]

    def cbr(self, name, x):
        return F.relu(self.m(name + ".bn")(self.m(name + ".conv")(x)))

    def forward(self, x):
        r = "cp.resnet."
        x = F.max_pool2d(F.relu(self.m(r + "bn1")(self.m(r + "conv1")(x))), 3, 2, 1)
        feats = []
        for layer in range(1, 5):
            for b in range(2):
                p = "%slayer%d.%d." % (r, layer, b)
                y = self.m(p + "bn2")(self.m(p + "conv2")(F.relu(self.m(p + "bn1")(self.m(p + "conv1")(x)))))
                if (p + "downsample/0").replace(".", "/") in self.mods:
                    x = self.m(p + "downsample.1")(self.m(p + "downsample.0")(x))
                x = F.relu(x + y)
            feats.append(x)
        f16, f32 = feats[2], feats[3]
        avg = self.cbr("cp.conv_avg", F.avg_pool2d(f32, f32.shape[2:]))
        feat = self.cbr("cp.arm32.conv", f32)
        att = torch.sigmoid(self.m("cp.arm32.bn_atten")(self.m("cp.arm32.conv_atten")(F.avg_pool2d(feat, feat.shape[2:]))))
        cp16 = self.cbr("cp.conv_head32", F.interpolate(feat * att + avg, f16.shape[2:], mode="nearest"))
        return self.m("conv_out32.conv_out")(self.cbr("conv_out32.conv", cp16))


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
        if r["call"] == "postprocess":
            text = "`postprocess` %d x 512^2: %.2f ms vs the numpy restatement on the host %.0f ms (%.0fx)" % (
                r["images"], r["n3dt_us"] / 1e3, r["other_us"] / 1e3, r["other_over_n3dt"])
        else:
            text = "`%s` %d x 512^2: %.2f ms vs torch fp32 %.2f ms (%.2fx, %.1f %% of the bf16 MFMA peak end to end)" % (
                r["call"], r["images"], r["n3dt_us"] / 1e3, r["other_us"] / 1e3, r["other_over_n3dt"], 100 * r["fraction_of_bf16_peak_end_to_end"])
        parts.append("**%s: slower**" % text if r["other_over_n3dt"] < 1.0 else text)
    return "; ".join(parts)


README_BEGIN, README_END = "<!-- head_mask_time -->", "<!-- /head_mask_time -->"


def write_readme(path, rows):
    """replace what stands between the two markers of the README's row with the sentence measured now"""
    text = open(path).read()
    a, b = text.index(README_BEGIN) + len(README_BEGIN), text.index(README_END)
    with open(path, "w") as f:
        f.write(text[:a] + readme_fragment(rows) + text[b:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, nargs="+", default=[1, 16, 128], help="frames of 512 x 512")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--readme", default=None, help="a README file: the measured sentence between its %s markers is replaced" % README_BEGIN)
    args = ap.parse_args()
    assert args.iters >= 20 and args.warmup >= 5, "at least 20 timed calls after 5 warm-ups"
    import head_mask_restatement as hr
    dev = torch.device("cuda:0")
    S = 512
    sd = syn.head_mask_state_dict(hr.WEIGHTS_SEED, 19)
    net = HeadMask(sd, output=OUTPUT, size=S)
    ref = TorchParser(sd).to(dev).eval()
    rows = []
    with torch.no_grad():
        for n in args.images:
            gen = torch.Generator(device=dev).manual_seed(n)
            frames = torch.randint(0, 256, (n, S, S, 3), device=dev, generator=gen, dtype=torch.uint8)
            rgb, x = net.frames(frames)
            a, b = net.logits(x[:2]).double(), ref(x[:2]).double()
            diff = float((a - b).abs().max())
            assert diff <= 1e-2 * float(b.abs().max()), diff
            calls = {
                "logits": (lambda: net.logits(x), lambda: ref(x)),
                "masks": (lambda: net.masks(frames), lambda: F.interpolate(ref(x), (S, S), mode="bilinear", align_corners=True).argmax(1)),
            }
            for what, (mine, other) in calls.items():
                fns = {"n3dt": mine, "torch": other}
                us = {k: [] for k in fns}
                for _ in range(args.pairs):
                    for k, fn in fns.items():
                        us[k].append(round(median_us(fn, args.warmup, args.iters), 2))
                row = {"call": what, "images": n, "max_abs_difference_logits": diff, "us": us}
                row["n3dt_us"], row["other_us"] = statistics.median(us["n3dt"]), statistics.median(us["torch"])
                row["other_over_n3dt"] = round(row["other_us"] / row["n3dt_us"], 3)
                macs = conv_macs(S, S) * n
                row["conv_gflop_algorithmic"] = round(2 * macs / 1e9, 3)
                row["fraction_of_bf16_peak_end_to_end"] = round(3 * 2 * macs / (row["n3dt_us"] * 1e-6) / BF16_PEAK_FLOPS, 5)
                rows.append(row)
            # the post-process alone, on the device's own labels; the host side on the first image, scaled to n
            lab = net.parse(frames)
            head, eye = net.postprocess(lab, rgb)
            t0 = time.perf_counter()
            want = hr.postprocess(lab[0].cpu().numpy(), rgb[0].cpu().numpy())
            host_us = (time.perf_counter() - t0) * 1e6
            assert (head[0].cpu().numpy() == want[0]).all() and (eye[0].cpu().numpy() == want[1]).all()
            us = [round(median_us(lambda: net.postprocess(lab, rgb), args.warmup, args.iters), 2) for _ in range(args.pairs)]
            row = {"call": "postprocess", "images": n, "us": {"n3dt": us, "host_restatement_one_image": round(host_us, 1)},
                   "n3dt_us": statistics.median(us), "other_us": round(host_us * n, 1)}
            row["other_over_n3dt"] = round(row["other_us"] / row["n3dt_us"], 3)
            rows.append(row)
    result = {"iters": args.iters, "warmup": args.warmup, "pairs": args.pairs, "device": torch.cuda.get_device_name(0), "output": OUTPUT,
              "torch_side": "the 26 convolutions of output 2 as torch fp32 modules; for `masks` followed by the bilinear upsample and argmax; "
                            "`postprocess`: the numpy restatement on the host, one image timed and scaled to the batch",
              "frames": "uniform noise: the label maps are fragmented, the union-find's worst case rather than a face", "rows": rows}
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
