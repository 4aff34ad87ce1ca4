#!/usr/bin/env python3
"""Time n3dt.FaceRecon on the GPU against the same ResNet-50 assembled from torch fp32 modules (MIOpen), in one process.

The torch side is what a user would write without libn3dt: nn.Conv2d and nn.BatchNorm2d modules (eval mode) built from the same
state dict and the layer table (n3dt.face_recon.CONVS), F.relu, F.max_pool2d, the mean and the seven final layers as one linear
map, under torch.no_grad().  `forward` is timed at 1, 16 and 128 images of 224 x 224 against it; `expressions` -- the aligner in
front of the network -- at 1 and 16 frames of 256 x 256, where the torch side is the network alone on 224 x 224 crops (the
reference's aligner runs in PIL on the host and is not timed).  Both sides' coefficients are checked against each other before
anything is timed.  Each figure is the median of `--iters` calls (hipEvents around every call, host enqueue cost included) after
`--warmup`; the sides are taken ALTERNATELY, `--pairs` times, and the ratio is formed from the medians over the pairs.  The achieved
fraction of the bf16 MFMA peak is the convolutions' multiply-accumulates (counted from the table, times the three products of the
operand split) over the WHOLE call's time, so it is an end-to-end figure, not a kernel's.  Prints one JSON object; --out writes it to
that file too, --readme README.md rewrites the measured sentence of the README's row (between its two markers) from it.

Run under a time limit, e.g.  timeout -k 10 300 python tools/face_recon_time.py --out profiles/face_recon_time.json --readme README.md
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

from n3dt import FaceRecon, synthetic as syn  # noqa: E402
from n3dt.face_recon import BN_PARTS, CONVS, FEAT, HEAD_COLS, N_CONVS, conv_out  # noqa: E402

BF16_PEAK_FLOPS = 2.5e15  # dense bf16 MFMA, the device's specification


def conv_macs(H, W):
    """multiply-accumulates of the 53 convolutions and the head for ONE H x W image (true channel counts)"""
    total = 0.0
    h, w = conv_out(H, 7, 2, 3), conv_out(W, 7, 2, 3)
    total += h * w * 64 * 147
    h, w = conv_out(h, 3, 2, 1), conv_out(w, 3, 2, 1)
    b = 1
    while b < N_CONVS:
        down = b + 3 < N_CONVS and CONVS[b + 3][7] == 4
        s = CONVS[b + 1][5]
        ho, wo = conv_out(h, 3, s, 1), conv_out(w, 3, s, 1)
        total += h * w * CONVS[b][2] * CONVS[b][3]
        total += ho * wo * CONVS[b + 1][2] * CONVS[b + 1][3] * 9
        total += ho * wo * CONVS[b + 2][2] * CONVS[b + 2][3]
        if down:
            total += ho * wo * CONVS[b + 3][2] * CONVS[b + 3][3]
        h, w = ho, wo
        b += 4 if down else 3
    return total + FEAT * sum(HEAD_COLS)


class TorchFaceRecon(torch.nn.Module):
    def __init__(self, sd):
        super().__init__()
        self.convs, self.bns = torch.nn.ModuleList(), torch.nn.ModuleList()
        for conv, bn, cin, cout, k, s, p, _, _ in CONVS:
            c = torch.nn.Conv2d(cin, cout, k, s, p, bias=False)
            c.load_state_dict({"weight": sd[conv + ".weight"]})
            n = torch.nn.BatchNorm2d(cout)
            n.load_state_dict({part: sd["%s.%s" % (bn, part)] for part in BN_PARTS + ("num_batches_tracked",)})
            self.convs.append(c)
            self.bns.append(n)
        self.head = torch.nn.Linear(FEAT, sum(HEAD_COLS))
        self.head.load_state_dict({"weight": torch.cat([sd["final_layers.%d.weight" % i].reshape(c, FEAT) for i, c in enumerate(HEAD_COLS)]),
                                   "bias": torch.cat([sd["final_layers.%d.bias" % i] for i in range(len(HEAD_COLS))])})

    def unit(self, b, x):
        return self.bns[b](self.convs[b](x))

    def forward(self, x):
        x = F.max_pool2d(F.relu(self.unit(0, x)), 3, 2, 1)
        b = 1
        while b < N_CONVS:
            down = b + 3 < N_CONVS and CONVS[b + 3][7] == 4
            y = F.relu(self.unit(b + 1, F.relu(self.unit(b, x))))
            x = F.relu(self.unit(b + 2, y) + (self.unit(b + 3, x) if down else x))
            b += 4 if down else 3
        return self.head(x.mean(dim=(2, 3)))


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
        text = "`%s` %d x %d^2: %.2f ms vs torch fp32 %.2f ms (%.2fx, %.1f %% of the bf16 MFMA peak end to end)" % (
            r["call"], r["images"], r["side"], r["n3dt_us"] / 1e3, r["torch_us"] / 1e3, r["torch_over_n3dt"], 100 * r["fraction_of_bf16_peak_end_to_end"])
        parts.append("**%s: slower**" % text if r["torch_over_n3dt"] < 1.0 else text)
    return "; ".join(parts)


README_BEGIN, README_END = "<!-- face_recon_time -->", "<!-- /face_recon_time -->"


def write_readme(path, rows):
    """replace what stands between the two markers of the README's row with the sentence measured now"""
    text = open(path).read()
    a, b = text.index(README_BEGIN) + len(README_BEGIN), text.index(README_END)
    with open(path, "w") as f:
        f.write(text[:a] + readme_fragment(rows) + text[b:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--forward", type=int, nargs="+", default=[1, 16, 128], help="images of 224 x 224")
    ap.add_argument("--expressions", type=int, nargs="+", default=[1, 16], help="frames of 256 x 256")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--readme", default=None, help="a README file: the measured sentence between its %s markers is replaced" % README_BEGIN)
    args = ap.parse_args()
    assert args.iters >= 20 and args.warmup >= 5, "at least 20 timed calls after 5 warm-ups"
    dev = torch.device("cuda:0")
    sd = syn.face_recon_state_dict(5)
    net = FaceRecon(sd, syn.face_recon_lm3d())
    ref = TorchFaceRecon(sd).to(dev).eval()
    rows = []
    with torch.no_grad():
        for what, counts in (("forward", args.forward), ("expressions", args.expressions)):
            for n in counts:
                gen = torch.Generator(device=dev).manual_seed(n)
                if what == "forward":
                    x = torch.rand(n, 3, 224, 224, device=dev, generator=gen)
                    mine = lambda: net.forward(x)  # noqa: E731
                else:
                    frames = torch.rand(n, 3, 256, 256, device=dev, generator=gen)
                    # a face about 100 pixels between the eyes' line and the mouth, somewhere near the middle: s close to 1
                    lm5 = torch.tensor([[88.0, 104.0], [168.0, 104.0], [128.0, 150.0], [96.0, 186.0], [160.0, 186.0]], dtype=torch.float64, device=dev)
                    lm = lm5[None] + 4.0 * torch.rand(n, 5, 2, dtype=torch.float64, device=dev, generator=gen)
                    x, _, status = net.align(frames, lm)
                    assert int(status.max()) == 0
                    mine = lambda: net.expressions(frames, lm)  # noqa: E731
                diff = float((net.forward(x).double() - ref(x).double()).abs().max())
                assert diff <= 1e-2, diff  # fp32 torch modules against the split-bf16 kernels, coefficients of O(10)
                fns = {what: mine, "torch": lambda: ref(x)}
                us = {k: [] for k in fns}
                for _ in range(args.pairs):
                    for k, fn in fns.items():
                        us[k].append(round(median_us(fn, args.warmup, args.iters), 2))
                row = {"call": what, "images": n, "side": 224 if what == "forward" else 256, "max_abs_difference_coeffs": diff, "us": us}
                row["n3dt_us"], row["torch_us"] = statistics.median(us[what]), statistics.median(us["torch"])
                row["torch_over_n3dt"] = round(row["torch_us"] / row["n3dt_us"], 3)
                macs = conv_macs(224, 224) * n
                row["conv_gflop_algorithmic"] = round(2 * macs / 1e9, 3)
                row["fraction_of_bf16_peak_end_to_end"] = round(3 * 2 * macs / (row["n3dt_us"] * 1e-6) / BF16_PEAK_FLOPS, 5)
                rows.append(row)
    result = {"iters": args.iters, "warmup": args.warmup, "pairs": args.pairs, "device": torch.cuda.get_device_name(0),
              "torch_side": "the network alone in torch fp32 modules; for `expressions` on the 224 x 224 crops, the aligner untimed", "rows": rows}
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
