#!/usr/bin/env python3
"""Measure, on the CPU, the rounding floor the GPU tolerance of tests/test_gpu_lpips.py is derived from, over exactly that test's
cases (tests/lpips_restatement.SMALL_CASES and BIG_CASES, every image, both input modes for the small ones).

Two re-runs of the float64 restatement, each compared with it by the relative error of the score and of every layer value:
  (a) float32   the same torch ops in plain float32;
  (b) split     float32 everywhere, and every convolution as the kernel forms it: an im2col product in the kernel's K order
                (k = tap * C_in + c_in), both operands split x = hi + lo into two bf16s, the lo * lo product dropped, and the
                three products of each 16-wide K step added to a float32 accumulator step by step (what the MFMA chain does).
The floor is the larger of the two maxima, taken for the scores and for the layer values separately (a layer value of a 31 x 31
image is ONE pixel, a score at 512 x 512 averages thousands); each test bound is 4 x its floor.  Writes
profiles/lpips_band.json.

Usage:  python tools/lpips_band.py [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "nerf-3dtalker-code_amd"))

import lpips_restatement as lr  # noqa: E402
from n3dt import synthetic as syn  # noqa: E402


def bf16_split(x):
    hi = x.to(torch.bfloat16).float()
    lo = (x - hi).to(torch.bfloat16).float()
    return hi, lo


def split_conv(x, w, b, stride, padding):
    x, w, b = x.float(), w.float(), b.float()
    cout, cin, k, _ = w.shape
    n, _, h, wd = x.shape
    ho, wo = (h + 2 * padding - k) // stride + 1, (wd + 2 * padding - k) // stride + 1
    cols = F.unfold(x, k, padding=padding, stride=stride)                        # [n, cin * k * k, L], rows (c, tap)
    cols = cols.view(n, cin, k * k, -1).permute(0, 3, 2, 1).reshape(n, -1, k * k * cin)  # [n, L, K], columns (tap, c)
    wm = w.view(cout, cin, k * k).permute(2, 1, 0).reshape(k * k * cin, cout)    # [K, cout]
    kp = (cols.shape[2] + 15) // 16 * 16
    cols, wm = F.pad(cols, (0, kp - cols.shape[2])), F.pad(wm, (0, 0, 0, kp - wm.shape[0]))
    (ahi, alo), (bhi, blo) = bf16_split(cols), bf16_split(wm)
    acc = torch.zeros(n, cols.shape[1], cout, dtype=torch.float32)
    for s in range(0, kp, 16):
        acc = acc + alo[:, :, s:s + 16] @ bhi[s:s + 16]
        acc = acc + ahi[:, :, s:s + 16] @ blo[s:s + 16]
        acc = acc + ahi[:, :, s:s + 16] @ bhi[s:s + 16]
    return (acc + b).permute(0, 2, 1).reshape(n, cout, ho, wo)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lpips_band.json"))
    args = ap.parse_args()
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    sd = syn.lpips_alex_state_dict(lr.WEIGHTS_SEED)
    forms = {"float32": dict(dtype=torch.float32), "split": dict(dtype=torch.float32, conv=split_conv)}
    rows, worst = [], {k + part: 0.0 for k in forms for part in ("_score", "_layers")}
    for idx, (name, h, w, n) in enumerate(lr.SMALL_CASES + lr.BIG_CASES):
        pred, gt = (lr.to_float(t) for t in lr.case_images_u8(idx, h, w, n))
        for mode in ("reference", "standard") if idx < len(lr.SMALL_CASES) else ("reference",):
            ref_s, ref_l = lr.lpips_batch(pred, gt, sd, mode)
            ref = np.concatenate([ref_s[None], ref_l])
            row = {"case": name, "input_mode": mode, "min_value": float(ref.min())}
            for form, kw in forms.items():
                s, l = lr.lpips_batch(pred, gt, sd, mode, **kw)
                rel = np.abs(np.concatenate([s[None], l]) - ref) / ref
                row[form + "_score"], row[form + "_layers"] = float(rel[0].max()), float(rel[1:].max())
                for part in ("_score", "_layers"):
                    worst[form + part] = max(worst[form + part], row[form + part])
            rows.append(row)
            print(json.dumps(row))
    floor = {part: max(worst[k + "_" + part] for k in forms) for part in ("score", "layers")}
    out = {"what": "max relative error of the LPIPS score and of every layer value against the float64 restatement, on the CPU",
           "weights_seed": lr.WEIGHTS_SEED, "pair_seed": lr.PAIR_SEED, "torch": torch.__version__,
           "worst": worst, "floor": floor, "test_bound": {k: 4.0 * v for k, v in floor.items()}, "rows": rows}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("floor %s  bound %s" % (floor, {k: 4.0 * v for k, v in floor.items()}))


if __name__ == "__main__":
    main()
