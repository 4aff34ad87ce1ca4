#!/usr/bin/env python3
"""Tolerance bands of the VGG term's two precisions, set on the CPU.

The tests' float64 restatement of the reference's term (tests/test_vgg_cpu.py: vgg_term_reference) is run twice on both fixture
cases of tests/golden/vgg: exactly, and with activations and weights rounded to bf16 before every convolution (the gradient entering
each convolution rounds too, as the kernels' dgrad operands do).  The emulated error of every quantity the GPU test checks is
printed as JSON; tests/test_gpu_vgg.py sets each bf16 bound at twice the largest value seen here.

The same is done for plain float32 (the restatement run in float32 instead of float64): the term's gradient is discontinuous (the
L1 sign at every block end, every ReLU gate, every pool arg-max), and fp32 rounding alone flips enough of them on these inputs that
d_merge moves by ~1e-2 relative L2.  The N3DT_F32 d_merge bounds are twice that float32 error; its term bound stays 1e-4.

Usage:  python tools/vgg_bf16_band.py
"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "nerf-3dtalker-code_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

from test_vgg_cpu import vgg_term_reference, fixture_case, fixture_weights  # noqa: E402


def run(weights, merge, gt, bg, mask, bgv, round_bf16, dtype=torch.float64):
    x = merge.to(dtype).requires_grad_(True)
    loss, blocks = vgg_term_reference(weights, x, gt, mask, bgv, round_bf16=round_bf16, dtype=dtype)
    res = torch.nan_to_num(x, nan=0.0)
    head = (mask.to(dtype) >= 0.5).expand(-1, 3, -1, -1)
    total = (((0.0 + torch.mean((bg.to(dtype) - bgv) ** 2)) + F.mse_loss(res[head], gt.to(dtype)[head]))
             + torch.mean((res[~head] - bgv) ** 2)) + loss
    total.backward()
    return np.array([float(b) for b in blocks] + [float(loss), float(total)]), x.grad.double().numpy().reshape(-1)


def main():
    data = np.load(os.path.join(REPO, "tests", "golden", "vgg.npz"))
    with open(os.path.join(REPO, "tests", "golden", "vgg.json")) as f:
        m = json.load(f)
    _, weights = fixture_weights(m)
    out = {"bf16": {}, "float32": {}}
    for name in ("a", "b"):
        merge, gt, bg, mask, bgv, _ = fixture_case(data, m, name)
        t0, d0 = run(weights, merge, gt, bg, mask, bgv, False)
        for mode, kw in (("bf16", dict(round_bf16=True)), ("float32", dict(round_bf16=False, dtype=torch.float32))):
            t1, d1 = run(weights, merge, gt, bg, mask, bgv, **kw)
            out[mode][name] = {
                "term_rel": float(np.max(np.abs(t1 - t0) / np.abs(t0))),
                "d_merge_rel_l2": float(np.linalg.norm(d1 - d0) / np.linalg.norm(d0)),
                "d_merge_max_over_maxabs": float(np.abs(d1 - d0).max() / np.abs(d0).max()),
            }
    for mode in ("bf16", "float32"):
        o = out[mode]
        o["max"] = {k: max(o[n][k] for n in ("a", "b")) for k in o["a"]}
        o["bounds_2x"] = {k: 2 * v for k, v in o["max"].items()}
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
