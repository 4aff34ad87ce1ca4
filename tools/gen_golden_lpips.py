#!/usr/bin/env python3
"""Generate tests/golden/lpips.{npz,json}: seeded image pairs and the LPIPS-alex score and per-layer values the float64
restatement (tests/lpips_restatement.py) gives them with the seeded stand-in weights (n3dt.synthetic.lpips_alex_state_dict).

The AlexNet weights (2.5 M floats) are not stored: the manifest records their seed and a checksum.  The small cases' images are
stored as bytes (the float images are bytes / 255); the two real-size cases (256^2, 512^2) are stored as their seeds and expected
values only.  The `lpips` package is not a dependency of this project, so parity is unpinned to the dependency and the manifest
says so.

Regenerating reproduces every array bit for bit (tests/test_lpips_cpu.py checks them against the restatement).  Usage:  python tools/gen_golden_lpips.py [--out DIR]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "nerf-3dtalker-code_amd"))

import lpips_restatement as lr  # noqa: E402
from n3dt import synthetic as syn  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    args = ap.parse_args()
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    sd = syn.lpips_alex_state_dict(lr.WEIGHTS_SEED)
    arrays, cases = {}, []
    for idx, (name, h, w, n) in enumerate(lr.SMALL_CASES + lr.BIG_CASES):
        pred, gt = lr.case_images_u8(idx, h, w, n)
        stored = idx < len(lr.SMALL_CASES)
        case = {"name": name, "n": n, "height": h, "width": w, "index": idx, "images_stored": stored}
        for mode in ("reference", "standard"):
            if mode == "standard" and not stored:
                continue
            score, layers = lr.lpips_batch(lr.to_float(pred), lr.to_float(gt), sd, mode)
            arrays["%s/%s/score" % (name, mode)], arrays["%s/%s/layers" % (name, mode)] = score, layers
            print("%-10s %-9s score %s  layers(image 0) %s" % (name, mode, np.round(score, 4), np.round(layers[:, 0], 5)))
        if stored:
            arrays[name + "/pred_u8"], arrays[name + "/gt_u8"] = pred, gt
        cases.append(case)
    manifest = {
        "what": "LPIPS-alex of Utils/Eval_utils.compute_LPIPS for every image pair of each case, float64 restatement",
        "parity": "parity unpinned to the dependency",
        "libraries_assumed": {"lpips": "0.1.4"},
        "from_memory": "the scaling constants, AlexNet's layer geometry, the unit-normalisation epsilon 1e-10 and the lin layers' "
                       "shape are written from knowledge of lpips 0.1.4 and torchvision; neither package was importable",
        "weights": "n3dt.synthetic.lpips_alex_state_dict(seed): seeded stand-ins; the pretrained weights have never been run",
        "weights_seed": lr.WEIGHTS_SEED,
        "weights_checksum": float(sum(float(v.double().abs().sum()) for v in sd.values())),
        "pair_seed": lr.PAIR_SEED,
        "images": "float32 = stored bytes / 255 (tests/lpips_restatement.case_images_u8 regenerates them from the seeds)",
        "numpy": np.__version__,
        "cases": cases,
    }
    os.makedirs(args.out, exist_ok=True)
    np.savez_compressed(os.path.join(args.out, "lpips.npz"), **arrays)
    with open(os.path.join(args.out, "lpips.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %d cases" % len(cases))


if __name__ == "__main__":
    main()
