#!/usr/bin/env python3
"""Generate tests/golden/eval_metrics.{npz,json}: seeded float32 image pairs and the SSIM / PSNR the reference's validation
metrics give them (Utils/Eval_utils.py:11-48,54-66,101-106).

The libraries the reference calls (scikit-image 0.19.3, opencv-python 4.8.1.78) are not dependencies of this project, so
the expected values come from a written-down float64 formulation, in two independent forms that must agree to 1e-12:
  * skimage's own: scipy.ndimage.uniform_filter of X, Y, X^2, Y^2, XY in float64, cropped by 3 (used when scipy is importable);
  * tests/eval_restatement.py: direct means over sliding 7x7 windows (numpy only).
Parity is therefore unpinned to the dependency, and the manifest says so.

Cases (n, H, W): a single window (7x7), sizes below one 32x32 tile, exactly one tile, tiles cut on both edges (37x53), 2x2 tiles
(64x64).  Image kinds: `uniform` (independent uniform [0,1) noise), `smooth` (a seeded sinusoid pattern in [0.1, 0.9] plus 2 %
Gaussian noise on either side) and `flip` (gt is pred with one pixel replaced by 1 - value).  The images of one case take the
kinds listed for it, so a batch holds different images.

Regenerating reproduces the files bit for bit.  Usage:  python tools/gen_golden_eval.py [--out DIR]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import eval_restatement as er  # noqa: E402

SEED = 20240
CASES = [  # (name, H, W, the kind of every image)
    ("one_window_uniform", 7, 7, ("uniform",)),
    ("one_window_smooth", 7, 7, ("smooth",)),
    ("one_window_flip", 7, 7, ("flip",)),
    ("below_a_tile", 8, 13, ("uniform", "smooth", "flip")),
    ("cut_tiles", 37, 53, ("smooth", "flip")),
    ("one_tile", 32, 32, ("flip", "uniform")),
    ("four_tiles", 64, 64, ("smooth",)),
]


def make_pair(kind, H, W, rng):
    if kind == "uniform":
        return rng.random((3, H, W), dtype=np.float32), rng.random((3, H, W), dtype=np.float32)
    if kind == "smooth":
        yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
        base = np.stack([0.5 + 0.4 * np.sin(2.0 * np.pi * (fx * xx / W + fy * yy / H) + ph)
                         for fx, fy, ph in rng.random((3, 3)) * np.array([3.0, 3.0, 6.28])])
        a = np.clip(base + 0.02 * rng.standard_normal(base.shape), 0.0, 1.0).astype(np.float32)
        b = np.clip(base + 0.02 * rng.standard_normal(base.shape), 0.0, 1.0).astype(np.float32)
        return a, b
    if kind == "flip":
        a = rng.random((3, H, W), dtype=np.float32)
        b = a.copy()
        y, x = int(rng.integers(H)), int(rng.integers(W))
        b[:, y, x] = np.float32(1.0) - b[:, y, x]
        return a, b
    raise ValueError(kind)


def skimage_formulation(g1, g2):
    """structural_similarity's own steps on top of scipy.ndimage.uniform_filter (skimage/metrics/_structural_similarity.py)."""
    from scipy.ndimage import uniform_filter
    x, y = g1.astype(np.float64), g2.astype(np.float64)
    cov_norm = 49.0 / 48.0
    ux, uy = uniform_filter(x, size=7), uniform_filter(y, size=7)
    uxx, uyy, uxy = uniform_filter(x * x, size=7), uniform_filter(y * y, size=7), uniform_filter(x * y, size=7)
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    a1, a2, b1, b2 = 2 * ux * uy + er.C1, 2 * vxy + er.C2, ux ** 2 + uy ** 2 + er.C1, vx + vy + er.C2
    s = (a1 * a2) / (b1 * b2)
    return float(s[3:-3, 3:-3].mean(dtype=np.float64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    args = ap.parse_args()
    try:
        import scipy
        scipy_version = scipy.__version__
    except ImportError:
        scipy_version = None
    missing = []
    for mod in ("skimage", "cv2"):
        try:
            __import__(mod)
        except ImportError:
            missing.append(mod)
    arrays, cases, worst = {}, [], 0.0
    for idx, (name, H, W, kinds) in enumerate(CASES):
        rng = np.random.default_rng(SEED + idx)
        pairs = [make_pair(k, H, W, rng) for k in kinds]
        pred, gt = np.stack([p for p, _ in pairs]), np.stack([g for _, g in pairs])
        ssim_r, psnr = er.batch_metrics(pred, gt)
        ssim = ssim_r
        if scipy_version is not None:
            ssim = np.array([skimage_formulation(er.gray_bgr(er.quantise(p.transpose(1, 2, 0))), er.gray_bgr(er.quantise(g.transpose(1, 2, 0))))
                             for p, g in zip(pred, gt)])
            worst = max(worst, float(np.abs(ssim - ssim_r).max()))
            assert worst <= 1e-12, "the two formulations differ by %.3e on %s" % (worst, name)
        arrays[name + "/pred"], arrays[name + "/gt"] = pred, gt
        arrays[name + "/ssim"], arrays[name + "/psnr"] = ssim, psnr
        cases.append({"name": name, "n": len(kinds), "height": H, "width": W, "kinds": list(kinds), "seed": SEED + idx})
    manifest = {
        "what": "SSIM / PSNR of Utils/Eval_utils.calc_eval_metrics for every image of each case (the reference scores image 0 only)",
        "parity": "parity unpinned to the dependency",
        "libraries_assumed": {"scikit-image": "0.19.3", "opencv-python": "4.8.1.78"},
        "libraries_not_importable_when_generated": missing,
        "ssim_expected_from": ("scipy.ndimage.uniform_filter formulation, scipy %s" % scipy_version) if scipy_version else "tests/eval_restatement.py",
        "formulations_max_abs_difference": worst,
        "gray": {"B": er.BY15, "G": er.GY15, "R": er.RY15, "gray_shift": er.GRAY_SHIFT,
                 "note": "OpenCV 4.8 COLOR_BGR2GRAY for uint8, read from its source as remembered, not run; channel 0 is taken as B"},
        "quantisation": "uint8(min(max(float32(x) * float32(255), 0), 255)), NaN -> 0",
        "ssim": {"window": 7, "data_range": 255, "K1": er.K1, "K2": er.K2, "cov_norm": "49/48", "crop": 3, "dtype": "float64"},
        "psnr": "20 log10(255 / (sqrt(SSE / (H W 3)) + 2.220446049250313e-16))",
        "numpy": np.__version__,
        "cases": cases,
    }
    os.makedirs(args.out, exist_ok=True)
    np.savez_compressed(os.path.join(args.out, "eval_metrics.npz"), **arrays)
    with open(os.path.join(args.out, "eval_metrics.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %d cases, formulations within %.2e" % (len(cases), worst))


if __name__ == "__main__":
    main()
