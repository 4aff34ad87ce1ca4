"""LPIPS-alex as the reference's validation computes it (Utils/Eval_utils.py:108-115, lpips.LPIPS(net='alex'), version 0.1,
spatial=False, eval mode), restated with torch on the CPU in float64.

Written from the contract, not in the kernel's order: torch's own conv2d / max_pool2d on NCHW tensors, the reinterpretation as a
literal numpy reshape(-1, 3, h, w) of the HWC byte image.  The `lpips` package and torchvision are not dependencies of this
project; what is stated here about them is from knowledge of lpips 0.1.4 and has not been run against it: parity is unpinned to
the dependency.

`dtype` and `conv` exist for tools/lpips_band.py, which re-runs the very same steps in float32 and with split-bf16 operands to
measure the rounding floor the GPU tolerance is derived from.
"""
import numpy as np
import torch
import torch.nn.functional as F

from eval_restatement import quantise

SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
# torchvision alexnet().features: (index, C_in, C_out, kernel, stride, padding); a 3 / 2 max-pool sits in front of convs 1 and 2
CONVS = ((0, 3, 64, 11, 4, 2), (3, 64, 192, 5, 1, 2), (6, 192, 384, 3, 1, 1), (8, 384, 256, 3, 1, 1), (10, 256, 256, 3, 1, 1))
POOL_BEFORE = (False, True, True, False, False)
EPS = 1e-10


def reference_input(img):
    """img [3,H,W] float32 in the project's planar layout -> [1,3,H,W] float32 of byte values, as compute_LPIPS feeds the net: the
    [H,W,3] uint8 image the other metrics get, RESHAPED (not transposed) to [-1,3,H,W]."""
    _, h, w = img.shape
    hwc = np.ascontiguousarray(quantise(np.asarray(img, np.float32).transpose(1, 2, 0)))  # [H,W,3] uint8
    return torch.from_numpy(hwc.reshape(-1, 3, h, w).astype(np.float32))


def permuted_input(img):
    """What a proper HWC -> CHW transpose of the same bytes would feed: the quirk's counterfactual."""
    hwc = quantise(np.asarray(img, np.float32).transpose(1, 2, 0))
    return torch.from_numpy(np.ascontiguousarray(hwc.transpose(2, 0, 1))[None].astype(np.float32))


def standard_input(img):
    """The metric as its authors define it: channels as given, 2 clamp(x, 0, 1) - 1 (NaN counts as 0 before the map)."""
    x = np.clip(np.nan_to_num(np.asarray(img, np.float32), nan=0.0), 0.0, 1.0).astype(np.float32)
    return torch.from_numpy(np.float32(2.0) * x - np.float32(1.0))[None]


INPUTS = {"reference": reference_input, "permuted": permuted_input, "standard": standard_input}


def scaling(x):
    """lpips.ScalingLayer in float32, as the package computes it"""
    shift = torch.tensor(SHIFT, dtype=torch.float32).view(1, 3, 1, 1)
    scale = torch.tensor(SCALE, dtype=torch.float32).view(1, 3, 1, 1)
    return (x.float() - shift) / scale


def split_weights(sd):
    """([(weight, bias)] x 5, [lin [C]] x 5) from the torchvision / lpips names of n3dt.synthetic.lpips_alex_state_dict"""
    convs = [(sd["features.%d.weight" % c[0]], sd["features.%d.bias" % c[0]]) for c in CONVS]
    lins = [sd["lin%d.model.1.weight" % l].reshape(-1) for l in range(len(CONVS))]
    return convs, lins


def features(x, convs, dtype=torch.float64, conv=F.conv2d):
    """relu1..relu5 of the scaled input x [N,3,H,W]"""
    out = []
    x = x.to(dtype)
    for (w, b), (_, _, _, _, stride, pad), pool in zip(convs, CONVS, POOL_BEFORE):
        if pool:
            x = F.max_pool2d(x, kernel_size=3, stride=2)
        x = torch.relu(conv(x, w.to(dtype), b.to(dtype), stride=stride, padding=pad))
        out.append(x)
    return out


def distance(f0, f1, lin):
    """mean over pixels of sum_c w_c (n0_c - n1_c)^2 with n = f / (sqrt(sum_c f^2) + eps): [N]"""
    n0 = f0 / (torch.sqrt((f0 * f0).sum(dim=1, keepdim=True)) + EPS)
    n1 = f1 / (torch.sqrt((f1 * f1).sum(dim=1, keepdim=True)) + EPS)
    d = ((n0 - n1) ** 2 * lin.to(f0.dtype).view(1, -1, 1, 1)).sum(dim=1)
    return d.mean(dim=(1, 2))


def lpips_pair(pred, gt, sd, input_mode="reference", dtype=torch.float64, conv=F.conv2d):
    """pred, gt [3,H,W] float32 -> (score, [5 layer values]) as Python floats"""
    convs, lins = split_weights(sd)
    x = scaling(torch.cat([INPUTS[input_mode](pred), INPUTS[input_mode](gt)]))
    with torch.no_grad():
        feats = features(x, convs, dtype, conv)
        layers = [float(distance(f[:1], f[1:], lin)[0]) for f, lin in zip(feats, lins)]
    total = 0.0
    for v in layers:
        total += v
    return total, layers


def lpips_batch(pred, gt, sd, input_mode="reference", dtype=torch.float64, conv=F.conv2d):
    """pred, gt [B,3,H,W] -> (scores [B], layers [5,B]) float64 numpy"""
    res = [lpips_pair(p, g, sd, input_mode, dtype, conv) for p, g in zip(pred, gt)]
    return np.array([r[0] for r in res], np.float64), np.array([r[1] for r in res], np.float64).T.copy()


# ---- the seeded image pairs the fixtures, the band measurement and the GPU tests share ------------------------------------------
# (name, H, W, images): the smallest sizes at which each piece of the kernels can go wrong, and the real geometry
SMALL_CASES = (("min_31", 31, 31, 3), ("odd_35x47", 35, 47, 3), ("square_64", 64, 64, 3), ("odd_67x61", 67, 61, 3))
BIG_CASES = (("real_256", 256, 256, 1), ("real_512", 512, 512, 1))
WEIGHTS_SEED = 5
PAIR_SEED = 7000


def make_pair_u8(h, w, seed):
    """A smooth sinusoid pattern against its flipped, rescaled, noisy copy, as BYTES [3,H,W] (the float images are bytes / 255,
    which the quantiser inverts exactly): genuinely different images, so that all five layers contribute."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    base = np.stack([0.5 + 0.4 * np.sin(2.0 * np.pi * (fx * xx / w + fy * yy / h) + ph)
                     for fx, fy, ph in rng.random((3, 3)) * np.array([3.0, 3.0, 6.28])])
    a = np.clip(base + 0.02 * rng.standard_normal(base.shape), 0.0, 1.0)
    b = np.clip(0.5 + 0.7 * (base[:, ::-1, ::-1] - 0.5) + 0.05 * rng.standard_normal(base.shape), 0.0, 1.0)
    return np.round(a * 255.0).astype(np.uint8), np.round(b * 255.0).astype(np.uint8)


def case_images_u8(idx, h, w, n):
    """(pred, gt) uint8 [n,3,H,W] of case number idx in SMALL_CASES + BIG_CASES"""
    pairs = [make_pair_u8(h, w, PAIR_SEED + 10 * idx + i) for i in range(n)]
    return np.stack([p for p, _ in pairs]), np.stack([g for _, g in pairs])


def to_float(u8):
    return u8.astype(np.float32) / np.float32(255.0)
