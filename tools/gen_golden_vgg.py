#!/usr/bin/env python3
"""Generate tests/golden/vgg.{npz,json} from the reference's own loss object (Utils/HeadNeRFLossUtils.py:23-64, 66-85, 125-156,
196-236): HeadNeRFLossUtils(use_vgg_loss=True, device="cpu").calc_total_loss in float64, VGG term included.

Runs only where the reference is checked out (it imports it).  torchvision is replaced by the stand-in of
gen_golden.install_caller_standins(), extended here with `models.vgg16(pretrained=True)`: an object whose `.features` is an
nn.Sequential in torchvision's layer order (Conv2d / ReLU / MaxPool2d at torchvision's indices) carrying the seeded weights of
n3dt.synthetic.vgg16_features_state_dict(seed) -- the pretrained weights cannot be fetched offline, and none are stored: only the
seed and a checksum.

Inputs are quantised so that they are stored exactly and small: images as uint8 / 255, masks as uint8 / 4 (so 0.5 itself occurs),
NaN positions as a list.  Recorded per case: every loss key, the four block terms (forward hooks on the reference's four blocks), and
d(total_loss)/d(merge_img) by autograd on a seeded sample of 16384 entries (NaN positions included) with the full array's L2 norm
and max |.|, so that the file stays under 1 MiB.  Regenerating reproduces the file bit for bit (fixed seeds, float64, deterministic CPU ops).

Usage:  python tools/gen_golden_vgg.py [--out DIR]
"""
import argparse
import hashlib
import json
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.path.insert(0, os.path.join(REPO, "nerf-3dtalker-code_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

from n3dt import synthetic as syn  # noqa: E402
import gen_golden  # noqa: E402

WEIGHTS_SEED = 1234
CASES = (  # name, B, P, bg_type, seed, n NaN pixels
    ("a", 2, 64, "white", 31, 5),     # upscale to 224
    ("b", 1, 256, "black", 32, 6),    # downscale to 224
)
SAMPLE_B = 16384


def install_vgg_standin(seed):
    import torch.nn as nn
    sd = syn.vgg16_features_state_dict(seed)

    def vgg16(pretrained=False, **kw):
        layers, cin = [], 3
        for v in syn.VGG16_CFG:
            if v == "M":
                layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
            else:
                layers += [nn.Conv2d(cin, v, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
                cin = v
        feats = nn.Sequential(*layers)
        feats.load_state_dict({k[len("features."):]: v for k, v in sd.items()}, strict=True)
        m = types.SimpleNamespace(features=feats)
        return m

    tv = sys.modules["torchvision"]
    models = types.ModuleType("torchvision.models")
    models.vgg16 = vgg16
    tv.models = models
    sys.modules["torchvision.models"] = models
    return sd


def make_case(B, P, seed, n_nan):
    g = torch.Generator().manual_seed(seed)
    merge_u8 = torch.randint(0, 256, (B, 3, P, P), generator=g, dtype=torch.uint8)
    gt_u8 = torch.randint(0, 256, (B, 3, P, P), generator=g, dtype=torch.uint8)
    bg_u8 = torch.randint(0, 256, (1, 3, P, P), generator=g, dtype=torch.uint8)
    # a soft disk-ish mask, quantised to quarters: values 0, .25, .5 (head), .75, 1 on both sides of the boundary
    yy, xx = torch.meshgrid(torch.arange(P), torch.arange(P), indexing="ij")
    r = ((yy - P / 2.0) ** 2 + (xx - P / 2.0) ** 2).sqrt() / P
    q = (4 - ((r - 0.3) * 40).clamp(0, 4)).round().to(torch.uint8).view(1, 1, P, P).repeat(B, 1, 1, 1)
    flip = torch.randint(0, 2, q.shape, generator=g, dtype=torch.uint8)
    mask_q = torch.where((q > 0) & (q < 4), (q + flip - 1).clamp(1, 3), q)
    nan_idx = torch.randperm(B * 3 * P * P, generator=g)[:n_nan].sort().values
    return merge_u8, gt_u8, bg_u8, mask_q, nan_idx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    args = ap.parse_args()
    torch.use_deterministic_algorithms(True)
    torch.set_num_threads(1)  # one summation order, whatever the machine
    gen_golden.install_caller_standins()
    sd = install_vgg_standin(WEIGHTS_SEED)
    sys.path.insert(0, REF)
    from Utils.HeadNeRFLossUtils import HeadNeRFLossUtils

    arrays, cases = {}, []
    for name, B, P, bg_type, seed, n_nan in CASES:
        merge_u8, gt_u8, bg_u8, mask_q, nan_idx = make_case(B, P, seed, n_nan)
        merge = (merge_u8.float() / 255.0).double()
        merge.view(-1)[nan_idx] = float("nan")
        merge.requires_grad_(True)
        gt = (gt_u8.float() / 255.0).double()
        bg = (bg_u8.float() / 255.0).double()
        mask = (mask_q.float() / 4.0).double()
        lu = HeadNeRFLossUtils(bg_type=bg_type, use_vgg_loss=True, device="cpu")
        lu.vgg_loss_func.double()
        outs = []
        hooks = [blk.register_forward_hook(lambda m, i, o: outs.append(o)) for blk in lu.vgg_loss_func.blocks]
        res = lu.calc_total_loss(None, None, {"coarse_dict": {"merge_img": merge, "bg_img": bg}}, gt, mask, None)
        for h in hooks:
            h.remove()
        # the reference runs block i on x then on y (:53-56): outs = x0, y0, x1, y1, ...
        blocks = [float(torch.nn.functional.l1_loss(outs[2 * i], outs[2 * i + 1])) for i in range(4)]
        res["total_loss"].backward()
        keys = list(res.keys())
        d = merge.grad.float().numpy()
        k = name + "."
        arrays.update({k + "merge_u8": merge_u8.numpy(), k + "gt_u8": gt_u8.numpy(), k + "bg_u8": bg_u8.numpy(),
                       k + "mask_q": mask_q.numpy(), k + "nan_idx": nan_idx.numpy().astype(np.int64),
                       k + "terms": np.array([float(res[n]) for n in keys], dtype=np.float64),
                       k + "blocks": np.array(blocks, dtype=np.float64)})
        if d.size <= SAMPLE_B:
            arrays[k + "d_merge"] = d
        else:
            rng = np.random.default_rng(seed)
            idx = np.union1d(rng.choice(d.size, SAMPLE_B, replace=False), nan_idx.numpy()).astype(np.int64)
            arrays[k + "d_idx"] = idx
            arrays[k + "d_merge"] = d.reshape(-1)[idx]
        arrays[k + "d_norm"] = np.array([np.linalg.norm(d.astype(np.float64)), np.abs(d).max()], dtype=np.float64)
        cases.append({"name": name, "batch": B, "size": P, "bg_type": bg_type, "seed": seed, "n_nan": n_nan, "keys": keys,
                      "d_merge": "full" if d.size <= SAMPLE_B else "sample of %d entries at d_idx (NaN positions included)" % len(arrays[k + "d_idx"])})
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "vgg.npz")
    np.savez_compressed(path, **arrays)
    digest = hashlib.sha256()
    for n in sorted(arrays):
        digest.update(n.encode())
        digest.update(np.ascontiguousarray(arrays[n]).tobytes())
    manifest = {
        "name": "vgg", "generator": "tools/gen_golden_vgg.py",
        "what": "Utils/HeadNeRFLossUtils.py HeadNeRFLossUtils(bg_type, use_vgg_loss=True, device='cpu').calc_total_loss of the "
                "reference in float64 (VGGPerceptualLoss included): every loss key in the reference's order, the four block terms "
                "(forward hooks on its blocks) and autograd d(total_loss)/d(merge_img)",
        "inputs": "merge/gt/bg = uint8 / 255, mask = uint8 / 4 (head where >= 0.5), NaN written into merge at nan_idx (flat)",
        "torchvision_standin": "models.vgg16(pretrained=True).features = nn.Sequential in torchvision's layer order with the weights "
                               "of n3dt.synthetic.vgg16_features_state_dict(weights_seed); no weights stored",
        "weights_seed": WEIGHTS_SEED, "weights_checksum": syn.state_dict_checksum(sd),
        "arrays_sha256": digest.hexdigest(), "cases": cases,
    }
    with open(os.path.join(args.out, "vgg.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    print("wrote %s (%.1f KB)" % (path, os.path.getsize(path) / 1024.0))


if __name__ == "__main__":
    main()
