#!/usr/bin/env python3
"""Generate tests/golden/nr_grad.{json,npz}: the reference's own NeuralRenderer in float64 on the CPU -- image, input gradient
and every parameter gradient for a seeded cotangent -- for tests/test_nr_restatement_cpu.py, which holds the float64
restatement of the renderer (tests/nr_restatement.py) to it per entry.

Runs only where the reference is checked out (see tools/gen_golden.py, whose import of the reference's package and whose stand-in
for kornia's filter2d this uses).  Nothing of the reference travels: the fixture holds the inputs, the cotangent, the image and
the gradients; weights are regenerated from n3dt.synthetic.make_state_dict (the seed is stored, not the weights).

Usage:  python tools/gen_golden_nr_grad.py [--out DIR]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "nerf-3dtalker-code_amd"))

import gen_golden  # noqa: E402
import nr_restatement as nr  # noqa: E402
from n3dt import synthetic as syn  # noqa: E402

SEED = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=gen_golden.OUT)
    args = ap.parse_args()
    gen_golden.install_kornia_standin()
    sys.path.insert(0, gen_golden.REF)
    from NetWorks.neural_renderer import NeuralRenderer
    arrays, manifest = {}, {"seed": SEED, "cases": [], "blur": "filter2d stand-in of tools/gen_golden.py (reflect border, normalized)"}
    for ci, case in enumerate(nr.FIXTURE_CASES):
        fs, C, n, nb = case
        sd = syn.make_state_dict(nr.case_options(case), seed=SEED, bg_noise=0.1)
        net = NeuralRenderer(bg_type="white", feat_nc=C, out_dim=3, final_actvn=True, min_feat=32, featmap_size=fs, img_size=fs << n)
        own = {k[len("neural_render."):]: v for k, v in sd.items() if k.startswith("neural_render.")}
        net.load_state_dict(own, strict=True)
        net = net.double()
        _, x, d_img = nr.case_inputs(case, SEED)
        xt = torch.tensor(np.ascontiguousarray(x.transpose(0, 3, 1, 2)), requires_grad=True)   # the module takes [nb, C, h, w]
        img = net(xt)
        (img * torch.tensor(np.ascontiguousarray(d_img.transpose(0, 3, 1, 2)))).sum().backward()
        tag = "c%d_" % ci
        arrays[tag + "x"] = x.astype(np.float32)            # (0.5 randn and randn drawn in float32: exact)
        arrays[tag + "d_img"] = d_img.astype(np.float32)
        arrays[tag + "img"] = img.detach().numpy().transpose(0, 2, 3, 1)
        arrays[tag + "d_x"] = xt.grad.numpy().transpose(0, 2, 3, 1)
        names = []
        for name, p in net.named_parameters():
            if p.grad is None:
                continue  # bg_featmap is not part of this call
            names.append(name)
            arrays[tag + "g_" + name] = p.grad.numpy().reshape(p.shape[0], -1) if p.dim() == 4 else p.grad.numpy()
        manifest["cases"].append({"featmap_size": fs, "featmap_nc": C, "n_blocks": n, "maps": nb, "parameters": names,
                                  "weights_checksum": syn.state_dict_checksum(sd)})
    os.makedirs(args.out, exist_ok=True)
    np.savez_compressed(os.path.join(args.out, "nr_grad.npz"), **arrays)
    with open(os.path.join(args.out, "nr_grad.json"), "w") as f:
        json.dump(manifest, f, indent=1)
    print("wrote nr_grad: %d arrays, %d bytes" % (len(arrays), os.path.getsize(os.path.join(args.out, "nr_grad.npz"))))


if __name__ == "__main__":
    main()
