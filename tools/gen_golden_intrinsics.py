#!/usr/bin/env python3
"""Generate tests/golden/intrinsics.{npz,json}: the reference's own autograd with respect to the two inputs of ray generation
that the other gradient fixtures leave out, batch_inv_inmats and batch_xy (NetWorks/utils.py:113-163 builds the rays as
R . Kinv . [x, y, 1]; the module is plain PyTorch, so it differentiates with respect to both).

Runs only where the reference is checked out (it imports it, through tools/gen_golden.py and its stand-ins).  The reference's
HeadNeRFNet runs in float64 on the inputs of the existing cases `tiny_test`, `tiny_train` and `vd_train` -- same options, seeds,
weights (n3dt.synthetic, pinned by checksum) and stratified noise, so a test rebuilds them the way it does for those fixtures --
with batch_inv_inmats, batch_xy, batch_Rmats and batch_Tvecs requiring grad.  The loss is the sum of the three MSE data terms of
the existing gradient fixtures (gt = 0.5, disk mask).  Stored per case, as float32: grad_in.batch_inv_inmats [B,3,3] and
grad_in.batch_xy [B,2,N_r] of that float64 run, with its loss terms (float64).

grad_in.batch_Rmats / grad_in.batch_Tvecs are stored again as a cross-check that this generator builds the very cases of the
existing fixtures.  Those were written by tools/gen_golden.py, which runs the reference in FLOAT32 on 8 threads, and a float64
run cannot repeat a float32 one: ReLU gates within rounding of zero fall the other way and move the camera gradients by 0.3 - 2 %
of their scale (even one thread instead of eight moves them by 2e-5).  So the same case construction runs a second time the way
gen_golden.py runs it, float32 and 8 threads, and the cross-check entries and `loss_terms_f32` come from that run: they repeat the
existing fixtures exactly, which a different input, weight, seed or loss would not.  Nothing of the reference travels: arrays and
a manifest only.  Regenerating reproduces the file bit for bit (fixed seeds, fixed thread counts, deterministic CPU ops).

Usage:  python tools/gen_golden_intrinsics.py [--out DIR]
"""
import argparse
import hashlib
import io
import json
import os
import sys
import zipfile

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "nerf-3dtalker-code_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

from n3dt import synthetic as syn  # noqa: E402
from n3dt.options import BaseOptions  # noqa: E402
import gen_golden  # noqa: E402

CASES = (  # name (= the existing fixture whose inputs these are), mode, include_vd
    ("tiny_test", "test", False),
    ("tiny_train", "train", False),
    ("vd_train", "train", True),
)
GRAD_INPUTS = ("batch_inv_inmats", "batch_xy", "batch_Rmats", "batch_Tvecs")
B, T_RAND_SEED = 2, 7


def gen_case(HeadNeRFNet, mode, include_vd, double):
    """The case construction of gen_golden.gen_tiny / gen_vd (B=2, fs=8, N_s=8, pred 32), in float64 or as they run it."""
    f64 = (lambda v: v.double() if torch.is_tensor(v) and v.is_floating_point() else v) if double else (lambda v: v)
    torch.set_num_threads(1 if double else 8)  # float64: one summation order, whatever the machine; float32: gen_golden.main's
    opt = BaseOptions({"featmap_size": 8, "featmap_nc": 256, "pred_img_size": 32, "num_sample_coarse": 8})
    sd = syn.make_state_dict(opt, seed=0, bg_noise=0.1, include_vd=include_vd)
    net = HeadNeRFNet(opt, include_vd=include_vd, hier_sampling=False)
    net.load_state_dict(sd, strict=True)
    if double:
        net.double()
    inp = {k: f64(v) for k, v in syn.frame_inputs(opt, B, yaw_range=0.3).items()}
    for k in GRAD_INPUTS:
        inp[k] = inp[k].clone().requires_grad_(True)
    t_rand = syn.stratified_noise(B, opt.featmap_size ** 2, opt.num_sample_coarse, T_RAND_SEED) if mode == "train" else None
    coarse, _ = gen_golden.run_seams(net, inp, mode, f64(t_rand))
    assert coarse["merge_img"].dtype == (torch.float64 if double else torch.float32)
    gt = torch.full_like(coarse["merge_img"], 0.5)
    mask = f64(gen_golden.disk_mask(B, opt.pred_img_size))
    terms = gen_golden.losses(coarse, gt, mask)
    sum(terms).backward()
    arrays = {"grad_in." + k: gen_golden.np32(inp[k].grad) for k in GRAD_INPUTS}
    arrays["loss_terms"] = np.array([t.item() for t in terms], dtype=np.float64)
    return arrays, syn.state_dict_checksum(sd)


def arrays_sha256(arrays):
    digest = hashlib.sha256()
    for n in sorted(arrays):
        digest.update(n.encode())
        digest.update(np.ascontiguousarray(arrays[n]).tobytes())
    return digest.hexdigest()


def save_npz(path, arrays):
    """np.savez_compressed stamps every member with the time of writing; this writes the same .npz with a fixed stamp and in
    sorted order, so that the FILE, not only its arrays, comes out the same on every run."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for n in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[n]), allow_pickle=False)
            info = zipfile.ZipInfo(n + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    args = ap.parse_args()
    torch.use_deterministic_algorithms(True)
    torch.manual_seed(0)
    HeadNeRFNet, _ = gen_golden.import_reference()
    arrays, cases = {}, []
    for name, mode, include_vd in CASES:
        a, checksum = gen_case(HeadNeRFNet, mode, include_vd, double=True)
        a32, _ = gen_case(HeadNeRFNet, mode, include_vd, double=False)
        for k in ("grad_in.batch_inv_inmats", "grad_in.batch_xy", "loss_terms"):
            arrays[name + "." + k] = a[k]
        for k in ("grad_in.batch_Rmats", "grad_in.batch_Tvecs"):
            arrays[name + "." + k] = a32[k]
        arrays[name + ".loss_terms_f32"] = a32["loss_terms"]
        cases.append({"name": name, "mode": mode, "include_vd": include_vd, "batch": B, "weights_seed": 0, "bg_noise": 0.1,
                      "yaw_range": 0.3, "t_rand_seed": T_RAND_SEED if mode == "train" else None, "weights_checksum": checksum})
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "intrinsics.npz")
    save_npz(path, arrays)
    manifest = {
        "name": "intrinsics", "generator": "tools/gen_golden_intrinsics.py",
        "what": "NetWorks/HeadNeRFNet.py HeadNeRFNet.forward of the reference in float64 on the inputs of the fixtures named in `cases`: "
                "autograd d(loss)/d(batch_inv_inmats) [B,3,3] and d(loss)/d(batch_xy) [B,2,N_r], stored as float32 under "
                "'<case>.grad_in.<input>'; '<case>.loss_terms' in float64",
        "cross_check": "'<case>.grad_in.batch_Rmats', '<case>.grad_in.batch_Tvecs' and '<case>.loss_terms_f32': the same case run "
                       "the way tools/gen_golden.py wrote the fixtures named in `cases` (float32, 8 threads); they repeat those fixtures",
        "loss": "bg+head+nonhead MSE, gt=0.5, disk mask r=0.35*size, bg_value=1",
        "blur_note": "kornia.filters.filter2d stand-in (correlation, kernel/sum|k|, reflect pad); Blur parity unpinned",
        "featmap_size": 8, "featmap_nc": 256, "pred_img_size": 32, "num_sample_coarse": 8,
        "arrays_sha256": arrays_sha256(arrays), "cases": cases,
    }
    with open(os.path.join(args.out, "intrinsics.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    print("wrote %s (%.1f KB)" % (path, os.path.getsize(path) / 1024.0))


if __name__ == "__main__":
    main()
