#!/usr/bin/env python3
"""Generate tests/golden/face_recon.{npz,json}, face_recon_blocks.{npz,json} and face_recon_align.{npz,json} from the reference's
own 3-D face reconstruction net (s_face3d/models/networks.py: define_net_recon('resnet50', use_last_fc=False)) in float64 on the
CPU, and from its aligner (align_img of s_face3d/util/preprocess.py over its POS, extract_5p and resize_n_crop_img, and the
fallback / flip statement of CropAndExtract.generate, all cut out by ast, with the installed PIL; load_lm3d of s_face3d/util/load_mats.py on the reference's similarity_Lm3D_all.mat).

Runs only where the reference is checked out: it imports or cuts out the reference's code at generation time; nothing of it is
stored.  preprocess.py does not import under this numpy (it names np.VisibleDeprecationWarning) and align_img raises on its last
assignment (its trans_params array is ragged), hence the ast cut without that assignment; the integers w, h, left, up, which
resize_n_crop_img does not return, are read off its own resize() and crop() calls; networks.py imports kornia, which is stubbed
-- nothing on the paths driven here calls it.  Weights: n3dt.synthetic.face_recon_state_dict(WEIGHTS_SEED) loaded into the class with strict=True -- the pretrained
checkpoint is not available offline; only the seed and a checksum are stored.

Recorded per network case: per block (hooks on the reference's modules) the output's sum, abs-sum and every 331st element, and the
257 coefficients.  Per alignment case: the frames' landmarks, what POS and resize_n_crop_img gave (t, s, w, h, left, up), the PIL
crops as bytes, and the reference's coefficients of those crops.  lm3d_std as load_lm3d returns it.

The manifests carry the bounds the GPU tests use, MEASURED HERE ON THE CPU: the error of the restatement's emulation of the kernel's
arithmetic against these float64 values -- per block (each block alone on the fp32-rounded reference input), the coefficients end
to end, the expressions end to end from the frames -- and the restatement's unrounded resample against PIL's bytes / 255.  The GPU
tests allow 4 x those.  The reference alone must satisfy the fixture conditions, asserted here (see main).

Usage:  python tools/gen_golden_face_recon.py --ref DIR [--out DIR]
"""
import argparse
import ast
import hashlib
import json
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "nerf-3dtalker-code_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

from n3dt import synthetic as syn  # noqa: E402
from n3dt import face_recon as nf  # noqa: E402
import face_recon_restatement as fr  # noqa: E402

GPU_FACTOR = 4.0
ZERO_SHARE_CAP = 0.6
TRUNC_MARGIN = 1e-6
BYTE_CAP = 1e-3


def preprocess_functions(path):
    """align(img, lm, lm3D) -> (t, s, img_new): align_img compiled from the reference's own statements, over its own POS,
    extract_5p and resize_n_crop_img.  align_img as it stands raises under this numpy on its `trans_params` array (ragged: t holds
    arrays), so that one assignment and the return are left out and t, s and the image are returned instead."""
    from PIL import Image
    tree = ast.parse(open(path).read())
    wanted = ("POS", "extract_5p", "resize_n_crop_img", "align_img")
    defs = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in wanted]
    assert sorted(d.name for d in defs) == sorted(wanted), "preprocess.py no longer defines the four functions"
    align = [d for d in defs if d.name == "align_img"][0]
    dropped = [n for n in align.body if isinstance(n, ast.Return) or (isinstance(n, ast.Assign) and isinstance(n.targets[0], ast.Name) and n.targets[0].id == "trans_params")]
    assert len(dropped) == 2, "align_img no longer ends in the trans_params assignment and one return"
    align.body = [n for n in align.body if n not in dropped] + ast.parse("return t, s, img_new").body
    scope = {"np": np, "Image": Image}
    exec(compile(ast.fix_missing_locations(ast.Module(body=defs, type_ignores=[])), path, "exec"), scope)
    return scope["align_img"]


def landmark_lines(path):
    """prepare(self, lm1, W, H) -> lm1: the `if np.mean(lm1) == -1 ... else ...` statement of CropAndExtract.generate's frame loop
    (the fallback, or the y flip), compiled from the loader's own statement; `self` need only carry lm3d_std"""
    tree = ast.parse(open(path).read())
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "CropAndExtract"]
    assert len(cls) == 1
    gen = [n for n in cls[0].body if isinstance(n, ast.FunctionDef) and n.name == "generate"]
    assert len(gen) == 1
    found = [n for n in ast.walk(gen[0]) if isinstance(n, ast.If) and isinstance(n.test, ast.Compare) and "np.mean(lm1)" in ast.unparse(n.test)]
    assert len(found) == 1, "generate no longer holds one test of np.mean(lm1)"
    fn = ast.parse("def prepare(self, lm1, W, H):\n    return lm1").body[0]
    fn.body = found + fn.body
    scope = {"np": np}
    exec(compile(ast.fix_missing_locations(ast.Module(body=[fn], type_ignores=[])), path, "exec"), scope)
    return scope["prepare"]


class RecordingImage(object):
    """what resize_n_crop_img needs of a PIL image -- size, resize, crop -- handing each call on and keeping its arguments: the
    reference's own integers (w, h) and (left, up), which it does not return"""

    def __init__(self, img, calls=None):
        self.img, self.size, self.calls = img, img.size, {} if calls is None else calls

    def resize(self, size, resample=None):
        self.calls["resize"] = tuple(size)
        return RecordingImage(self.img.resize(size, resample=resample), self.calls)

    def crop(self, box):
        self.calls["crop"] = tuple(box)
        return self.img.crop(box)


def load_lm3d_function(path):
    from scipy.io import loadmat
    tree = ast.parse(open(path).read())
    defs = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "load_lm3d"]
    assert len(defs) == 1
    scope = {"np": np, "loadmat": loadmat, "osp": os.path}
    exec(compile(ast.fix_missing_locations(ast.Module(body=defs, type_ignores=[])), path, "exec"), scope)
    return scope["load_lm3d"]


def reference_blocks(net, x):
    """(inputs, skips, outputs) of the 56 blocks from the reference's own tensors, by hooks"""
    seen = {}

    def hook(name):
        return lambda mod, inp, out: seen.__setitem__(name, (inp[0].detach().clone(), out.detach().clone()))

    mods = dict(net.named_modules())
    hooks = [mods[c[1]].register_forward_hook(hook(c[1])) for c in nf.CONVS]  # each BatchNorm: its input is the conv's output
    hooks += [mods[c[0]].register_forward_hook(hook(c[0])) for c in nf.CONVS]
    hooks += [mods[n].register_forward_hook(hook(n)) for n in ("backbone.maxpool", "backbone.avgpool")]
    hooks += [mods[n].register_forward_hook(hook(n)) for n, m in mods.items() if n.count(".") == 2 and n.startswith("backbone.layer")]
    with torch.no_grad():
        y = net(x)
    for h in hooks:
        h.remove()
    ins, skips, outs = [None] * fr.N_BLOCKS, [None] * fr.N_BLOCKS, [None] * fr.N_BLOCKS
    for b, (conv, bn, _, _, _, _, _, role, relu) in enumerate(nf.CONVS):
        ins[b] = seen[conv][0]
        post = seen[bn][1]
        if role == 3:
            bottleneck = conv.rsplit(".", 1)[0]
            outs[b] = seen[bottleneck][1]                        # relu(bn3(conv3) + identity): the bottleneck's output
            down = bottleneck + ".downsample.1"
            skips[b] = seen[down][1] if down in seen else seen[bottleneck][0]
            assert float((torch.relu(post + skips[b]) - outs[b]).abs().max()) == 0.0
        else:
            outs[b] = torch.relu(post) if relu else post
    assert float((outs[0] - seen["backbone.maxpool"][0]).abs().max()) == 0.0  # the in-place ReLU's output is what the pool was fed
    ins[nf.POOL_BLOCK], outs[nf.POOL_BLOCK] = seen["backbone.maxpool"]
    ins[nf.AVG_BLOCK], outs[nf.AVG_BLOCK] = seen["backbone.avgpool"]
    ins[nf.HEAD_BLOCK], outs[nf.HEAD_BLOCK] = outs[nf.AVG_BLOCK], y
    return ins, skips, outs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    ap.add_argument("--ref", required=True, help="the checked-out reference project")
    args = ap.parse_args()
    sys.path.insert(0, args.ref)
    kornia, geometry = types.ModuleType("kornia"), types.ModuleType("kornia.geometry")
    geometry.warp_affine, kornia.geometry = None, geometry
    sys.modules.setdefault("kornia", kornia)
    sys.modules.setdefault("kornia.geometry", geometry)
    from PIL import Image
    import PIL
    from s_face3d.models import networks
    align_img = preprocess_functions(os.path.join(args.ref, "s_face3d", "util", "preprocess.py"))
    prepare = landmark_lines(os.path.join(args.ref, "XGaze_utils", "data_loader_xgaze_new.py"))
    lm3d_std = load_lm3d_function(os.path.join(args.ref, "s_face3d", "util", "load_mats.py"))(os.path.join(args.ref, "s_config"))
    lm3d_std = np.asarray(lm3d_std, dtype=np.float64)
    assert lm3d_std.shape == (5, 3)

    sd = syn.face_recon_state_dict(fr.WEIGHTS_SEED)
    net = networks.define_net_recon(net_recon="resnet50", use_last_fc=False, init_path="")
    assert list(net.state_dict().keys()) == list(nf.state_dict_keys().keys())
    assert all(m.eps == nf.BN_EPS for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d))
    net.load_state_dict(sd, strict=True)
    net = net.eval().double()
    checksum = float(sum(float(v.double().abs().sum()) for v in sd.values()))
    n_params = int(sum(p.numel() for p in net.parameters()))

    # ---- the network ------------------------------------------------------------------------------------------------------------
    arrays, samples, stats = {}, {}, {}
    bounds = {"block": [0.0] * fr.N_BLOCKS, "coeffs": 0.0}
    for case in fr.CASES:
        x = fr.fixture_images(case)
        ins, skips, outs = reference_blocks(net, x)
        e_ins, e_skips, e_outs = fr.chain(sd, x)
        worst = max(float((a - b).abs().max() / max(float(b.abs().max()), 1e-300)) for a, b in zip(e_outs, outs))
        assert worst < 1e-12, (case, worst)
        b = fr.measured_bounds(sd, x, ins, skips, outs)
        bounds["block"] = [max(p, q) for p, q in zip(bounds["block"], b["block"])]
        bounds["coeffs"] = max(bounds["coeffs"], b["coeffs"])
        zero = [float((o == 0).double().mean()) for o in outs]
        top = [float(o.abs().max()) for o in outs]
        assert max(zero) <= ZERO_SHARE_CAP, (case, max(zero), int(np.argmax(zero)))
        assert min(top) >= 1e-2 and max(top) <= 1e3, (case, min(top), max(top))
        y = outs[nf.HEAD_BLOCK]
        assert bool((y > 0).any()) and bool((y < 0).any())
        stats[case] = {"max_zero_share": max(zero), "min_abs_max": min(top), "max_abs_max": max(top),
                       "positive_share_of_coeffs": float((y > 0).double().mean())}
        sums = []
        for b_, act in enumerate(outs):
            s, sa, sample = fr.summary(act)
            sums.append([s, sa])
            samples["%s/block%02d/sample" % (case, b_)] = sample
        arrays[case + "/block_sums"] = np.array(sums)
        arrays[case + "/coeffs"] = y.numpy()
        print("%s: max zero share %.3f, |max| in [%.3g, %.3g], coeffs bound %.3g" % (case, max(zero), min(top), max(top), b["coeffs"]), flush=True)

    # ---- the aligner ------------------------------------------------------------------------------------------------------------
    align_arrays, align_stats = {"lm3d_std": lm3d_std}, {}
    pinv = nf.pos_pinv(lm3d_std)
    ts_err = byte_diff = byte_total = 0
    byte_worst, unq_bound, exp_bound = 0, 0.0, 0.0
    nearest = np.inf
    for case, (n, H, W) in fr.ALIGN_CASES.items():
        u8 = fr.fixture_frames(case)
        lms = fr.fixture_landmarks(case, lm3d_std)
        frames = fr.frames_f32(u8)
        m_crops, m_trans, m_geom, m_status, m_args = fr.align(frames.numpy(), lms, lm3d_std, True)
        u_crops = fr.align(frames.numpy(), lms, lm3d_std, False)[0]
        pil_crops = np.zeros((n, CROP, CROP, 3), dtype=np.uint8)
        ref_trans, ref_geom, ref_status = np.zeros((n, 5)), np.zeros((n, 4), dtype=np.int64), np.zeros(n, dtype=np.int64)
        for i in range(n):
            lm1 = np.array(lms[i], dtype=np.float64)
            if not np.isfinite(lm1).all():
                ref_status[i] = 1  # the reference has no such path: lstsq raises or returns NaN
                assert m_status[i] == 1
                continue
            img = RecordingImage(Image.fromarray(u8[i]))
            w0, h0 = img.size
            lm1 = prepare(types.SimpleNamespace(lm3d_std=lm3d_std), lm1, w0, h0)  # generate's own statement
            t, s, img_new = align_img(img, lm1, lm3d_std)                          # align_img's own statements
            pil_crops[i] = np.array(img_new)
            (w, h), (left, up) = img.calls["resize"], img.calls["crop"][:2]        # what the reference handed PIL
            assert all(isinstance(v, (int, np.integer)) for v in (w, h, left, up)) and img.calls["crop"][2:] == (left + 224., up + 224.)
            ref_trans[i] = [w0, h0, float(s), t[0].item(), t[1].item()]
            ref_geom[i] = [int(w), int(h), int(left), int(up)]
            # conditions: the restatement's pseudo-inverse against the reference's lstsq; every truncation's argument away from an integer
            err = np.abs(m_trans[i] - ref_trans[i]) / np.maximum(np.abs(ref_trans[i]), 1.0)
            ts_err = max(ts_err, float(err.max()))
            assert m_status[i] == 0 and tuple(m_geom[i]) == tuple(ref_geom[i]), (case, i, m_geom[i], ref_geom[i])
            dist = [abs(a - round(a)) for a in m_args[i]]
            if np.mean(lms[i]) == -1:
                # the fallback: ill-conditioned in the reference itself (tests/face_recon_restatement.fixture_landmarks); the
                # arguments that sit on an integer are named, the others hold the margin
                fallback_on_integer = [k for k, d_ in zip(("w", "h", "left", "up"), dist) if d_ <= TRUNC_MARGIN]
                assert fallback_on_integer == ["up"], fallback_on_integer
                fallback_distance = max(d_ for d_ in dist if d_ <= TRUNC_MARGIN)
                assert fallback_distance <= 1e-10  # on the integer up to the solver's rounding, not merely near it
                dist = [d_ for d_ in dist if d_ > TRUNC_MARGIN]
            nearest = min(nearest, min(dist))
            got = np.floor(m_crops[i].transpose(1, 2, 0) * 255.0 + 0.5).astype(np.int64)
            d = np.abs(got - pil_crops[i].astype(np.int64))
            byte_diff += int((d != 0).sum())
            byte_total += d.size
            byte_worst = max(byte_worst, int(d.max()))
            unq_bound = max(unq_bound, float(np.abs(u_crops[i].transpose(1, 2, 0) - pil_crops[i] / 255.0).max()))
        # the reference's coefficients of its own crops, and the emulation end to end from the frames
        x_ref = torch.as_tensor(pil_crops / 255.).permute(0, 3, 1, 2).float().double()  # generate's im_t is float32
        with torch.no_grad():
            ref_coeffs = net(x_ref)
        emu = fr.chain(sd, torch.as_tensor(m_crops).float(), True)[2][nf.HEAD_BLOCK].double()
        ok = ref_status == 0
        exp_bound = max(exp_bound, float((emu[ok][:, 80:144] - ref_coeffs[ok][:, 80:144]).abs().max()))
        align_arrays[case + "/frames_u8"] = u8
        align_arrays[case + "/points"] = np.array([np.asarray(l).shape[0] for l in lms], dtype=np.int64)
        align_arrays[case + "/landmarks"] = np.stack([np.concatenate((np.asarray(l, dtype=np.float64), np.zeros((68 - np.asarray(l).shape[0], 2)))) for l in lms])
        align_arrays[case + "/crops_u8"] = pil_crops
        align_arrays[case + "/trans_params"], align_arrays[case + "/geom"], align_arrays[case + "/status"] = ref_trans, ref_geom, ref_status
        align_arrays[case + "/coeffs"] = ref_coeffs.numpy()
        align_stats[case] = {"s": ref_trans[:, 2].tolist(), "geom": ref_geom.tolist(), "status": ref_status.tolist(),
                             "nonzero_share_of_crop": [float((pil_crops[i] != 0).mean()) for i in range(n)]}
    share = byte_diff / float(byte_total)
    print("aligner: t, s relative error %.3g; nearest truncation argument to an integer %.3g; bytes differing %.3g (worst %d levels); "
          "unrounded bound %.4g; expressions bound %.3g" % (ts_err, nearest, share, byte_worst, unq_bound, exp_bound), flush=True)
    assert nearest > TRUNC_MARGIN and TRUNC_MARGIN >= 100.0 * ts_err * 4096.0, (nearest, ts_err)
    assert share <= BYTE_CAP and byte_worst <= 1, (share, byte_worst)
    s_all = np.concatenate([np.array(v["s"])[np.array(v["status"]) == 0] for v in align_stats.values()])
    assert s_all.min() < 1.0 < s_all.max()
    g = np.concatenate([np.array(v["geom"])[np.array(v["status"]) == 0] for v in align_stats.values()])
    assert (g[:, 2] < 0).any() and (g[:, 3] < 0).any() and (g[:, 2] + CROP > g[:, 0]).any() and (g[:, 3] + CROP > g[:, 1]).any()
    assert ((g[:, 2] > 0) & (g[:, 3] > 0)).any(), "no crop starts inside the resized image"

    os.makedirs(args.out, exist_ok=True)
    written = []
    for name, group in (("face_recon", arrays), ("face_recon_blocks", samples), ("face_recon_align", align_arrays)):
        path = os.path.join(args.out, name + ".npz")
        np.savez_compressed(path, **group)
        written.append(path)
    digests = {}
    for name, group in (("face_recon", arrays), ("face_recon_blocks", samples), ("face_recon_align", align_arrays)):
        d = hashlib.sha256()
        for n_ in sorted(group):
            d.update(n_.encode())
            d.update(np.ascontiguousarray(group[n_]).tobytes())
        digests[name] = d.hexdigest()
    with open(os.path.join(args.out, "face_recon_blocks.json"), "w") as fjson:
        json.dump({"name": "face_recon_blocks", "generator": "tools/gen_golden_face_recon.py", "sample_stride": fr.SAMPLE_STRIDE,
                   "what": "every 331st element of each of the 56 blocks' float64 outputs (CASE/blockNN/sample) for the cases of "
                           "face_recon.npz; a file of its own for the size limit", "arrays_sha256": digests["face_recon_blocks"]},
                  fjson, indent=1, sort_keys=True)
    with open(os.path.join(args.out, "face_recon_align.json"), "w") as fjson:
        json.dump({
            "name": "face_recon_align", "generator": "tools/gen_golden_face_recon.py", "pil_version": PIL.__version__,
            "what": "align_img of s_face3d/util/preprocess.py over its POS, extract_5p and resize_n_crop_img (cut out by ast) behind "
                    "CropAndExtract.generate's landmark lines, with PIL's BICUBIC: per case the frames, the landmarks ([n,68,2], the "
                    "first `points` rows used), trans_params (w0, h0, s, t0, t1), geom (w, h, left, up), the PIL crops as bytes, and "
                    "the reference net's 257 coefficients of crops_u8 / 255; lm3d_std as load_lm3d returns it; status 1: a frame "
                    "the reference has no path for (non-finite landmarks), its rows are zeros",
            "cases": {k: list(v) for k, v in fr.ALIGN_CASES.items()}, "input_seed": fr.INPUT_SEED, "weights_seed": fr.WEIGHTS_SEED,
            "conditions": {"truncation_margin": TRUNC_MARGIN, "nearest_truncation_argument": float(nearest),
                           "t_s_relative_error_of_the_pseudo_inverse": ts_err, "byte_cap": BYTE_CAP, "bytes_differing_share": share,
                           "bytes_worst_levels": byte_worst,
                           "fallback_on_integer": fallback_on_integer, "fallback_distance_to_integer": float(fallback_distance),
                           "fallback": "the reference's fallback puts t at (w0 / 2, h0 / 2) exactly; one of its truncations always sits "
                                       "on an integer; the margin is asserted for every other argument of every frame"},
            "bounds": {"how": "expressions: max |emulation end to end from the frames (the restatement's byte crop, then the emulated "
                              "network) - the reference's exp of PIL's crop|; unquantized: max |the restatement's unrounded crop - PIL's "
                              "bytes / 255|; the GPU tests allow gpu_factor x these", "gpu_factor": GPU_FACTOR, "expressions": exp_bound,
                       "unquantized": unq_bound},
            "stats": align_stats, "arrays_sha256": digests["face_recon_align"]}, fjson, indent=1, sort_keys=True)
    manifest = {
        "name": "face_recon", "generator": "tools/gen_golden_face_recon.py",
        "what": "s_face3d/models/networks.py's define_net_recon('resnet50', use_last_fc=False) in float64 on the CPU, eval mode: per "
                "case the 257 coefficients and per block the output's sum and abs-sum",
        "inputs": "tests/face_recon_restatement.fixture_images(case): [n,3,H,W] in [0,1] on a grid of 1/256, seeded",
        "cases": {k: list(v) for k, v in fr.CASES.items()}, "block_names": nf.block_names(),
        "state_dict_keys": [[k, list(v.shape)] for k, v in net.state_dict().items()],
        "weights": "n3dt.synthetic.face_recon_state_dict(weights_seed): seeded stand-ins, not the pretrained net_recon",
        "weights_seed": fr.WEIGHTS_SEED, "weights_checksum": checksum, "input_seed": fr.INPUT_SEED, "n_params": n_params,
        "bn_eps": nf.BN_EPS,
        "parity_unpinned": {
            "weights": "the pretrained net_recon checkpoint has never been run through this code",
            "landmarks": "KeypointExtractor (face_alignment's FAN) and Preprocesser.crop: the landmarks stay the caller's",
            "resize_256": "cv2.resize to 256 in front of the aligner",
            "training": "training of the regressor, and use_last_fc=True",
        },
        "conditions": {"zero_share_cap": ZERO_SHARE_CAP, "abs_max_range": [1e-2, 1e3]},
        "bounds": {
            "how": "max |emulation - float64 reference| on the CPU over all cases; emulation = BatchNorm folded in float64, fp32 weights, "
                   "operands split into two bf16, three products, fp32 accumulation, float64 tails (tests/face_recon_restatement.py); "
                   "per block the block alone on the fp32-rounded reference input (and skip); the coefficients end to end; the GPU "
                   "tests allow gpu_factor x these",
            "gpu_factor": GPU_FACTOR, "block": bounds["block"], "coeffs": bounds["coeffs"],
        },
        "stats": stats, "arrays_sha256": digests["face_recon"], "block_samples": "tests/golden/face_recon_blocks.npz",
        "alignment": "tests/golden/face_recon_align.npz",
    }
    with open(os.path.join(args.out, "face_recon.json"), "w") as fjson:
        json.dump(manifest, fjson, indent=1, sort_keys=True)
    for path in written:
        assert os.path.getsize(path) < (1 << 20), (path, os.path.getsize(path))
        print("wrote %s (%.1f KB)" % (path, os.path.getsize(path) / 1024.0))
    print(json.dumps({"bounds": manifest["bounds"], "stats": stats}, indent=1))


CROP = nf.CROP

if __name__ == "__main__":
    main()
