#!/usr/bin/env python3
"""Generate tests/golden/head_mask.{npz,json} and head_mask_blocks.{npz,json} from the reference's own face parser
(DataProcess/BiSeNet.py over DataProcess/resnet.py) in float64 on the CPU.

Runs only where the reference is checked out: the class and function definitions of the two files are cut out with ast at
generation time and compiled into a namespace of this tool's making; nothing of them is stored.  BiSeNet.py imports torchvision,
which is absent, and resnet.py is never imported as a module: Resnet18.__init__ calls init_weight, which calls
modelzoo.load_url on an https address.  The namespace's `modelzoo` is a stand-in whose load_url returns {} without touching the
network, and the tool asserts that the stand-in was what got called.  Weights: n3dt.synthetic.head_mask_state_dict(WEIGHTS_SEED)
loaded into the class with strict=True -- faceparsing_model.pth is not available offline; only the seed and a checksum are stored.

Recorded per end-to-end case: the three low-resolution logit maps (hooks on the heads' last convolutions) in full where they have
at most FULL_CAP elements, else as sum, abs-sum and every 257th element; the reference's label map from pred_res[2] (argmax of its
own upsampled output), five bit planes packed; the pixels whose float64 top-two margin lies below the exclusion threshold.  Per
block alone, for the small cases: the output's sum, abs-sum and every 257th element.

The manifest carries the bounds the GPU tests use, MEASURED HERE ON THE CPU: the error of the restatement's emulation of the
kernel's arithmetic against these float64 values -- per block (each block alone on the fp32-rounded reference inputs) and the
three logit maps end to end.  The GPU tests allow 4 x those.  The reference alone must satisfy the fixture conditions, asserted
here (see main).

Usage:  python tools/gen_golden_head_mask.py --ref DIR [--out DIR]
"""
import argparse
import ast
import hashlib
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "nerf-3dtalker-code_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

from n3dt import synthetic as syn  # noqa: E402
from n3dt import head_mask as nh  # noqa: E402
import head_mask_restatement as hr  # noqa: E402

GPU_FACTOR = 4.0
ZERO_SHARE_CAP = 0.6
LOW_MARGIN_CAP = 0.01
CLASS_SHARE = 0.01
FULL_CAP = 10000


class ModelZooStandIn(object):
    """what the cut-out namespace sees as `modelzoo`: load_url hands back an empty state dict and counts its calls"""

    def __init__(self):
        self.calls = 0

    def load_url(self, *args, **kwargs):
        self.calls += 1
        return {}


def reference_classes(ref):
    """BiSeNet, compiled from the class and function definitions of the reference's two files over a stand-in modelzoo"""
    zoo = ModelZooStandIn()
    scope = {"torch": torch, "nn": nn, "F": F, "modelzoo": zoo, "resnet18_url": "stand-in: nothing is fetched"}
    for name in ("resnet.py", "BiSeNet.py"):
        path = os.path.join(ref, "DataProcess", name)
        tree = ast.parse(open(path).read())
        defs = [n for n in tree.body if isinstance(n, (ast.ClassDef, ast.FunctionDef))]
        assert defs, path
        exec(compile(ast.fix_missing_locations(ast.Module(body=defs, type_ignores=[])), path, "exec"), scope)
    return scope["BiSeNet"], zoo


def reference_blocks(net, x):
    """(ins, outs, upsampled outputs) of the 37 blocks from the reference's own tensors, by hooks"""
    seen = {}

    def hook(name):
        def keep(mod, inp, out):
            if torch.is_tensor(out):  # the backbone and the context path return tuples: their parts are hooked themselves
                seen[name] = (inp[0].detach().clone(), out.detach().clone())
        return keep

    hooks = [m.register_forward_hook(hook(n)) for n, m in net.named_modules() if n]
    with torch.no_grad():
        ups = net(x)
    for h in hooks:
        h.remove()
    ins, outs = [None] * hr.N_BLOCKS, [None] * hr.N_BLOCKS
    r = "cp.resnet."
    ins[0], outs[0] = dict(x=seen[r + "conv1"][0]), torch.relu(seen[r + "bn1"][1])
    assert float((outs[0] - seen[r + "maxpool"][0]).abs().max()) == 0.0
    ins[nh.POOL_BLOCK], outs[nh.POOL_BLOCK] = dict(x=seen[r + "maxpool"][0]), seen[r + "maxpool"][1]
    b = 1
    for layer in range(1, 5):
        for i in range(2):
            p = "%slayer%d.%d" % (r, layer, i)
            down = p + ".downsample.1" in seen
            ins[b], outs[b] = dict(x=seen[p][0]), torch.relu(seen[p + ".bn1"][1])
            assert float((outs[b] - seen[p + ".conv2"][0]).abs().max()) == 0.0
            if down:
                ins[b + 2], outs[b + 2] = dict(x=seen[p][0]), seen[p + ".downsample.1"][1]
            shortcut = outs[b + 2] if down else seen[p][0]
            ins[b + 1], outs[b + 1] = dict(x=outs[b], aux=shortcut), seen[p][1]
            assert float((torch.relu(shortcut + seen[p + ".bn2"][1]) - outs[b + 1]).abs().max()) == 0.0
            b += 3 if down else 2
    assert b == nh.ARM16
    f8, f16, f32 = (seen["%slayer%d.1" % (r, k)][1] for k in (2, 3, 4))
    vec = lambda name: seen[name][1].flatten(1)  # noqa: E731
    ins[nh.AVG], outs[nh.AVG] = dict(x=f32), vec("cp.conv_avg")
    for arm, feat, conv, att in (("cp.arm32", f32, nh.ARM32, nh.ARM32_ATT), ("cp.arm16", f16, nh.ARM16, nh.ARM16_ATT)):
        ins[conv], outs[conv] = dict(x=feat), seen[arm + ".conv"][1]
        ins[att], outs[att] = dict(x=outs[conv]), vec(arm + ".sigmoid_atten")
    ins[nh.HEAD32] = dict(x=outs[nh.ARM32], scale=outs[nh.ARM32_ATT], addvec=outs[nh.AVG], size=tuple(f16.shape[2:]))
    outs[nh.HEAD32] = cp16 = seen["cp.conv_head32"][1]
    ins[nh.HEAD16] = dict(x=outs[nh.ARM16], scale=outs[nh.ARM16_ATT], aux=cp16, size=tuple(f8.shape[2:]))
    outs[nh.HEAD16] = cp8 = seen["cp.conv_head16"][1]
    ins[nh.FFM_BLK], outs[nh.FFM_BLK] = dict(x=f8, aux=cp8), seen["ffm.convblk"][1]
    ins[nh.FFM_1], outs[nh.FFM_1] = dict(x=outs[nh.FFM_BLK]), vec("ffm.relu")
    ins[nh.FFM_2], outs[nh.FFM_2] = dict(x=seen["ffm.relu"][1]), vec("ffm.sigmoid")
    ins[nh.OUT] = dict(x=outs[nh.FFM_BLK], scale=outs[nh.FFM_2])
    for head, blk, feat in (("conv_out", nh.OUT, None), ("conv_out16", nh.OUT16, cp8), ("conv_out32", nh.OUT32, cp16)):
        if feat is not None:
            ins[blk] = dict(x=feat)
        outs[blk] = seen[head + ".conv"][1]
        ins[blk + 1], outs[blk + 1] = dict(x=outs[blk]), seen[head + ".conv_out"][1]
    # what the reference itself fed the two resampling convolutions and the fusion head: the restated fetch transform, exactly
    fed = {nh.HEAD32: seen["cp.conv_head32"][0], nh.HEAD16: seen["cp.conv_head16"][0], nh.OUT: seen["conv_out"][0]}
    for blk, t in fed.items():
        a = ins[blk]
        v = a["x"] * a["scale"][:, :, None, None] + (a["addvec"][:, :, None, None] if "addvec" in a else a["aux"] if "aux" in a else a["x"])
        if "size" in a:
            v = F.interpolate(v, a["size"], mode="nearest")
        assert float((v - t).abs().max()) <= 1e-12 * max(float(t.abs().max()), 1.0), blk
    assert all(o is not None for o in outs)
    return ins, outs, ups


def pack_labels(lab):
    """uint8 labels < 32 -> five bit planes, packed"""
    flat = np.asarray(lab, dtype=np.uint8).reshape(-1)
    return np.packbits(np.stack([(flat >> k) & 1 for k in range(5)]), axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    ap.add_argument("--ref", required=True, help="the checked-out reference project")
    args = ap.parse_args()
    BiSeNet, zoo = reference_classes(args.ref)
    sd = syn.head_mask_state_dict(hr.WEIGHTS_SEED, hr.N_CLASSES)
    net = BiSeNet(n_classes=hr.N_CLASSES)
    assert zoo.calls == 1, "Resnet18.init_weight did not go through the stand-in modelzoo"
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == list(nh.state_dict_keys(hr.N_CLASSES).items())
    assert all(m.eps == nh.BN_EPS for m in net.modules() if isinstance(m, nn.BatchNorm2d))
    net.load_state_dict(sd, strict=True)
    net = net.eval().double()
    checksum = float(sum(float(v.double().abs().sum()) for v in sd.values()))

    arrays, samples, stats = {}, {}, {}
    bounds = {"block": [0.0] * hr.N_BLOCKS, "logits": [0.0, 0.0, 0.0]}
    per_case = {}
    for case, (n, H, W) in hr.CASES.items():
        x = hr.normalise(hr.fixture_frames(case)).double()
        ins, outs, ups = reference_blocks(net, x)
        e_ins, e_outs = hr.chain(sd, x)
        worst = max(float((a - b).abs().max() / max(float(b.abs().max()), 1e-300)) for a, b in zip(e_outs, outs))
        assert worst < 1e-12, (case, worst)
        for o, blk in enumerate(hr.LOGIT_BLOCKS):  # the restated upsample against the class's own outputs
            assert float((hr.upsample(outs[blk], H, W) - ups[o]).abs().max()) <= 1e-12 * float(ups[o].abs().max())
        b = hr.measured_bounds(sd, x, ins, outs)
        per_case[case] = b
        if case in hr.BLOCK_CASES:
            bounds["block"] = [max(p, q) for p, q in zip(bounds["block"], b["block"])]
        bounds["logits"] = [max(p, q) for p, q in zip(bounds["logits"], b["logits"])]
        print("%s: logits bounds %s" % (case, ["%.3g" % v for v in b["logits"]]), flush=True)
        if case in hr.BLOCK_CASES:
            zero = [float((o == 0).double().mean()) for o in outs]
            top = [float(o.abs().max()) for o in outs]
            assert max(zero) <= ZERO_SHARE_CAP, (case, max(zero), int(np.argmax(zero)))
            assert min(top) >= 1e-2 and max(top) <= 1e3, (case, min(top), max(top))
            sums = []
            for b_, act in enumerate(outs):
                s, sa, sample = hr.summary(act)
                sums.append([s, sa])
                samples["%s/block%02d/sample" % (case, b_)] = sample
            arrays[case + "/block_sums"] = np.array(sums)
            stats[case] = {"max_zero_share": max(zero), "min_abs_max": min(top), "max_abs_max": max(top)}
        for o, blk in enumerate(hr.LOGIT_BLOCKS):
            s, sa, sample = hr.summary(outs[blk])
            arrays["%s/logits%d/sums" % (case, o)] = np.array([s, sa])
            arrays["%s/logits%d/%s" % (case, o, "full" if outs[blk].numel() <= FULL_CAP else "sample")] = outs[blk].numpy() if outs[blk].numel() <= FULL_CAP else sample
        per_case[case]["ups2"], per_case[case]["labels"] = ups[2], ups[2].numpy().argmax(1).astype(np.uint8)
        per_case[case]["lg2"] = outs[hr.LOGIT_BLOCKS[2]].numpy()

    # ---- the labels, judged with the final bound ----------------------------------------------------------------------------------
    threshold = 2.0 * GPU_FACTOR * bounds["logits"][2]
    for case, (n, H, W) in hr.CASES.items():
        lab, ups2 = per_case[case]["labels"], per_case[case]["ups2"]
        low = hr.margins(ups2) < threshold
        share = float(low.mean())
        counts = np.bincount(lab.reshape(-1), minlength=hr.N_CLASSES) / float(lab.size)
        big = np.nonzero(counts >= CLASS_SHARE)[0]
        rule = hr.labels_from_logits(per_case[case]["lg2"], H, W)
        assert np.array_equal(rule[~low], lab[~low]), case  # the kernel's label rule on float64 logits: the argmax outside the set
        assert share <= LOW_MARGIN_CAP, (case, share)
        assert len(big) >= 6 and (4 in big or 5 in big) and 17 in big and any(1 <= c <= 13 for c in big), (case, counts.round(3).tolist())
        arrays[case + "/labels_packed"] = pack_labels(lab)
        arrays[case + "/low_margin"] = np.flatnonzero(low.reshape(-1)).astype(np.int32)
        stats.setdefault(case, {}).update({"low_margin_share": share, "class_shares": counts.round(4).tolist(),
                                           "classes_with_1_percent": [int(c) for c in big]})
        print("%s: low-margin share %.4g, classes >= 1%%: %s" % (case, share, big.tolist()), flush=True)

    os.makedirs(args.out, exist_ok=True)
    digests = {}
    for name, group in (("head_mask", arrays), ("head_mask_blocks", samples)):
        path = os.path.join(args.out, name + ".npz")
        np.savez_compressed(path, **group)
        assert os.path.getsize(path) < (1 << 20), (path, os.path.getsize(path))
        print("wrote %s (%.1f KB)" % (path, os.path.getsize(path) / 1024.0))
        d = hashlib.sha256()
        for n_ in sorted(group):
            d.update(n_.encode())
            d.update(np.ascontiguousarray(group[n_]).tobytes())
        digests[name] = d.hexdigest()
    with open(os.path.join(args.out, "head_mask_blocks.json"), "w") as fjson:
        json.dump({"name": "head_mask_blocks", "generator": "tools/gen_golden_head_mask.py", "sample_stride": hr.SAMPLE_STRIDE,
                   "what": "every 257th element of each of the 37 blocks' float64 outputs (CASE/blockNN/sample) for the small cases of "
                           "head_mask.npz; a file of its own for the size limit", "cases": list(hr.BLOCK_CASES),
                   "arrays_sha256": digests["head_mask_blocks"]}, fjson, indent=1, sort_keys=True)
    manifest = {
        "name": "head_mask", "generator": "tools/gen_golden_head_mask.py",
        "what": "DataProcess/BiSeNet.py's BiSeNet(19) over DataProcess/resnet.py's Resnet18 (definitions cut out by ast, modelzoo "
                "replaced by a stand-in) in float64 on the CPU, eval mode: per case the three low-resolution logit maps, the labels "
                "argmax(pred_res[2]) as five packed bit planes, the flat indices of the low-margin pixels; per small case the blocks' "
                "sums and abs-sums",
        "inputs": "tests/head_mask_restatement.normalise(fixture_frames(case)): seeded uint8 frames through ToTensor + Normalize in fp32",
        "cases": {k: list(v) for k, v in hr.CASES.items()}, "block_cases": list(hr.BLOCK_CASES), "block_names": nh.block_names(),
        "state_dict_keys": [[k, list(v.shape)] for k, v in net.state_dict().items()], "n_classes": hr.N_CLASSES,
        "weights": "n3dt.synthetic.head_mask_state_dict(weights_seed, 19): seeded stand-ins, not faceparsing_model.pth",
        "weights_seed": hr.WEIGHTS_SEED, "weights_checksum": checksum, "input_seed": hr.INPUT_SEED, "bn_eps": nh.BN_EPS,
        "full_cap": FULL_CAP, "sample_stride": hr.SAMPLE_STRIDE,
        "parity_unpinned": {
            "weights": "the pretrained faceparsing_model.pth has never been run through this code",
            "connected_components": "OpenCV's connectedComponents numbering on area ties",
            "ellipse": "getStructuringElement(MORPH_ELLIPSE), restated from knowledge of it",
            "hue": "cvtColor's 8-bit hue tables, restated from knowledge of them",
            "resize": "cv2.resize (INTER_LINEAR, fixed point) is not reproduced",
        },
        "conditions": {"zero_share_cap": ZERO_SHARE_CAP, "abs_max_range": [1e-2, 1e3], "low_margin_cap": LOW_MARGIN_CAP,
                       "low_margin_threshold": threshold, "class_share": CLASS_SHARE},
        "bounds": {
            "how": "max |emulation - float64 reference| on the CPU; emulation = BatchNorm folded in float64, fp32 weights, operands split "
                   "into two bf16, three products, fp32 accumulation, the fetch transform in fp32, float64 small stage "
                   "(tests/head_mask_restatement.py); per block the block alone on the fp32-rounded reference inputs over the small "
                   "cases; the three logit maps end to end over all cases; the GPU tests allow gpu_factor x these",
            "gpu_factor": GPU_FACTOR, "block": bounds["block"], "logits": bounds["logits"],
            "logits_per_case": {c: per_case[c]["logits"] for c in hr.CASES},
        },
        "stats": stats, "arrays_sha256": digests["head_mask"], "block_samples": "tests/golden/head_mask_blocks.npz",
    }
    with open(os.path.join(args.out, "head_mask.json"), "w") as fjson:
        json.dump(manifest, fjson, indent=1, sort_keys=True)
    print(json.dumps({"bounds": manifest["bounds"], "stats": stats}, indent=1))


if __name__ == "__main__":
    main()
