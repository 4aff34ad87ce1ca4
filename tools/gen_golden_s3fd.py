#!/usr/bin/env python3
"""Generate tests/golden/s3fd.{npz,json} and tests/golden/s3fd_blocks.{npz,json} from the reference's own S3FD face detector
(face_detection/detection/sfd/{net_s3fd,detect,bbox,sfd_detector}.py under face_detection/api.py) in float64 on the CPU, and from
its loader's box code (get_smoothened_boxes and the pad lines of face_detect in XGaze_utils/data_loader_xgaze_new.py, cut out by
ast).

Runs only where the reference is checked out: it imports the reference's classes and functions at generation time; nothing of it
is stored.  cv2 is not installed here and is stubbed; nothing on the paths driven here calls it.  Weights:
n3dt.synthetic.s3fd_state_dict(WEIGHTS_SEED) loaded into the class with strict=True -- the pretrained detector is not available
offline; only the seed and a checksum are stored.  Inputs: byte frames, tests/s3fd_restatement.fixture_frames; the reference reads
them as bytes (BGR), the detector as float32 u8 / 255 (RGB).

Recorded per case: per block (hooks on the reference's 19 convolutions, 3 norms and 12 head convolutions; a block's ReLU output
and a pool's output are the tensors the reference's next module is fed) the sum, abs-sum and every 211th element; the twelve head
maps; the scores and decoded boxes of every head position (F.softmax and the reference's batch_decode); the detections of
SFDDetector.detect_from_batch; the rects of FaceAlignment.get_detections_for_batch; for the clip the padded and smoothed boxes for
its first 2, 3, 4, 5 and 9 frames; and one case with the second bias setting in which nothing is detected.

The manifest carries the bounds the GPU tests use, MEASURED HERE ON THE CPU: the error of the restatement's emulation of the
kernel's arithmetic against these float64 values -- per block (each block alone on the fp32-rounded reference input), for the head
maps, the scores and the box coordinates end to end.  The GPU tests allow 4 x the emulation's error.

The reference alone must satisfy the fixture conditions, asserted here (see check_conditions).  The stand-in conf heads carry one
face bias per level; `--search N` looks for a weights seed and biases for which the conditions can hold (search_face_biases), and
the pair that passed the full run is kept in tests/s3fd_restatement.WEIGHTS_SEED and n3dt.synthetic.S3FD_FACE_BIAS.

Usage:  python tools/gen_golden_s3fd.py [--out DIR] [--ref DIR]
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
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "nerf-3dtalker-code_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

from n3dt import synthetic as syn  # noqa: E402
from n3dt import s3fd as ns  # noqa: E402
import s3fd_restatement as sr  # noqa: E402

GPU_FACTOR = 4.0
SKIP_CAP = 0.02


def loader_functions(path):
    """(get_smoothened_boxes, pad) compiled from the reference loader's own statements: the function as it stands, and the four
    assignments y1, y2, x1, x2 of face_detect's loop as pad(rect, image, wav_pads) -> [x1, y1, x2, y2]"""
    tree = ast.parse(open(path).read())
    smooth = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "get_smoothened_boxes"]
    detect = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "face_detect"]
    assert len(smooth) == 1 and len(detect) == 1, "the loader no longer defines the two functions"
    loop = [n for n in detect[0].body if isinstance(n, ast.For) and isinstance(n.target, ast.Tuple)
            and [e.id for e in n.target.elts] == ["rect", "image"]]
    assert len(loop) == 1
    assigns = [n for n in loop[0].body if isinstance(n, ast.Assign) and n.targets[0].id in ("y1", "y2", "x1", "x2")]
    assert [n.targets[0].id for n in assigns] == ["y1", "y2", "x1", "x2"]
    unpack = ast.parse("pady1, pady2, padx1, padx2 = wav_pads").body
    ret = ast.parse("def pad(rect, image, wav_pads):\n    return [x1, y1, x2, y2]").body[0]
    ret.body = unpack + assigns + ret.body
    mod = ast.fix_missing_locations(ast.Module(body=smooth + [ret], type_ignores=[]))
    scope = {"np": np}
    exec(compile(mod, path, "exec"), scope)
    return scope["get_smoothened_boxes"], scope["pad"]


class Double(torch.nn.Module):
    """the reference's detect.py casts its input to float32: run the float64 network behind it and keep its output"""

    def __init__(self, net):
        super().__init__()
        self.net = net
        self.last = None

    def forward(self, x):
        self.last = self.net(x.double())
        return [t.clone() for t in self.last]


def reference_run(net, SFDDetector, FaceAlignment, batch_decode, u8):
    """everything the reference computes for frames u8 [n,H,W,3] RGB bytes"""
    mods = [getattr(net, c[0]) for c in ns.CONVS] + [getattr(net, n) for n in ns.NORMS]
    mods += [getattr(net, "%s_mbox_%s" % (s, part)) for s in ns.LEVEL_SOURCES for part in ("conf", "loc")]
    seen = {}
    hooks = [m.register_forward_hook(lambda mod, inp, out, i=i: seen.__setitem__(i, (inp[0].detach().clone(), out.detach().clone())))
             for i, m in enumerate(mods)]
    wrapped = Double(net)
    det = object.__new__(SFDDetector)
    det.device, det.verbose, det.face_detector = "cpu", False, wrapped
    fa = object.__new__(FaceAlignment)
    fa.face_detector = det
    images_bgr = np.ascontiguousarray(u8[..., ::-1])
    with torch.no_grad():
        rects = fa.get_detections_for_batch(images_bgr)      # reverses to RGB, then SFDDetector.detect_from_batch
        dets = det.detect_from_batch(u8.copy())
    for h in hooks:
        h.remove()
    maps = [t.detach().clone() for t in wrapped.last]
    # the blocks' inputs and outputs, from the reference's own tensors
    ins, outs = [None] * sr.N_BLOCKS, [None] * sr.N_BLOCKS
    pool = 0
    for c, conv in enumerate(ns.CONVS):
        ins[c] = seen[c][0]
        level = conv[7]
        if level and level <= 3:
            outs[c] = seen[ns.N_CONVS + level - 1][0]            # the L2Norm's input: the ReLU output
        elif level:
            outs[c] = seen[ns.N_CONVS + 3 + 2 * (level - 1)][0]  # the conf head's input
        else:
            outs[c] = seen[c + 1][0]
        if conv[6]:
            if not level:
                outs[c] = F.relu(seen[c][1])  # only the pool sees it: the ReLU of the module's own output
            ins[ns.FIRST_POOL + pool], outs[ns.FIRST_POOL + pool] = outs[c], seen[c + 1][0]
            pool += 1
    for l in range(3):
        ins[ns.FIRST_NORM + l], outs[ns.FIRST_NORM + l] = seen[ns.N_CONVS + l]
    for l in range(6):
        conf, loc = seen[ns.N_CONVS + 3 + 2 * l], seen[ns.N_CONVS + 3 + 2 * l + 1]
        ins[ns.FIRST_HEAD + l], outs[ns.FIRST_HEAD + l] = conf[0], torch.cat((conf[1], loc[1]), dim=1)
    # scores and decoded boxes of every position by the reference's own functions
    scores, boxes = [], []
    for l in range(6):
        cls, reg = maps[2 * l], maps[2 * l + 1]
        n, _, h, w = cls.shape
        stride = 2 ** (l + 2)
        scores.append(F.softmax(cls, dim=1)[:, 1].reshape(n, h * w))
        pri = torch.Tensor([[stride / 2 + x * stride, stride / 2 + y * stride, stride * 4 / 1.0, stride * 4 / 1.0] for y in range(h) for x in range(w)])
        boxes.append(batch_decode(reg.permute(0, 2, 3, 1).reshape(n, h * w, 4), pri.view(1, h * w, 4), [0.1, 0.2]))
    return {"rects": rects, "dets": dets, "maps": maps, "ins": ins, "outs": outs,
            "score": torch.cat(scores, dim=1).numpy(), "box": torch.cat(boxes, dim=1).numpy()}


def check_conditions(name, ref, bounds, stats):
    """the fixture conditions, of the reference alone"""
    score, box = ref["score"], ref["box"]
    share = (score > 0.5).mean(axis=1)
    assert share.min() >= 0.005 and share.max() <= 0.20, (name, share)
    margin = 100.0 * bounds["score"]
    print("%s: above 0.5 per image %s, nearest to 0.5 %s (score bound %.3g)" % (name, (score > 0.5).sum(axis=1), np.abs(score - 0.5).min(axis=1), bounds["score"]))
    kept_counts = []
    for i in range(score.shape[0]):
        visited = []
        dets, _ = sr.greedy_nms(score[i], box[i], sr.MAX_FACES, visited)
        kept_counts.append(len(dets))
        assert not visited or np.abs(np.array(visited) - 0.3).min() > 1e-3, (name, i, "an overlap within 1e-3 of 0.3")
        assert np.abs(score[i] - 0.5).min() > margin, (name, i, "a score within 100 x the bound of 0.5")
        cand = np.nonzero(score[i] > 0.5 - margin)[0]
        order = cand[np.argsort(score[i][cand])]
        gaps = np.diff(score[i][order])
        same = np.all(box[i][order][1:] == box[i][order][:-1], axis=1)
        assert gaps.size == 0 or gaps[~same].min() > margin, (name, i, "two scores within 100 x the bound", float(gaps.min()))
    zero = [float((o == 0).double().mean()) for o in ref["outs"]]
    assert max(zero) <= 0.6, (name, max(zero), int(np.argmax(zero)))
    stats[name] = {"share_above_half": share.tolist(), "kept": kept_counts, "max_zero_share": max(zero)}
    return kept_counts


def skipped_coordinates(ref, window):
    """(coordinates compared, skipped, top-box coordinates skipped): a kept detection's coordinate is skipped where the
    reference's real value, clipped at 0, lies within `window` of an integer"""
    total = skipped = top = 0
    for dets in ref["dets"]:
        for j, d in enumerate(dets):
            for v in np.clip(np.asarray(d[:4], dtype=np.float64), 0, None):
                near = abs(v - round(v)) <= window and v > window
                total += 1
                skipped += near
                top += near and j == 0
    return total, skipped, top


def search_face_biases(seed, case_maps, margin, trials):
    """Which per-level face biases could satisfy the score conditions for this seed: the bias of a level's face logit shifts
    c1 - c0 of every position of that level alike, so the reference runs once with zero biases and the candidates -- random
    draws around each level's largest c1 - c0 -- are judged on the shifted scores.  Prints the first draw for which every image
    has 0.5 - 20 % of its positions above 0.5, no score within `margin` of 0.5 and no two scores above 0.5 within `margin` of each
    other, or the best draw.  `margin` stands for 100 x the score bound, which is only measured by the full run."""
    diffs, firsts = [], []
    for case, maps in zip(sr.CASES, case_maps):
        d = torch.cat([(maps[2 * l][:, 1] - maps[2 * l][:, 0]).reshape(maps[0].shape[0], -1) for l in range(6)], dim=1).numpy()
        diffs.append(list(d))
        firsts.append(np.cumsum([0] + [h * w for h, w in ns.level_sizes(*sr.CASES[case][1:])]))
    tops = []
    for l in range(6):
        per_image = [d[f[l]:f[l + 1]].max() for case_diffs, f in zip(diffs, firsts) for d in case_diffs]
        tops.append((min(per_image), max(per_image)))
    rng = np.random.default_rng(seed)
    best = (0, None, "")
    for _ in range(trials):
        fb = np.array([-rng.uniform(lo - 3.0, hi + 3.0) for lo, hi in tops])
        passed, images, why = 0, 0, ""
        for case_diffs, f in zip(diffs, firsts):
            shift = np.concatenate([np.full(f[l + 1] - f[l], fb[l]) for l in range(6)])
            for d in case_diffs:
                sc = np.sort(1.0 / (1.0 + np.exp(-(d + shift))))
                above = sc[sc > 0.5 - margin]
                share = (sc > 0.5).mean()
                fails = (share < 0.005, share > 0.2, np.abs(sc - 0.5).min() <= margin, above.size > 1 and np.diff(above).min() <= margin)
                if any(fails):
                    why += "%d:%s " % (images, "".join("LHTG"[j] for j in range(4) if fails[j]))  # low, high, threshold, gap
                else:
                    passed += 1
                images += 1
        if passed > best[0]:
            best = (passed, [round(float(v), 3) for v in fb], why)
        if passed == images:
            break
    print("seed %d: %d of %d images pass with face biases %s %s" % (seed, best[0], images, best[1], best[2]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--seed", type=int, default=sr.WEIGHTS_SEED, help="weights seed; one for which the conditions hold is kept in "
                    "tests/s3fd_restatement.WEIGHTS_SEED (try --seed N until the assertions pass)")
    ap.add_argument("--face-bias", type=lambda v: [float(x) for x in v.split(",")], default=syn.S3FD_FACE_BIAS,
                    help="six comma-separated values, for tuning n3dt.synthetic.S3FD_FACE_BIAS; the committed fixture is written with the "
                    "module's own value only")
    ap.add_argument("--search", type=int, default=0, help="for this many seeds from --seed on, look for per-level face biases for "
                    "which the score conditions would hold with a score bound of --margin / 100 (search_face_biases); writes nothing")
    ap.add_argument("--margin", type=float, default=9e-3)
    ap.add_argument("--trials", type=int, default=40000)
    args = ap.parse_args()
    sys.path.insert(0, args.ref)
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    from face_detection.api import FaceAlignment
    from face_detection.detection.sfd.bbox import batch_decode
    from face_detection.detection.sfd.net_s3fd import s3fd
    from face_detection.detection.sfd.sfd_detector import SFDDetector
    get_smoothened_boxes, pad = loader_functions(os.path.join(args.ref, "XGaze_utils", "data_loader_xgaze_new.py"))

    seed = args.seed

    def reference_net(face_bias):
        sd = syn.s3fd_state_dict(seed, face_bias)
        net = s3fd()
        assert list(net.state_dict().keys()) == list(ns.state_dict_keys().keys())
        net.load_state_dict(sd, strict=True)
        return sd, net.eval().double()

    if args.search:
        for seed in range(args.seed, args.seed + args.search):
            _, net = reference_net((0.0,) * 6)
            maps = [reference_run(net, SFDDetector, FaceAlignment, batch_decode, sr.fixture_frames(case))["maps"] for case in sr.CASES]
            search_face_biases(seed, maps, args.margin, args.trials)
        return
    assert args.seed == sr.WEIGHTS_SEED and tuple(args.face_bias) == tuple(syn.S3FD_FACE_BIAS) or args.out != os.path.join(REPO, "tests", "golden"), \
        "the committed fixture is written with tests/s3fd_restatement.WEIGHTS_SEED and n3dt.synthetic.S3FD_FACE_BIAS only"
    sd, net = reference_net(args.face_bias)
    checksum = float(sum(float(v.double().abs().sum()) for v in sd.values()))
    n_params = int(sum(p.numel() for p in net.parameters()))

    arrays, samples, stats = {}, {}, {}
    bounds = {"block": [0.0] * sr.N_BLOCKS, "heads": [0.0] * 12, "score": 0.0, "box": 0.0}
    refs = {}
    for case in sr.CASES:
        u8 = sr.fixture_frames(case)
        ref = refs[case] = reference_run(net, SFDDetector, FaceAlignment, batch_decode, u8)
        frames = sr.frames_f32(u8)
        # the restatement must already agree with the class and functions it restates (on the bytes: the float frames' 255 u
        # differs from the byte by one float32 rounding of u, which the measured bounds below include)
        x_exact = torch.as_tensor(u8).permute(0, 3, 1, 2).double() - torch.tensor(ns.MEANS, dtype=torch.float64)[None, :, None, None]
        e_outs = sr.chain(sd, x_exact)[1]
        worst = max(float((x - y).abs().max() / max(float(y.abs().max()), 1e-300)) for x, y in zip(e_outs, ref["outs"]))
        assert worst < 1e-12, (case, worst)
        e_maps = sr.head_maps(e_outs)
        assert max(float((x - y).abs().max()) for x, y in zip(e_maps, ref["maps"])) < 1e-12
        r_score, r_box = sr.scores_and_boxes(ref["maps"])
        assert np.abs(r_score - ref["score"]).max() < 1e-12 and np.abs(r_box - ref["box"]).max() < 1e-9
        b = sr.measured_bounds(sd, frames, ref["ins"], ref["outs"], ref["maps"], ref["score"], ref["box"])
        bounds["block"] = [max(x, y) for x, y in zip(bounds["block"], b["block"])]
        bounds["heads"] = [max(x, y) for x, y in zip(bounds["heads"], b["heads"])]
        bounds["score"], bounds["box"] = max(bounds["score"], b["score"]), max(bounds["box"], b["box"])

    kept = {}
    for case, ref in refs.items():
        kept[case] = check_conditions(case, ref, bounds, stats)
        # the NMS-equivalence argument: the greedy tail on the recorded scores and boxes IS the reference's detections
        for i, dets in enumerate(ref["dets"]):
            mine, _ = sr.greedy_nms(ref["score"][i], ref["box"][i], 1 << 30)
            assert len(mine) == len(dets) and all(np.array_equal(np.asarray(a, dtype=np.float64), m) for a, m in zip(dets, mine)), (case, i)
            assert ref["rects"][i] == sr.top_rect(mine)
    assert max(max(k) for k in kept.values()) >= 3, kept

    window = GPU_FACTOR * bounds["box"]
    total = skipped = top = 0
    for ref in refs.values():
        t, s, p = skipped_coordinates(ref, window)
        total, skipped, top = total + t, skipped + s, top + p
    assert top == 0 and skipped <= SKIP_CAP * total, (total, skipped, top)

    # the empty case: the second bias setting, on case "b"
    sd_empty, net_empty = reference_net(syn.S3FD_EMPTY_FACE_BIAS)
    empty = reference_run(net_empty, SFDDetector, FaceAlignment, batch_decode, sr.fixture_frames("b"))
    assert float(empty["score"].max()) < 0.5 - 100.0 * bounds["score"]
    assert all(r is None for r in empty["rects"]) and all(len(d) == 0 for d in empty["dets"])

    for case, ref in refs.items():
        arrays[case + "/frames_u8"] = sr.fixture_frames(case)
        for k, m in enumerate(ref["maps"]):
            arrays["%s/head%02d" % (case, k)] = m.numpy()
        arrays[case + "/score"], arrays[case + "/box"] = ref["score"], ref["box"]
        n = len(ref["dets"])
        count = np.array([len(d) for d in ref["dets"]], dtype=np.int32)
        dets = np.zeros((n, max(1, int(count.max())), 5))
        for i, d in enumerate(ref["dets"]):
            for j, row in enumerate(d):
                dets[i, j] = row
        arrays[case + "/dets"], arrays[case + "/count"] = dets, count
        arrays[case + "/rects"] = np.array([r if r is not None else (-1, -1, -1, -1) for r in ref["rects"]], dtype=np.int64)
        sums = []
        for b_, act in enumerate(ref["outs"]):
            s, sa, sample = sr.summary(act)
            sums.append([s, sa])
            samples["%s/block%02d/sample" % (case, b_)] = sample
        arrays[case + "/block_sums"] = np.array(sums)
    # the loader's pads and smoothing on the clip's first F rects
    H, W = sr.CASES["clip"][1:]
    image = np.zeros((H, W, 3), dtype=np.uint8)
    for F_ in sr.SMOOTH_CASES:
        rects = refs["clip"]["rects"][:F_]
        padded = np.array([pad(r, image, list(sr.PADS)) for r in rects])
        arrays["clip/padded%d" % F_] = padded.copy()
        arrays["clip/smoothed%d" % F_] = np.array(get_smoothened_boxes(padded.copy(), T=sr.SMOOTH_T))

    os.makedirs(args.out, exist_ok=True)
    path, blocks_path = os.path.join(args.out, "s3fd.npz"), os.path.join(args.out, "s3fd_blocks.npz")
    np.savez_compressed(path, **arrays)
    np.savez_compressed(blocks_path, **samples)
    digest, blocks_digest = hashlib.sha256(), hashlib.sha256()
    for d, group in ((digest, arrays), (blocks_digest, samples)):
        for n in sorted(group):
            d.update(n.encode())
            d.update(np.ascontiguousarray(group[n]).tobytes())
    with open(os.path.join(args.out, "s3fd_blocks.json"), "w") as fjson:
        json.dump({"name": "s3fd_blocks", "generator": "tools/gen_golden_s3fd.py", "sample_stride": sr.SAMPLE_STRIDE,
                   "what": "every 211th element of each of the 33 blocks' float64 outputs (CASE/blockNN/sample) for the cases of s3fd.npz; a "
                           "file of its own for the size limit",
                   "arrays_sha256": blocks_digest.hexdigest()}, fjson, indent=1, sort_keys=True)
    manifest = {
        "name": "s3fd", "generator": "tools/gen_golden_s3fd.py",
        "what": "face_detection/detection/sfd (the reference's s3fd class, batch_detect, batch_decode, nms, SFDDetector.detect_from_batch) "
                "under FaceAlignment.get_detections_for_batch, in float64 on the CPU, and the loader's pad lines and get_smoothened_boxes: "
                "per case the twelve head maps, every position's score and decoded box, the detections, the rects, per block the "
                "output's sum and abs-sum; for the clip the padded and smoothed boxes of its first F frames",
        "inputs": "frames_u8 [n,H,W,3] RGB bytes: the reference reads them as bytes (BGR), the detector as float32 u8 / 255 [n,3,H,W]",
        "cases": {k: list(v) for k, v in sr.CASES.items()}, "smooth_cases": list(sr.SMOOTH_CASES), "pads": list(sr.PADS), "smooth": sr.SMOOTH_T,
        "block_names": ns.block_names(), "state_dict_keys": [[k, list(v.shape)] for k, v in net.state_dict().items()],
        "weights": "n3dt.synthetic.s3fd_state_dict(weights_seed, face_bias): seeded stand-ins, not the pretrained detector",
        "weights_seed": seed, "weights_checksum": checksum, "input_seed": sr.INPUT_SEED, "n_params": n_params,
        "face_bias": list(syn.S3FD_FACE_BIAS), "empty_face_bias": list(syn.S3FD_EMPTY_FACE_BIAS), "empty_case": "b",
        "empty_max_score": float(empty["score"].max()),
        "parity_unpinned": {
            "weights": "the pretrained s3fd-619a316812.pth has never been run through this code",
            "byte_frames": "the reference reads byte frames, the detector float frames: 255 u is not rounded to a byte",
            "float32_tail": "the reference decodes and suppresses in float32 on real runs; the tail here is float64, pinned to the "
                            "float64 run of the reference's functions within the recorded margins only",
        },
        "bounds": {
            "how": "max |emulation - float64 reference| on the CPU over all cases; emulation = fp32 weights, operands split into two "
                   "bf16, three products, fp32 accumulation, float64 tails (tests/s3fd_restatement.py); per block the block alone on "
                   "the fp32-rounded reference input; head maps, scores and box coordinates end to end from the float frames; the "
                   "GPU tests allow gpu_factor x these",
            "gpu_factor": GPU_FACTOR, "block": bounds["block"], "heads": bounds["heads"], "score": bounds["score"], "box": bounds["box"],
        },
        "coordinates": {"how": "a kept detection's coordinate is compared as an integer unless the reference's real value lies within "
                               "gpu_factor x bounds.box of an integer", "compared": int(total), "skipped": int(skipped),
                        "skipped_share": skipped / float(total), "cap": SKIP_CAP, "top_box_skipped": int(top)},
        "stats": stats, "arrays_sha256": digest.hexdigest(), "block_samples": "tests/golden/s3fd_blocks.npz",
    }
    with open(os.path.join(args.out, "s3fd.json"), "w") as fjson:
        json.dump(manifest, fjson, indent=1, sort_keys=True)
    for written in (path, blocks_path):
        assert os.path.getsize(written) < (1 << 20), written
        print("wrote %s (%.1f KB)" % (written, os.path.getsize(written) / 1024.0))
    print(json.dumps({k: manifest[k] for k in ("bounds", "coordinates", "stats", "n_params")}, indent=1))


if __name__ == "__main__":
    main()
