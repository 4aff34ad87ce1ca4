#!/usr/bin/env python3
"""Generate tests/golden/syncnet.{npz,json} from the reference's own SyncNet_color (wav_models/syncnet.py over wav_models/conv.py) in
float64, eval mode, on the CPU.

Runs only where the reference is checked out: it imports the reference's class at generation time; nothing of it is stored.
Weights: n3dt.synthetic.syncnet_state_dict(WEIGHTS_SEED) loaded into the class with strict=True -- the pretrained expert is not
available offline; only the seed and a checksum are stored.  Inputs: N_WINDOWS face windows as bytes (/ 255) and mel windows as
bytes (/ 32 - 4), tests/syncnet_restatement.fixture_inputs.  Recorded: both embeddings, the cosines and, per block, the sum, the
abs-sum and every 97th element of the activation (forward hooks on the reference's blocks).

The manifest also carries the bounds the GPU tests use, MEASURED HERE ON THE CPU: the error of the restatement's emulation of the
kernel's arithmetic (folded weights, operands split into two bf16, three products, fp32 accumulation) against these float64
values -- per block (each block alone on the fp32-rounded reference input), for the embeddings and for the cosine -- and, for
orientation, the reference's class in plain float32.  The GPU tests allow 4 x the emulation's error.

Unpinned, and recorded as such: the face-window convention (not in the reference; written from knowledge of Wav2Lip), OpenCV's
fixed-point byte resize (not reproduced), and the real weights (never run through this code).

Usage:  python tools/gen_golden_syncnet.py [--out DIR] [--ref DIR]
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "nerf-3dtalker-code_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

from n3dt import synthetic as syn  # noqa: E402
import syncnet_restatement as sr  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    sys.path.insert(0, args.ref)
    from wav_models.syncnet import SyncNet_color

    sd = syn.syncnet_state_dict(sr.WEIGHTS_SEED)
    checksum = float(sum(float(v.double().abs().sum()) for v in sd.values()))
    ref = SyncNet_color()
    ref.load_state_dict(sd, strict=True)
    ref.eval()
    n_params = int(sum(p.numel() for p in ref.parameters()))
    ref32 = SyncNet_color()
    ref32.load_state_dict(sd, strict=True)
    ref32.eval()
    ref = ref.double()

    faces_u8, mel_u8 = sr.fixture_inputs()
    faces, mel = sr.faces_from_u8(faces_u8), sr.mel_from_u8(mel_u8)

    acts = []
    hooks = [m.register_forward_hook(lambda mod, inp, out: acts.append(out.detach().clone()))
             for m in list(ref.face_encoder) + list(ref.audio_encoder)]
    with torch.no_grad():
        a, f = ref(mel, faces)
        a32, f32 = ref32(mel.float(), faces.float())
    for h in hooks:
        h.remove()
    assert len(acts) == 31
    cos = (a * f).sum(dim=1)

    # the restatement must already agree with the class it restates
    r_acts, r_a, r_f, r_cos = sr.chain64(sd, faces, mel)
    worst = max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(r_acts, acts))
    assert worst < 1e-12 and float((r_cos - cos).abs().max()) < 1e-12, worst

    bounds = sr.measured_bounds(sd, faces, mel, acts, a, f, cos)
    arrays = {"faces_u8": faces_u8, "mel_u8": mel_u8, "audio_emb": a.numpy(), "face_emb": f.numpy(), "cos": cos.numpy()}
    sums, scales = [], []
    for b, act in enumerate(acts):
        s, sa, sample = sr.summary(act)
        sums.append([s, sa])
        scales.append(float(act.abs().max()))
        arrays["block%02d/sample" % b] = sample
    arrays["block_sums"] = np.array(sums, dtype=np.float64)

    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "syncnet.npz")
    np.savez_compressed(path, **arrays)
    digest = hashlib.sha256()
    for n in sorted(arrays):
        digest.update(n.encode())
        digest.update(np.ascontiguousarray(arrays[n]).tobytes())
    manifest = {
        "name": "syncnet", "generator": "tools/gen_golden_syncnet.py",
        "what": "wav_models/syncnet.py SyncNet_color (the reference's class) in float64, eval mode, on the CPU: both embeddings "
                "[n,512], their cosines [n], and per block the activation's sum, abs-sum and every 97th element",
        "inputs": "face windows = faces_u8 / 255 [n,15,48,96]; mel windows = mel_u8 / 32 - 4 [n,1,80,16]",
        "n_windows": sr.N_WINDOWS, "sample_stride": sr.SAMPLE_STRIDE,
        "weights": "n3dt.synthetic.syncnet_state_dict(weights_seed): seeded stand-ins, not the pretrained expert",
        "weights_seed": sr.WEIGHTS_SEED, "weights_checksum": checksum, "input_seed": sr.INPUT_SEED, "n_params": n_params,
        "block_shapes": [list(x.shape[1:]) for x in acts], "block_max_abs": scales,
        "pinned": ["every block (conv, batch norm, residual, ReLU)", "the normalisation", "the cosine"],
        "parity_unpinned": {
            "window_convention": "lower half of a 96x96 crop, BGR, /255, five frames along the channels: written from knowledge of "
                                 "Wav2Lip; the reference holds no code that feeds SyncNet_color",
            "opencv_resize": "OpenCV's fixed-point resize on bytes is not reproduced: the prologue resamples floats bilinearly with "
                             "half-pixel centres in float64",
            "weights": "the pretrained lipsync_expert.pth has never been run through this code",
        },
        "bounds": {
            "how": "max |emulation - float64 reference| on the CPU over the fixture's windows; emulation = folded fp32 weights, "
                   "operands split into two bf16, three products, fp32 accumulation (tests/syncnet_restatement.py); per block the "
                   "block alone on the fp32-rounded reference input; the GPU tests allow gpu_factor x these",
            "gpu_factor": 4.0, "block": bounds["block"], "embedding": bounds["embedding"], "cos": bounds["cos"],
        },
        "float32_class_error": {"embedding": max(float((a32.double() - a).abs().max()), float((f32.double() - f).abs().max()))},
        "stats": {"embedding_max": float(max(a.max(), f.max())), "embedding_zero_share": float(((a == 0).double().mean() + (f == 0).double().mean()) / 2),
                  "cos": cos.tolist()},
        "arrays_sha256": digest.hexdigest(),
    }
    with open(os.path.join(args.out, "syncnet.json"), "w") as fjson:
        json.dump(manifest, fjson, indent=1, sort_keys=True)
    print("wrote %s (%.1f KB)" % (path, os.path.getsize(path) / 1024.0))
    print(json.dumps({k: manifest[k] for k in ("bounds", "float32_class_error", "stats", "n_params")}, indent=1))


if __name__ == "__main__":
    main()
