#!/usr/bin/env python3
"""Generate tests/golden/wav2lip.{npz,json} from the reference's own Wav2Lip (wav_models/wav2lip.py over wav_models/conv.py) in
float64, eval mode, on the CPU.

Runs only where the reference is checked out: it imports the reference's class at generation time; nothing of it is stored.
Weights: n3dt.synthetic.wav2lip_state_dict(WEIGHTS_SEED) loaded into the class with strict=True -- the pretrained generator is not
available offline; only the seed and a checksum are stored.  Inputs: N_WINDOWS face inputs as bytes (/ 255, rows 48..95 of
channels 0..2 zero) and mel windows as bytes (/ 32 - 4), tests/wav2lip_restatement.fixture_inputs.  Recorded: the float64 image
[3,3,96,96]; per block (forward hooks on the reference's 51 blocks, the last being the plain output convolution, i.e. the
pre-sigmoid logits) the sum, the abs-sum and every 97th element of the activation; the same three of one 5-D call
[1,3,1,80,16] / [1,6,3,96,96] of the same windows.  Three pairs of files, each within the size limit for a committed file:
tests/golden/wav2lip.{npz,json} (inputs, image, sums, the 5-D call, the manifest with the bounds), wav2lip_logits.{npz,json} (the
pre-sigmoid logits [3,3,96,96] in full) and wav2lip_blocks.{npz,json} (the per-block samples).

The manifest also carries the bounds the GPU tests use, MEASURED HERE ON THE CPU: the error of the restatement's emulation of the
kernel's arithmetic against these float64 values -- per block (each block alone on the fp32-rounded reference input), for the
logits and for the image end to end.  The GPU tests allow 4 x the emulation's error.

The reference alone must satisfy the fixture conditions, asserted here: the image spans at least [0.2, 0.8], at most 1 % of it
lies outside (0.02, 0.98), and no block's output is more than 60 % zeros.

Unpinned, and recorded as such: OpenCV's byte resize (not reproduced) and the real weights (never run through this code).

Usage:  python tools/gen_golden_wav2lip.py [--out DIR] [--ref DIR]
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
import wav2lip_restatement as wr  # noqa: E402


def reference_blocks(ref):
    """the reference's 51 block modules in state-dict order"""
    mods = [m for seq in ref.face_encoder_blocks for m in seq] + list(ref.audio_encoder)
    mods += [m for seq in ref.face_decoder_blocks for m in seq]
    return mods + [ref.output_block[0], ref.output_block[1]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    sys.path.insert(0, args.ref)
    from wav_models.wav2lip import Wav2Lip

    sd = syn.wav2lip_state_dict(wr.WEIGHTS_SEED)
    checksum = float(sum(float(v.double().abs().sum()) for v in sd.values()))
    ref = Wav2Lip()
    ref.load_state_dict(sd, strict=True)
    ref.eval()
    n_params = int(sum(p.numel() for p in ref.parameters()))
    ref = ref.double()

    faces_u8, mel_u8 = wr.fixture_inputs()
    faces, mel = wr.faces_from_u8(faces_u8), wr.mel_from_u8(mel_u8)

    acts = {}
    mods = reference_blocks(ref)
    assert len(mods) == wr.N_BLOCKS
    hooks = [m.register_forward_hook(lambda mod, inp, out, b=b: acts.__setitem__(b, out.detach().clone())) for b, m in enumerate(mods)]
    with torch.no_grad():
        image = ref(mel, faces)
    for h in hooks:
        h.remove()
    acts = [acts[b] for b in range(wr.N_BLOCKS)]
    with torch.no_grad():
        image5 = ref(mel[None], faces.permute(1, 0, 2, 3)[None])
    assert tuple(image5.shape) == (1, 3, wr.N_WINDOWS, 96, 96)

    # the restatement must already agree with the class it restates
    r_acts, r_image = wr.chain64(sd, faces, mel)
    worst = max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(r_acts, acts))
    assert worst < 1e-12 and float((r_image - image).abs().max()) < 1e-12, worst

    # the fixture conditions, of the reference alone
    outside = float(((image <= 0.02) | (image >= 0.98)).double().mean())
    zero_share = [float((a == 0).double().mean()) for a in acts]
    assert float(image.min()) <= 0.2 and float(image.max()) >= 0.8, (float(image.min()), float(image.max()))
    assert outside <= 0.01, outside
    assert max(zero_share) <= 0.6, max(zero_share)

    bounds = wr.measured_bounds(sd, faces, mel, acts, image)
    arrays = {"faces_u8": faces_u8, "mel_u8": mel_u8, "image": image.numpy()}
    sums, scales, samples = [], [], {}
    for b, act in enumerate(acts):
        s, sa, sample = wr.summary(act)
        sums.append([s, sa])
        scales.append(float(act.abs().max()))
        samples["block%02d/sample" % b] = sample
    arrays["block_sums"] = np.array(sums, dtype=np.float64)
    s5, sa5, sample5 = wr.summary(image5)
    arrays["image5/sums"] = np.array([s5, sa5], dtype=np.float64)
    arrays["image5/sample"] = sample5

    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "wav2lip.npz")
    np.savez_compressed(path, **arrays)
    blocks_path = os.path.join(args.out, "wav2lip_blocks.npz")
    np.savez_compressed(blocks_path, **samples)
    digest, blocks_digest = hashlib.sha256(), hashlib.sha256()
    for d, group in ((digest, arrays), (blocks_digest, samples)):
        for n in sorted(group):
            d.update(n.encode())
            d.update(np.ascontiguousarray(group[n]).tobytes())
    logits_path = os.path.join(args.out, "wav2lip_logits.npz")
    np.savez_compressed(logits_path, logits=acts[-1].numpy())
    with open(os.path.join(args.out, "wav2lip_logits.json"), "w") as fjson:
        json.dump({"name": "wav2lip_logits", "generator": "tools/gen_golden_wav2lip.py",
                   "what": "the float64 output of the reference's plain output convolution (output_block.1, before the sigmoid) "
                           "[n,3,96,96] for the windows of wav2lip.npz; a file of its own for the size limit",
                   "arrays_sha256": hashlib.sha256(b"logits" + np.ascontiguousarray(acts[-1].numpy()).tobytes()).hexdigest()},
                  fjson, indent=1, sort_keys=True)
    with open(os.path.join(args.out, "wav2lip_blocks.json"), "w") as fjson:
        json.dump({"name": "wav2lip_blocks", "generator": "tools/gen_golden_wav2lip.py", "sample_stride": wr.SAMPLE_STRIDE,
                   "what": "every 97th element of each of the 51 blocks' float64 activations for the windows of wav2lip.npz "
                           "(block%02d/sample); a file of its own because both together pass the size limit for a committed file",
                   "arrays_sha256": blocks_digest.hexdigest()}, fjson, indent=1, sort_keys=True)
    manifest = {
        "name": "wav2lip", "generator": "tools/gen_golden_wav2lip.py",
        "what": "wav_models/wav2lip.py Wav2Lip (the reference's class) in float64, eval mode, on the CPU: the image [n,3,96,96], per "
                "block the activation's sum, abs-sum and every 97th element (block 50: the pre-sigmoid logits), and the same three "
                "of one 5-D call of the same windows",
        "inputs": "face inputs = faces_u8 / 255 [n,6,96,96]; mel windows = mel_u8 / 32 - 4 [n,1,80,16]",
        "n_windows": wr.N_WINDOWS, "sample_stride": wr.SAMPLE_STRIDE,
        "weights": "n3dt.synthetic.wav2lip_state_dict(weights_seed): seeded stand-ins, not the pretrained generator",
        "weights_seed": wr.WEIGHTS_SEED, "weights_checksum": checksum, "input_seed": wr.INPUT_SEED, "n_params": n_params,
        "head_scales": [syn.WAV2LIP_HEAD_WEIGHT_SCALE, syn.WAV2LIP_HEAD_BIAS_SCALE],
        "block_shapes": [list(x.shape[1:]) for x in acts], "block_max_abs": scales, "block_zero_share": zero_share,
        "pinned": ["every block (convolution or transposed convolution, batch norm, residual, ReLU)", "the concatenations",
                   "the output convolution and the sigmoid", "the 5-D form's flattening"],
        "parity_unpinned": {
            "opencv_resize": "OpenCV's fixed-point resize on bytes is not reproduced: prologue and paste resample floats bilinearly with "
                             "half-pixel centres in float64",
            "weights": "the pretrained wav2lip.pth has never been run through this code",
        },
        "bounds": {
            "how": "max |emulation - float64 reference| on the CPU over the fixture's windows; emulation = folded fp32 weights, "
                   "operands split into two bf16, three products, fp32 accumulation, the output convolution in float64 from fp32 "
                   "operands (tests/wav2lip_restatement.py); per block the block alone on the fp32-rounded reference input; logits "
                   "and image end to end; the GPU tests allow gpu_factor x these",
            "gpu_factor": 4.0, "block": bounds["block"], "logits": bounds["logits"], "image": bounds["image"],
        },
        "stats": {"image_min": float(image.min()), "image_max": float(image.max()), "image_outside_002_098": outside,
                  "logits_min": float(acts[-1].min()), "logits_max": float(acts[-1].max()), "max_zero_share": max(zero_share)},
        "arrays_sha256": digest.hexdigest(), "block_samples": "tests/golden/wav2lip_blocks.npz", "logits": "tests/golden/wav2lip_logits.npz",
    }
    with open(os.path.join(args.out, "wav2lip.json"), "w") as fjson:
        json.dump(manifest, fjson, indent=1, sort_keys=True)
    for written in (path, blocks_path, logits_path):
        assert os.path.getsize(written) < (1 << 20), written
        print("wrote %s (%.1f KB)" % (written, os.path.getsize(written) / 1024.0))
    print(json.dumps({k: manifest[k] for k in ("bounds", "stats", "n_params")}, indent=1))


if __name__ == "__main__":
    main()
