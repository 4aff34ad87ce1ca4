#!/usr/bin/env python3
"""Generate tests/golden/audio2style.{npz,json} from the reference's own Audio2style (talker_trainer.py:407-461) in float64 on the CPU.

Runs only where the reference is checked out.  Importing talker_trainer.py as a whole runs its trainer-side imports (data loaders,
evaluation helpers, tensorboard, the renderer); the two classes this fixture needs, RNNModel and Audio2style, use torch.nn only.
So the generator installs gen_golden's caller stand-ins (plus `torch.utils.tensorboard`, absent here), and compiles exactly those two
class definitions out of the reference's file (its own source text, located with `ast`) into a namespace holding torch and nn.

Weights: torch.manual_seed(WEIGHTS_SEED) then Audio2style(), the reference's constructor; only the seed and a checksum are stored.
Inputs: mel = uint8 / 32 - 4 (exact in float32), w = seeded float64 [T, 64].  Cases T = 1, 2, 5, 16, each in train mode (dropout on,
the reference's own Bernoulli draws after torch.manual_seed(MASK_SEED + T), recorded as bit-packed keep masks) and eval mode.
Recorded per case: the output, both LSTM layers' outputs (float32; they do not depend on the mode), and for L = sum(w * out) every
parameter gradient's L2 norm and max |.| and a seeded sample of N_SAMPLE entries; fc1 has no gradient (recorded by name).

The bounds (`band`): the same class, weights, inputs and masks run in plain float32, every metric's error against float64, worst over
the cases, times two (the project's rule, tools/vgg_bf16_band.py), floored at BAND_FLOOR of the quantity's scale.

Regenerating reproduces the file bit for bit (fixed seeds, float64, one thread, deterministic CPU ops).
Usage:  python tools/gen_golden_a2s.py [--out DIR]
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
REF = "/root/reference"
sys.path.insert(0, os.path.join(REPO, "nerf-3dtalker-code_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

from n3dt import synthetic as syn  # noqa: E402
import gen_golden  # noqa: E402

WEIGHTS_SEED = 2024
MEL_SEED = 300
W_SEED = 400
MASK_SEED = 500
CASES = (1, 2, 5, 16)
N_SAMPLE = 64
BAND_FLOOR = 1e-5


def install_standins():
    gen_golden.install_caller_standins()
    if "torch.utils.tensorboard" not in sys.modules:
        tb = types.ModuleType("torch.utils.tensorboard")
        tb.SummaryWriter = object
        sys.modules["torch.utils.tensorboard"] = tb


def reference_classes(path=os.path.join(REF, "talker_trainer.py")):
    """(RNNModel, Audio2style) compiled from the reference's own class definitions."""
    src = open(path).read()
    tree = ast.parse(src)
    keep = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name in ("RNNModel", "Audio2style")]
    assert [n.name for n in keep] == ["RNNModel", "Audio2style"], "talker_trainer.py no longer defines the two classes"
    ns = {"torch": torch, "nn": torch.nn, "F": torch.nn.functional, "__name__": "talker_trainer"}
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    return ns["RNNModel"], ns["Audio2style"]


def case_inputs(T):
    g = torch.Generator().manual_seed(MEL_SEED + T)
    mel_u8 = torch.randint(0, 256, (T, 80, 16), generator=g, dtype=torch.uint8)
    w = torch.randn(T, 64, generator=torch.Generator().manual_seed(W_SEED + T), dtype=torch.float64)
    return mel_u8, w


def run(ref, mel, w, train, masks=None):
    """out, layer outputs (0, 1), gradients by name; in train mode with `masks` None the reference draws its own (returned)."""
    ref.train(train)
    drops = [ref.linear1[2], ref.linear2[2], ref.linear3[2]]
    drawn, hooks = [], []
    for i, d in enumerate(drops):
        if masks is None:
            hooks.append(d.register_forward_hook(lambda m, inp, out: drawn.append(out != 0)))
        else:
            hooks.append(d.register_forward_hook(lambda m, inp, out, i=i: inp[0] * masks[i].to(inp[0].dtype) * 2.0 if m.training else out))
    layer1 = []
    hooks.append(ref.rnn.register_forward_hook(lambda m, inp, out: layer1.append(out[0].detach().clone())))
    ref.zero_grad(set_to_none=True)
    out = ref(mel.to(next(ref.parameters()).dtype))
    (out * w.to(out.dtype)).sum().backward()
    for h in hooks:
        h.remove()
    # layer 0's output: a one-layer bidirectional LSTM with the l0 weights (the reference's module returns the last layer only)
    dt = out.dtype
    l0 = torch.nn.LSTM(1280, 640, 1, batch_first=True, bidirectional=True).to(dt)
    l0.load_state_dict({k[len("rnn.rnn."):]: v for k, v in ref.state_dict().items() if k.startswith("rnn.rnn.") and "_l0" in k})
    with torch.no_grad():
        layer0 = l0(torch.flatten(mel.to(dt), 1).unsqueeze(0))[0][0]
    grads = {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in ref.named_parameters()}
    return out.detach(), (layer0, layer1[0]), grads, (drawn if masks is None else masks)


def rel_max(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    args = ap.parse_args()
    torch.use_deterministic_algorithms(True)
    torch.set_num_threads(1)
    install_standins()
    _, Audio2style = reference_classes()
    torch.manual_seed(WEIGHTS_SEED)
    ref = Audio2style()
    sd32 = {k: v.detach().clone() for k, v in ref.state_dict().items()}
    checksum = syn.state_dict_checksum(sd32)
    ref64 = ref.double()
    ref32 = Audio2style()
    ref32.load_state_dict(sd32, strict=True)

    arrays, cases = {}, []
    err = {"out": 0.0, "layer": 0.0, "g_norm": 0.0, "g_max": 0.0, "g_entry": 0.0}
    names = [n for n, _ in ref64.named_parameters()]
    for T in CASES:
        mel_u8, w = case_inputs(T)
        mel = mel_u8.double() / 32.0 - 4.0
        k = "T%d." % T
        arrays[k + "mel_u8"] = mel_u8.numpy()
        arrays[k + "w"] = w.numpy()
        for mode in ("train", "eval"):
            train = mode == "train"
            if train:
                torch.manual_seed(MASK_SEED + T)
            out, layers, grads, masks = run(ref64, mel, w, train)
            out32, layers32, grads32, _ = run(ref32, mel.float(), w, train, masks=masks if train else None)
            if mode == "eval":
                for i in range(2):
                    arrays[k + "layer%d" % i] = layers[i].float().numpy()
                    err["layer"] = max(err["layer"], rel_max(layers32[i], layers[i]))
            if train:
                for i, m in enumerate(masks):
                    arrays[k + "train.mask%d" % i] = np.packbits(m.numpy().astype(np.uint8), axis=None)
            arrays[k + mode + ".out"] = out.numpy()
            err["out"] = max(err["out"], rel_max(out32, out))
            gnames = [n for n in names if grads[n] is not None]
            rng = np.random.default_rng(T * 10 + train)
            norms, idx, vals = [], [], []
            for n in gnames:
                d, d32 = grads[n].reshape(-1), grads32[n].reshape(-1)
                nrm, mx = float(d.norm()), float(d.abs().max())
                norms.append([nrm, mx])
                ix = np.sort(rng.choice(d.numel(), min(N_SAMPLE, d.numel()), replace=False)).astype(np.int64)
                idx.append(ix)
                vals.append(d.numpy()[ix])
                if nrm == 0.0:  # W_hh at T = 1: h_prev is h0 = 0
                    assert float(d32.abs().max()) == 0.0, n
                    continue
                err["g_norm"] = max(err["g_norm"], abs(float(d32.double().norm()) - nrm) / nrm)
                err["g_max"] = max(err["g_max"], abs(float(d32.double().abs().max()) - mx) / mx)
                err["g_entry"] = max(err["g_entry"], float((d32.double() - d).abs().max()) / mx)
            arrays[k + mode + ".gnorm"] = np.array(norms, dtype=np.float64)
            arrays[k + mode + ".gidx"] = np.stack(idx)
            arrays[k + mode + ".gval"] = np.stack(vals)
        cases.append({"T": T, "modes": ["train", "eval"]})
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "audio2style.npz")
    np.savez_compressed(path, **arrays)
    digest = hashlib.sha256()
    for n in sorted(arrays):
        digest.update(n.encode())
        digest.update(np.ascontiguousarray(arrays[n]).tobytes())
    manifest = {
        "name": "audio2style", "generator": "tools/gen_golden_a2s.py",
        "what": "talker_trainer.py Audio2style (the reference's class definitions) in float64 on the CPU: output [T,64], both LSTM "
                "layers' outputs [T,1280] (float32), and for L = sum(w * out) every parameter gradient's L2 norm, max |.| and a "
                "seeded sample of entries; train mode with the reference's own dropout draws (bit-packed keep masks), eval mode",
        "inputs": "mel = mel_u8 / 32 - 4 [T,80,16]; w [T,64] float64",
        "weights_seed": WEIGHTS_SEED, "weights_checksum": checksum, "mask_seed": MASK_SEED,
        "state_dict": [[k, list(v.shape)] for k, v in sd32.items()],
        "n_params": int(sum(v.numel() for v in sd32.values())),
        "grad_names": gnames, "no_grad": [n for n in names if n not in gnames],
        "f32_error": err, "band_floor": BAND_FLOOR,
        "band": {k: max(2.0 * v, BAND_FLOOR) for k, v in err.items()},
        "arrays_sha256": digest.hexdigest(), "cases": cases,
    }
    with open(os.path.join(args.out, "audio2style.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    print("wrote %s (%.1f KB)" % (path, os.path.getsize(path) / 1024.0))


if __name__ == "__main__":
    main()
