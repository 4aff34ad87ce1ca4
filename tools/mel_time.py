#!/usr/bin/env python3
"""Time the audio front end (n3dt.MelFrontend: melspectrogram + windows) on the GPU for 1 s, 10 s and 60 s of 16 kHz audio, in one
process, against
  * torch ops on the same GPU: pre-emphasis, torch.stft (reflect padding, periodic Hann window), the basis product, log10 and
    clamp, an index gather for the windows -- what a user would write without libn3dt -- in float64 and in float32;
  * the numpy restatement (tests/mel_restatement.py) on the CPU, wall clock.
All sides are compared with the restatement before anything is timed; the float32 figure is the error a single-precision
spectrogram makes.  Each GPU figure is the median of `--iters` calls (hipEvents around every call, host enqueue cost included)
after `--warmup`; n3dt and torch are taken ALTERNATELY, `--pairs` times, and the ratio is formed from the medians over the pairs.
The launches per call are counted by the tool with torch.profiler (device kernels of one call; copies are not kernels), or
reported as null where the profiler records no device activity.  Prints one JSON object.

Run under a time limit, e.g.  timeout -k 10 300 python tools/mel_time.py
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "nerf-3dtalker-code_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import mel_restatement as mr  # noqa: E402
from n3dt import MelFrontend, mel_basis  # noqa: E402
from n3dt import mel as nm  # noqa: E402

FPS = 25.0


class TorchFrontend(object):
    def __init__(self, dev, dtype):
        self.dtype = dtype
        self.basis = torch.from_numpy(mel_basis()).to(dev, dtype)
        self.window = torch.hann_window(800, periodic=True, dtype=dtype, device=dev)

    def melspectrogram(self, wav):
        x = wav.to(self.dtype)
        y = torch.cat([x[:1], x[1:] - 0.97 * x[:-1]])
        D = torch.stft(y, 800, hop_length=200, win_length=800, window=self.window, center=True, pad_mode="reflect", return_complex=True)
        S = 20.0 * torch.log10(torch.clamp(self.basis @ D.abs(), min=1e-5)) - 20.0
        return torch.clamp(8.0 * ((S + 100.0) / 100.0) - 4.0, -4.0, 4.0)

    def windows(self, mel, cols):
        return mel[:, cols].permute(1, 0, 2).to(torch.float32).contiguous()


def median_us(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev) * 1e3


def count_launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if str(e.device_type).endswith("CUDA")]
        kernels = [n for n in names if not n.lower().startswith(("memcpy", "memset", "copybuffer", "fillbuffer"))]
        return len(kernels) if names else None
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, nargs="+", default=[1.0, 10.0, 60.0])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=5)
    args = ap.parse_args()
    assert args.iters >= 20 and args.warmup >= 5, "at least 20 timed calls after 5 warm-ups"
    dev = torch.device("cuda:0")
    front = MelFrontend()
    sides = {"torch_f64": TorchFrontend(dev, torch.float64), "torch_f32": TorchFrontend(dev, torch.float32)}
    out = {"iters": args.iters, "warmup": args.warmup, "pairs": args.pairs, "fps": FPS, "cases": []}
    for sec in args.seconds:
        L = int(round(sec * 16000))
        rng = np.random.default_rng(L)
        t = np.arange(L) / 16000.0
        wav_np = (0.3 * np.sin(2 * np.pi * (200.0 + 300.0 * t) * t) + 0.01 * rng.standard_normal(L)).astype(np.float32)
        wav = torch.from_numpy(wav_np).to(dev)
        T = nm.num_frames(L)
        ids = list(range(int(sec * FPS)))
        starts = nm.window_starts(ids, T, FPS, "chunk")
        cols = torch.as_tensor([[s + c for c in range(16)] for s in starts], device=dev)
        t0 = time.perf_counter()
        want = mr.melspectrogram(wav_np)
        want_w = mr.gather(want.astype(np.float32), mr.chunk_starts(ids, T, FPS))
        numpy_us = (time.perf_counter() - t0) * 1e6
        case = {"seconds": sec, "samples": L, "mel_frames": T, "windows": len(ids), "numpy_cpu_us": round(numpy_us, 1)}
        got = front.melspectrogram(wav, dtype=torch.float64)
        case["max_abs_error"] = {"n3dt": float(np.abs(got.cpu().numpy() - want).max())}
        assert case["max_abs_error"]["n3dt"] <= 1e-9, case
        assert tuple(front.windows(front.melspectrogram(wav), ids, fps=FPS).shape) == want_w.shape
        fns = {"n3dt": lambda: front.windows(front.melspectrogram(wav), ids, fps=FPS)}
        for name, side in sides.items():
            try:
                case["max_abs_error"][name] = float(np.abs(side.melspectrogram(wav).double().cpu().numpy() - want).max())
                fns[name] = (lambda s: lambda: s.windows(s.melspectrogram(wav), cols))(side)
            except Exception as e:  # no FFT library for this device: the side is reported as missing, not timed
                case["max_abs_error"][name] = "unavailable: %s" % (str(e).splitlines()[0][:120],)
        assert not isinstance(case["max_abs_error"].get("torch_f64"), float) or case["max_abs_error"]["torch_f64"] <= 1e-9, case
        us = {k: [] for k in fns}
        for _ in range(args.pairs):
            for k, fn in fns.items():
                us[k].append(round(median_us(fn, args.warmup, args.iters), 2))
        case["us"] = us
        case["median_us"] = {k: statistics.median(v) for k, v in us.items()}
        case["launches_per_call"] = {k: count_launches(fn) for k, fn in fns.items()}
        for k in fns:
            if k != "n3dt":
                case[k + "_over_n3dt"] = round(case["median_us"][k] / case["median_us"]["n3dt"], 3)
        out["cases"].append(case)
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
