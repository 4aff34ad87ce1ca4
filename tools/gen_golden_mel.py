#!/usr/bin/env python3
"""Generate tests/golden/mel.{npz,json}: seeded 16 kHz waveforms, their float64 mel spectrogram and the windows the reference's
two rules cut from it -- all from tests/mel_restatement.py (numpy only; no GPU, no librosa, nothing of the reference is imported).

Lengths: 401 (the shortest the reflect padding takes), 800, 999, 1000 (either side of a hop), 3201, 16000, 40000.  Every waveform
is a seeded mix of sections, so that the set reaches every branch of the arithmetic:
  chirp    a linear sweep 100 Hz -> 7 kHz, amplitude 0.5, over Gaussian noise of standard deviation 2e-3
  tone     three loud high-frequency tones (amplitude 40 each) over noise of 1e-2: mel amplitudes above 10, the +4 clip
  silence  exact zeros (runs of 1000 samples and more in the long signals): the 1e-5 amplitude floor, the -4 clip
  quiet    the chirp section scaled by 1e-3: values between the floor and the -4 clip, and just above it
  noise    Gaussian noise of standard deviation 1e-3
The generator asserts that between 1 % and 50 % of all values sit at each clip.

Windows: for the 16000- and 40000-sample signals, the start tables and the gathered [N, 80, 16] windows (as fp32, gathered from the
fp32-rounded mel) of both rules at 25 and 30 fps, for the video frames 0, 1, 2, 3, 7 and the last three of the clip.

Parity to librosa itself is unpinned (it is not installed): the manifest says so.  Regenerating reproduces the files bit for bit.
Usage:  python tools/gen_golden_mel.py [--out DIR]
"""
import argparse
import io
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import mel_restatement as mr  # noqa: E402

SEED = 31500
# (name, length, [(section kind, number of samples)]): the sections tile the signal
CASES = [
    ("len401", 401, [("noise", 200), ("chirp", 201)]),
    ("len800", 800, [("tone", 800)]),
    ("len999", 999, [("chirp", 500), ("noise", 499)]),
    ("len1000", 1000, [("quiet", 1000)]),
    ("len3201", 3201, [("chirp", 1000), ("silence", 1201), ("tone", 1000)]),
    ("len16000", 16000, [("chirp", 4000), ("silence", 3000), ("tone", 3000), ("quiet", 3000), ("noise", 3000)]),
    ("len40000", 40000, [("tone", 12000), ("silence", 6000), ("chirp", 8000), ("noise", 4000), ("quiet", 4000), ("tone", 6000)]),
]
WINDOW_CASES = ("len16000", "len40000")
FPS = (25.0, 30.0)


def section(kind, n, rng):
    t = np.arange(n, dtype=np.float64) / mr.SR
    if kind in ("chirp", "quiet"):
        dur = max(n, 2) / mr.SR
        x = 0.5 * np.sin(2.0 * np.pi * (100.0 * t + 0.5 * (7000.0 - 100.0) / dur * t * t) + rng.random() * 6.28)
        return (x + 2e-3 * rng.standard_normal(n)) * (1e-3 if kind == "quiet" else 1.0)
    if kind == "tone":
        return sum(40.0 * np.sin(2.0 * np.pi * f * t + rng.random() * 6.28) for f in (4300.0, 5600.0, 6900.0)) + 1e-2 * rng.standard_normal(n)
    if kind == "silence":
        return np.zeros(n)
    if kind == "noise":
        return 1e-3 * rng.standard_normal(n)
    raise ValueError(kind)


def waveform(idx, sections):
    rng = np.random.default_rng(SEED + idx)
    return np.concatenate([section(k, n, rng) for k, n in sections]).astype(np.float32)


def video_frames(T, fps):
    """0, 1, 2, 3, 7 and the last three video frames of a clip whose mel has T columns"""
    last = int((T - 1) * fps / 80.0)
    return [0, 1, 2, 3, 7, last - 2, last - 1, last]


def build():
    arrays, cases = {}, []
    for idx, (name, L, sections) in enumerate(CASES):
        assert sum(n for _, n in sections) == L
        wav = waveform(idx, sections)
        mel = mr.melspectrogram(wav)
        assert mel.shape == (80, 1 + L // 200) and np.isfinite(mel).all()
        arrays[name + "/wav"], arrays[name + "/mel"] = wav, mel
        case = {"name": name, "length": L, "frames": mel.shape[1], "sections": [[k, n] for k, n in sections], "seed": SEED + idx}
        if name in WINDOW_CASES:
            mel32 = mel.astype(np.float32)
            T = mel.shape[1]
            case["windows"] = []
            for fps in FPS:
                ids = video_frames(T, fps)
                for rule, starts in (("chunk", mr.chunk_starts(ids, T, fps)), ("centered", mr.centered_starts(ids, fps))):
                    key = "%s/%s_%d" % (name, rule, int(fps))
                    arrays[key] = mr.gather(mel32, starts)
                    case["windows"].append({"key": key, "rule": rule, "fps": fps, "frame_ids": ids, "starts": starts})
        cases.append(case)
    values = np.concatenate([arrays[c["name"] + "/mel"].ravel() for c in cases])
    low, high = float((values == -4.0).mean()), float((values == 4.0).mean())
    assert 0.01 <= low <= 0.5, "share of values at the -4 clip: %.4f" % low
    assert 0.01 <= high <= 0.5, "share of values at the +4 clip: %.4f" % high
    assert any(k == "silence" and n >= 1000 for c in CASES for k, n in c[2])
    manifest = {
        "what": "wav_audio.melspectrogram (wav_hparams.py) of seeded waveforms and the windows of data_loader_xgaze.py:262-270 "
                "('chunk') and :516-523 ('centered'), from tests/mel_restatement.py in float64",
        "parity": "parity unpinned to the dependency",
        "libraries_not_run": ["librosa"],
        "conventions_from_knowledge_of_librosa": ["stft(center=True) pads by reflection without the edge sample", "periodic Hann window",
                                                  "filters.mel: Slaney scale (htk=False), area normalisation, returned as float32"],
        "parameters": {"sample_rate": mr.SR, "n_fft": mr.N_FFT, "hop": mr.HOP, "n_mels": mr.N_MELS, "fmin": mr.FMIN, "fmax": mr.FMAX,
                       "preemphasis": mr.PREEMPHASIS, "min_level_db": mr.MIN_LEVEL_DB, "ref_level_db": mr.REF_LEVEL_DB,
                       "max_abs_value": mr.MAX_ABS},
        "share_at_minus_4": low, "share_at_plus_4": high,
        "cases": cases,
    }
    return arrays, manifest


def file_bytes(arrays, manifest):
    """the two files' bytes (numpy's zip writer stamps no time: the same arrays give the same bytes)"""
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    return buf.getvalue(), (json.dumps(manifest, indent=1, sort_keys=True) + "\n").encode()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    args = ap.parse_args()
    arrays, manifest = build()
    npz, js = file_bytes(arrays, manifest)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "mel.npz"), "wb") as f:
        f.write(npz)
    with open(os.path.join(args.out, "mel.json"), "wb") as f:
        f.write(js)
    print("wrote %d cases, %d bytes; share at -4: %.4f, at +4: %.4f" % (len(manifest["cases"]), len(npz), manifest["share_at_minus_4"],
                                                                       manifest["share_at_plus_4"]))


if __name__ == "__main__":
    main()
