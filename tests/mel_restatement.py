"""Float64 restatement of the audio front end, numpy only: what n3dt.MelFrontend must compute.

The reference's wav_audio.melspectrogram with wav_hparams.py, step by step: pre-emphasis, reflect padding, framing, periodic Hann
window, |DFT| (numpy.fft.rfft), Slaney mel basis rounded to fp32, amplitude to dB, symmetric normalisation with clipping; and the
two rules by which the reference cuts 16-column windows.  Written from the formulation, not from the kernel: it shares no code with
n3dt/mel.py or csrc/mel_core.h, and tests/test_mel_cpu.py pins its pieces to scipy and numpy one by one.
"""
import numpy as np

SR = 16000
N_FFT = 800
HOP = 200
N_MELS = 80
FMIN, FMAX = 55.0, 7600.0
PREEMPHASIS = 0.97
MIN_LEVEL_DB = -100.0
REF_LEVEL_DB = 20.0
MAX_ABS = 4.0
STEP = 16


def preemphasis(x):
    x = np.asarray(x, np.float64)
    y = x.copy()
    y[1:] = x[1:] - PREEMPHASIS * x[:-1]
    return y


def reflect_pad(y, pad=N_FFT // 2):
    """pad samples mirrored about the first and the last sample, which are not repeated"""
    L = len(y)
    if L < pad + 1:
        raise ValueError("reflect padding of %d needs at least %d samples" % (pad, pad + 1))
    out = np.empty(L + 2 * pad, np.float64)
    out[pad:pad + L] = y
    for j in range(1, pad + 1):
        out[pad - j] = y[j]
        out[pad + L - 1 + j] = y[L - 1 - j]
    return out


def hann_periodic(n=N_FFT):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)


def frames(yp):
    T = 1 + (len(yp) - N_FFT) // HOP
    return np.stack([yp[HOP * t:HOP * t + N_FFT] for t in range(T)])  # [T, 800]


def windowed_frames(x):
    return frames(reflect_pad(preemphasis(x))) * hann_periodic()[None, :]


def dft_direct(frame, bins=None):
    """the DFT sum term by term, twiddle angles reduced exactly: (k n) mod 800"""
    n = np.arange(N_FFT)
    ks = range(N_FFT // 2 + 1) if bins is None else bins
    out = []
    for k in ks:
        ang = 2.0 * np.pi * ((k * n) % N_FFT) / N_FFT
        out.append(complex(np.sum(frame * np.cos(ang)), -np.sum(frame * np.sin(ang))))
    return np.array(out)


def magnitudes(x):
    return np.abs(np.fft.rfft(windowed_frames(x), axis=1)).T  # [401, T]


def hz_to_mel(f):
    f = float(f)
    if f < 1000.0:
        return f * 3.0 / 200.0
    return 15.0 + np.log(f / 1000.0) * 27.0 / np.log(6.4)


def mel_to_hz(m):
    m = float(m)
    if m < 15.0:
        return m * 200.0 / 3.0
    return 1000.0 * np.exp((m - 15.0) * np.log(6.4) / 27.0)


def mel_basis():
    e = np.array([mel_to_hz(m) for m in np.linspace(hz_to_mel(FMIN), hz_to_mel(FMAX), N_MELS + 2)])
    f = np.linspace(0.0, SR / 2.0, N_FFT // 2 + 1)
    B = np.zeros((N_MELS, len(f)), np.float64)
    for i in range(N_MELS):
        up = (f - e[i]) / (e[i + 1] - e[i])
        down = (e[i + 2] - f) / (e[i + 2] - e[i + 1])
        B[i] = np.maximum(0.0, np.minimum(up, down)) * (2.0 / (e[i + 2] - e[i]))
    return B.astype(np.float32)


def normalise(amp):
    S = 20.0 * np.log10(np.maximum(1e-5, amp)) - REF_LEVEL_DB
    return np.clip((2.0 * MAX_ABS) * ((S - MIN_LEVEL_DB) / (-MIN_LEVEL_DB)) - MAX_ABS, -MAX_ABS, MAX_ABS)


def melspectrogram(x, basis=None):
    """x [L] (any float dtype; fp32 values are taken exactly) -> [80, 1 + L // 200] float64"""
    B = (mel_basis() if basis is None else np.asarray(basis, np.float32)).astype(np.float64)
    return normalise(B @ magnitudes(x))


def chunk_starts(frame_ids, T, fps):
    out = []
    for i in frame_ids:
        s = int(i * (80. / fps))
        if s + STEP > T:
            s = T - STEP
        out.append(s)
    return out


def centered_starts(frame_ids, fps):
    return [int(80. * ((i - 2) / float(fps))) for i in frame_ids]


def gather(mel, starts):
    """[N, 80, 16]: columns start .. start + 15, each clamped into the spectrogram"""
    T = mel.shape[1]
    return np.stack([mel[:, [min(max(s + c, 0), T - 1) for c in range(STEP)]] for s in starts])
