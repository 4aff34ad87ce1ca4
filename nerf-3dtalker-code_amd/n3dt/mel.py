"""The audio front end on libn3dt: a 16 kHz waveform to the mel windows Audio2style reads (csrc/mel.hip).

The reference computes them on the CPU: `wav_audio.melspectrogram` (librosa + scipy, `wav_hparams.py`) gives mel [80, T], and the
data loader cuts one 16-column window per video frame (XGaze_utils/data_loader_xgaze.py:256-270, :516-523).  Here both run on the
device in float64: pre-emphasis 0.97, reflect padding of 400, periodic Hann window of 800, hop 200, |DFT|, an 80-band Slaney mel
basis between 55 and 7600 Hz rounded to fp32, 20 log10(max(1e-5, .)) - 20, then 8 (S + 100) / 100 - 4 clipped to [-4, 4].

librosa is not a dependency and has never been run against this code: its conventions (centre = reflect padding, periodic Hann,
Slaney scale with area normalisation, the basis returned as fp32) are written from knowledge of the library; `MelFrontend` takes
librosa's own matrix as `mel_basis=` where it is at hand.  File decoding and resampling are the caller's.  There is no CPU path.
"""
import ctypes

import numpy as np
import torch

from . import ops
from ._host import PackedCache, gpu_tensor
from ._lib import check, lib

# wav_hparams.py
SAMPLE_RATE = 16000
N_FFT = 800
HOP = 200
N_MELS = 80
FMIN = 55.0
FMAX = 7600.0
PAD = N_FFT // 2
N_BINS = N_FFT // 2 + 1
MIN_SAMPLES = PAD + 1
WINDOW_COLS = 16          # mel_step_size
MEL_PER_SECOND = 80.0     # SAMPLE_RATE / HOP

WINDOW_RULES = ("chunk", "centered")


def _hz_to_mel(f):
    """Slaney's scale: 200/3 Hz per mel below 1000 Hz, logarithmic with step ln(6.4) / 27 above"""
    f = np.asarray(f, np.float64)
    lin = f / (200.0 / 3.0)
    log = 15.0 + np.log(np.maximum(f, 1000.0) / 1000.0) / (np.log(6.4) / 27.0)
    return np.where(f >= 1000.0, log, lin)


def _mel_to_hz(m):
    m = np.asarray(m, np.float64)
    lin = m * (200.0 / 3.0)
    log = 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0))
    return np.where(m >= 15.0, log, lin)


def mel_basis():
    """The [80, 401] fp32 mel basis of the reference's parameters: triangular filters between 82 edges equally spaced on Slaney's
    mel scale from 55 to 7600 Hz, each scaled by 2 / (its width in Hz); float64 arithmetic, rounded once."""
    edges = _mel_to_hz(np.linspace(_hz_to_mel(FMIN), _hz_to_mel(FMAX), N_MELS + 2))
    freqs = np.linspace(0.0, SAMPLE_RATE / 2.0, N_BINS)
    lower = (freqs[None, :] - edges[:-2, None]) / (edges[1:-1] - edges[:-2])[:, None]
    upper = (edges[2:, None] - freqs[None, :]) / (edges[2:] - edges[1:-1])[:, None]
    tri = np.maximum(0.0, np.minimum(lower, upper))
    return (tri * (2.0 / (edges[2:] - edges[:-2]))[:, None]).astype(np.float32)


_builtin_basis = mel_basis  # MelFrontend's argument carries the function's name


def twiddle_table():
    """cos(2 pi n / 800), n = 0 .. 799, float64: the kernel's only source of twiddles and of the Hann window"""
    return np.cos(2.0 * np.pi * np.arange(N_FFT, dtype=np.float64) / N_FFT)


def num_frames(n_samples):
    return 1 + n_samples // HOP


def window_starts(frame_ids, n_mel_frames, fps=25.0, rule="chunk"):
    """The first mel column of every video frame's window, in Python floats as the reference computes them.
    "chunk" (data_loader_xgaze.py:262-270, Audio2style's input): int(i * (80. / fps)), moved back to T - 16 where the window would
    pass the end.  "centered" (:516-523): int(80. * ((i - 2) / float(fps))); its columns are clamped one by one when gathered."""
    if rule not in WINDOW_RULES:
        raise ValueError("windows: rule must be 'chunk' or 'centered', got %r" % (rule,))
    T = int(n_mel_frames)
    if rule == "chunk" and T < WINDOW_COLS:
        raise ValueError("windows: the 'chunk' rule needs at least %d mel frames, got %d" % (WINDOW_COLS, T))
    out = []
    for i in frame_ids:
        i = int(i)
        if rule == "chunk":
            start = int(i * (MEL_PER_SECOND / fps))
            if start + WINDOW_COLS > T:
                start = T - WINDOW_COLS
        else:
            start = int(MEL_PER_SECOND * ((i - 2) / float(fps)))
        if not -2 ** 31 + WINDOW_COLS <= start < 2 ** 31 - WINDOW_COLS:
            raise ValueError("windows: frame id %d is out of range" % i)
        out.append(start)
    return out


def _check_wav(who, wav, min_samples):
    gpu_tensor(who, "the waveform", wav, copy=False)
    if wav.dtype != torch.float32 or wav.dim() != 1 or not wav.is_contiguous():
        raise ValueError("%s: the waveform must be float32 [L], contiguous, got %s %s" % (who, wav.dtype, tuple(wav.shape)))
    if wav.shape[0] < min_samples:
        raise ValueError("%s: the waveform must have at least %d samples (the reflect padding of %d), got %d"
                         % (who, MIN_SAMPLES, PAD, wav.shape[0]))
    return wav.detach()


def _check_dtype(who, dtype):
    if dtype not in (torch.float32, torch.float64):
        raise ValueError("%s: dtype must be torch.float32 or torch.float64, got %s" % (who, dtype))


class MelFrontend(object):
    """wav -> mel -> Audio2style windows on the device.

        front = n3dt.MelFrontend()
        mel = front.melspectrogram(wav)                        # wav [L] fp32 at 16 kHz on the GPU -> [80, 1 + L // 200]
        windows = front.windows(mel, range(n_frames), fps=25.0)  # [n_frames, 80, 16] fp32, Audio2style's input

    `mel_basis`: an [80, 401] matrix to use in place of `n3dt.mel_basis()` (librosa.filters.mel's own, for instance); it is rounded
    to fp32.  The basis, the twiddle table and the kernel's workspace are uploaded once per device."""

    def __init__(self, mel_basis=None):
        basis = _builtin_basis() if mel_basis is None else mel_basis
        if torch.is_tensor(basis):
            basis = basis.detach().cpu().numpy()
        basis = np.ascontiguousarray(np.asarray(basis), dtype=np.float32)
        if basis.shape != (N_MELS, N_BINS):
            raise ValueError("MelFrontend: mel_basis must be [%d, %d], got %s" % (N_MELS, N_BINS, basis.shape))
        self.basis = basis
        self._dev = PackedCache(lambda: (), self._upload)  # nothing is watched: the tables are constants

    def _upload(self, device, _):
        """(basis, table, workspace) on `device`, uploaded on the stream that is current at first use; a call on another stream
        waits for that upload's event first (PackedCache).  The workspace is written with the same values by every call, so calls
        on two streams may share it."""
        basis = torch.from_numpy(self.basis).to(device)
        table = torch.from_numpy(twiddle_table()).to(device)
        ws = torch.empty(max(lib().n3dt_mel_workspace_bytes(), 256), dtype=torch.uint8, device=device)
        return (basis, table, ws), ()

    def _frames(self, wav, offset, prev, total, first, n, dtype):
        """frames first .. first + n - 1 from the run `wav` (n3dt_mel_spectrogram); enqueues on the current stream"""
        out = torch.empty(N_MELS, n, dtype=dtype, device=wav.device)
        if n == 0:
            return out
        basis, table, ws = self._dev.get(wav.device)
        check(lib().n3dt_mel_spectrogram(wav.shape[0], ops._ptr(wav), offset, ops._ptr(prev), total, first, n, ops._ptr(basis),
                                         ops._ptr(table), ops._ptr(out), n, int(dtype == torch.float64), ops._ptr(ws),
                                         ctypes.c_size_t(ws.numel()), ops._stream()), "n3dt_mel_spectrogram")
        return out

    def melspectrogram(self, wav, dtype=torch.float32):
        """wav [L] (GPU, fp32, contiguous, 16 kHz, L >= 401) -> [80, 1 + L // 200] of `dtype`: torch.float64 is the unrounded
        result, torch.float32 the same values rounded once.  Stream-ordered, no synchronisation, capturable, bitwise reproducible.
        NaN samples give NaN values and nothing raises: the reference's host-side `isnan` check is the caller's to do."""
        _check_dtype("melspectrogram", dtype)
        wav = _check_wav("melspectrogram", wav, MIN_SAMPLES)
        L = wav.shape[0]
        return self._frames(wav, 0, None, L, 0, num_frames(L), dtype)

    def windows(self, mel, frame_ids, fps=25.0, rule="chunk"):
        """mel [80, T] (GPU, fp32 or float64) and video frame ids -> [N, 80, 16] fp32, one window per id (see window_starts for
        the two rules).  Columns outside [0, T - 1] repeat the nearest one.  One small upload of the start table, one launch."""
        gpu_tensor("windows", "mel", mel, copy=False)
        if mel.dtype not in (torch.float32, torch.float64) or mel.dim() != 2 or mel.shape[0] != N_MELS or mel.shape[1] < 1:
            raise ValueError("windows: mel must be float32 or float64 [80, T], got %s %s" % (mel.dtype, tuple(mel.shape)))
        mel = mel.detach().contiguous()
        T = mel.shape[1]
        starts = window_starts(frame_ids, T, fps, rule)
        out = torch.empty(len(starts), N_MELS, WINDOW_COLS, dtype=torch.float32, device=mel.device)
        if not starts:
            return out
        start = torch.tensor(starts, dtype=torch.int32).to(mel.device, non_blocking=False)
        check(lib().n3dt_mel_windows(T, ops._ptr(mel), T, int(mel.dtype == torch.float64), len(starts), ops._ptr(start), ops._ptr(out),
                                     ops._stream()), "n3dt_mel_windows")
        return out

    def stream(self, dtype=torch.float32):
        """A `MelStream` over this front end: live audio in blocks of any size, the same bits as `melspectrogram`."""
        return MelStream(self, dtype)


class MelStream(object):
    """The streaming form of `MelFrontend.melspectrogram`.

        s = front.stream()
        for block in blocks:          # fp32 GPU tensors of any length, 0 included
            cols = s.push(block)      # [80, n]: every frame that became computable, n >= 0
        tail = s.flush()              # the remaining frames (they reflect about the last sample)

    Frame t is emitted once 200 t + 401 samples have arrived.  The concatenation of every push's result and the flush's equals
    `melspectrogram` of the concatenated blocks bit for bit, whatever the partition.  The stream keeps the samples its next frame
    still reads (600 to 800 plus what has not made a frame yet) and the pre-emphasis carry on the device; the counts it steers by
    are block lengths, known on the host, so nothing synchronises.  After flush() the stream is spent."""

    def __init__(self, front, dtype=torch.float32):
        _check_dtype("MelStream", dtype)
        self.front, self.dtype = front, dtype
        self.received = 0      # samples pushed so far
        self.next_frame = 0    # the first frame not yet emitted
        self._buf = None       # samples _offset .. received
        self._prev = None      # sample _offset - 1, [1]
        self._offset = 0
        self._done = False

    def _emit(self, total, upto):
        n = upto - self.next_frame
        out = self.front._frames(self._buf, self._offset, self._prev, total, self.next_frame, n, self.dtype)
        self.next_frame = upto
        return out

    def push(self, block):
        if self._done:
            raise ValueError("MelStream: push after flush")
        block = _check_wav("MelStream.push", block, 0)
        if self._buf is not None and block.device != self._buf.device:
            raise ValueError("MelStream.push: the stream lives on %s, the block on %s" % (self._buf.device, block.device))
        self._buf = block.clone() if self._buf is None else torch.cat([self._buf, block])
        self.received += block.shape[0]
        ready = (self.received - MIN_SAMPLES) // HOP + 1 if self.received >= MIN_SAMPLES else 0
        out = self._emit(-1, max(ready, self.next_frame))
        # drop what no later frame reads: frame next_frame starts at sample 200 next_frame - 400
        keep_from = self.next_frame * HOP - PAD
        if keep_from > self._offset:
            cut = keep_from - self._offset
            self._prev = self._buf[cut - 1:cut].clone()
            self._buf = self._buf[cut:].clone()
            self._offset = keep_from
        return out

    def flush(self):
        if self._done:
            raise ValueError("MelStream: flush after flush")
        if self.received < MIN_SAMPLES:
            raise ValueError("MelStream.flush: the stream received %d samples, a spectrogram needs at least %d" % (self.received, MIN_SAMPLES))
        self._done = True
        out = self._emit(self.received, num_frames(self.received))
        self._buf = self._prev = None
        return out
