"""Host side of the audio front end (n3dt.mel, n3dt_mel_spectrogram, n3dt_mel_windows), no GPU: the exports and their documented
refusals, the float64 restatement against the recorded fixtures, against scipy / numpy piece by piece and against known answers,
the mel basis' properties, the window start tables against a literal transcription of the reference's two loops, and the kernel's
per-frame arithmetic (csrc/mel_core.h) run on the CPU under the address and undefined-behaviour sanitizers."""
import ctypes
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import mel_restatement as mr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (401, 800, 999, 1000, 3201, 16000, 40000)


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("mel")


@pytest.fixture(scope="module")
def generator():
    spec = importlib.util.spec_from_file_location("gen_golden_mel", os.path.join(REPO, "tools", "gen_golden_mel.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_new_symbols_are_declared_and_exported():
    import n3dt
    from n3dt import _lib
    L = _lib.lib()
    header = open(os.path.join(REPO, "include", "n3dt.h")).read()
    declared = set(re.findall(r"\b(n3dt_mel[a-z0-9_]*)\s*\(", header))
    assert declared == {"n3dt_mel_workspace_bytes", "n3dt_mel_spectrogram", "n3dt_mel_windows"}
    for name in declared:
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert L.n3dt_abi_version() == 5
    for name in ("MelFrontend", "MelStream", "mel_basis"):
        assert hasattr(n3dt, name), name
    assert callable(n3dt.audio.clip_audiostyle)
    assert L.n3dt_mel_workspace_bytes() == 401 * 80 * 4  # the basis transposed, fp32


def _spectrogram_args(L):
    d = ctypes.c_void_p(256)
    need = L.n3dt_mel_workspace_bytes()
    # n_samples, wav, wav_offset, prev_sample, total_samples, first_frame, n_frames, basis, table, out, out_ld, out_is_f64, ws, bytes, stream
    return [1000, d, 0, None, 1000, 0, 6, d, d, d, 6, 1, d, need, None]


def test_spectrogram_refuses_null_pointers_a_short_workspace_and_short_signals():
    """Validation is host code and runs before anything is enqueued."""
    from n3dt import _lib
    L = _lib.lib()
    good = _spectrogram_args(L)
    for i in (1, 7, 8, 9, 12):
        args = list(good)
        args[i] = None
        assert L.n3dt_mel_spectrogram(*args) == -1 and b"NULL" in L.n3dt_last_error(), i
    args = list(good)
    args[13] -= 1
    assert L.n3dt_mel_spectrogram(*args) == -1 and b"workspace too small" in L.n3dt_last_error()
    for n in (400, 1, 0, -5):
        args = list(good)
        args[0], args[4], args[6], args[10] = n, n, 1, 1
        assert L.n3dt_mel_spectrogram(*args) == -1 and b">= 401" in L.n3dt_last_error(), n
    for i, misaligned, word in ((8, 260, b"8-byte"), (9, 260, b"8-byte"), (1, 258, b"4-byte"), (7, 258, b"4-byte")):
        args = list(good)
        args[i] = ctypes.c_void_p(misaligned)
        assert L.n3dt_mel_spectrogram(*args) == -1 and word in L.n3dt_last_error(), i


def test_spectrogram_refuses_a_run_that_does_not_hold_what_the_frames_read():
    from n3dt import _lib
    L = _lib.lib()
    d = ctypes.c_void_p(256)

    def call(**kw):
        args = _spectrogram_args(L)
        for k, v in kw.items():
            args[{"n_samples": 0, "offset": 2, "prev": 3, "total": 4, "first": 5, "n": 6, "ld": 10}[k]] = v
        return L.n3dt_mel_spectrogram(*args), L.n3dt_last_error()
    assert call(n=7)[1].find(b"frames past") >= 0                           # 1000 samples are 6 frames
    assert call(ld=5)[1].find(b"out_ld") >= 0
    assert call(n=0)[0] == -1 and call(n=(1 << 24) + 1)[0] == -1
    assert call(total=-1)[1].find(b"ends before") >= 0                      # frames 4 and 5 pass the end: they need total_samples
    assert call(total=1200)[1].find(b"must end at the signal's end") >= 0
    assert call(offset=200, total=1200, first=0, n=1, prev=d)[1].find(b"must start there") >= 0   # frame 0 reflects about sample 0
    assert call(offset=200, total=1200, first=3, n=1)[1].find(b"prev_sample is NULL") >= 0
    assert call(offset=400, total=1400, first=3, n=1, prev=d)[1].find(b"starts after") >= 0       # frame 3 reads from sample 200
    for k in ("offset", "first"):
        assert call(**{k: -1})[0] == -1


def test_windows_entry_point_refuses_bad_arguments():
    from n3dt import _lib
    L = _lib.lib()
    d = ctypes.c_void_p(256)
    good = [81, d, 81, 0, 4, d, d, None]  # T, mel, mel_ld, mel_is_f64, n_windows, start, out, stream
    for i in (1, 5, 6):
        args = list(good)
        args[i] = None
        assert L.n3dt_mel_windows(*args) == -1 and b"NULL" in L.n3dt_last_error(), i
    for i, v in ((0, 0), (2, 80), (4, 0)):
        args = list(good)
        args[i] = v
        assert L.n3dt_mel_windows(*args) == -1, i
    args = list(good)
    args[1], args[3] = ctypes.c_void_p(260), 1
    assert L.n3dt_mel_windows(*args) == -1 and b"misaligned" in L.n3dt_last_error()


def test_python_layer_raises_on_cpu_tensors_wrong_dtypes_and_short_signals():
    import torch
    import n3dt
    front = n3dt.MelFrontend()
    with pytest.raises(ValueError, match="GPU"):
        front.melspectrogram(torch.zeros(1000))
    with pytest.raises(ValueError, match="GPU"):
        front.windows(torch.zeros(80, 20), [0])
    with pytest.raises(ValueError, match="GPU"):
        front.stream().push(torch.zeros(10))
    with pytest.raises(ValueError, match="dtype"):
        front.melspectrogram(torch.zeros(1000), dtype=torch.float16)
    with pytest.raises(ValueError, match="received 0 samples"):
        front.stream().flush()
    with pytest.raises(ValueError, match=r"\[80, 401\]"):
        n3dt.MelFrontend(mel_basis=np.zeros((80, 400), np.float32))
    from n3dt import mel
    with pytest.raises(ValueError, match="rule"):
        mel.window_starts([0], 81, rule="middle")
    with pytest.raises(ValueError, match="at least 16"):
        mel.window_starts([0], 15, rule="chunk")
    a2s = n3dt.Audio2style()
    for kw in ({"n_frames": 0}, {"n_frames": 3, "frames_per_sequence": 0}, {"n_frames": 3, "frames_per_sequence": n3dt.audio.MAX_T + 1}):
        with pytest.raises(ValueError, match="clip_audiostyle"):
            n3dt.audio.clip_audiostyle(a2s, front, torch.zeros(16000), **kw)
    with pytest.raises(ValueError, match="GPU"):
        n3dt.audio.clip_audiostyle(a2s, front, torch.zeros(16000), 3)


def test_named_constants_agree_between_the_header_the_package_and_the_restatement():
    from n3dt import mel
    core = open(os.path.join(REPO, "nerf-3dtalker-code_amd", "csrc", "mel_core.h")).read()

    def c(name):
        return float(re.search(r"#define %s \(?(-?[0-9.e]+)\)?" % name, core).group(1))
    assert (c("MEL_SAMPLE_RATE"), c("MEL_NFFT"), c("MEL_HOP"), c("MEL_NMELS")) == (mel.SAMPLE_RATE, mel.N_FFT, mel.HOP, mel.N_MELS) == (mr.SR, mr.N_FFT, mr.HOP, mr.N_MELS)
    assert (c("MEL_FMIN"), c("MEL_FMAX")) == (mel.FMIN, mel.FMAX) == (mr.FMIN, mr.FMAX) == (55.0, 7600.0)
    assert (c("MEL_PREEMPHASIS"), c("MEL_MIN_LEVEL_DB"), c("MEL_REF_LEVEL_DB"), c("MEL_MAX_ABS_VALUE")) == (mr.PREEMPHASIS, mr.MIN_LEVEL_DB, mr.REF_LEVEL_DB, mr.MAX_ABS) == (0.97, -100.0, 20.0, 4.0)
    assert c("MEL_WINDOW_COLS") == mel.WINDOW_COLS == mr.STEP == 16
    assert np.array_equal(mel.twiddle_table(), np.cos(2.0 * np.pi * np.arange(800) / 800))


def test_restatement_reproduces_every_fixture_value(fixture):
    data, manifest = fixture
    assert manifest["parity"] == "parity unpinned to the dependency"
    assert tuple(c["length"] for c in manifest["cases"]) == LENGTHS
    kinds = {k for c in manifest["cases"] for k, _ in c["sections"]}
    assert kinds == {"chirp", "tone", "silence", "quiet", "noise"}
    values = []
    for c in manifest["cases"]:
        wav, mel = data[c["name"] + "/wav"], data[c["name"] + "/mel"]
        assert wav.dtype == np.float32 and wav.shape == (c["length"],)
        assert mel.dtype == np.float64 and mel.shape == (80, 1 + c["length"] // 200) == (80, c["frames"])
        assert np.array_equal(mr.melspectrogram(wav), mel), c["name"]
        values.append(mel.ravel())
        for w in c.get("windows", []):
            starts = mr.chunk_starts(w["frame_ids"], mel.shape[1], w["fps"]) if w["rule"] == "chunk" else mr.centered_starts(w["frame_ids"], w["fps"])
            assert starts == w["starts"]
            assert np.array_equal(mr.gather(mel.astype(np.float32), starts), data[w["key"]]) and data[w["key"]].dtype == np.float32
    values = np.concatenate(values)
    for clip in (-4.0, 4.0):  # every branch of the normalisation is in the set
        assert 0.01 <= (values == clip).mean() <= 0.5, clip
    assert ((values > -4.0) & (values < 4.0)).mean() > 0.4
    long_zero_run = data["len16000/wav"][4000:7000]
    assert len(long_zero_run) >= 1000 and not long_zero_run.any()


def test_regenerating_the_fixtures_gives_identical_bytes(generator):
    npz, js = generator.file_bytes(*generator.build())
    assert npz == open(os.path.join(REPO, "tests", "golden", "mel.npz"), "rb").read()
    assert js == open(os.path.join(REPO, "tests", "golden", "mel.json"), "rb").read()
    assert len(npz) < 1 << 19


def test_restatement_pieces_equal_scipy_and_numpy(fixture):
    """Each step of the restatement against the library call the reference (or librosa underneath it) makes."""
    signal = pytest.importorskip("scipy.signal")
    data, _ = fixture
    x = data["len3201/wav"].astype(np.float64)
    # lfilter's direct form computes x[n] + (-0.97) x[n-1]: the same two roundings
    assert np.array_equal(mr.preemphasis(x), signal.lfilter([1, -0.97], [1], x))
    # scipy takes the cosine over its own grid of angles (linspace(-pi, pi)): an angle near 2 pi differs by up to 2 ulp(2 pi) =
    # 1.8e-15 between the two grids, the window's slope is at most 0.5, and each side rounds once more (1.1e-16)
    assert np.abs(mr.hann_periodic() - signal.get_window("hann", 800, fftbins=True)).max() <= 0.5 * 1.8e-15 + 2.3e-16
    y = mr.preemphasis(x)
    assert np.array_equal(mr.reflect_pad(y), np.pad(y, 400, mode="reflect"))
    for L in (401, 999):
        assert np.array_equal(mr.reflect_pad(y[:L]), np.pad(y[:L], 400, mode="reflect"))
    wf = mr.windowed_frames(data["len3201/wav"])
    assert wf.shape == (17, 800)
    for t in (0, 5, 16):  # a left-reflected, an interior (chirp into silence) and a right-reflected frame (the loud tone)
        D, R = mr.dft_direct(wf[t]), np.fft.rfft(wf[t])
        assert np.abs(D - R).max() <= 1e-9 * np.abs(R).max(), t


def test_mel_basis_properties():
    import n3dt
    B = n3dt.mel_basis()
    assert B.shape == (80, 401) and B.dtype == np.float32 and (B >= 0).all()
    assert np.array_equal(B, mr.mel_basis())  # two writings of the same formulas
    assert (B.sum(axis=1) > 0).all()                      # no empty filter
    assert ((B > 0).sum(axis=0) <= 2).all()               # at most two filters overlap any bin
    area = B.astype(np.float64).sum(axis=1) * 20.0        # bins are 20 Hz apart
    assert (np.abs(area - 1.0) <= 0.05).all(), (area.min(), area.max())
    f = np.linspace(0.0, 8000.0, 401)
    assert not B[:, (f <= 55.0) | (f >= 7600.0)].any()
    peak = f[B.argmax(axis=1)]
    assert (np.diff(peak) > 0).all() and peak[0] < 150.0 and peak[-1] > 7000.0
    # Slaney's scale: 1000 Hz is mel 15, 6400 Hz is mel 42
    assert mr.hz_to_mel(1000.0) == 15.0 and abs(mr.hz_to_mel(6400.0) - 42.0) < 1e-12 and abs(mr.mel_to_hz(42.0) - 6400.0) < 1e-9


def test_known_answers(fixture):
    data, manifest = fixture
    for L in LENGTHS:
        out = mr.melspectrogram(np.zeros(L, np.float32))
        assert out.shape == (80, 1 + L // 200) and (out == -4.0).all()
    with pytest.raises(ValueError):
        mr.melspectrogram(np.zeros(400, np.float32))
    # a mel amplitude of exactly 1e-4 is the -4 edge, 10 the +4 edge, 1e-5 and below the floor (-4.8 before the clip)
    assert mr.normalise(np.array([1e-4]))[0] == pytest.approx(-4.0, abs=1e-12) and mr.normalise(np.array([10.0]))[0] == 4.0
    assert mr.normalise(np.array([0.0, 1e-9, 1e-5])).tolist() == [-4.0, -4.0, -4.0]
    assert mr.normalise(np.array([0.1]))[0] == pytest.approx(0.8, abs=1e-12)
    assert np.isnan(mr.normalise(np.array([np.nan]))[0])
    # a full-scale sine at a bin centre: pre-emphasis gain |1 - 0.97 e^{-jw}| times the window's sum / 2 = 200
    k = 100
    x = np.sin(2.0 * np.pi * k * np.arange(4000) / 800.0).astype(np.float32)
    w = 2.0 * np.pi * k / 800.0
    gain = abs(1.0 - 0.97 * np.exp(-1j * w))
    assert abs(mr.magnitudes(x)[k, 10] - 200.0 * gain) < 1e-3


def _reference_chunk_loop(ids, mel_len, fps, mel_step_size=16):
    """data_loader_xgaze.py:262-270, transcribed: the start index of the one chunk it appends for frame idx"""
    out = []
    for idx in ids:
        mel_idx_multiplier = 80. / fps
        i = idx
        start_idx = int(i * mel_idx_multiplier)
        if start_idx + mel_step_size > mel_len:
            out.append(mel_len - mel_step_size)
        else:
            out.append(start_idx)
    return out


def _reference_centered_loop(num_frames, fps, mel_len, syncnet_mel_step_size=16):
    """data_loader_xgaze.py:516-523, transcribed: (start index, the clamped column list) of every frame"""
    out = []
    for i in range(num_frames):
        start_frame_num = i - 2
        start_idx = int(80. * (start_frame_num / float(fps)))
        end_idx = start_idx + syncnet_mel_step_size
        seq = list(range(start_idx, end_idx))
        seq = [min(max(item, 0), mel_len - 1) for item in seq]
        out.append((start_idx, seq))
    return out


@pytest.mark.parametrize("fps", [25.0, 30.0])
def test_window_start_tables_equal_the_reference_loops(fps):
    from n3dt import mel
    for T in (16, 81, 201):
        n_video = int(T * fps / 80.0) + 3
        ids = list(range(n_video))
        assert mel.window_starts(ids, T, fps, "chunk") == _reference_chunk_loop(ids, T, fps) == mr.chunk_starts(ids, T, fps)
        ref = _reference_centered_loop(n_video, fps, T)
        starts = mel.window_starts(ids, T, fps, "centered")
        assert starts == [s for s, _ in ref] == mr.centered_starts(ids, fps)
        cols = np.arange(T, dtype=np.float64)[None, :].repeat(80, axis=0)
        assert [list(map(int, w[0])) for w in mr.gather(cols, starts)] == [seq for _, seq in ref]
    assert mel.window_starts([0, 1, 2, 3], 81, 25.0, "centered") == [-6, -3, 0, 3]   # int() truncates towards zero
    assert mel.window_starts([0, 1, 2, 3], 81, 30.0, "centered") == [-5, -2, 0, 2]
    assert mel.window_starts([20, 21, 25, 400], 81, 25.0, "chunk") == [64, 65, 65, 65]


SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _host_compiler(tmp_path):
    """(compiler, sanitizer flags) of a host C++ compiler, or None when there is none.  The flags are empty when the compiler
    cannot link the address and undefined-behaviour sanitizers.  Their runtimes are linked statically where the compiler can."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    found = [shutil.which(name) for name in (os.environ.get("CXX"), "g++", "c++", "clang++") if name]
    found = [cxx for cxx in found if cxx]
    for cxx in found:
        for extra in (["-static-libasan", "-static-libubsan"], []):
            if subprocess.run([cxx] + SANITIZE + extra + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode == 0:
                return cxx, SANITIZE + extra
    return (found[0], []) if found else None


def test_frame_walk_on_the_host_under_sanitizers(fixture, tmp_path):
    """csrc/mel_core.h -- the code the kernel is compiled from -- over the 999-sample fixture on the CPU: two frames reflected on the
    left, one interior, two reflected on the right; the program also recomputes the frames a mid-signal run can hold from the
    shortest such run and insists on the same bits.  Any read outside the waveform, the table, the basis or the frame memory ends
    the program through the sanitizer.  Where the compiler has no sanitizer runtimes the numbers are still checked, on an
    unsanitised build, and only the sanitizer claim is skipped."""
    from n3dt import mel
    found = _host_compiler(tmp_path)
    if found is None:
        pytest.skip("no host C++ compiler found (tried $CXX, g++, c++, clang++)")
    cxx, flags = found
    exe = tmp_path / "mel_core_host"
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off"] + flags +
                           [os.path.join(REPO, "tests", "mel_core_host.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    data, _ = fixture
    wav, want = data["len999/wav"], data["len999/mel"]
    raw = tmp_path / "len999.bin"
    with open(raw, "wb") as f:
        f.write(np.array([len(wav)], np.int64).tobytes())
        f.write(wav.tobytes())
        f.write(mel.twiddle_table().tobytes())
        f.write(np.ascontiguousarray(mel.mel_basis()).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([str(exe), str(raw)], capture_output=True, text=True, env=env, timeout=120)
    assert run.returncode == 0 and not run.stderr.strip(), "sanitizer or program error (%d):\n%s" % (run.returncode, run.stderr)
    rows = [line.split() for line in run.stdout.strip().splitlines()]
    assert [(int(r[0]), int(r[1])) for r in rows] == [(t, i) for t in range(5) for i in range(80)]
    got = np.array([float(r[2]) for r in rows]).reshape(5, 80).T
    err = np.abs(got - want).max()
    print("len999: max |d mel| %.3e" % err)
    assert err <= 1e-9
    if not flags:
        pytest.skip("%s cannot link -fsanitize=address,undefined: the frame walk's numbers were checked (they hold), "
                    "the sanitizer claim was not" % cxx)
