"""Host side of the lip-sync metric (n3dt.SyncNet / n3dt.SyncMeter, n3dt_syncnet_*), no GPU: the exports and their documented
refusals, the float64 restatement against the fixture recorded from the reference's class, its resample against
F.interpolate, the state-dict loader, the meter's window starts and drop rule against a literal loop, and the kernels' index
arithmetic (csrc/syncnet_core.h) walked over the convolution kernel's grid on the CPU under the address and
undefined-behaviour sanitizers."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import syncnet_restatement as sr
from test_eval_metrics_cpu import _host_compiler

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"n3dt_syncnet_packed_bytes", "n3dt_syncnet_pack", "n3dt_syncnet_workspace_bytes", "n3dt_syncnet_face_windows", "n3dt_syncnet_fwd",
       "n3dt_syncnet_block"}


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("syncnet")


@pytest.fixture(scope="module")
def weights():
    from n3dt import synthetic as syn
    return syn.syncnet_state_dict(sr.WEIGHTS_SEED)


@pytest.fixture(scope="module")
def restated(fixture, weights):
    data, _ = fixture
    faces, mel = sr.faces_from_u8(data["faces_u8"]), sr.mel_from_u8(data["mel_u8"])
    return (faces, mel) + tuple(sr.chain64(weights, faces, mel))


def test_new_symbols_are_declared_and_exported():
    from n3dt import _lib
    L = _lib.lib()
    header = open(os.path.join(REPO, "include", "n3dt.h")).read()
    declared = set(re.findall(r"\b(n3dt_syncnet[a-z0-9_]*)\s*\(", header))
    assert declared == NEW
    for name in declared:
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert L.n3dt_abi_version() == 5
    assert ctypes.sizeof(_lib.SyncnetParams) == 6 * 31 * ctypes.sizeof(ctypes.c_void_p)
    import n3dt
    assert n3dt.SyncNet is n3dt.eval_utils.SyncNet and n3dt.SyncMeter is n3dt.eval_utils.SyncMeter


def test_sizes_follow_the_table():
    from n3dt import _lib
    from n3dt.syncnet import BLOCKS, block_shapes
    L = _lib.lib()
    assert L.n3dt_syncnet_workspace_bytes(0) == 0 and b"n outside 1..1024" in L.n3dt_last_error()
    assert L.n3dt_syncnet_workspace_bytes(1025) == 0 and b"n outside 1..1024" in L.n3dt_last_error()
    # packed: hi + lo bf16 matrices with C_in padded to 16 (15 -> 16, 1 -> 16), then the folded biases, each rounded up to 256 bytes
    mats = [kh * kw * ((cin + 15) // 16 * 16) * cout * 4 for cin, cout, (kh, kw), _, _, _ in BLOCKS]
    biases = [(cout * 4 + 255) // 256 * 256 for _, cout, _, _, _, _ in BLOCKS]
    assert all(m % 256 == 0 for m in mats)
    assert L.n3dt_syncnet_packed_bytes() == sum(mats) + sum(biases)
    assert 65e6 < L.n3dt_syncnet_packed_bytes() < 67e6
    # workspace: the face windows, two copies of the largest map (block 0's output, 50 x 98 x 32), two 512-vectors, per window
    shapes = block_shapes()
    assert shapes[0] == ((15, 48, 96), (32, 48, 96)) and shapes[1][1] == (64, 46, 47) and shapes[16][1] == (512, 1, 1)
    assert shapes[17] == ((1, 80, 16), (32, 80, 16)) and shapes[20][1] == (64, 27, 16) and shapes[23][1] == (128, 9, 6)
    assert shapes[26][1] == (256, 3, 3) and shapes[30][1] == (512, 1, 1)
    for n in (1, 3, 128):
        assert L.n3dt_syncnet_workspace_bytes(n) == 4 * n * (15 * 48 * 96 + 2 * 50 * 98 * 32 + 2 * 512)


def test_entry_points_refuse_bad_arguments_before_anything_is_enqueued():
    from n3dt import _lib
    L = _lib.lib()
    d = ctypes.c_void_p(4096)
    need = L.n3dt_syncnet_workspace_bytes(3)
    # n, packed, mel, faces, frames, boxes, n_boxes, H, W, audio_emb, face_emb, cos, ws, ws_bytes, stream
    good = [3, d, d, d, None, None, 0, 0, 0, d, d, d, d, need, None]
    for i in (1, 2, 12):
        args = list(good)
        args[i] = None
        assert L.n3dt_syncnet_fwd(*args) == -1 and b"NULL" in L.n3dt_last_error(), i
    args = list(good)
    args[13] = need - 1
    assert L.n3dt_syncnet_fwd(*args) == -1 and b"workspace too small" in L.n3dt_last_error()
    for i, what in ((11, b"8-byte"), (2, b"16-byte"), (3, b"16-byte"), (9, b"16-byte"), (10, b"16-byte"), (1, b"256-byte"), (12, b"256-byte")):
        args = list(good)
        args[i] = ctypes.c_void_p(4096 + 4)
        assert L.n3dt_syncnet_fwd(*args) == -1 and what in L.n3dt_last_error(), i
    args = list(good)
    args[4] = d  # face windows AND frames
    assert L.n3dt_syncnet_fwd(*args) == -1 and b"exactly one" in L.n3dt_last_error()
    args[3] = None  # frames alone: boxes, n_boxes and the frame size are checked
    assert L.n3dt_syncnet_fwd(*args) == -1 and b"2..4096" in L.n3dt_last_error()
    args[7], args[8] = 64, 64
    assert L.n3dt_syncnet_fwd(*args) == -1 and b"NULL" in L.n3dt_last_error()
    args[5], args[6] = d, 5
    assert L.n3dt_syncnet_fwd(*args) == -1 and b"n_boxes" in L.n3dt_last_error()
    args = list(good)
    args[3] = None
    assert L.n3dt_syncnet_fwd(*args) == -1 and b"exactly one" in L.n3dt_last_error()
    for n in (0, 1025):
        assert L.n3dt_syncnet_fwd(n, *good[1:]) == -1 and b"n outside" in L.n3dt_last_error()
    assert L.n3dt_syncnet_face_windows(3, 64, 64, d, d, 2, d, None) == -1 and b"n_boxes" in L.n3dt_last_error()
    assert L.n3dt_syncnet_face_windows(3, 1, 64, d, d, 1, d, None) == -1 and b"2..4096" in L.n3dt_last_error()
    assert L.n3dt_syncnet_face_windows(3, 64, 64, d, d, 7, None, None) == -1 and b"NULL" in L.n3dt_last_error()
    for block in (-1, 31):
        assert L.n3dt_syncnet_block(block, 1, d, d, d, d, 1 << 40, None) == -1 and b"block outside 0..30" in L.n3dt_last_error()
    assert L.n3dt_syncnet_block(0, 1, d, None, d, d, 1 << 40, None) == -1 and b"NULL" in L.n3dt_last_error()
    assert L.n3dt_syncnet_block(0, 1, d, d, d, d, 16, None) == -1 and b"workspace too small" in L.n3dt_last_error()
    p = _lib.SyncnetParams()
    assert L.n3dt_syncnet_pack(ctypes.byref(p), d, None) == -1 and b"NULL parameter" in L.n3dt_last_error()
    assert L.n3dt_syncnet_pack(None, d, None) == -1 and L.n3dt_syncnet_pack(ctypes.byref(p), None, None) == -1
    assert L.n3dt_syncnet_pack(ctypes.byref(p), ctypes.c_void_p(4100), None) == -1 and b"256-byte" in L.n3dt_last_error()


def test_cpu_tensors_raise(weights):
    from n3dt import SyncMeter, SyncNet
    net = SyncNet(weights)
    mel, faces = torch.zeros(1, 1, 80, 16), torch.zeros(1, 15, 48, 96)
    for call in (lambda: net(mel, faces), lambda: net.cos(mel, faces), lambda: net.layers(mel, faces), lambda: net.block(0, faces),
                 lambda: net.face_windows(torch.zeros(5, 3, 32, 32), (0, 32, 0, 32)), lambda: SyncMeter(net, torch.zeros(80, 100))):
        with pytest.raises(ValueError, match="GPU"):
            call()
    with pytest.raises(TypeError, match="SyncNet"):
        SyncMeter(object(), torch.zeros(80, 100))


def test_stand_in_weights_are_seeded_and_have_the_stated_statistics(weights):
    from n3dt import synthetic as syn
    from n3dt.syncnet import BLOCKS, block_names
    again = syn.syncnet_state_dict(sr.WEIGHTS_SEED)
    assert sorted(weights) == sorted(again) and all(torch.equal(weights[k], again[k]) for k in weights)
    assert not torch.equal(weights["face_encoder.0.conv_block.0.weight"], syn.syncnet_state_dict(sr.WEIGHTS_SEED + 1)["face_encoder.0.conv_block.0.weight"])
    assert len(weights) == 31 * 7
    for name, (cin, cout, (kh, kw), _, _, _) in zip(block_names(), BLOCKS):
        w, b = weights[name + ".conv_block.0.weight"], weights[name + ".conv_block.0.bias"]
        bound = (cin * kh * kw) ** -0.5 * (1.0 + 2.0 ** -22)  # fp32 rounding of the product; torch's default: kaiming_uniform_(a = sqrt(5)) is U(-1 / sqrt(fan_in), 1 / sqrt(fan_in))
        assert tuple(w.shape) == (cout, cin, kh, kw) and float(w.abs().max()) <= bound and float(b.abs().max()) <= bound
        assert float(w.abs().max()) > 0.9 * bound
        var, gamma = weights[name + ".conv_block.1.running_var"], weights[name + ".conv_block.1.weight"]
        assert 0.5 <= float(var.min()) and float(var.max()) <= 1.5 and 0.5 <= float(gamma.min()) and float(gamma.max()) <= 1.5
        for k in ("running_mean", "bias"):
            assert float(weights["%s.conv_block.1.%s" % (name, k)].abs().max()) < 0.6
    assert sum(v.numel() for k, v in weights.items() if "running" not in k and "num_batches" not in k) == 16435072


def test_loader_takes_the_reference_keys_and_names_what_is_missing(weights):
    from n3dt.syncnet import SyncNet, load_syncnet
    plain = load_syncnet(weights)
    assert len(plain) == 31 and all(len(b) == 6 for b in plain)
    wrapped = {"module." + k: v for k, v in weights.items()}
    wrapped["module.extra.thing"] = torch.zeros(3)
    for a, b in zip(plain, load_syncnet(wrapped)):
        assert all(torch.equal(s, t) for s, t in zip(a, b))
    without = {k: v for k, v in weights.items() if "num_batches_tracked" not in k}
    assert len(SyncNet(without).weights) == 31
    for key in ("face_encoder.0.conv_block.0.weight", "audio_encoder.13.conv_block.1.running_var", "face_encoder.16.conv_block.1.bias",
                "audio_encoder.3.conv_block.0.bias"):
        sd = {k: v for k, v in weights.items() if k != key}
        with pytest.raises(KeyError, match=re.escape(key)):
            SyncNet(sd)
    sd = dict(weights)
    sd["face_encoder.1.conv_block.0.weight"] = torch.zeros(64, 32, 3, 3)  # the 5 x 5 block
    with pytest.raises(ValueError, match=r"face_encoder\.1\.conv_block\.0\.weight"):
        SyncNet(sd)
    sd = dict(weights)
    sd["audio_encoder.0.conv_block.1.running_mean"] = torch.zeros(64)
    with pytest.raises(ValueError, match=r"audio_encoder\.0\.conv_block\.1\.running_mean"):
        SyncNet(sd)
    with pytest.raises(TypeError):
        SyncNet([1, 2, 3])


def test_restatement_reproduces_every_fixture_value(fixture, weights, restated):
    data, manifest = fixture
    assert manifest["weights_seed"] == sr.WEIGHTS_SEED and manifest["input_seed"] == sr.INPUT_SEED and manifest["n_windows"] == sr.N_WINDOWS == 3
    assert sorted(manifest["parity_unpinned"]) == ["opencv_resize", "weights", "window_convention"]
    checksum = float(sum(float(v.double().abs().sum()) for v in weights.values()))
    assert abs(checksum - manifest["weights_checksum"]) <= 1e-9 * checksum, "the seeded weight generator drifted from the fixture"
    faces_u8, mel_u8 = sr.fixture_inputs()
    assert np.array_equal(faces_u8, data["faces_u8"]) and np.array_equal(mel_u8, data["mel_u8"])
    _, _, acts, a, f, cos = restated
    assert len(acts) == 31 and [list(x.shape[1:]) for x in acts] == manifest["block_shapes"]
    for b, act in enumerate(acts):
        s, sa, sample = sr.summary(act)
        want_s, want_sa = data["block_sums"][b]
        assert abs(sa / want_sa - 1.0) <= 1e-12 and abs(s - want_s) <= 1e-12 * want_sa, b
        want = data["block%02d/sample" % b]
        assert sample.shape == want.shape and np.abs(sample - want).max() <= 1e-12 * np.abs(want).max(), b
        assert 0.05 < float(act.abs().max()) < 50.0 and abs(float(act.abs().max()) / manifest["block_max_abs"][b] - 1.0) < 1e-12  # O(1) through all blocks
    for got, key in ((a, "audio_emb"), (f, "face_emb"), (cos, "cos")):
        assert np.abs(got.numpy() - data[key]).max() <= 1e-12 * np.abs(data[key]).max(), key
    assert np.abs(np.linalg.norm(data["face_emb"], axis=1) - 1.0).max() < 1e-14
    assert 0.2 < data["cos"].min() and data["cos"].max() < 0.5 and float((data["audio_emb"] == 0).mean()) > 0.3


def test_bounds_are_measured_from_the_emulation_alone(fixture, weights, restated):
    """The manifest's bounds are the emulation's error on the machine that generated the fixture.  Another CPU sums the fp32
    convolutions in another order; what this machine measures must sit within the same 4 x the GPU gets (figures printed)."""
    _, manifest = fixture
    bounds = manifest["bounds"]
    assert bounds["gpu_factor"] == 4.0 and len(bounds["block"]) == 31
    assert all(1e-7 < v < 1e-4 for v in bounds["block"]) and 1e-8 < bounds["cos"] < bounds["embedding"] < 1e-5
    # split operands drop lo * lo, 2^-18 relative per product: far above the float32 class (recorded for orientation), far below bf16
    assert manifest["float32_class_error"]["embedding"] < bounds["embedding"] < 1e-3
    faces, mel, acts, a, f, cos = restated
    here = sr.measured_bounds(weights, faces, mel, acts, a, f, cos)
    for b in range(31):
        print("block %2d: emulation error here %.3e, recorded %.3e" % (b, here["block"][b], bounds["block"][b]))
        assert here["block"][b] <= 4.0 * bounds["block"][b], b
    print("embedding %.3e (recorded %.3e), cos %.3e (recorded %.3e)" % (here["embedding"], bounds["embedding"], here["cos"], bounds["cos"]))
    assert here["embedding"] <= 4.0 * bounds["embedding"] and here["cos"] <= 4.0 * bounds["cos"]


def test_folded_batch_norm_is_the_formula(weights, restated):
    """conv with w' = w s and b' = (b - mean) s + beta, s = gamma / sqrt(var + eps), in float64, is the unfolded block"""
    from n3dt.syncnet import BLOCKS
    faces, mel, acts = restated[:3]
    ins = sr.block_inputs(acts, faces, mel)
    for b in (0, 3, 16, 17, 20, 30):
        w, bias, gamma, beta, mean, var = sr.block_params(weights, b)
        s = gamma / torch.sqrt(var + 1e-5)
        y = F.conv2d(ins[b], w * s[:, None, None, None], (bias - mean) * s + beta, stride=BLOCKS[b][3], padding=BLOCKS[b][4])
        y = torch.relu(y + ins[b] if BLOCKS[b][5] else y)
        assert float((y - acts[b]).abs().max()) <= 1e-13 * float(acts[b].abs().max()), b
        w32, b32 = sr.fold(weights, b)
        assert w32.dtype == torch.float32 and float((w32.double() - w * s[:, None, None, None]).abs().max()) <= 2.0 ** -24 * float(w32.abs().max())
        hi, lo = sr.split(w32)
        assert float((w32 - hi - lo).abs().max()) <= 2.0 ** -16 * float(w32.abs().max())


@pytest.mark.parametrize("box", [(7, 138, 20, 137), (0, 160, 0, 160), (100, 160, 90, 160), (3, 35, 5, 37), (50, 51, 60, 61)])
def test_resample_is_torchs_bilinear_with_half_pixel_centres(box):
    """131 x 117 down, the whole frame, a box touching the corner, a 32 x 32 box up, a single pixel: F.interpolate in float64"""
    g = torch.Generator().manual_seed(5)
    frame = torch.rand(3, 160, 160, generator=g, dtype=torch.float64)
    y1, y2, x1, x2 = box
    want = F.interpolate(frame[None, :, y1:y2, x1:x2], size=(96, 96), mode="bilinear", align_corners=False, antialias=False)[0]
    got = sr.resample96(frame.numpy()[:, y1:y2, x1:x2])
    assert got.shape == (3, 96, 96) and np.abs(got - want.numpy()).max() <= 1e-14


def test_face_windows_follow_the_window_convention():
    g = torch.Generator().manual_seed(6)
    frames = torch.rand(7, 3, 40, 50, generator=g, dtype=torch.float64).numpy()
    boxes = [(i, 30 + i, 2 * i, 33 + 2 * i) for i in range(7)]
    win = sr.face_windows(frames, boxes)
    assert win.shape == (3, 15, 48, 96)
    for i in range(3):
        for t in range(5):
            y1, y2, x1, x2 = boxes[i + t]
            full = F.interpolate(torch.as_tensor(frames[i + t:i + t + 1, :, y1:y2, x1:x2]), size=(96, 96), mode="bilinear", align_corners=False)[0].numpy()
            for c in range(3):  # BGR, the lower half
                assert np.abs(win[i, 3 * t + c] - full[2 - c, 48:]).max() <= 1e-14, (i, t, c)
    one = sr.face_windows(frames, (0, 40, 0, 50))
    assert np.array_equal(one, sr.face_windows(frames, [(0, 40, 0, 50)] * 7))
    dirty = frames.copy()
    dirty[0, 0, 3, 3], dirty[1, 1, 4, 4], dirty[2, 2, 5, 5], dirty[3, 0, 6, 6] = np.nan, -0.5, 1.5, np.inf
    clean = np.clip(np.nan_to_num(dirty, nan=0.0, posinf=1.0), 0.0, 1.0)
    assert np.array_equal(sr.face_windows(dirty, (0, 40, 0, 50)), sr.face_windows(clean, (0, 40, 0, 50)))


def test_window_starts_and_the_drop_rule_against_a_literal_loop():
    from n3dt.syncnet import device_starts, window_start, window_starts
    for fps in (25.0, 25, 30.0, 29.97, 24.0, 23.976, 60.0, 12.5):
        for n_frames, T in ((4, 100), (5, 16), (5, 15), (30, 100), (30, 97), (200, 400), (1000, 3201)):
            kept, dropped = [], 0
            for i in range(max(n_frames - 4, 0)):  # the reference's crop_audio_window, then get_segmented_mels' give-up
                start_idx = int(80. * (i / float(fps)))
                if start_idx + 16 > T:
                    dropped += 1
                else:
                    kept.append(start_idx)
            assert (kept, dropped) == sr.meter_starts(n_frames, T, fps)
            # in one piece, and in pieces
            assert window_starts(0, max(n_frames - 4, 0), T, fps) == (kept, dropped)
            pieces, lost, at = [], 0, 0
            for size in (1, 7, 2, 1000):
                size = min(size, max(n_frames - 4, 0) - at)
                k, d = window_starts(at, size, T, fps)
                pieces, lost, at = pieces + k, lost + d, at + size
            assert (pieces, lost) == (kept, dropped)
            assert kept == sorted(kept)  # the starts grow: the kept windows are a prefix
            if kept:  # the device-side starts are the same integers (float64 division and product are IEEE on both sides)
                assert device_starts(0, len(kept), fps, "cpu").tolist() == kept
    assert [window_start(i, 25.0) for i in range(6)] == [0, 3, 6, 9, 12, 16]


def test_meter_result_is_the_literal_mean():
    cos = np.array([0.5, 0.25, 1.0, 0.0])
    res = sr.meter_result(cos)
    assert res["sync_conf"] == 0.4375 and abs(res["sync_loss"] - (np.log(2) + np.log(4) + 0.0 + 100.0) / 4) < 1e-15
    a = np.eye(5)[[0, 1, 2, 3]]
    f = np.eye(5)[[1, 2, 3, 4]]  # face window i looks like audio window i + 1
    res = sr.meter_result(np.zeros(4), a, f, max_shift=2)
    assert res["curve"] == [0.0, 0.0, 0.0, 1.0, 0.0] and res["offset"] == 1


# the window counts the GPU test runs blocks at, and one more
COUNTS = (1, 2, 3)


def test_index_walk_on_the_host_under_sanitizers(tmp_path):
    """csrc/syncnet_core.h -- the functions the convolution kernel takes its rows, halo cells, taps, residual reads and stores from,
    and the prologue its source pixels -- over the kernel's full grid on the CPU, all 31 blocks, n = 1, 2, 3 (n = 1: M = 1 in the
    1x1 blocks and 9 in the 3x3 ones), both instantiations of the kernel.  The program re-types the kernel's loop nest (its header
    says so) but takes the epilogue's row map, the pack kernel's decode and the MFMA step's weight address from csrc/conv_frag.h
    as the kernels do, and walks the pack of every block: every (k, n) packed once, the decode the inverse of the address read,
    the padded channels' rows zero.  A read outside a buffer ends the program through the sanitizer; a read of the wrong
    element, or an output element stored twice or never, fails the program's own check.  Where the compiler has no sanitizer
    runtimes the indices are still checked, on an unsanitised build, and only the sanitizer claim is skipped."""
    from n3dt.syncnet import block_shapes
    found = _host_compiler(tmp_path)
    if found is None:
        pytest.skip("no host C++ compiler found (tried $CXX, g++, c++, clang++)")
    cxx, flags = found
    exe = tmp_path / "syncnet_core_host"
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off"] + flags +
                           [os.path.join(REPO, "tests", "syncnet_core_host.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([str(exe)] + [str(n) for n in COUNTS], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0 and not run.stderr.strip(), "sanitizer or program error:\n" + run.stderr
    rows = [[int(v) for v in line.split()] for line in run.stdout.strip().splitlines()]
    assert [tuple(r[:2]) for r in rows] == [(n, b) for n in COUNTS for b in range(31)]
    shapes = block_shapes()
    for r in rows:  # the extents are the table's, which the fixture pins to the reference's class
        n, b = r[:2]
        (cin, hi, wi), (cout, ho, wo) = shapes[b]
        assert r[2:6] == [hi, wi, ho, wo] and r[8] == cout
        assert r[11] == n * r[6] * r[7] * cout  # every cell of the padded output, once
        assert r[10] > 0
    if not flags:
        pytest.skip("%s cannot link -fsanitize=address,undefined: the index walk was checked (it holds), the sanitizer claim was not" % cxx)
