"""Host side of the S3FD face detector (n3dt.S3FD, n3dt_s3fd_*), no GPU: the exports and their documented refusals, the table and
state-dict keys against the fixture, the float64 restatement (tests/s3fd_restatement.py) against the fixture recorded from the
reference's own class and functions (tests/golden/s3fd*), the NMS-equivalence argument against the reference's recorded
detections, the pads and the smoothing against the reference's recorded boxes (F < T included), the fixture's own conditions, and
the kernels' index arithmetic (csrc/s3fd_core.h) walked over the kernels' grids on the CPU under the address and
undefined-behaviour sanitizers."""
import os
import subprocess

import numpy as np
import pytest
import torch

import s3fd_restatement as sr
from test_eval_metrics_cpu import _host_compiler

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"n3dt_s3fd_packed_bytes", "n3dt_s3fd_pack", "n3dt_s3fd_max_images", "n3dt_s3fd_positions", "n3dt_s3fd_workspace_bytes",
       "n3dt_s3fd_heads", "n3dt_s3fd_detect", "n3dt_s3fd_boxes", "n3dt_s3fd_block_workspace_bytes", "n3dt_s3fd_block"}


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("s3fd")


@pytest.fixture(scope="module")
def weights(fixture):
    from n3dt import synthetic as syn
    m = fixture[1]
    assert m["weights_seed"] == sr.WEIGHTS_SEED and m["face_bias"] == list(syn.S3FD_FACE_BIAS) and m["empty_face_bias"] == list(syn.S3FD_EMPTY_FACE_BIAS)
    sd = syn.s3fd_state_dict(sr.WEIGHTS_SEED)
    checksum = float(sum(float(v.double().abs().sum()) for v in sd.values()))
    assert abs(checksum - m["weights_checksum"]) <= 1e-9 * m["weights_checksum"], "the stand-in weights drifted from the fixture"
    return sd


@pytest.fixture(scope="module")
def chains(fixture, weights):
    """the float64 restatement of every case on the bytes the reference read, computed once"""
    data, _ = fixture
    from n3dt.s3fd import MEANS
    out = {}
    for case in sr.CASES:
        u8 = data[case + "/frames_u8"]
        assert np.array_equal(u8, sr.fixture_frames(case))
        x = torch.as_tensor(u8).permute(0, 3, 1, 2).double() - torch.tensor(MEANS, dtype=torch.float64)[None, :, None, None]
        out[case] = sr.chain(weights, x)
    return out


def test_exports_abi_and_refusals():
    from n3dt import _lib
    L = _lib.lib()
    assert NEW <= set(_lib.EXPORTS) and L.n3dt_abi_version() == 5
    assert L.n3dt_s3fd_packed_bytes() % 256 == 0 and L.n3dt_s3fd_packed_bytes() > 2 * 2 * 20_000_000  # hi + lo bf16 of 22.4 M weights
    assert L.n3dt_s3fd_workspace_bytes(1, 31, 64) == 0 and b"32..4096" in L.n3dt_last_error()
    assert L.n3dt_s3fd_workspace_bytes(1, 64, 4097) == 0
    assert L.n3dt_s3fd_workspace_bytes(0, 64, 64) == 0 and b"max_images" in L.n3dt_last_error()
    assert L.n3dt_s3fd_positions(16, 64) == 0
    cap = L.n3dt_s3fd_max_images(512, 512)
    assert 1 <= cap <= 1024
    assert 0 < L.n3dt_s3fd_workspace_bytes(cap, 512, 512) <= 4 << 30
    assert L.n3dt_s3fd_workspace_bytes(cap + 1, 512, 512) == 0
    assert L.n3dt_s3fd_max_images(32, 32) == 1024
    assert L.n3dt_s3fd_block_workspace_bytes(33, 1, 8, 8) == 0 and b"0..32" in L.n3dt_last_error()
    assert L.n3dt_s3fd_block_workspace_bytes(19, 1, 1, 8) == 0  # a pool of a one-row map is empty
    # entry points refuse before anything is enqueued: no device is touched here
    import ctypes
    d = ctypes.c_void_p(256)
    assert L.n3dt_s3fd_detect(1, 64, 64, d, d, 0, None, d, d, d, d, ctypes.c_size_t(1 << 40), None) == -1 and b"max_faces" in L.n3dt_last_error()
    assert L.n3dt_s3fd_detect(1, 64, 64, d, d, 16, None, d, d, d, d, ctypes.c_size_t(16), None) == -1 and b"workspace too small" in L.n3dt_last_error()
    assert L.n3dt_s3fd_heads(1, 16, 64, d, d, None, d, ctypes.c_size_t(1 << 40), None) == -1
    assert L.n3dt_s3fd_boxes(0, 64, 64, 1, d, d, 0, 10, 0, 0, 5, d, d, d, None) == -1 and b"n_frames" in L.n3dt_last_error()
    assert L.n3dt_s3fd_boxes(4, 64, 64, 1, d, d, 0, 10, 0, 0, 65, d, d, d, None) == -1 and b"smooth" in L.n3dt_last_error()
    assert L.n3dt_s3fd_block(3, 1, 8, 8, d, d, d, d, ctypes.c_size_t(16), None) == -1
    assert L.n3dt_s3fd_pack(None, d, None) == -1


def test_table_sizes_and_keys_against_the_fixture(fixture, weights):
    from n3dt import _lib, s3fd
    data, m = fixture
    assert m["block_names"] == s3fd.block_names() and len(m["block_names"]) == _lib.S3FD_BLOCKS == sr.N_BLOCKS
    keys = s3fd.state_dict_keys()
    recorded = m["state_dict_keys"]  # the reference class's own state dict, in its order
    assert list(keys) == [k for k, _ in recorded] == list(weights)
    assert all(tuple(shape) == keys[k] == tuple(weights[k].shape) for k, shape in recorded)
    assert len(keys) == 2 * _lib.S3FD_PARAMS + 3
    assert m["n_params"] == sum(int(np.prod(v)) for v in keys.values())
    L = _lib.lib()
    for case, (n, H, W) in sr.CASES.items():
        sizes = s3fd.level_sizes(H, W)
        assert [tuple(data["%s/head%02d" % (case, 2 * l)].shape[2:]) for l in range(6)] == sizes
        assert L.n3dt_s3fd_positions(H, W) == s3fd.positions(H, W) == data[case + "/score"].shape[1]
    assert s3fd.level_sizes(37, 70)[3] == (5, 6) and s3fd.level_sizes(32, 32) == [(8, 8), (4, 4), (2, 2), (5, 5), (3, 3), (2, 2)]
    assert s3fd.level_sizes(37, 70)[2] == (2, 4)  # conv5_3's 2 x 4 map: pool5 leaves 1 x 2 (fc6: 5 x 6); every pool floored a row or a column away
    with pytest.raises(KeyError):
        s3fd.load_s3fd({k: v for k, v in weights.items() if k != "fc7.bias"})
    with pytest.raises(KeyError):
        s3fd.load_s3fd(dict(weights, extra=torch.zeros(1)))
    with pytest.raises(ValueError):
        s3fd.load_s3fd(dict(weights, **{"fc6.weight": torch.zeros(1024, 512, 1, 1)}))
    with pytest.raises(ValueError):
        s3fd.S3FD(weights).detect(torch.zeros(1, 3, 64, 64))  # no CPU path


def test_restatement_reproduces_the_reference(fixture, chains):
    """every block's output (sum, abs-sum, every 211th element), the twelve head maps, the scores and the decoded boxes, within
    1e-12 of the largest value"""
    data, _ = fixture
    blocks = np.load(os.path.join(REPO, "tests", "golden", "s3fd_blocks.npz"))
    for case, (ins, outs) in chains.items():
        for b, act in enumerate(outs):
            s, sa, sample = sr.summary(act)
            want = data[case + "/block_sums"][b]
            scale = max(float(act.abs().max()), 1e-300)
            assert abs(s - want[0]) <= 1e-12 * max(want[1], 1.0) and abs(sa - want[1]) <= 1e-12 * max(want[1], 1.0), (case, b)
            assert np.abs(sample - blocks["%s/block%02d/sample" % (case, b)]).max() <= 1e-12 * scale, (case, b)
        maps = sr.head_maps(outs)
        for k, mp in enumerate(maps):
            assert np.abs(mp.numpy() - data["%s/head%02d" % (case, k)]).max() <= 1e-12, (case, k)
        score, box = sr.scores_and_boxes(maps)
        assert np.abs(score - data[case + "/score"]).max() <= 1e-12
        assert np.abs(box - data[case + "/box"]).max() <= 1e-9  # coordinates reach the hundreds


def test_greedy_tail_equals_the_reference_detections(fixture):
    """The argument of DESIGN 3.18: batch_detect's 0.05 threshold and its replication of every passing position to all images add
    only boxes at or below 0.5 and exact duplicates; greedy NMS visits boxes in descending score, so whether a box above 0.5 is
    kept depends only on boxes above it; the additions are dropped by the final score > 0.5 and, ranking below, suppress nothing
    that survives.  Checked: the greedy tail on the reference's recorded scores and boxes IS what detect_from_batch returned, bit
    for bit, and its top box is get_detections_for_batch's rect."""
    data, m = fixture
    kept = []
    for case in sr.CASES:
        score, box, dets, count, rects = (data["%s/%s" % (case, k)] for k in ("score", "box", "dets", "count", "rects"))
        for i in range(score.shape[0]):
            mine, left = sr.greedy_nms(score[i], box[i], 1 << 30)
            assert left == 0 and len(mine) == count[i] and np.array_equal(mine, dets[i, :count[i]]), (case, i)
            assert np.all(np.diff(mine[:, 4]) < 0)
            assert sr.top_rect(mine) == tuple(int(v) for v in rects[i])
            capped, left = sr.greedy_nms(score[i], box[i], 2)
            assert np.array_equal(capped, mine[:2]) and (left > 0) == (len(mine) > 2 or left > 0)
            kept.append(len(mine))
    assert max(kept) >= 3 and min(kept) >= 1


def test_fixture_conditions(fixture):
    data, m = fixture
    margin = 100.0 * m["bounds"]["score"]
    for case in sr.CASES:
        score = data[case + "/score"]
        share = (score > 0.5).mean(axis=1)
        assert share.min() >= 0.005 and share.max() <= 0.20
        assert np.abs(score - 0.5).min() > margin
        assert m["stats"][case]["max_zero_share"] <= 0.6
    c = m["coordinates"]
    assert c["top_box_skipped"] == 0 and c["skipped"] <= c["cap"] * c["compared"] and c["cap"] == 0.02
    assert m["empty_max_score"] < 0.5 - margin
    assert m["bounds"]["gpu_factor"] == 4.0 and len(m["bounds"]["block"]) == sr.N_BLOCKS and len(m["bounds"]["heads"]) == 12


def test_pads_and_smoothing_against_the_reference(fixture):
    """the loader's pad lines and get_smoothened_boxes (recorded from the reference's own statements) on the clip's first F rects,
    F = 2, 3, 4 (the negative slice), 5 and 9"""
    data, m = fixture
    _, H, W = sr.CASES["clip"]
    rects = [tuple(int(v) for v in r) for r in data["clip/rects"]]
    for F_ in m["smooth_cases"]:
        padded = [sr.pad_rect(r, H, W, m["pads"]) for r in rects[:F_]]
        assert np.array_equal(np.array(padded), data["clip/padded%d" % F_])
        smoothed = sr.smooth_boxes(padded, m["smooth"])
        assert np.array_equal(np.array(smoothed), data["clip/smoothed%d" % F_]), F_
        boxes, found = sr.crop_boxes(rects[:F_], H, W, m["pads"], m["smooth"])
        assert all(found) and boxes == [[b[1], b[3], b[0], b[2]] for b in smoothed]
    # the windows, literally: numpy's slices on an index array
    for F_ in range(1, 13):
        for T in range(1, 9):
            idx = np.arange(F_)
            for i in range(F_):
                window = idx[len(idx) - T:] if i + T > len(idx) else idx[i:i + T]
                start = F_ - T if i + T > F_ else i
                if start < 0:
                    start = max(0, F_ + start)
                assert window[0] == start and window[-1] == (F_ - 1 if i + T > F_ else i + T - 1)
    assert sr.crop_boxes([None, (3, 4, 30, 40)], 64, 96, (0, 10, 0, 0), 0) == ([[0, 64, 0, 96], [4, 50, 3, 30]], [False, True])


def test_emulation_stays_within_its_recorded_bounds(fixture, weights, chains):
    """the bounds in the manifest are the emulation's own error: measured again here for the smallest case"""
    data, m = fixture
    case = "c"
    ins, outs = chains[case]
    frames = sr.frames_f32(data[case + "/frames_u8"])
    maps = [torch.as_tensor(data["%s/head%02d" % (case, k)]) for k in range(12)]
    b = sr.measured_bounds(weights, frames, ins, outs, maps, data[case + "/score"], data[case + "/box"])
    assert all(x <= y * (1 + 1e-6) + 1e-300 for x, y in zip(b["block"], m["bounds"]["block"]))
    assert all(x <= y * (1 + 1e-6) for x, y in zip(b["heads"], m["bounds"]["heads"]))
    assert b["score"] <= m["bounds"]["score"] * (1 + 1e-6) and b["box"] <= m["bounds"]["box"] * (1 + 1e-6)


def test_index_walk_on_the_host_under_sanitizers(tmp_path):
    """csrc/s3fd_core.h over the convolution kernel's grid, the pool, the norm and the pack on the CPU: every block at the fixture
    shapes and at n = 1, 3 for 32 x 32, the smallest legal frame (fc6 on a 1 x 1 map with halo 3).  A stand-alone program with its
    own main, built here with the host compiler under -fsanitize=address,undefined and run directly.  It counts the stores: every
    cell of every map once, halo included, none outside the carve; every load inside its map and the convolution's own tap."""
    from n3dt import s3fd
    found = _host_compiler(tmp_path)
    if found is None:
        pytest.skip("no host C++ compiler found (tried $CXX, g++, c++, clang++)")
    cxx, flags = found
    exe = tmp_path / "s3fd_core_host"
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off"] + flags +
                           [os.path.join(REPO, "tests", "s3fd_core_host.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    shapes = [sr.CASES[c] for c in ("a", "b", "c", "clip")] + [(1, 32, 32), (3, 32, 32)]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([str(exe)] + [str(v) for s in shapes for v in s], capture_output=True, text=True, env=env, timeout=900)
    assert run.returncode == 0 and not run.stderr.strip(), "sanitizer or program error:\n" + run.stderr
    rows = [[int(v) for v in line.split()] for line in run.stdout.strip().splitlines()]
    assert len(rows) == len(shapes) * sr.N_BLOCKS
    for k, (n, H, W) in enumerate(shapes):
        mine = rows[k * sr.N_BLOCKS:(k + 1) * sr.N_BLOCKS]
        assert sorted(r[3] for r in mine) == list(range(sr.N_BLOCKS))
        for r in mine:
            assert r[:3] == [n, H, W]
            cin, cout, ho, wo = s3fd.block_shape(r[3], r[4], r[5])
            assert r[6:9] == [ho, wo, cout] and r[9] >= n * ho * wo * cout and ho >= 1 and wo >= 1
        fc6 = [r for r in mine if r[3] == 13][0]
        assert fc6[6] == fc6[4] + 4 and fc6[7] == fc6[5] + 4
        if (H, W) == (32, 32):
            assert fc6[4:6] == [1, 1]
    if not flags:
        pytest.skip("%s cannot link -fsanitize=address,undefined: the index walk was checked (it holds), the sanitizer claim was not" % cxx)
