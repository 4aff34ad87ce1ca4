"""Host side of the 3-D face reconstruction net (n3dt.FaceRecon, n3dt_face_recon_*), no GPU: the exports and their documented
refusals, the tables and state-dict keys against the fixture, the float64 restatement (tests/face_recon_restatement.py) against the
fixture recorded from the reference's own class and functions (tests/golden/face_recon*), its byte resample against the installed
PIL run live, the POS pseudo-inverse against the reference's recorded t and s, the emulation against its recorded bounds, the
fixture's own conditions, and the kernels' index arithmetic (csrc/face_recon_core.h) walked over the kernels' grids on the CPU under
the address and undefined-behaviour sanitizers."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import face_recon_restatement as fr
from test_eval_metrics_cpu import _host_compiler

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"n3dt_face_recon_packed_bytes", "n3dt_face_recon_pack", "n3dt_face_recon_max_images", "n3dt_face_recon_workspace_bytes",
       "n3dt_face_recon_fwd", "n3dt_face_recon_block_workspace_bytes", "n3dt_face_recon_block", "n3dt_face_recon_align"}


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("face_recon")


@pytest.fixture(scope="module")
def aligned(golden):
    return golden("face_recon_align")


@pytest.fixture(scope="module")
def weights(fixture):
    from n3dt import synthetic as syn
    m = fixture[1]
    assert m["weights_seed"] == fr.WEIGHTS_SEED
    sd = syn.face_recon_state_dict(fr.WEIGHTS_SEED)
    checksum = float(sum(float(v.double().abs().sum()) for v in sd.values()))
    assert abs(checksum - m["weights_checksum"]) <= 1e-9 * m["weights_checksum"], "the stand-in weights drifted from the fixture"
    return sd


@pytest.fixture(scope="module")
def chains(weights):
    """the float64 restatement of the three small cases, computed once"""
    return {case: fr.chain(weights, fr.fixture_images(case)) for case in fr.SMALL_CASES}


def test_exports_abi_and_refusals():
    from n3dt import _lib
    import n3dt
    L = _lib.lib()
    assert NEW <= set(_lib.EXPORTS) and L.n3dt_abi_version() == 5
    assert hasattr(n3dt, "FaceRecon") and hasattr(n3dt, "load_face_recon")
    assert ctypes.sizeof(_lib.FaceReconParams) == 8 * (6 * 53 + 2 * 7)
    packed = L.n3dt_face_recon_packed_bytes()
    assert packed % 256 == 0 and packed > 2 * 2 * 23_000_000 + 4 * 257 * 2048  # hi + lo bf16 of 23.5 M conv weights, the fp32 head
    assert L.n3dt_face_recon_workspace_bytes(1, 31, 64) == 0 and b"32..4096" in L.n3dt_last_error()
    assert L.n3dt_face_recon_workspace_bytes(1, 64, 4097) == 0
    assert L.n3dt_face_recon_workspace_bytes(0, 64, 64) == 0 and b"max_images" in L.n3dt_last_error()
    assert L.n3dt_face_recon_max_images(16, 64) == 0
    for H, W in ((224, 224), (4096, 4096)):
        cap = L.n3dt_face_recon_max_images(H, W)
        assert 1 <= cap <= 1024
        assert 0 < L.n3dt_face_recon_workspace_bytes(cap, H, W) <= 4 << 30
        assert cap == 1024 or L.n3dt_face_recon_workspace_bytes(cap + 1, H, W) == 0
    assert L.n3dt_face_recon_max_images(32, 32) == 1024 and L.n3dt_face_recon_max_images(224, 224) >= 128
    assert L.n3dt_face_recon_block_workspace_bytes(56, 1, 8, 8) == 0 and b"0..55" in L.n3dt_last_error()
    assert L.n3dt_face_recon_block_workspace_bytes(55, 1, 2, 2) == 0  # the head takes [n,2048,1,1]
    assert L.n3dt_face_recon_block_workspace_bytes(0, 1, 1, 8) == 0
    # entry points refuse before anything is enqueued: no device is touched here
    d, big = ctypes.c_void_p(256), ctypes.c_size_t(1 << 40)
    assert L.n3dt_face_recon_fwd(1, 64, 64, d, d, d, d, ctypes.c_size_t(16), None) == -1 and b"workspace too small" in L.n3dt_last_error()
    assert L.n3dt_face_recon_fwd(1, 16, 64, d, d, d, d, big, None) == -1
    assert L.n3dt_face_recon_fwd(1, 64, 64, d, None, d, d, big, None) == -1 and b"NULL" in L.n3dt_last_error()
    assert L.n3dt_face_recon_block(3, 1, 8, 8, d, d, None, d, d, big, None) == -1 and b"identity as skip" in L.n3dt_last_error()
    assert L.n3dt_face_recon_block(2, 1, 8, 8, d, d, d, d, d, big, None) == -1 and b"only a bottleneck's third" in L.n3dt_last_error()
    assert L.n3dt_face_recon_block(2, 1, 8, 8, d, d, None, d, d, ctypes.c_size_t(16), None) == -1
    assert L.n3dt_face_recon_align(0, 64, 64, d, d, 68, d, d, 1, d, d, d, d, None) == -1 and b"n outside" in L.n3dt_last_error()
    assert L.n3dt_face_recon_align(1, 64, 64, d, d, 6, d, d, 1, d, d, d, d, None) == -1 and b"68 or 5" in L.n3dt_last_error()
    assert L.n3dt_face_recon_align(1, 1, 64, d, None, 0, d, d, 1, d, d, d, d, None) == -1
    assert L.n3dt_face_recon_pack(None, d, None) == -1
    p = _lib.FaceReconParams()
    assert L.n3dt_face_recon_pack(ctypes.byref(p), d, None) == -1 and b"NULL parameter" in L.n3dt_last_error()


def test_tables_and_keys_against_the_fixture(fixture, aligned, weights):
    from n3dt import _lib, face_recon as nf
    data, m = fixture
    assert m["block_names"] == nf.block_names() and len(m["block_names"]) == _lib.FACE_RECON_BLOCKS == fr.N_BLOCKS == 56
    assert nf.N_CONVS == _lib.FACE_RECON_CONVS == 53 and sum(nf.HEAD_COLS) == _lib.FACE_RECON_COEFFS == 257
    keys = nf.state_dict_keys()
    recorded = m["state_dict_keys"]  # the reference class's own state dict, in its order
    assert list(keys) == [k for k, _ in recorded] == list(weights)
    assert all(tuple(shape) == keys[k] == tuple(weights[k].shape) for k, shape in recorded)
    assert m["n_params"] == sum(int(np.prod(v)) for k, v in keys.items() if not k.endswith(("running_mean", "running_var", "num_batches_tracked")))
    assert m["bn_eps"] == nf.BN_EPS
    assert [c[7] for c in nf.CONVS].count(4) == 4 and [c[7] for c in nf.CONVS].count(3) == 16
    assert [(c[0], c[5]) for c in nf.CONVS if c[5] == 2] == [("backbone.conv1", 2), ("backbone.layer2.0.conv2", 2), ("backbone.layer2.0.downsample.0", 2),
                                                           ("backbone.layer3.0.conv2", 2), ("backbone.layer3.0.downsample.0", 2),
                                                           ("backbone.layer4.0.conv2", 2), ("backbone.layer4.0.downsample.0", 2)]
    for case, (n, H, W) in fr.CASES.items():
        assert data[case + "/coeffs"].shape == (n, 257) and data[case + "/block_sums"].shape == (56, 2)
    # odd maps: 72 x 56 -> 36 x 28 -> 18 x 14 -> 9 x 7 -> 5 x 4 -> 3 x 2
    sizes, hw = [], (72, 56)
    for b in (0, nf.POOL_BLOCK, 12, 25, 44):  # the stem, the pool, layer2.0 / layer3.0 / layer4.0's conv2
        hw = nf.block_shape(b, *hw)[2:]
        sizes.append(hw)
    assert sizes == [(36, 28), (18, 14), (9, 7), (5, 4), (3, 2)]
    assert [nf.CONVS[b][0] for b in (12, 25, 44)] == ["backbone.layer2.0.conv2", "backbone.layer3.0.conv2", "backbone.layer4.0.conv2"]
    assert aligned[0]["lm3d_std"].shape == (5, 3) and aligned[0]["lm3d_std"].dtype == np.float64
    with pytest.raises(KeyError):
        nf.load_face_recon({k: v for k, v in weights.items() if k != "backbone.bn1.running_var"})
    with pytest.raises(KeyError):
        nf.load_face_recon(dict(weights, extra=torch.zeros(1)))
    with pytest.raises(ValueError):
        nf.load_face_recon(dict(weights, **{"backbone.conv1.weight": torch.zeros(64, 3, 3, 3)}))
    bare = {k: v for k, v in weights.items() if not k.endswith("num_batches_tracked")}
    assert len(nf.load_face_recon({"net_recon": bare})[1]) == 7
    with pytest.raises(ValueError):
        nf.FaceRecon(weights, aligned[0]["lm3d_std"]).forward(torch.zeros(1, 3, 64, 64))  # no CPU path
    with pytest.raises(ValueError):
        nf.FaceRecon(weights, aligned[0]["lm3d_std"]).align(torch.zeros(1, 3, 64, 64))


def test_restatement_reproduces_the_reference(fixture, chains, weights):
    """every block's output (sum, abs-sum, every 331st element) and the coefficients, within 1e-12 of the largest value"""
    data, _ = fixture
    blocks = np.load(os.path.join(REPO, "tests", "golden", "face_recon_blocks.npz"))
    for case in fr.CASES:
        ins, skips, outs = chains[case] if case in chains else fr.chain(weights, fr.fixture_images(case))
        for b, act in enumerate(outs):
            s, sa, sample = fr.summary(act)
            want = data[case + "/block_sums"][b]
            scale = max(float(act.abs().max()), 1e-300)
            assert abs(s - want[0]) <= 1e-12 * max(want[1], 1.0) and abs(sa - want[1]) <= 1e-12 * max(want[1], 1.0), (case, b)
            assert np.abs(sample - blocks["%s/block%02d/sample" % (case, b)]).max() <= 1e-12 * scale, (case, b)
        want = data[case + "/coeffs"]
        assert np.abs(outs[-1].numpy() - want).max() <= 1e-12 * np.abs(want).max(), case


def test_byte_resample_against_the_installed_pil(aligned):
    """the restatement's two-pass bicubic against PIL run live, on noise, up- and downscales between 0.6 and 2.5 and crops over
    every border: at most 1e-3 of the bytes differ, none by more than one level"""
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(12)
    differing = total = 0
    for H, W, s, left, up in ((64, 64, 2.5, -20, 30), (96, 80, 0.6, -80, -90), (50, 70, 1.37, 10, -40), (64, 48, 0.93, -100, 5), (40, 40, 1.0, -90, -92)):
        u8 = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
        w, h = int(W * s), int(H * s)
        want = np.array(Image.fromarray(u8).resize((w, h), resample=Image.BICUBIC).crop((left, up, left + 224, up + 224))).astype(np.int64)
        got = fr.crop(u8.transpose(2, 0, 1) / 255.0, (w, h, left, up), True)
        got = np.floor(got.transpose(1, 2, 0) * 255.0 + 0.5).astype(np.int64)
        d = np.abs(got - want)
        assert d.max() <= 1, (H, W, s)
        differing, total = differing + int((d != 0).sum()), total + d.size
    print("%d of %d bytes differ from PIL's" % (differing, total))
    assert differing <= 1e-3 * total


def test_alignment_against_the_reference(aligned):
    """the POS pseudo-inverse against the reference's recorded t and s (its lstsq), the truncated integers, the byte crops against
    the recorded PIL crops, the fallback and the status frame"""
    data, m = aligned
    lm3d = data["lm3d_std"]
    differing = total = 0
    for case in fr.ALIGN_CASES:
        u8 = data[case + "/frames_u8"]
        assert np.array_equal(u8, fr.fixture_frames(case))
        lms = fr.fixture_landmarks(case, lm3d)
        for i, lm in enumerate(lms):
            stored = data[case + "/landmarks"][i][:int(data[case + "/points"][i])]
            assert stored.shape == lm.shape and np.array_equal(stored, lm, equal_nan=True)
        crops, trans, geom, status, args = fr.align(fr.frames_f32(u8).numpy(), lms, lm3d, True)
        assert np.array_equal(status, data[case + "/status"]) and np.array_equal(geom, data[case + "/geom"])
        ok = status == 0
        ref = data[case + "/trans_params"]
        assert (np.abs(trans[ok] - ref[ok]) / np.maximum(np.abs(ref[ok]), 1.0)).max() <= 1e-12
        assert not crops[~ok].any()
        got = np.floor(crops.transpose(0, 2, 3, 1) * 255.0 + 0.5).astype(np.int64)
        d = np.abs(got - data[case + "/crops_u8"].astype(np.int64))
        assert d.max() <= 1
        differing, total = differing + int((d != 0).sum()), total + d.size
    assert differing <= m["conditions"]["byte_cap"] * total
    # landmarks None: the fallback, the same as a frame of -1
    fb = fr.five_points(None, 96, 80, lm3d)
    assert np.array_equal(fb, fr.five_points(np.full((68, 2), -1.0), 96, 80, lm3d)) and np.array_equal(fb, (lm3d[:, :2] + 1) / 2 * np.array([80.0, 96.0]))


def test_fixture_conditions(fixture, aligned):
    _, m = fixture
    for case in fr.CASES:
        st = m["stats"][case]
        assert st["max_zero_share"] <= 0.6 == m["conditions"]["zero_share_cap"]
        assert 1e-2 <= st["min_abs_max"] and st["max_abs_max"] <= 1e3
        assert 0.0 < st["positive_share_of_coeffs"] < 1.0
    assert m["bounds"]["gpu_factor"] == 4.0 and len(m["bounds"]["block"]) == fr.N_BLOCKS and m["bounds"]["coeffs"] > 0
    data, a = aligned
    c = a["conditions"]
    assert c["truncation_margin"] == 1e-6 and c["nearest_truncation_argument"] > 1e-6
    assert 100.0 * c["t_s_relative_error_of_the_pseudo_inverse"] * 4096.0 <= 1e-6
    assert c["byte_cap"] == 1e-3 and c["bytes_differing_share"] <= 1e-3 and c["bytes_worst_levels"] <= 1
    assert c["fallback_on_integer"] == ["up"] and c["fallback_distance_to_integer"] <= 1e-10  # on the integer, not merely near it
    assert a["bounds"]["gpu_factor"] == 4.0 and a["bounds"]["expressions"] > 0 and 0 < a["bounds"]["unquantized"] < 2.0 / 255.0
    s = np.concatenate([data[k + "/trans_params"][data[k + "/status"] == 0, 2] for k in fr.ALIGN_CASES])
    g = np.concatenate([data[k + "/geom"][data[k + "/status"] == 0] for k in fr.ALIGN_CASES])
    assert s.min() < 1.0 < s.max()
    assert (g[:, 2] < 0).any() and (g[:, 3] < 0).any() and (g[:, 2] + 224 > g[:, 0]).any() and (g[:, 3] + 224 > g[:, 1]).any()
    pts = np.concatenate([data[k + "/points"] for k in fr.ALIGN_CASES])
    assert set(pts.tolist()) == {5, 68} and sum(int(data[k + "/status"].sum()) for k in fr.ALIGN_CASES) == 1


def test_emulation_stays_within_its_recorded_bounds(fixture, aligned, weights, chains):
    """the bounds in the manifests are the emulation's own error: measured again here for the smallest case, and the expressions
    end to end for one alignment case"""
    data, m = fixture
    ins, skips, outs = chains["c"]
    b = fr.measured_bounds(weights, fr.fixture_images("c"), ins, skips, outs)
    assert all(x <= y * (1 + 1e-6) + 1e-300 for x, y in zip(b["block"], m["bounds"]["block"]))
    assert b["coeffs"] <= m["bounds"]["coeffs"] * (1 + 1e-6)
    adata, am = aligned
    crops = fr.align(fr.frames_f32(adata["p/frames_u8"]).numpy(), fr.fixture_landmarks("p", adata["lm3d_std"]), adata["lm3d_std"], True)[0]
    emu = fr.chain(weights, torch.as_tensor(crops).float(), True)[2][-1].double().numpy()
    ok = adata["p/status"] == 0
    err = float(np.abs(emu[ok][:, 80:144] - adata["p/coeffs"][ok][:, 80:144]).max())
    assert err <= am["bounds"]["expressions"] * (1 + 1e-6)


def test_index_walk_on_the_host_under_sanitizers(tmp_path):
    """csrc/face_recon_core.h over the convolution kernel's grid, the stem's gather, the pool, the average, the head, the pack and
    the resample's tap ranges on the CPU: every block at the fixture shapes and at n = 1, 3 for 32 x 32, the smallest legal image
    (layer 4 on a 1 x 1 map).  A stand-alone program with its own main, built here with the host compiler under
    -fsanitize=address,undefined and run directly.  It counts the stores: every cell of every map once, halo included, none outside
    the carve; every load inside the map its block was handed and the convolution's own tap."""
    from n3dt import face_recon as nf
    found = _host_compiler(tmp_path)
    if found is None:
        pytest.skip("no host C++ compiler found (tried $CXX, g++, c++, clang++)")
    cxx, flags = found
    exe = tmp_path / "face_recon_core_host"
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off"] + flags +
                           [os.path.join(REPO, "tests", "face_recon_core_host.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    shapes = [fr.CASES[c] for c in fr.CASES] + [(1, 32, 32), (3, 32, 32)]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([str(exe)] + [str(v) for s in shapes for v in s], capture_output=True, text=True, env=env, timeout=900)
    assert run.returncode == 0 and not run.stderr.strip(), "sanitizer or program error:\n" + run.stderr
    rows = [[int(v) for v in line.split()] for line in run.stdout.strip().splitlines()]
    assert len(rows) == len(shapes) * fr.N_BLOCKS
    for k, (n, H, W) in enumerate(shapes):
        mine = rows[k * fr.N_BLOCKS:(k + 1) * fr.N_BLOCKS]
        assert sorted(r[3] for r in mine) == list(range(fr.N_BLOCKS))
        for r in mine:
            assert r[:3] == [n, H, W]
            cin, cout, ho, wo = nf.block_shape(r[3], r[4], r[5])
            assert r[6:9] == [ho, wo, cout] and r[9] >= n * ho * wo * cout and ho >= 1 and wo >= 1
        last = [r for r in mine if r[3] == 52][0]
        assert last[6:8] == [(H + 31) // 32, (W + 31) // 32]
        if (H, W) == (32, 32):
            assert last[6:8] == [1, 1]
    if not flags:
        pytest.skip("%s cannot link -fsanitize=address,undefined: the index walk was checked (it holds), the sanitizer claim was not" % cxx)
