"""Host side of LPIPS (n3dt.eval_utils.LPIPS, n3dt_lpips), no GPU: the exports and their documented refusals, the float64
restatement against its recorded fixtures, the reference's reshape quirk and what it is worth, the state-dict loader, and the
kernels' index arithmetic (csrc/lpips_core.h) walked over the kernels' grids on the CPU under the address and
undefined-behaviour sanitizers."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import lpips_restatement as lr
from test_eval_metrics_cpu import _host_compiler

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"n3dt_lpips_packed_bytes", "n3dt_lpips_pack", "n3dt_lpips_workspace_bytes", "n3dt_lpips"}


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("lpips")


@pytest.fixture(scope="module")
def weights():
    from n3dt import synthetic as syn
    return syn.lpips_alex_state_dict(lr.WEIGHTS_SEED)


def test_new_symbols_are_declared_and_exported():
    from n3dt import _lib
    L = _lib.lib()
    header = open(os.path.join(REPO, "include", "n3dt.h")).read()
    declared = set(re.findall(r"\b(n3dt_lpips[a-z0-9_]*)\s*\(", header))
    assert declared == NEW
    for name in declared:
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert L.n3dt_abi_version() == 5
    assert ctypes.sizeof(_lib.LpipsParams) == 15 * ctypes.sizeof(ctypes.c_void_p)


def test_size_queries_name_the_limit_they_refuse():
    from n3dt import _lib
    L = _lib.lib()
    q = L.n3dt_lpips_workspace_bytes
    assert q(1, 30, 64) == 0 and b">= 31" in L.n3dt_last_error()
    assert q(1, 64, 30) == 0 and b">= 31" in L.n3dt_last_error()
    assert q(1, 2049, 64) == 0 and b"<= 2048" in L.n3dt_last_error()
    assert q(0, 64, 64) == 0 and b"batch" in L.n3dt_last_error()
    assert q(65, 64, 64) == 0 and b"batch" in L.n3dt_last_error()
    assert q(64, 31, 31) > 0 and q(1, 2048, 2048) > 0
    # 31 x 31, one pair: in0 2*35*35*3, relu1 2*7*7*64, pool1 2*7*7*64, relu2 2*3*3*192, pool2 2*3*3*192, relu3 2*3*3*384,
    # relu4 2*3*3*256, relu5 2*256 floats, each rounded up to 64, then 5 * 128 doubles
    floats = [7350, 6272, 6272, 3456, 3456, 6912, 4608, 512]
    assert q(1, 31, 31) == sum((f + 63) // 64 * 64 for f in floats) * 4 + 5 * 128 * 8
    # the packed weights: hi + lo bf16 matrices with K padded to 16 (conv1: 363 -> 368), biases and lin weights in fp32
    mats = [368 * 64, 1600 * 192, 1728 * 384, 3456 * 256, 2304 * 256]
    assert L.n3dt_lpips_packed_bytes() == sum(m * 4 for m in mats) + 2 * sum(c * 4 for c in (64, 192, 384, 256, 256))


def test_entry_points_refuse_bad_arguments_before_anything_is_enqueued():
    from n3dt import _lib
    L = _lib.lib()
    d = ctypes.c_void_p(4096)
    need = L.n3dt_lpips_workspace_bytes(3, 35, 47)
    good = [3, 35, 47, 0, d, d, d, d, d, d, need, None]
    for i in (4, 5, 6, 7, 9):
        args = list(good)
        args[i] = None
        assert L.n3dt_lpips(*args) == -1 and b"NULL" in L.n3dt_last_error(), i
    args = list(good)
    args[10] = need - 1
    assert L.n3dt_lpips(*args) == -1 and b"workspace too small" in L.n3dt_last_error()
    for i, what in ((7, b"8-byte"), (8, b"8-byte"), (5, b"4-byte"), (6, b"4-byte"), (4, b"256-byte"), (9, b"256-byte")):
        args = list(good)
        args[i] = ctypes.c_void_p(4096 + 2)
        assert L.n3dt_lpips(*args) == -1 and what in L.n3dt_last_error(), i
    args = list(good)
    args[3] = 2
    assert L.n3dt_lpips(*args) == -1 and b"input_mode" in L.n3dt_last_error()
    for geom in ((0, 35, 47), (65, 35, 47), (3, 30, 47), (3, 35, 30), (3, 2049, 47)):
        assert L.n3dt_lpips(*geom, 0, d, d, d, d, d, d, 1 << 40, None) == -1
    p = _lib.LpipsParams()
    assert L.n3dt_lpips_pack(ctypes.byref(p), d, None) == -1 and b"NULL parameter" in L.n3dt_last_error()
    assert L.n3dt_lpips_pack(None, d, None) == -1 and L.n3dt_lpips_pack(ctypes.byref(p), None, None) == -1


def test_cpu_tensors_and_both_lpips_arguments_raise(weights):
    from n3dt import LPIPS, calc_eval_metrics, image_metrics, validate
    lp = LPIPS(weights)
    x = torch.rand(1, 3, 32, 32)
    with pytest.raises(ValueError, match="GPU"):
        lp(x, x)
    with pytest.raises(ValueError, match="GPU"):
        lp.layers(x, x)
    with pytest.raises(ValueError, match="GPU"):
        image_metrics(x, x, lpips=lp)
    with pytest.raises(ValueError, match="not both"):
        calc_eval_metrics({"coarse_dict": {"merge_img": x}}, x, None, lpips=lp, lpips_fn=lambda a, b: 0.0)
    with pytest.raises(ValueError, match="not both"):
        validate(None, [], lpips=lp, lpips_fn=lambda a, b: 0.0)
    with pytest.raises(ValueError, match="input_mode"):
        LPIPS(weights, input_mode="bgr")


def test_stand_in_weights_are_seeded_and_shaped_as_the_real_ones(weights):
    from n3dt import synthetic as syn
    again = syn.lpips_alex_state_dict(lr.WEIGHTS_SEED)
    assert sorted(weights) == sorted(again) and all(torch.equal(weights[k], again[k]) for k in weights)
    assert not torch.equal(weights["features.0.weight"], syn.lpips_alex_state_dict(lr.WEIGHTS_SEED + 1)["features.0.weight"])
    assert len(weights) == 15
    for layer, (idx, cin, cout, k, _, _) in enumerate(lr.CONVS):
        w, b, lin = weights["features.%d.weight" % idx], weights["features.%d.bias" % idx], weights["lin%d.model.1.weight" % layer]
        assert tuple(w.shape) == (cout, cin, k, k) and tuple(b.shape) == (cout,) and tuple(lin.shape) == (1, cout, 1, 1)
        assert abs(float(w.std()) / (2.0 / (cin * k * k)) ** 0.5 - 1.0) < 0.05  # He-normal
        assert float(b.abs().max()) <= 0.01 and float(lin.min()) >= 0.0 and float(lin.max()) > 1.0


def test_loader_accepts_both_key_forms_and_names_what_is_missing(weights):
    from n3dt.eval_utils import LPIPS, load_lpips_alex
    tv = load_lpips_alex(weights)
    own = {"scaling_layer.shift": torch.zeros(1, 3, 1, 1), "scaling_layer.scale": torch.ones(1, 3, 1, 1)}
    for layer, (idx, _, cout, _, _, _) in enumerate(lr.CONVS):
        for part in ("weight", "bias"):
            own["net.slice%d.%d.%s" % (layer + 1, idx, part)] = weights["features.%d.%s" % (idx, part)]
        own["lins.%d.model.1.weight" % layer] = weights["lin%d.model.1.weight" % layer]
    got = load_lpips_alex(own)
    assert len(tv) == len(got) == 5
    for a, b in zip(tv, got):
        assert all(torch.equal(s, t) for s, t in zip(a, b)) and a[2].dim() == 1
    assert len(LPIPS(own).weights) == 5
    for key in ("features.6.bias", "lin3.model.1.weight", "features.0.weight"):
        sd = {k: v for k, v in weights.items() if k != key}
        with pytest.raises(KeyError, match=re.escape(key)):
            LPIPS(sd)
    sd = dict(weights)
    sd["features.3.weight"] = torch.zeros(192, 64, 3, 3)
    with pytest.raises(ValueError, match=r"features\.3\.weight"):
        LPIPS(sd)
    sd = dict(weights)
    sd["lin4.model.1.weight"] = torch.zeros(1, 384, 1, 1)
    with pytest.raises(ValueError, match=r"lin4\.model\.1\.weight"):
        LPIPS(sd)
    with pytest.raises(TypeError):
        LPIPS([1, 2, 3])


def test_restatement_reproduces_every_fixture_value(fixture, weights):
    data, manifest = fixture
    assert manifest["parity"] == "parity unpinned to the dependency"
    assert manifest["weights_seed"] == lr.WEIGHTS_SEED and manifest["pair_seed"] == lr.PAIR_SEED
    checksum = float(sum(float(v.double().abs().sum()) for v in weights.values()))
    assert abs(checksum - manifest["weights_checksum"]) <= 1e-9 * checksum, "the seeded weight generator drifted from the fixture"
    cases = lr.SMALL_CASES + lr.BIG_CASES
    assert [(c["name"], c["height"], c["width"], c["n"]) for c in manifest["cases"]] == list(cases)
    for idx, (name, h, w, n) in enumerate(cases):
        pred, gt = lr.case_images_u8(idx, h, w, n)
        stored = idx < len(lr.SMALL_CASES)
        if stored:  # the images are in the fixture, and the generator still makes them
            assert np.array_equal(pred, data[name + "/pred_u8"]) and np.array_equal(gt, data[name + "/gt_u8"]), name
        for mode in ("reference", "standard") if stored else ("reference",):
            score, layers = lr.lpips_batch(lr.to_float(pred), lr.to_float(gt), weights, mode)
            want_s, want_l = data["%s/%s/score" % (name, mode)], data["%s/%s/layers" % (name, mode)]
            assert want_l.shape == (5, n) and want_s.shape == (n,)
            assert np.abs(score / want_s - 1.0).max() <= 1e-12 and np.abs(layers / want_l - 1.0).max() <= 1e-12, (name, mode)
            # the pairs are genuinely different: every layer contributes, none of them alone
            assert want_l.min() > 5e-3 and (want_l.max(axis=0) < want_s).all() and want_s.min() > 0.2, (name, mode)


def test_the_reshape_quirk_is_worth_far_more_than_any_tolerance(fixture, weights):
    """compute_LPIPS reshapes the HWC bytes to [1,3,H,W]; a proper permute gives another number by 5 % or more (printed), three
    orders of magnitude above the GPU test's relative bound, so matching the reference form pins the quirk."""
    import test_gpu_lpips as gpu
    data, _ = fixture
    for idx, (name, h, w, _) in enumerate(lr.SMALL_CASES + lr.BIG_CASES[:1]):
        pred, gt = (lr.to_float(t[0]) for t in lr.case_images_u8(idx, h, w, 1))
        ref = lr.lpips_pair(pred, gt, weights, "reference")[0]
        perm = lr.lpips_pair(pred, gt, weights, "permuted")[0]
        assert abs(ref / data[name + "/reference/score"][0] - 1.0) <= 1e-12
        print("%s: reshape %.6f, permute %.6f, relative difference %.3f" % (name, ref, perm, abs(perm - ref) / ref))
        assert abs(perm - ref) / ref >= 0.05 >= 1000 * gpu.SCORE_TOL, name


def test_reinterpretation_is_a_reshape_of_the_hwc_bytes():
    img = np.arange(3 * 5 * 7, dtype=np.float32).reshape(3, 5, 7) / np.float32(255.0)
    x = lr.reference_input(img).numpy()[0]
    flat = (np.arange(3 * 5 * 7).reshape(3, 5, 7)).transpose(1, 2, 0).ravel()  # the HWC bytes
    assert np.array_equal(x.ravel(), flat.astype(np.float32))
    assert x[0, 0, :6].tolist() == [0.0, 35.0, 70.0, 1.0, 36.0, 71.0]  # R, G, B of pixel 0, then of pixel 1, along one "row"
    assert np.array_equal(lr.permuted_input(img).numpy()[0], np.arange(105, dtype=np.float32).reshape(3, 5, 7))


def _window(lo, hi, extent):
    return max(lo, 0), min(hi, extent - 1)


def test_a_single_pixel_moves_only_its_receptive_windows(weights):
    """One changed input value at (c, y, x): relu1 moves only where an 11x11 / stride 4 / pad 2 field holds it, relu2 only inside
    that window through the 3 / 2 pool and the 5x5 / pad 2 convolution -- in standard mode at (y, x) itself, in reference mode
    at the place the reshape sends the byte to."""
    h, w = 67, 61
    convs, _ = lr.split_weights(weights)
    a = lr.to_float(lr.case_images_u8(3, h, w, 1)[0][0])
    c, y, x = 1, 40, 23
    b = a.copy()
    b[c, y, x] = np.float32(1.0) - b[c, y, x]
    f = (y * w + x) * 3 + c  # the byte's place in the HWC buffer
    spots = {"standard": (y, x), "reference": ((f % (h * w)) // w, f % w)}
    assert spots["reference"] != spots["standard"]
    for mode, (sy, sx) in spots.items():
        xin = lr.scaling(torch.cat([lr.INPUTS[mode](a), lr.INPUTS[mode](b)]))
        changed = (xin[0] != xin[1]).nonzero()
        assert len(changed) == 1 and changed[0, 1:].tolist() == [sy, sx], mode
        with torch.no_grad():
            feats = lr.features(xin, convs)
        h1, w1 = feats[0].shape[2:]
        # relu1 (oy, ox) reads rows 4 oy - 2 .. 4 oy + 8
        y1, x1 = _window(-(-(sy - 8) // 4), (sy + 2) // 4, h1), _window(-(-(sx - 8) // 4), (sx + 2) // 4, w1)
        # pool1 (py) reads relu1 rows 2 py .. 2 py + 2; conv2 reaches 2 further on either side
        h2, w2 = feats[1].shape[2:]
        y2 = _window(-(-(y1[0] - 2) // 2) - 2, y1[1] // 2 + 2, h2)
        x2 = _window(-(-(x1[0] - 2) // 2) - 2, x1[1] // 2 + 2, w2)
        for feat, (ya, yb), (xa, xb) in ((feats[0], y1, x1), (feats[1], y2, x2)):
            moved = (feat[0] != feat[1]).any(dim=0)
            assert moved.any()
            outside = moved.clone()
            outside[ya:yb + 1, xa:xb + 1] = False
            assert not outside.any(), mode
            assert moved[ya:yb + 1, xa:xb + 1].float().mean() > 0.5, mode  # and the window is not wider than what moves


def test_test_bounds_are_four_times_the_measured_floor():
    """tests/test_gpu_lpips.py writes its two bounds as constants; they are 4 x the floors tools/lpips_band.py measured
    (profiles/lpips_band.json), rounded to three digits."""
    import test_gpu_lpips as gpu
    with open(os.path.join(REPO, "profiles", "lpips_band.json")) as f:
        band = json.load(f)
    assert band["weights_seed"] == lr.WEIGHTS_SEED and band["pair_seed"] == lr.PAIR_SEED
    assert {(r["case"], r["input_mode"]) for r in band["rows"]} == (
        {(c[0], m) for c in lr.SMALL_CASES for m in ("reference", "standard")} | {(c[0], "reference") for c in lr.BIG_CASES})
    for part, tol in (("score", gpu.SCORE_TOL), ("layers", gpu.LAYER_TOL)):
        floor = max(band["worst"]["float32_" + part], band["worst"]["split_" + part])
        assert floor == band["floor"][part]
        assert abs(tol / (4.0 * floor) - 1.0) < 5e-3, part


# the GPU test's shapes: every small size at B = 1 and 3, and the two real geometries at B = 1
SHAPES = tuple((b, h, w) for _, h, w, _ in lr.SMALL_CASES for b in (1, 3)) + tuple((n, h, w) for _, h, w, n in lr.BIG_CASES)


def test_index_walk_on_the_host_under_sanitizers(tmp_path):
    """csrc/lpips_core.h -- the functions the convolution, pool and halo kernels and the prologue's gather take their addresses
    from -- over those kernels' full grids on the CPU, for every shape and batch size of the GPU test: the smallest legal input
    (every late map 1x1, M < 64), non-square sizes whose conv1 and pool floors drop rows, B = 1 and 3, and 256^2 and 512^2.  The
    program re-types the kernels' loop nests (its header says so) but takes the epilogue's row map, the pack kernel's decode and
    the MFMA step's weight address from csrc/conv_frag.h as the kernels do, and walks the pack of every layer: every (k, n) packed
    once, the decode the inverse of the address read, the rows k >= K zero.  The prologue's output decode and the distance
    kernel are not walked.  A read outside a buffer ends the program through the sanitizer; a read of the wrong
    element fails the program's own check.  Where the compiler has no sanitizer runtimes the indices are still checked, on an
    unsanitised build, and only the sanitizer claim is skipped."""
    found = _host_compiler(tmp_path)
    if found is None:
        pytest.skip("no host C++ compiler found (tried $CXX, g++, c++, clang++)")
    cxx, flags = found
    exe = tmp_path / "lpips_core_host"
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off"] + flags +
                           [os.path.join(REPO, "tests", "lpips_core_host.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([str(exe)] + [str(v) for s in SHAPES for v in s], capture_output=True, text=True, env=env, timeout=120)
    assert run.returncode == 0 and not run.stderr.strip(), "sanitizer or program error:\n" + run.stderr
    rows = [[int(v) for v in line.split()] for line in run.stdout.strip().splitlines()]
    assert [tuple(r[:3]) for r in rows] == list(SHAPES)
    for r in rows:  # the extents are torch's own
        x = torch.zeros(1, 3, r[1], r[2])
        convs = [(torch.zeros(c[2], c[1], c[3], c[3]), torch.zeros(c[2])) for c in lr.CONVS]
        assert [v for f in lr.features(x, convs, torch.float32) for v in f.shape[2:]] == r[3:13]
        assert r[13] > 100000
    assert rows[0][3:13] == [7, 7, 3, 3, 1, 1, 1, 1, 1, 1] and rows[-1][:5] == [1, 512, 512, 127, 127]
    assert lr.features(torch.zeros(1, 3, 512, 512), convs, torch.float32)[0].shape[2:] == (127, 127)
    if not flags:
        pytest.skip("%s cannot link -fsanitize=address,undefined: the index walk was checked (it holds), the sanitizer claim was not" % cxx)
