"""The head-mask generator without a GPU: the restatement against tests/golden/head_mask*.{npz,json} (the reference's BiSeNet in
float64, tools/gen_golden_head_mask.py), the emulation against its own recorded bounds, the post-process pieces against
scipy.ndimage, the hue formula against the real-valued hue for all 2^24 colours, the state-dict keys, the callers' argument checks,
and csrc/head_mask_core.h's index arithmetic walked by a stand-alone host program under the address and undefined-behaviour
sanitizers."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import head_mask_restatement as hr
from test_eval_metrics_cpu import _host_compiler

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"n3dt_head_mask_packed_bytes", "n3dt_head_mask_pack", "n3dt_head_mask_max_images", "n3dt_head_mask_workspace_bytes", "n3dt_head_mask_fwd",
       "n3dt_head_mask_block_workspace_bytes", "n3dt_head_mask_block", "n3dt_head_mask_frames", "n3dt_head_mask_resize", "n3dt_head_mask_labels", "n3dt_head_mask_green",
       "n3dt_head_mask_postprocess_workspace_bytes", "n3dt_head_mask_postprocess"}


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("head_mask")


@pytest.fixture(scope="module")
def weights(fixture):
    from n3dt import synthetic as syn
    m = fixture[1]
    assert m["weights_seed"] == hr.WEIGHTS_SEED and m["n_classes"] == hr.N_CLASSES
    sd = syn.head_mask_state_dict(hr.WEIGHTS_SEED, hr.N_CLASSES)
    checksum = float(sum(float(v.double().abs().sum()) for v in sd.values()))
    assert abs(checksum - m["weights_checksum"]) <= 1e-9 * m["weights_checksum"], "the stand-in weights drifted from the fixture"
    return sd


@pytest.fixture(scope="module")
def chains(weights):
    """the float64 restatement of the small cases and of the 65-image case, computed once"""
    return {case: hr.chain(weights, hr.normalise(hr.fixture_frames(case)).double()) for case in ("a", "b", "c", "d")}


def test_exports_abi_and_refusals():
    from n3dt import _lib
    import n3dt
    L = _lib.lib()
    assert NEW <= set(_lib.EXPORTS) and L.n3dt_abi_version() == 5
    assert hasattr(n3dt, "HeadMask") and hasattr(n3dt, "load_head_mask")
    assert ctypes.sizeof(_lib.HeadMaskParams) == 8 + 8 * 5 * 36 + 8
    packed = L.n3dt_head_mask_packed_bytes()
    assert packed % 256 == 0 and packed > 2 * 2 * 12_000_000  # hi + lo bf16 of about 13 M convolution weights
    assert L.n3dt_head_mask_workspace_bytes(1, 31, 64) == 0 and b"32..4096" in L.n3dt_last_error()
    assert L.n3dt_head_mask_workspace_bytes(1, 64, 4097) == 0
    assert L.n3dt_head_mask_workspace_bytes(0, 64, 64) == 0 and b"max_images" in L.n3dt_last_error()
    assert L.n3dt_head_mask_max_images(16, 64) == 0
    for H, W in ((512, 512), (4096, 4096)):
        cap = L.n3dt_head_mask_max_images(H, W)
        assert 1 <= cap <= 1024
        assert 0 < L.n3dt_head_mask_workspace_bytes(cap, H, W) <= 4 << 30
        assert cap == 1024 or L.n3dt_head_mask_workspace_bytes(cap + 1, H, W) == 0
    assert L.n3dt_head_mask_max_images(32, 32) == 1024 and L.n3dt_head_mask_max_images(512, 512) >= 64
    assert L.n3dt_head_mask_block_workspace_bytes(37, 1, 8, 8, 8, 8) == 0 and b"0..36" in L.n3dt_last_error()
    assert L.n3dt_head_mask_block_workspace_bytes(3, 1, 8, 8, 4, 4) == 0 and b"24 and 25" in L.n3dt_last_error()
    assert L.n3dt_head_mask_block_workspace_bytes(24, 1, 5, 5, 3, 3) > 0
    assert L.n3dt_head_mask_block_workspace_bytes(24, 1, 3, 3, 5, 5) == 0
    # entry points refuse before anything is enqueued: no device is touched here
    d, big = ctypes.c_void_p(256), ctypes.c_size_t(1 << 40)
    assert L.n3dt_head_mask_fwd(1, 64, 64, 19, d, d, 4, 0, None, None, d, d, ctypes.c_size_t(16), None) == -1 and b"workspace too small" in L.n3dt_last_error()
    assert L.n3dt_head_mask_fwd(1, 64, 64, 19, d, d, 5, 0, None, None, d, d, big, None) == -1 and b"selected output" in L.n3dt_last_error()
    assert L.n3dt_head_mask_fwd(1, 64, 64, 33, d, d, 4, 0, None, None, d, d, big, None) == -1 and b"n_classes" in L.n3dt_last_error()
    assert L.n3dt_head_mask_fwd(1, 64, 64, 19, d, d, 0, 0, None, None, d, d, big, None) == -1 and b"outputs" in L.n3dt_last_error()
    assert L.n3dt_head_mask_fwd(1, 16, 64, 19, d, d, 4, 0, None, None, d, d, big, None) == -1
    assert L.n3dt_head_mask_block(2, 1, 8, 8, 8, 8, 19, d, d, None, None, None, d, d, big, None) == -1 and b"takes aux" in L.n3dt_last_error()
    assert L.n3dt_head_mask_block(1, 1, 8, 8, 8, 8, 19, d, d, d, None, None, d, d, big, None) == -1 and b"no aux" in L.n3dt_last_error()
    assert L.n3dt_head_mask_block(1, 1, 8, 8, 8, 8, 19, d, d, None, d, None, d, d, big, None) == -1 and b"take a scale" in L.n3dt_last_error()
    assert L.n3dt_head_mask_block(24, 1, 8, 8, 4, 4, 19, d, d, None, None, d, d, d, big, None) == -1 and b"needs a scale" in L.n3dt_last_error()
    assert L.n3dt_head_mask_labels(1, 0, 4, 4, 32, 32, d, d, None) == -1 and b"n_classes" in L.n3dt_last_error()
    assert L.n3dt_head_mask_labels(1, 19, 4, 4, 32, 5000, d, d, None) == -1
    assert L.n3dt_head_mask_green(0, 8, 8, d, 36, 70, d, None) == -1 and L.n3dt_head_mask_green(1, 8, 8, None, 36, 70, d, None) == -1
    assert L.n3dt_head_mask_frames(1, 8, 8, d, 0, None, d, None) == -1
    assert L.n3dt_head_mask_resize(1, 8, 8, 5, d, 16, 16, d, None) == -1 and b"channels" in L.n3dt_last_error()
    assert L.n3dt_head_mask_resize(1, 8, 0, 3, d, 16, 16, d, None) == -1
    assert L.n3dt_head_mask_postprocess_workspace_bytes(1, 0, 8) == 0
    need = L.n3dt_head_mask_postprocess_workspace_bytes(2, 512, 512)
    assert need >= 2 * 512 * 512 * 12
    assert L.n3dt_head_mask_postprocess(1, 8, 8, d, d, d, d, 65, 3, 1, 1, 3, 7, 36, 70, d, d, d, big, None) == -1 and b"element" in L.n3dt_last_error()
    assert L.n3dt_head_mask_postprocess(1, 8, 8, d, d, d, d, 3, 3, 3, 1, 3, 7, 36, 70, d, d, d, big, None) == -1 and b"anchor" in L.n3dt_last_error()
    assert L.n3dt_head_mask_postprocess(1, 8, 8, d, d, d, d, 3, 3, 1, 1, 3, 7, 36, 70, d, d, d, ctypes.c_size_t(16), None) == -1
    assert L.n3dt_head_mask_pack(None, d, None) == -1
    p = _lib.HeadMaskParams()
    p.n_classes, p.bn_eps = 19, 1e-5
    assert L.n3dt_head_mask_pack(ctypes.byref(p), d, None) == -1 and b"NULL parameter" in L.n3dt_last_error()
    p.n_classes = 40
    assert L.n3dt_head_mask_pack(ctypes.byref(p), d, None) == -1 and b"n_classes" in L.n3dt_last_error()


def test_tables_keys_and_callers_checks(fixture, weights):
    from n3dt import HeadMask, _lib, head_mask as nh
    _, m = fixture
    assert m["block_names"] == nh.block_names() and len(m["block_names"]) == _lib.HEAD_MASK_BLOCKS == hr.N_BLOCKS == 37
    assert [[k, list(v)] for k, v in nh.state_dict_keys(19).items()] == m["state_dict_keys"]
    assert list(weights.keys()) == [k for k, _ in m["state_dict_keys"]]
    assert sum(1 for c in nh.CONVS if c[7] == nh.SMALL) == 5 and sum(1 for c in nh.CONVS if c[7] != nh.SMALL) == 31
    # the 26 convolutions output 2 needs: the restatement's chain runs exactly those
    x = hr.normalise(hr.fixture_frames("b")).double()
    ran = [b for b, o in enumerate(hr.chain(weights, x, outputs=4)[1][:nh.N_CONVS]) if o is not None]
    assert len(ran) == 26 and set(ran) == set(range(20)) | {nh.AVG, nh.ARM32, nh.ARM32_ATT, nh.HEAD32, nh.OUT32, nh.OUT32 + 1}
    assert nh.feature_sizes(88, 72) == ((44, 36), (22, 18), (11, 9), (6, 5), (3, 3))
    assert nh.feature_sizes(42, 104)[0] == (21, 52) and nh.feature_sizes(42, 104)[4] == (2, 4) and nh.feature_sizes(32, 32)[4] == (1, 1)
    # load_head_mask is strict; num_batches_tracked may be absent
    nh.load_head_mask({k: v for k, v in weights.items() if not k.endswith("num_batches_tracked")})
    with pytest.raises(KeyError, match="unexpected"):
        nh.load_head_mask(dict(weights, extra=torch.zeros(1)))
    with pytest.raises(KeyError, match="no key"):
        nh.load_head_mask({k: v for k, v in weights.items() if k != "ffm.conv1.weight"})
    with pytest.raises(ValueError, match="shape"):
        nh.load_head_mask(dict(weights, **{"conv_out.conv_out.weight": torch.zeros(18, 256, 1, 1)}))
    with pytest.raises(ValueError):
        nh.load_head_mask(weights, n_classes=11)
    for bad in (dict(n_classes=0), dict(n_classes=33), dict(output=3), dict(size=16), dict(hue_range=(70, 36)), dict(erosion_iters=-1),
                dict(eye_element=np.ones((65, 3))), dict(lut=np.zeros(255, dtype=np.uint8))):
        with pytest.raises(ValueError):
            HeadMask(weights, **bad)
    net = HeadMask(weights)
    assert net.size == 512 and net.output == 2 and net.hue_range == (36, 70) and net.erosion_iters == 7 and net.anchor == (10, 10)
    with pytest.raises(ValueError, match="GPU tensor"):
        net.forward(torch.zeros(1, 3, 64, 64))
    with pytest.raises(ValueError, match="GPU tensor"):
        net.masks(torch.zeros(1, 64, 64, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="GPU tensor"):
        net.postprocess(torch.zeros(1, 64, 64, dtype=torch.uint8), torch.zeros(1, 64, 64, 3, dtype=torch.uint8))
    # the default element: 20 x 20, symmetric about its anchor's row and column, full in the middle rows
    el = nh.ellipse()
    assert el.shape == (20, 20) and el[10].all() and not el[0, :10].any() and el[0, 10] == 1 and np.array_equal(el[1:], el[1:][::-1])
    lut = nh.default_lut()
    assert lut[1:14].all() and lut[17] == 2 and lut.sum() == 15


def test_restatement_reproduces_the_reference(fixture, chains):
    """every block's output (sum, abs-sum, every 257th element) and the logit maps, within 1e-12 of the largest value; the labels of
    the reference outside its low-margin pixels"""
    data, m = fixture
    blocks = np.load(os.path.join(REPO, "tests", "golden", "head_mask_blocks.npz"))
    for case, (ins, outs) in chains.items():
        n, H, W = hr.CASES[case]
        if case in hr.BLOCK_CASES:
            for b, act in enumerate(outs):
                s, sa, sample = hr.summary(act)
                scale = max(float(act.abs().max()), 1e-300)
                assert abs(sa - data[case + "/block_sums"][b][1]) <= 1e-12 * sa and abs(s - data[case + "/block_sums"][b][0]) <= 1e-12 * sa
                assert float(np.abs(sample - blocks["%s/block%02d/sample" % (case, b)]).max()) <= 1e-12 * scale, (case, b)
        for o, blk in enumerate(hr.LOGIT_BLOCKS):
            key = "%s/logits%d/" % (case, o)
            scale = float(outs[blk].abs().max())
            if key + "full" in data.files:
                assert float(np.abs(outs[blk].numpy() - data[key + "full"]).max()) <= 1e-12 * scale
            else:
                assert float(np.abs(hr.summary(outs[blk])[2] - data[key + "sample"]).max()) <= 1e-12 * scale
        ref = hr.unpack_labels(data[case + "/labels_packed"], n * H * W).reshape(n, H, W)
        lab = hr.labels_from_logits(outs[hr.LOGIT_BLOCKS[2]].numpy(), H, W)
        direct = hr.upsample(outs[hr.LOGIT_BLOCKS[2]], H, W).numpy().argmax(1)
        skip = np.zeros(n * H * W, dtype=bool)
        skip[data[case + "/low_margin"]] = True
        assert not ((lab != ref).reshape(-1) & ~skip).any() and not ((direct != ref).reshape(-1) & ~skip).any()


def test_fixture_conditions(fixture):
    _, m = fixture
    c = m["conditions"]
    assert c["low_margin_threshold"] == 2 * m["bounds"]["gpu_factor"] * m["bounds"]["logits"][2] and m["bounds"]["gpu_factor"] == 4
    for case in hr.CASES:
        st = m["stats"][case]
        big = st["classes_with_1_percent"]
        assert st["low_margin_share"] <= c["low_margin_cap"] == 0.01
        assert len(big) >= 6 and (4 in big or 5 in big) and 17 in big and any(1 <= k <= 13 for k in big)
    for case in hr.BLOCK_CASES:
        st = m["stats"][case]
        assert st["max_zero_share"] <= 0.6 and st["min_abs_max"] >= 1e-2 and st["max_abs_max"] <= 1e3
    for name in ("head_mask.npz", "head_mask_blocks.npz"):
        assert os.path.getsize(os.path.join(REPO, "tests", "golden", name)) < (1 << 20)


def test_emulation_stays_within_its_recorded_bounds(fixture, weights, chains):
    """the bounds in the manifest are the emulation's own error: measured again here for two cases"""
    _, m = fixture
    for case in ("b", "c"):
        ins, outs = chains[case]
        got = hr.measured_bounds(weights, hr.normalise(hr.fixture_frames(case)).double(), ins, outs)
        for b in range(hr.N_BLOCKS):
            assert got["block"][b] <= m["bounds"]["block"][b] * 1.5 + 1e-12, (case, b)  # the fp32 sums' order is the BLAS's own
        for o in range(3):
            assert got["logits"][o] <= m["bounds"]["logits_per_case"][case][o] * 1.5 + 1e-9
            assert got["logits"][o] <= m["bounds"]["logits"][o] * 1.5


def test_post_process_pieces_against_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(17)
    for H, W, p in ((64, 64, 0.3), (96, 80, 0.25), (40, 70, 0.35)):
        mask = rng.random((H, W)) < p
        roots = hr.component_roots(mask)
        lab, count = ndimage.label(mask, structure=np.ones((3, 3)))
        assert count > 3
        for k in range(1, count + 1):
            idx = np.flatnonzero(lab.reshape(-1) == k)
            assert (roots.reshape(-1)[idx] == idx[0]).all()          # one root per component: its smallest raster index
        assert (roots[~mask] == -1).all()
        img = np.where(mask, rng.integers(1, 3, size=(H, W)), 0).astype(np.uint8)
        areas = ndimage.sum_labels(mask, lab, index=np.arange(1, count + 1))
        best = 1 + int(np.argmax(areas))                              # scipy numbers in raster order of first pixels: first = smallest root
        assert np.array_equal(hr.largest_component(img), np.where(lab == best, img, 0))
        # the erosion: the reference's float filter, one pass at a time
        kernel = np.array([[0, 0.25, 0], [0.25, -1.0, 0.25], [0, 0.25, 0]])
        t = np.where(img == 1, 2.0, np.where(img == 2, 1.0, 0.0))
        for _ in range(7):
            res = ndimage.correlate(t, kernel, mode="constant", cval=0.0)
            t[(img == 2) & (res < -0.01)] = 0.0
        want = t.astype(np.uint8)
        want = np.where(want == 1, 2, np.where(want == 2, 1, want)).astype(np.uint8)
        assert np.array_equal(hr.erode_hair(img, 7), want)
        assert not np.array_equal(hr.erode_hair(img, 7), img)
        # the dilation: the element reflected about its anchor is scipy's structure with its origin
        from n3dt.head_mask import ellipse
        eyes = (rng.random((H, W)) < 0.002)
        eyes[0, 0] = eyes[H - 1, W - 1] = True
        for el, anchor in ((ellipse(), (10, 10)), (ellipse(5, 7), (2, 3)), (np.array([[1, 1, 0], [0, 1, 0]], dtype=np.uint8), (1, 1))):
            got = hr.dilate(np.where(eyes, 255, 0).astype(np.uint8), el, anchor, 3)
            eh, ew = el.shape
            flipped = el[::-1, ::-1].astype(bool)
            origin = ((eh - 1 - anchor[0]) - eh // 2, (ew - 1 - anchor[1]) - ew // 2)
            want = ndimage.binary_dilation(eyes, structure=flipped, iterations=3, origin=origin)
            assert np.array_equal(got != 0, want), (el.shape, anchor)


def test_hue_is_within_one_level_of_the_real_hue_for_all_colours():
    c = np.arange(1 << 24, dtype=np.int64)
    b, g, r = c >> 16, (c >> 8) & 255, c & 255
    got = hr.hue(b, g, r)
    v, lo = np.maximum(np.maximum(b, g), r), np.minimum(np.minimum(b, g), r)
    d = (v - lo).astype(np.float64)
    with np.errstate(all="ignore"):
        deg = np.where(v == r, 60.0 * (g - b) / d, np.where(v == g, 120.0 + 60.0 * (b - r) / d, 240.0 + 60.0 * (r - g) / d))
    deg = np.where(d == 0, 0.0, np.where(deg < 0, deg + 360.0, deg))
    want = np.rint(deg / 2.0)
    diff = np.abs(got - want)
    diff = np.minimum(diff, 180 - diff)
    assert got.min() >= 0 and got.max() <= 180 and diff.max() <= 1
    # the reference's filter takes the true R as B: a saturated green is cleared, red and blue are not
    assert hr.green(np.array([[20, 200, 30]], dtype=np.uint8))[0] and not hr.green(np.array([[200, 30, 20]], dtype=np.uint8))[0]
    assert not hr.green(np.array([[30, 20, 200]], dtype=np.uint8))[0]


def test_byte_resize_is_torchs_half_pixel_bilinear():
    rng = np.random.default_rng(9)
    for (h, w), (H, W) in (((48, 72), (64, 64)), ((64, 64), (48, 72)), ((33, 35), (33, 35)), ((5, 7), (40, 3))):
        img = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        want = F.interpolate(torch.as_tensor(img).permute(2, 0, 1)[None].double(), (H, W), mode="bilinear", align_corners=False)[0].permute(1, 2, 0)
        got = hr.resize_bytes(img, H, W)
        assert np.abs(got.astype(np.float64) - want.numpy()).max() <= 0.5 + 1e-9
        if (h, w) == (H, W):
            assert np.array_equal(got, img)
    assert np.array_equal(hr.resize_bytes(img[:, :, 0], H, W), hr.resize_bytes(img, H, W)[:, :, 0])


def test_label_rule_is_the_argmax_of_the_upsampled_volume():
    g = torch.Generator().manual_seed(5)
    for (h, w), (H, W) in (((4, 5), (32, 37)), ((1, 1), (8, 8)), ((3, 3), (88, 72)), ((8, 8), (64, 64))):
        lg = torch.randn(2, 19, h, w, generator=g).float()
        up = F.interpolate(lg.double(), (H, W), mode="bilinear", align_corners=True)
        lab = hr.labels_from_logits(lg.numpy(), H, W)
        ok = hr.margins(up) > 1e-9
        assert np.array_equal(lab[ok], up.numpy().argmax(1)[ok]) and ok.mean() > 0.99
    tie = torch.zeros(1, 3, 2, 2)
    assert (hr.labels_from_logits(tie.numpy(), 5, 5) == 0).all()   # the first maximum wins


def test_index_walk_on_the_host_under_sanitizers(tmp_path):
    """csrc/head_mask_core.h over the convolution kernel's grid, the stem's gather, the pool, the small stage and the label rule's
    taps on the CPU, for every shape of the GPU tests and the smallest legal image: each output cell written once, no address
    outside its map, and the nearest rule equal to torch's own table for every (in, out) <= 64.  A stand-alone program with its own
    main, built here with the host compiler under -fsanitize=address,undefined and run directly."""
    found = _host_compiler(tmp_path)
    if found is None:
        pytest.skip("no host C++ compiler found (tried $CXX, g++, c++, clang++)")
    cxx, flags = found
    exe = tmp_path / "head_mask_core_host"
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off"] + flags +
                           [os.path.join(REPO, "tests", "head_mask_core_host.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    table = np.zeros((64, 64, 64), dtype=np.int32)
    for n_in in range(1, 65):
        src = torch.arange(float(n_in)).view(1, 1, n_in, 1)
        for n_out in range(1, 65):
            table[n_in - 1, n_out - 1, :n_out] = F.interpolate(src, (n_out, 1), mode="nearest").view(-1).to(torch.int32).numpy()
    path = tmp_path / "nearest.bin"
    table.tofile(str(path))
    shapes = [hr.CASES[c] for c in hr.CASES] + [(1, 32, 32), (3, 33, 47)]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([str(exe), "--nearest", str(path)] + [str(v) for s in shapes for v in s], capture_output=True, text=True, env=env, timeout=900)
    assert run.returncode == 0 and not run.stderr.strip(), "sanitizer or program error:\n" + run.stderr
    rows = [[int(v) for v in line.split()] for line in run.stdout.strip().splitlines()]
    assert len(rows) == len(shapes)
    for (n, H, W), (steps, convs, stores, loads) in zip(shapes, rows):
        assert convs == 31 + 24 and steps > 7 * 26 and stores > n * (H // 2) * (W // 2) * 64 and loads > stores
