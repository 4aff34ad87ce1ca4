"""Host side of the AWing FAN landmark detector (n3dt.FAN, n3dt_fan_*), no GPU: the exports and their documented refusals, the
tables, state-dict keys and parameter counts against the fixture, the float64 restatement (tests/fan_restatement.py) against the
fixture recorded from the reference's own classes (tests/golden/fan*), its decode against the reference's calculate_points on every
decode case, the fixture's own conditions, the emulation against its recorded bounds, and the kernels' index arithmetic
(csrc/fan_core.h) walked over the kernels' grids on the CPU under the address and undefined-behaviour sanitizers."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import fan_restatement as fr
from test_eval_metrics_cpu import _host_compiler

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"n3dt_fan_packed_bytes", "n3dt_fan_pack", "n3dt_fan_max_images", "n3dt_fan_workspace_bytes", "n3dt_fan_fwd", "n3dt_fan_block_workspace_bytes",
       "n3dt_fan_block", "n3dt_fan_crops", "n3dt_fan_points", "n3dt_fan_tail"}
PARAMS = {1: (6333603, 336), 2: (12273414, 603), 4: (24153036, 1137)}  # measured on the reference's class, num_landmarks = 98

_WEIGHTS = {}


def weights(M, N=98):
    """the stand-in weights, once per module run"""
    from n3dt import synthetic as syn
    if (M, N) not in _WEIGHTS:
        _WEIGHTS[(M, N)] = syn.fan_state_dict(fr.WEIGHTS_SEED, M, N)
    return _WEIGHTS[(M, N)]


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("fan")


def ref_gates(data, case):
    M, N, n = fr.CASES[case]
    return [torch.as_tensor(np.unpackbits(data["%s/gates%d" % (case, s)])[:n * fr.CELLS].reshape(n, 64, 64)).bool() for s in range(M - 1)]


@pytest.fixture(scope="module")
def chains(fixture):
    """the float64 restatement of every case with the reference's gates forced, computed once: {case: (heat maps, record)}"""
    data, m = fixture
    out = {}
    for case, (M, N, n) in fr.CASES.items():
        sd = weights(M, N)
        checksum = float(sum(float(v.double().abs().sum()) for v in sd.values()))
        want = m["cases"][case]["weights_checksum"]
        assert m["weights_seed"] == fr.WEIGHTS_SEED and abs(checksum - want) <= 1e-9 * want, "the stand-in weights drifted from the fixture"
        rec = {}
        heats, _ = fr.forward(sd, fr.fixture_images(case), M, N, gates=ref_gates(data, case), record=rec)
        out[case] = (heats, rec)
    return out


def test_exports_abi_and_refusals():
    from n3dt import _lib
    import n3dt
    L = _lib.lib()
    assert NEW <= set(_lib.EXPORTS) and L.n3dt_abi_version() == 5
    assert hasattr(n3dt, "FAN") and hasattr(n3dt, "load_fan")
    assert ctypes.sizeof(_lib.FanParams) == 8 + 8 * (6 * 200 + 2)
    packed = L.n3dt_fan_packed_bytes(4, 98)
    assert packed % 256 == 0 and packed > 2 * 2 * 24_000_000  # hi + lo bf16 of 24 M weights
    assert L.n3dt_fan_packed_bytes(5, 98) == 0 and b"1..4" in L.n3dt_last_error()
    assert L.n3dt_fan_packed_bytes(4, 128) == 0 and b"1..127" in L.n3dt_last_error()
    assert L.n3dt_fan_workspace_bytes(4, 98, 0) == 0 and b"max_images" in L.n3dt_last_error()
    for M in (1, 4):
        cap = L.n3dt_fan_max_images(M, 98)
        assert 16 <= cap <= 1024 and 0 < L.n3dt_fan_workspace_bytes(M, 98, cap) <= 4 << 30
        assert cap == 1024 or L.n3dt_fan_workspace_bytes(M, 98, cap + 1) == 0
    assert L.n3dt_fan_block_workspace_bytes(82, 4, 98, 1, 8, 8) == 0 and b"no such block" in L.n3dt_last_error()
    assert L.n3dt_fan_block_workspace_bytes(6 + 19 + 17, 2, 98, 1, 8, 8) == 0  # the last stack has no bl
    assert L.n3dt_fan_block_workspace_bytes(0, 1, 98, 1, 64, 64) == 0 and b"CoordConv" in L.n3dt_last_error()
    assert L.n3dt_fan_block_workspace_bytes(4, 1, 98, 1, 7, 8) == 0 and b"even" in L.n3dt_last_error()
    assert L.n3dt_fan_block_workspace_bytes(1, 1, 98, 3, 12, 10) > 0
    # entry points refuse before anything is enqueued: no device is touched here
    d, big = ctypes.c_void_p(256), ctypes.c_size_t(1 << 40)
    assert L.n3dt_fan_fwd(2, 98, 0, 1, d, d, 1, d, d, d, ctypes.c_size_t(16), None) == -1 and b"workspace too small" in L.n3dt_last_error()
    assert L.n3dt_fan_fwd(2, 98, 0, 1, d, None, 1, d, d, d, big, None) == -1 and b"NULL" in L.n3dt_last_error()
    assert L.n3dt_fan_fwd(0, 98, 0, 1, d, d, 1, d, d, d, big, None) == -1
    assert L.n3dt_fan_block(5, 2, 98, 0, 1, 8, 8, d, d, None, None, d, d, big, None) == -1 and b"takes a skip" in L.n3dt_last_error()
    assert L.n3dt_fan_block(1, 2, 98, 0, 1, 8, 8, d, d, d, None, d, d, big, None) == -1 and b"takes no skip" in L.n3dt_last_error()
    assert L.n3dt_fan_block(25, 2, 98, 0, 1, 64, 64, d, d, None, None, d, d, big, None) == -1 and b"takes gates" in L.n3dt_last_error()
    assert L.n3dt_fan_block(6, 2, 98, 0, 1, 64, 64, d, d, None, d, d, d, big, None) == -1 and b"no gates" in L.n3dt_last_error()
    assert L.n3dt_fan_crops(0, 64, 64, d, d, d, None) == -1 and b"n outside" in L.n3dt_last_error()
    assert L.n3dt_fan_points(1, 98, d, 97 * 4096, d, d, None) == -1 and b"frame_stride" in L.n3dt_last_error()
    assert L.n3dt_fan_points(1, 128, d, 1 << 20, d, d, None) == -1
    assert L.n3dt_fan_tail(1, 98, 68, 64, 64, d, d, d, None, 1, d, d, None) == -1 and b"points_out" in L.n3dt_last_error()
    assert L.n3dt_fan_pack(None, d, None) == -1
    p = _lib.FanParams()
    p.num_modules, p.num_landmarks = 1, 98
    assert L.n3dt_fan_pack(ctypes.byref(p), d, None) == -1 and b"NULL parameter" in L.n3dt_last_error()


def test_tables_keys_and_parameter_counts(fixture):
    from n3dt import fan as nf
    data, m = fixture
    for M, (params, nkeys) in PARAMS.items():
        keys = nf.state_dict_keys(M, 98)
        assert len(keys) == nkeys
        assert sum(int(np.prod(v)) for k, v in keys.items() if not k.endswith(("running_mean", "running_var", "num_batches_tracked"))) == params
        table = nf.conv_table(M, 98)
        assert len(table) == 12 + 47 * M and sum(r is None for r in table) == 2
        assert len(nf.block_names(M)) == 6 + 19 * M - 2
        assert [nf.block_index(b, M) for b in nf.block_names(M)] == sorted(nf.block_index(b, M) for b in nf.block_names(M))
    for case, (M, N, n) in fr.CASES.items():
        c = m["cases"][case]
        keys = nf.state_dict_keys(M, N)
        recorded = [line.split(" ") for line in bytes(data[case + "/state_dict_keys"]).decode().split("\n")]  # the reference class's own, in its order
        recorded = [(k, tuple(int(d) for d in shape.split("x")) if shape else ()) for k, shape in recorded]
        assert len(recorded) == c["n_keys"] == PARAMS[M][1] and [k for k, _ in recorded] == list(keys) == list(weights(M, N))
        assert all(shape == keys[k] == tuple(weights(M, N)[k].shape) for k, shape in recorded)
        assert c["n_params"] == PARAMS[M][0]
    assert len(nf.MAP_98_TO_68) == 68 and nf.MAP_98_TO_68[16] == (32, 32) and nf.MAP_98_TO_68[18] == (34, 41) and nf.MAP_98_TO_68[25] == (45, 47)
    assert nf.MAP_98_TO_68[36:42] == tuple((i, i) for i in (60, 61, 63, 64, 65, 67)) and nf.MAP_98_TO_68[67] == (95, 95)
    c = nf.coords(64)
    assert torch.equal(c, fr.coords(64).float()) and float(c[0, 63, 0]) == 1.0 and float(c[0, 0, 63]) == -1.0 and float(c[1, 0, 63]) == 1.0  # xx: rows
    sd = weights(1)
    with pytest.raises(KeyError):
        nf.load_fan({k: v for k, v in sd.items() if k != "bn1.running_var"}, 1, 98)
    with pytest.raises(KeyError):
        nf.load_fan(dict(sd, extra=torch.zeros(1)), 1, 98)
    with pytest.raises(ValueError):
        nf.load_fan(dict(sd, **{"conv1.conv.weight": torch.zeros(64, 3, 7, 7)}), 1, 98)
    bare = {k: v for k, v in sd.items() if not k.endswith("num_batches_tracked")}
    assert len(nf.load_fan({"state_dict": bare}, 1, 98)) == len(bare)
    net = nf.FAN(sd, num_modules=1)
    with pytest.raises(ValueError):
        net.forward(torch.zeros(1, 3, 256, 256))  # no CPU path
    with pytest.raises(ValueError):
        net.points(torch.zeros(1, 98, 64, 64))
    with pytest.raises(ValueError):
        net.landmarks(torch.zeros(1, 3, 64, 64))
    with pytest.raises(ValueError):
        nf.FAN(sd, num_modules=5)
    with pytest.raises(ValueError):
        nf.FAN(sd, num_modules=1, map98to68=[(0, 98)])


def test_restatement_reproduces_the_reference(fixture, chains):
    """every stack's heat map of every case (sum, abs-sum, every 331st element) within 1e-12 of the largest value, and the
    ConvBlocks, the pool and the upsample-add alone on the small maps"""
    data, _ = fixture
    for case, (M, N, n) in fr.CASES.items():
        for s, h in enumerate(chains[case][0]):
            a, b, sample = fr.summary(h)
            want = data["%s/heat%d/sums" % (case, s)]
            assert abs(a - want[0]) <= 1e-12 * want[1] and abs(b - want[1]) <= 1e-12 * want[1], (case, s)
            assert np.abs(sample - data["%s/heat%d/sample" % (case, s)]).max() <= 1e-12 * float(h.abs().max()), (case, s)
    blocks = np.load(os.path.join(REPO, "tests", "golden", "fan_blocks.npz"))
    sd = weights(2)
    names = sorted({k.split("/")[0] for k in blocks.files} - {"avg_pool", "upsample_add"})
    assert len(names) == 3 + 2 * 13 + 2
    for name in names:
        cin = sd[name + ".bn1.weight"].shape[0]
        for shape in fr.BLOCK_SHAPES:
            y = fr.run_block(sd, name, fr.block_input(name, shape, cin))
            a, b, sample = fr.summary(y)
            key = "%s/%dx%dx%d" % ((name,) + shape)
            assert abs(a - blocks[key + "/sums"][0]) <= 1e-12 * blocks[key + "/sums"][1], key
            assert np.abs(sample - blocks[key + "/sample"]).max() <= 1e-12 * float(y.abs().max()), key
    x = fr.block_input("avg_pool", fr.POOL_SHAPE, 256)
    assert np.abs(fr.summary(fr.pool(x.double()))[2] - blocks["avg_pool/sample"]).max() <= 1e-12
    up = fr.block_input("upsample_add", (fr.POOL_SHAPE[0], 2 * fr.POOL_SHAPE[1], 2 * fr.POOL_SHAPE[2]), 256)
    assert np.abs(fr.summary(fr.upadd(x.double(), up.double()))[2] - blocks["upsample_add/sample"]).max() <= 1e-12


def test_decode_restatement_is_the_reference_exactly(fixture, chains):
    data, m = fixture
    assert sorted(m["decode"]) == sorted(fr.DECODE_CASES)
    for case in fr.DECODE_CASES:
        got = fr.decode(fr.decode_heatmaps(case))
        if m["decode"][case]["raises_index_error"]:
            assert got is None and case == "cell4095"
        else:
            assert np.array_equal(got, data["decode/" + case]), case
    assert fr.decode(fr.decode_heatmaps("cell0"))[0, 0] in (0.25, 0.5, 0.75)  # the wrap to cell 4095 of the same map
    for case, (M, N, n) in fr.CASES.items():  # the reference's own points of its fp32 last heat map
        h = chains[case][0][-1].float().numpy()
        for f in range(n):
            got = fr.decode(h[f, :N])
            assert got is not None and np.array_equal(got, data[case + "/points"][f]), (case, f)


def test_fixture_conditions(fixture):
    _, m = fixture
    c = m["conditions"]
    assert (c["zero_share_cap"], c["gate_cap"], c["landmark_cap"], c["gate_side_min"], c["min_rows"]) == (0.6, 1e-3, 0.05, 0.10, 16)
    assert "np_float" in m and "restated" in m["glue"]
    for case, (M, N, n) in fr.CASES.items():
        st = m["stats"][case]
        assert 1e-2 <= st["abs_max_min"] and st["abs_max_max"] <= 1e3 and st["max_zero_share"] <= 0.6
        assert st["argmax_rows"] >= 16 and st["interior_rows"] >= 14
        assert len(st["gate_set_share"]) == M - 1 and all(0.10 <= v <= 0.90 for v in st["gate_set_share"])
        assert st["restatement_rel_err"] <= 1e-12 and len(m["bounds"]["heat"][case]) == M and min(m["bounds"]["heat"][case]) > 0
    tot = m["stats"]["all"]
    assert tot["unstable_gate_cells"] <= 1e-3 * tot["gate_cells"] and tot["gate_cells"] == (3 + 3) * 4096
    assert tot["unstable_landmarks"] <= 0.05 * tot["landmarks"] and tot["landmarks"] == 98 * (2 + 6 + 4)
    assert m["bounds"]["gpu_factor"] == 4.0 == fr.GPU_FACTOR


def test_emulation_stays_within_its_recorded_bounds(fixture, chains):
    """the bounds in the manifest are the emulation's own error: measured again here for the one-stack case, block by block on the
    fp32-rounded reference inputs and end to end"""
    data, m = fixture
    M, N, n = fr.CASES["m1"]
    sd = weights(M, N)
    heats, rec = chains["m1"]
    for name, (xin, skip, gate, out) in rec.items():
        e = fr.run_block(sd, name, xin.float(), None if skip is None else skip.float(), gate, emulate=True)
        r = fr.run_block(sd, name, xin.float(), None if skip is None else skip.float(), gate)
        assert float((e - r).abs().max()) <= m["bounds"]["block"]["m1/" + name] * (1 + 1e-6) + 1e-300, name
    emu, _ = fr.forward(sd, fr.fixture_images("m1"), M, N, emulate=True)
    assert float((emu[0] - heats[0]).abs().max()) <= m["bounds"]["heat"]["m1"][0] * (1 + 1e-6)


def test_index_walk_on_the_host_under_sanitizers(tmp_path):
    """csrc/fan_core.h over the convolution kernel's grid, the stem's gather, the slice stores, the pools and upsample-adds, the
    pack and the decode's index rules on the CPU: the whole forward at (num_modules, n) = (1, 2), (2, 3), (4, 1) and the blocks
    alone at the test shapes.  A stand-alone program with its own main, built here with the host compiler under
    -fsanitize=address,undefined and run directly.  It counts the stores (every element of every slice once, none outside) and
    checks that every load lands on floats an earlier step of the plan wrote, inside the map the step was handed."""
    found = _host_compiler(tmp_path)
    if found is None:
        pytest.skip("no host C++ compiler found (tried $CXX, g++, c++, clang++)")
    cxx, flags = found
    exe = tmp_path / "fan_core_host"
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off"] + flags +
                           [os.path.join(REPO, "tests", "fan_core_host.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")

    def run(*args):
        r = subprocess.run([str(exe)] + [str(a) for a in args], capture_output=True, text=True, env=env, timeout=900)
        assert r.returncode == 0 and not r.stderr.strip(), "sanitizer or program error:\n" + r.stderr
        return [[int(v) for v in line.split()] for line in r.stdout.strip().splitlines()]

    for M, N, n in fr.CASES.values():
        rows = run("forward", M, N, n)
        convs = [r for r in rows if r[0] == 0]
        assert len(convs) == 12 + 47 * M - 2 and sorted(r[1] for r in convs) == sorted(j for j in range(12 + 47 * M) if (j - 12) % 47 < 45 or j < 12 + 47 * (M - 1))
        assert len([r for r in rows if r[0] == 1]) == 1 + 4 * M and len([r for r in rows if r[0] == 2]) == 4 * M
        last = [r for r in convs if r[1] == 12 + 47 * (M - 1) + 44][0]
        assert last[2:6] == [64, 64, 64, 64] and last[6] == n * 4096 * 112  # N + 1 = 99 padded to 112 stored channels
        assert convs[0][1:6] == [0, 256, 256, 128, 128] and convs[0][6] == n * 128 * 128 * 64
    for b in (1, 2, 3, 6 + 1, 6 + 14, 6 + 19 + 9):
        for n, H, W in fr.BLOCK_SHAPES:
            rows = run("block", b, 2, 98, n, H, W)
            assert len(rows) == (4 if b in (1, 3) else 3) and all(r[4:6] == [H, W] for r in rows)
    n, H, W = fr.POOL_SHAPE
    assert run("block", 4, 2, 98, n, H, W)[0][4:7] == [H // 2, W // 2, n * (H // 2) * (W // 2) * 256]
    assert run("block", 5, 2, 98, n, H, W)[0][4:7] == [2 * H, 2 * W, n * 4 * H * W * 256]
    for b in (6 + 15, 6 + 16, 6 + 17, 6 + 18):
        assert len(run("block", b, 2, 98, 3, 5, 7)) == 1
    if not flags:
        pytest.skip("%s cannot link -fsanitize=address,undefined: the index walk was checked (it holds), the sanitizer claim was not" % cxx)
