"""Host side of the validation metrics (n3dt.eval_utils, n3dt_eval_metrics), no GPU: the two exports and their documented
refusals, the float64 restatement against the recorded fixtures and against known answers, and the kernels' per-tile arithmetic
(csrc/eval_metrics_core.h) walked over the tile grid on the CPU under the address and undefined-behaviour sanitizers."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import eval_restatement as er

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C1 = (0.01 * 255.0) ** 2
PSNR_IDENTICAL = 20.0 * math.log10(255.0 / 2.220446049250313e-16)


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("eval_metrics")


def test_new_symbols_are_declared_and_exported():
    from n3dt import _lib
    L = _lib.lib()
    header = open(os.path.join(REPO, "include", "n3dt.h")).read()
    declared = set(re.findall(r"\b(n3dt_eval_metrics[a-z0-9_]*)\s*\(", header))
    assert declared == {"n3dt_eval_metrics", "n3dt_eval_metrics_workspace_bytes"}
    for name in declared:
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert L.n3dt_abi_version() == 5


def test_workspace_query_names_the_limit_it_refuses():
    from n3dt import _lib
    L = _lib.lib()
    q = L.n3dt_eval_metrics_workspace_bytes
    assert q(1, 6, 32) == 0 and b">= 7" in L.n3dt_last_error()
    assert q(1, 32, 6) == 0 and b">= 7" in L.n3dt_last_error()
    assert q(0, 32, 32) == 0 and b"n_images" in L.n3dt_last_error()
    assert q(1, 1 << 16, 1 << 15) == 0 and b"2^31" in L.n3dt_last_error()
    assert q(1, (1 << 16) - 1, 1 << 15) > 0  # one row below the limit is a geometry the library takes
    # (3, 8, 13): one 32x32 tile per image, one (double, uint64) partial per tile
    assert q(3, 8, 13) == 3 * 16
    assert q(2, 37, 53) == 2 * 4 * 16 and q(1, 512, 512) == 256 * 16


def test_entry_point_refuses_null_pointers_and_a_short_workspace():
    """Validation is host code and runs before anything is enqueued."""
    from n3dt import _lib
    L = _lib.lib()
    d = ctypes.c_void_p(256)
    need = L.n3dt_eval_metrics_workspace_bytes(3, 8, 13)
    good = [3, 8, 13, d, d, d, d, d, need, None]
    for i in (3, 4, 5, 6, 7):
        args = list(good)
        args[i] = None
        assert L.n3dt_eval_metrics(*args) == -1 and b"NULL" in L.n3dt_last_error(), i
    args = list(good)
    args[8] = need - 1
    assert L.n3dt_eval_metrics(*args) == -1 and b"workspace too small" in L.n3dt_last_error()
    # ssim, psnr and the workspace are written as doubles: 8-byte aligned; pred and gt are read as floats: 4-byte aligned
    for i in (5, 6, 7):
        args = list(good)
        args[i] = ctypes.c_void_p(260)
        assert L.n3dt_eval_metrics(*args) == -1 and b"8-byte aligned" in L.n3dt_last_error(), i
    for i in (3, 4):
        args = list(good)
        args[i] = ctypes.c_void_p(258)
        assert L.n3dt_eval_metrics(*args) == -1 and b"4-byte aligned" in L.n3dt_last_error(), i
    for geom in ((0, 8, 13), (3, 6, 13), (3, 8, 6), (1, 1 << 16, 1 << 15)):
        assert L.n3dt_eval_metrics(*geom, d, d, d, d, d, 1 << 40, None) == -1


def test_cpu_tensors_raise():
    import torch
    from n3dt import calc_eval_metrics, image_metrics
    x = torch.rand(1, 3, 16, 16)
    with pytest.raises(ValueError, match="GPU"):
        image_metrics(x, x)
    with pytest.raises(ValueError, match="GPU"):
        calc_eval_metrics({"coarse_dict": {"merge_img": x}}, x, None)
    with pytest.raises(ValueError, match="display"):
        calc_eval_metrics({"coarse_dict": {"merge_img": x}}, x, None, vis=True)


def test_restatement_reproduces_every_fixture_value(fixture):
    data, manifest = fixture
    assert manifest["parity"] == "parity unpinned to the dependency"
    assert [(c["n"], c["height"], c["width"]) for c in manifest["cases"]].count((1, 7, 7)) == 3
    assert {(c["n"], c["height"], c["width"]) for c in manifest["cases"]} == {(1, 7, 7), (3, 8, 13), (2, 37, 53), (2, 32, 32), (1, 64, 64)}
    assert {k for c in manifest["cases"] for k in c["kinds"]} == {"uniform", "smooth", "flip"}
    for c in manifest["cases"]:
        pred, gt = data[c["name"] + "/pred"], data[c["name"] + "/gt"]
        assert pred.dtype == np.float32 and pred.shape == (c["n"], 3, c["height"], c["width"]) == gt.shape
        ssim, psnr = er.batch_metrics(pred, gt)
        assert np.abs(ssim - data[c["name"] + "/ssim"]).max() <= 1e-12, c["name"]
        assert np.abs(psnr - data[c["name"] + "/psnr"]).max() <= 1e-12, c["name"]


def test_known_answers():
    rng = np.random.default_rng(5)
    a = rng.random((3, 19, 23), dtype=np.float32)
    ssim, psnr = er.metrics(a, a)
    assert ssim == 1.0 and abs(psnr - PSNR_IDENTICAL) <= 1e-12 and abs(psnr - 361.2019987) < 1e-6
    zeros, ones = np.zeros((3, 64, 64), np.float32), np.ones((3, 64, 64), np.float32)
    ssim, psnr = er.metrics(zeros, ones)
    assert abs(ssim - C1 / (65025.0 + C1)) <= 1e-12 and abs(ssim - 9.9990001e-5) < 1e-12
    assert abs(psnr) <= 1e-12


def test_quantise_inverts_k_over_255_and_clamps():
    k = np.arange(256)
    assert np.array_equal(er.quantise((k / 255).astype(np.float32)), k)
    x = np.array([np.nan, -0.1, 1.3, -np.inf, np.inf, -0.0, 0.999999], np.float32)
    assert er.quantise(x).tolist() == [0, 0, 255, 0, 255, 0, 254]
    # grey: channel 0 carries OpenCV's B weight
    assert er.gray_bgr(np.array([[[255, 0, 0]], [[0, 255, 0]], [[0, 0, 255]], [[255, 255, 255]]], np.uint8)).ravel().tolist() == [29, 150, 76, 255]


SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _host_compiler(tmp_path):
    """(compiler, sanitizer flags) of a host C++ compiler, or None when there is none.  The flags are empty when the compiler
    cannot link the address and undefined-behaviour sanitizers.  Their runtimes are linked statically where the compiler can
    (gcc needs to be told, clang does so by default): a statically linked runtime does not care what else the process has
    loaded."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    found = [shutil.which(name) for name in (os.environ.get("CXX"), "g++", "c++", "clang++") if name]
    found = [cxx for cxx in found if cxx]
    for cxx in found:
        for extra in (["-static-libasan", "-static-libubsan"], []):
            if subprocess.run([cxx] + SANITIZE + extra + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode == 0:
                return cxx, SANITIZE + extra
    return (found[0], []) if found else None


def test_tile_walk_on_the_host_under_sanitizers(fixture, tmp_path):
    """csrc/eval_metrics_core.h -- the code the kernels are compiled from -- over the kernel's tile grid on the CPU: tiles cut on
    both edges with halos crossing tile boundaries (2 x 37 x 53) and images smaller than a tile (3 x 8 x 13).  Any read outside the
    images, the workspace or the tile memory ends the program through the sanitizer.  Where the compiler has no sanitizer
    runtimes the numbers are still checked, on an unsanitised build, and only the sanitizer claim is skipped."""
    found = _host_compiler(tmp_path)
    if found is None:
        pytest.skip("no host C++ compiler found (tried $CXX, g++, c++, clang++)")
    cxx, flags = found
    exe = tmp_path / "eval_core_host"
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off"] + flags +
                           [os.path.join(REPO, "tests", "eval_core_host.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    data, manifest = fixture
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    for name in ("cut_tiles", "below_a_tile"):
        pred, gt = data[name + "/pred"], data[name + "/gt"]
        n, _, H, W = pred.shape
        raw = tmp_path / (name + ".bin")
        with open(raw, "wb") as f:
            f.write(np.array([n, H, W], np.int32).tobytes())
            f.write(np.ascontiguousarray(pred).tobytes())
            f.write(np.ascontiguousarray(gt).tobytes())
        run = subprocess.run([str(exe), str(raw)], capture_output=True, text=True, env=env, timeout=120)
        assert run.returncode == 0 and not run.stderr.strip(), "sanitizer or program error:\n" + run.stderr
        rows = [line.split() for line in run.stdout.strip().splitlines()]
        assert [int(r[0]) for r in rows] == list(range(n))
        ssim, psnr = np.array([float(r[1]) for r in rows]), np.array([float(r[2]) for r in rows])
        print(name, "max |dSSIM| %.3e  max |dPSNR| %.3e" % (np.abs(ssim - data[name + "/ssim"]).max(), np.abs(psnr - data[name + "/psnr"]).max()))
        assert np.abs(ssim - data[name + "/ssim"]).max() <= 1e-9, name
        assert np.abs(psnr - data[name + "/psnr"]).max() <= 1e-9, name
    if not flags:
        pytest.skip("%s cannot link -fsanitize=address,undefined: the tile walk's numbers were checked (they hold), "
                    "the sanitizer claim was not" % cxx)
