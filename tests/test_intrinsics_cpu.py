"""Gradients to batch_inv_inmats and batch_xy, the parts that need no GPU: the new entry point's export and
argument checks, the fixture tests/golden/intrinsics.* and the intrinsics variables of n3dt.fitting.FittingState."""
import ctypes
import hashlib
import os
import re

import numpy as np
import torch

from conftest import GOLDEN, REPO, load_golden

CASES = ("tiny_test", "tiny_train", "vd_train")
CAM_INPUTS = ("batch_inv_inmats", "batch_xy", "batch_Rmats", "batch_Tvecs")


def test_render_bwd_cam_is_exported_with_the_declared_argtypes():
    """n3dt_render_bwd_cam = n3dt_render_bwd's 28 arguments with d_Kinv, d_xy behind d_T: the ctypes table, the header and the
    library agree, and the ABI version did not move (n3dt_render_bwd keeps its signature)."""
    from n3dt import _lib
    L = _lib.lib()
    assert "n3dt_render_bwd_cam" in _lib.EXPORTS and "n3dt_render_bwd" in _lib.EXPORTS
    old, new = L.n3dt_render_bwd.argtypes, L.n3dt_render_bwd_cam.argtypes
    assert len(old) == 28 and len(new) == 30
    assert list(new) == list(old[:25]) + [ctypes.c_void_p, ctypes.c_void_p] + list(old[25:])
    assert L.n3dt_render_bwd_cam.restype is ctypes.c_int
    assert L.n3dt_abi_version() == 5
    with open(os.path.join(REPO, "include", "n3dt.h")) as f:
        header = f.read()
    decl = re.search(r"\bint n3dt_render_bwd_cam\(([^;]*)\);", header).group(1)
    names = [a.split()[-1].lstrip("*") for a in decl.split(",")]
    assert len(names) == 30 and names[23:27] == ["d_R", "d_T", "d_Kinv", "d_xy"]
    decl_old = re.search(r"\bint n3dt_render_bwd\(([^;]*)\);", header).group(1)
    assert [a.split()[-1].lstrip("*") for a in decl_old.split(",")] == names[:25] + names[27:]


def test_render_bwd_cam_refuses_intrinsics_gradients_without_the_camera_inputs():
    """d_Kinv or d_xy without xy, R, T, Kinv: N3DT_EINVAL and a message naming the function, before any launch (no device
    here; the stand-in pointers are never dereferenced)."""
    from n3dt import _lib, ops
    L = _lib.lib()
    g = ops.make_geom(2, 64, 8, 384, 256, 179, 127, 64, 8, 2, 2.5, -3.5)
    P = ctypes.c_void_p(4096)
    mp = _lib.MlpParams()
    sv, ws = L.n3dt_render_train_saved_bytes(ctypes.byref(g)), L.n3dt_render_train_workspace_bytes(ctypes.byref(g))
    EINVAL, EWS = -1, -2

    def bwd(cam, d_R=None, d_T=None, d_Kinv=None, d_xy=None, sv_b=sv, p=mp):
        return L.n3dt_render_bwd_cam(ctypes.byref(g), _lib.F32, ctypes.byref(p) if p is not None else None, None, P, P, P, P, P, None, None,
                                     P, ctypes.c_size_t(sv_b), None, P, P, P, None, *cam, None, d_R, d_T, d_Kinv, d_xy, P,
                                     ctypes.c_size_t(ws), None)
    for miss in range(4):  # each of xy, R, T, Kinv missing in turn
        cam = [P] * 4
        cam[miss] = None
        for kw in ({"d_Kinv": P}, {"d_xy": P}, {"d_Kinv": P, "d_xy": P}, {"d_R": P, "d_Kinv": P}):
            assert bwd(cam, **kw) == EINVAL, (miss, kw)
            msg = L.n3dt_last_error()
            assert b"n3dt_render_bwd_cam" in msg and b"xy, R, T, Kinv" in msg, msg
    assert bwd([None] * 4, d_xy=P) == EINVAL and b"n3dt_render_bwd_cam" in L.n3dt_last_error()
    # the conventions of the entry point it extends
    assert bwd([P] * 4, d_Kinv=P, sv_b=sv - 1) == EWS and b"n3dt_render_bwd_cam: saved buffer too small" in L.n3dt_last_error()
    assert bwd([P] * 4, d_Kinv=P, p=None) == EINVAL and b"n3dt_render_bwd_cam" in L.n3dt_last_error()


def _sha256(arrays):
    digest = hashlib.sha256()
    for n in sorted(arrays.files):
        digest.update(n.encode())
        digest.update(np.ascontiguousarray(arrays[n]).tobytes())
    return digest.hexdigest()


def test_fixture_matches_its_manifest():
    data, m = load_golden("intrinsics")
    assert m["generator"] == "tools/gen_golden_intrinsics.py" and [c["name"] for c in m["cases"]] == list(CASES)
    assert _sha256(data) == m["arrays_sha256"]
    assert os.path.getsize(os.path.join(GOLDEN, "intrinsics.npz")) < 64 * 1024
    n_r = m["featmap_size"] ** 2
    for c in m["cases"]:
        B = c["batch"]
        shapes = {"batch_inv_inmats": (B, 3, 3), "batch_xy": (B, 2, n_r), "batch_Rmats": (B, 3, 3), "batch_Tvecs": (B, 3, 1)}
        for k in CAM_INPUTS:
            a = data["%s.grad_in.%s" % (c["name"], k)]
            assert a.dtype == np.float32 and a.shape == shapes[k] and np.isfinite(a).all() and np.abs(a).max() > 0, (c["name"], k)
        # the third row of d Kinv is a real gradient: the reference's autograd fills it
        assert np.abs(data[c["name"] + ".grad_in.batch_inv_inmats"][:, 2]).min() > 0
        # same case as the fixture it is named after: same weights, same loss
        _, m0 = load_golden(c["name"])
        assert np.allclose(c["weights_checksum"], m0["weights_checksum"], rtol=1e-12)
        assert c["t_rand_seed"] == m0["t_rand_seed"] and c["batch"] == m0["batch"] and c["mode"] == m0["mode"]


def test_fixture_camera_gradients_equal_the_existing_fixtures_to_float32_rounding():
    """d R and d T of the new fixture against the same entries of tiny_test / tiny_train / vd_train: <= 1e-6 of max|ref|.
    They hold only because the generator builds the very same cases; its cross-check entries come from a run made the way
    tools/gen_golden.py wrote those fixtures (float32, 8 threads), since no other run repeats a float32 one this closely (a
    float64 run differs by 0.3 - 2 % of the tensor's scale through ReLU gates near zero, one thread instead of eight by 2e-5)."""
    data, _ = load_golden("intrinsics")
    for name in CASES:
        old, _ = load_golden(name)
        for k in ("batch_Rmats", "batch_Tvecs"):
            a, b = data["%s.grad_in.%s" % (name, k)].astype(np.float64), old["grad_in." + k].astype(np.float64)
            assert a.shape == b.shape
            err = float(np.abs(a - b).max() / np.abs(b).max())
            print(name, k, "%.3e" % err)
            assert err <= 1e-6, (name, k, err)


def test_fixture_float64_run_is_the_same_case():
    """The float64 run that gives d Kinv and d xy is the case of the float32 run and of the existing fixture: the three loss
    terms of all three agree to float32 rounding of the forward (1e-6 absolute, the bound tests/test_gpu_train.py puts on them;
    the float32 run's to 1e-9)."""
    data, _ = load_golden("intrinsics")
    for name in CASES:
        old, _ = load_golden(name)
        assert np.abs(data[name + ".loss_terms_f32"] - old["loss_terms"]).max() <= 1e-9, name
        assert np.abs(data[name + ".loss_terms"] - old["loss_terms"]).max() <= 1e-6, name


def _cam_info(n=2):
    from n3dt import synthetic as syn
    return {"batch_Rmats": torch.diag(torch.tensor([1.0, -1.0, -1.0])).repeat(n, 1, 1), "batch_Tvecs": torch.tensor([[[0.0], [0.0], [12.0]]]).repeat(n, 1, 1),
            "batch_inv_inmats": syn.inv_intrinsics(16, n)}


def test_fitting_state_without_intrinsics_is_as_it_was():
    from n3dt import fitting
    cam = _cam_info()
    shape, appea = torch.zeros(2, 179), torch.zeros(2, 127)
    st = fitting.FittingState(shape, appea, cam, opt_cam=False)
    assert st.build_code_and_cam()[1] is cam and len(st.variables()) == 3
    st = fitting.FittingState(shape, appea, cam, opt_cam=False, opt_intrinsics=False)
    assert st.build_code_and_cam()[1] is cam and not hasattr(st, "delta_logf")
    st = fitting.FittingState(shape, appea, cam)  # opt_cam: a new dict of the same three entries, the intrinsics the base tensor itself
    c = st.build_code_and_cam()[1]
    assert sorted(c) == ["batch_Rmats", "batch_Tvecs", "batch_inv_inmats"] and c["batch_inv_inmats"] is cam["batch_inv_inmats"]
    assert torch.equal(c["batch_Rmats"], cam["batch_Rmats"]) and torch.equal(c["batch_Tvecs"], cam["batch_Tvecs"])
    assert len(st.variables()) == 5
    assert [g["lr"] for g in st.make_optimizer()[0].param_groups] == [0.015, 0.015, 0.01, 0.001, 0.001]


def test_fitting_state_rebuilds_the_intrinsics_differentiably():
    from n3dt import fitting
    cam = _cam_info()
    K0 = cam["batch_inv_inmats"]
    assert float(K0[0, 0, 2].abs()) > 0  # a principal point off the origin: c0 is exercised
    st = fitting.FittingState(torch.zeros(2, 179), torch.zeros(2, 127), cam, opt_cam=False, opt_intrinsics=True)
    assert st.delta_logf.shape == (2, 1) and st.delta_center.shape == (2, 2) and len(st.variables()) == 5
    c = st.build_code_and_cam()[1]
    assert c["batch_Rmats"] is cam["batch_Rmats"] and c["batch_Tvecs"] is cam["batch_Tvecs"]
    assert float((c["batch_inv_inmats"].detach() - K0).abs().max()) <= 1e-7  # zero deltas: the base matrix
    f0 = 1.0 / K0[:, 0, 0]
    c0 = -K0[:, :2, 2] * f0[:, None]
    with torch.no_grad():
        st.delta_logf.copy_(torch.tensor([[0.1], [-0.2]]))
        st.delta_center.copy_(torch.tensor([[0.5, -0.25], [0.0, 1.0]]))
    K = st.build_code_and_cam()[1]["batch_inv_inmats"]
    f, ctr = f0 * torch.exp(st.delta_logf[:, 0].detach()), c0 + st.delta_center.detach()
    want = torch.zeros(2, 3, 3)
    want[:, 0, 0] = want[:, 1, 1] = 1.0 / f
    want[:, 0, 2], want[:, 1, 2], want[:, 2, 2] = -ctr[:, 0] / f, -ctr[:, 1] / f, 1.0
    assert float((K.detach() - want).abs().max()) <= 1e-7
    assert torch.allclose(st.focal().detach(), f, rtol=1e-6)
    # gradient reaches both variables; d K[0,0] / d logf = -1/f
    K[:, 0, 0].sum().backward()
    assert torch.allclose(st.delta_logf.grad[:, 0], -1.0 / f, rtol=1e-5) and float(st.delta_center.grad.abs().max()) == 0.0
    st.delta_logf.grad = None
    st.build_code_and_cam()[1]["batch_inv_inmats"][:, :2, 2].sum().backward()
    assert torch.allclose(st.delta_center.grad, (-1.0 / f)[:, None].expand(2, 2), rtol=1e-5)
    opt, _ = st.make_optimizer()
    assert [g["lr"] for g in opt.param_groups] == [0.015, 0.015, 0.01, 0.001]
    assert [id(p) for p in opt.param_groups[-1]["params"]] == [id(st.delta_logf), id(st.delta_center)]
    both = fitting.FittingState(torch.zeros(2, 179), torch.zeros(2, 127), cam, opt_intrinsics=True)
    assert [g["lr"] for g in both.make_optimizer()[0].param_groups] == [0.015, 0.015, 0.01, 0.001, 0.001, 0.001] and len(both.variables()) == 7
