"""The 2-D renderer's training kernels (csrc/train_nr.hip, the save epilogue of neural_render_x16.inc / nr_fused_x16.inc,
nr_train16.h) pinned stage by stage against the float64 restatement of tests/nr_restatement.py -- see that module for the
restatement, the comparison rule (per entry, relative to S, the sum of |terms|), the storage points of the bf16 backwards and
the floors, all of which come from the CPU alone (test_nr_restatement_cpu.py).  Bounds are 4 x the floor of the case.

Through ops.neural_render_train_fwd / ops.neural_render_bwd with the parameter structs of NeuralRenderer._rparams_from, not
through the module.  x = 0.5 randn, cotangent = randn per pixel, seeds from nr.GPU_CASES.

  case (featmap side, channels, blocks, maps)
  (4, 256, 1, 1)   4 x 4 maps are all border.  M = 16 pixels: the 2-byte-gather dW kernel, the latency form of the block kernel.
  (4, 256, 3, 2)   M a multiple of 32: the LDS row-major dW route and its 8 XCD partials; block 2 is the 32 x 64 block
                   (launch_dw16_x<.., 0>); three levels of the RGB pyramid.
  (8, 256, 2, 3)   nb h h not a power of two.
  (5, 256, 2, 3)   the general n3dt_div path, odd side; bf16 is fused here too.
  (4, 256, 4, 1)   four blocks: the last is 32 -> 32, the channel clamp.
  (6, 64, 3, 2), (5, 32, 1, 1)   the library builds featmap_nc == 256 only: both are refused, which is what is asserted; the
                   restatement is pinned at them on the CPU.  With 256 channels every geometry takes the fused bf16 path, so the
                   layered bf16 backward (nr_bwd<nrt_bf16>) is out of reach of an in-process test.

Exact fp32 path: image, every saved activation, every gate outside the gate band (all of them where the band is empty), every
gradient entry.  Measured (largest error / S per family, and the bound it is held to, printed by the test) -- DESIGN 3.8.
bf16 path (fused): forward stages teacher-forced from `saved` with check_bf16 (+ the fused path's hid, which is not saved: the last
block's is still in the workspace after a forward, so block k's is read after a forward over the first k + 1 blocks, whose
saved maps are the same bits); backward teacher-forced on the stored activations and gates with store = bf16_rne."""
import ctypes
import functools
import os
import types

import numpy as np
import pytest
import torch

import nr_restatement as nr
import x16_stagewise as xs

pytestmark = pytest.mark.gpu

CASES = list(nr.GPU_CASES)
PROPERTY_CASE = (4, 256, 3, 2)


def dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def cpu(case):
    """the float64 reference of a case, computed once and shared"""
    P, x, d_img = nr.case_inputs(case, nr.GPU_CASES[case])
    f = nr.forward(x, P)
    return P, x, d_img, f


def planar(a):
    return np.ascontiguousarray(a.transpose(0, 3, 1, 2))


def call(case, precision, n_blocks=None, d_img=None, frozen=False, prefill=None, env=None, maps=None):
    """one forward + backward.  n_blocks: only the first blocks (forward only).  prefill: {name: array} the gradient tensors (and
    "d_featmap") start from.  env: an environment switch read per call.  maps: only the first `maps` feature maps."""
    from n3dt import _lib, ops
    from n3dt.headnerf import NeuralRenderer
    P, x, d_img0, _ = cpu(case)
    fs, C, n, nb = case
    nb = maps or nb
    k = n_blocks or n
    prec = {"fp32": _lib.F32, "bf16": _lib.BF16}[precision]
    names = P.names()
    flat = dict(zip(names, P.flat()))
    sub = nr.Params(**{f: getattr(P, f)[:k + 1 if f.startswith("rgb") else k] for f in nr.Params.FIELDS})
    names = sub.names()
    tensors = [torch.from_numpy(np.ascontiguousarray(flat[nm], dtype=np.float32)).to(dev()) for nm in names]
    shim = types.SimpleNamespace(n_blocks=k)
    rp = NeuralRenderer._rparams_from(shim, tensors)
    geom = ops.make_geom(nb, fs * fs, 1, 384, C, 1, 1, 0, fs, k, 0, 0)   # NeuralRenderer._geom
    xd = torch.from_numpy(x[:nb].astype(np.float32)).to(dev()).contiguous()
    old = {}
    for key, val in (env or {}).items():
        old[key] = os.environ.get(key)
        os.environ[key] = val
    try:
        img, saved = ops.neural_render_train_fwd(geom, nb, rp, xd, prec)
        torch.cuda.synchronize()
        out = {"img": img.cpu().numpy().transpose(0, 2, 3, 1), "saved": saved.cpu().numpy(), "names": names}
        if precision == "bf16":
            # hid of the LAST block [4][M][CO] at the start of the workspace (nr_train16.h:62-64, 86: Nr16Ws.hid = 0)
            h = fs << (k - 1)
            co = nr.nr_ch(C, k)
            wsbuf = ops.WORKSPACE.get("nr_train", 1, dev())
            raw = wsbuf[:2 * 4 * nb * h * h * co].cpu().numpy().view(np.uint16).reshape(2, 2, nb, h, h, co)
            out["hid_bits"] = np.ascontiguousarray(raw.transpose(2, 3, 0, 4, 1, 5)).reshape(nb, 2 * h, 2 * h, co)   # planes -> raster
        if n_blocks is not None:
            return out
        grads = [torch.zeros_like(t) if prefill is None else torch.from_numpy(np.ascontiguousarray(prefill[nm], dtype=np.float32)).to(dev())
                 for nm, t in zip(names, tensors)]
        rg = None if frozen else NeuralRenderer._rparams_from(shim, grads)
        dd = torch.from_numpy(planar((d_img0 if d_img is None else d_img)[:nb]).astype(np.float32)).to(dev())
        if prefill is None:
            d_feat = ops.neural_render_bwd(geom, nb, rp, rg, xd, dd, saved, prec)
        else:  # ops.neural_render_bwd with a pre-filled d_featmap (it allocates its own)
            d_feat = torch.from_numpy(np.ascontiguousarray(prefill["d_featmap"], dtype=np.float32)).to(dev())
            wbytes = ops.lib().n3dt_neural_render_train_workspace_bytes(ctypes.byref(geom), nb)
            ws = ops.WORKSPACE.get("nr_train", wbytes, dev())
            ops.check(ops.lib().n3dt_neural_render_bwd(ctypes.byref(geom), nb, prec, ctypes.byref(rp), ctypes.byref(rg), ops._ptr(xd), ops._ptr(dd),
                                                       ops._ptr(saved), saved.numel(), ops._ptr(d_feat), ops._ptr(ws), wbytes, ops._stream()),
                      "n3dt_neural_render_bwd")
        torch.cuda.synchronize()
        out["grads"] = {"d_featmap": d_feat.cpu().numpy().astype(np.float64)}
        if not frozen:
            out["grads"].update({nm: g.cpu().numpy().astype(np.float64) for nm, g in zip(names, grads)})
        return out
    finally:
        for key, val in old.items():
            if val is None:
                del os.environ[key]
            else:
                os.environ[key] = val


@functools.lru_cache(maxsize=None)
def run(case, precision):
    return call(case, precision)


def report(tag, maxima, bound):
    print("%-28s %s" % (tag, "  ".join("%s %.3g (bound %.3g)" % (k, maxima[k], bound[k]) for k in nr.FAMILIES if k in maxima)))


def exact_tape(case):
    """the float64 tape with the KERNEL's gates: equal to the restatement's outside the gate band (asserted), free inside it"""
    P, x, d_img, f = cpu(case)
    sm = nr.SavedMaps(run(case, "fp32")["saved"], case, "exact")
    tape = nr.tape_from_forward(f)
    for k in ("t1", "tv", "net"):
        for i in range(P.n):
            mine, theirs = getattr(tape, "g_" + k)[i], getattr(sm, k)[i] > 0
            differ = mine != theirs
            assert not np.any(differ & ~nr.gate_band(f, k, i)), "%s[%d]: %d gates outside the band differ" % (k, i, int((differ & ~nr.gate_band(f, k, i)).sum()))
            if case in nr.STRICT_GATE_CASES:
                assert not differ.any()
            getattr(tape, "g_" + k)[i] = theirs
    return sm, tape


@pytest.mark.parametrize("case", CASES, ids=str)
def test_exact_path_forward_matches_the_restatement(case):
    """image within 4 x the float32 floor of the image; t1, tv, bl, net of every block within 4 x NR_F32_STAGE_FLOOR of the
    stage's |b| + sum |w x| (bl: the blur of its input's magnitude); the saved image is the returned one; every gate sign outside
    the gate band equals the restatement's"""
    P, x, d_img, f = cpu(case)
    r = run(case, "fp32")
    sm, _ = exact_tape(case)
    err = float(np.abs(r["img"] - f["img"]).max())
    print(case, "image: largest error %.3g (bound %.3g)" % (err, nr.MARGIN * nr.NR_F32_IMAGE_FLOOR))
    assert err <= nr.MARGIN * nr.NR_F32_IMAGE_FLOOR
    assert np.array_equal(sm.img, r["img"].astype(np.float64))
    for i in range(P.n):
        bl_mag = nr.blur(nr.shuffle(f["tv_mag"][i] + nr.repeat4(np.abs(f["x"][i]))))
        for k, got, mag in (("t1", sm.t1[i], f["t1_mag"][i]), ("tv", sm.tv[i], f["tv_mag"][i]), ("bl", sm.bl[i], bl_mag), ("net", sm.net[i], f["net_mag"][i])):
            rel = float((np.abs(got - f[k][i]) / mag).max())
            print(case, "%s[%d]: largest error %.3g of the magnitude (bound %.3g)" % (k, i, rel, nr.MARGIN * nr.NR_F32_STAGE_FLOOR))
            assert rel <= nr.MARGIN * nr.NR_F32_STAGE_FLOOR, (k, i, rel)


@pytest.mark.parametrize("case", CASES, ids=str)
def test_exact_path_gradients_match_the_restatement_per_entry(case):
    """every entry of d_featmap and of every weight and bias gradient within 4 x NR_F32_FLOOR x S"""
    P, x, d_img, f = cpu(case)
    _, tape = exact_tape(case)
    want = nr.backward(d_img, P, tape)
    bound = nr.bound_of(nr.NR_F32_FLOOR[case])
    maxima, lines = nr.compare(run(case, "fp32")["grads"], want, nr.scale(d_img, P, tape), bound, tag="fp32 %s" % (case,))
    report("fp32 %s" % (case,), maxima, bound)
    assert not lines, "\n".join(lines)


@functools.lru_cache(maxsize=None)
def bf16_maps(case):
    """SavedMaps of the bf16 run; on the fused path with every block's hid (see the module docstring)"""
    P, x, d_img, f = cpu(case)
    r = run(case, "bf16")
    sm = nr.SavedMaps(r["saved"], case, "fused")
    for k in range(1, P.n + 1):
        rk = r if k == P.n else call(case, "bf16", n_blocks=k)
        if k < P.n:
            part = nr.SavedMaps(rk["saved"], (case[0], case[1], k, case[3]), "fused")
            for name in ("t1", "tv", "net"):
                for i in range(k):
                    assert np.array_equal(part.bits[name][i], sm.bits[name][i]), "the forward over %d blocks stores other bits in %s[%d]" % (k, name, i)
        sm.hid_bits[k - 1] = rk["hid_bits"]
        sm.hid[k - 1] = xs.bf16_to_f64(rk["hid_bits"])
    return sm


@pytest.mark.parametrize("case", CASES, ids=str)
def test_bf16_forward_stages_from_the_stored_maps(case):
    """check_bf16 (x16_stagewise, unchanged: U, the one-ulp rule, AMBIGUOUS_CAP, WIDE_CAP; the activation is the LeakyReLU) on every
    stage of the fused bf16 training forward, each recomputed in float64 from the stage's own stored input.  The image from the stored activation maps: the RGB
    pyramid is fp32 arithmetic on them, |img - img64| <= 0.25 (4 NR_F32_STAGE_FLOOR + 2^-18) sum |terms| + 4 NR_F32_IMAGE_FLOOR
    (0.25: the sigmoid's largest slope; 2^-18: the matrix-pipe blur kernel feeds feat_2_rgb's weights as hi + lo bf16 halves,
    nr_blur_mfma.inc:12-14, which leaves 2^-18 of each; the last term: expf and the fused kernel's v_rcp_f32, 1 ulp)."""
    P, x, d_img, f = cpu(case)
    sm = bf16_maps(case)
    tags = []
    for tag, z, mag, act, bits in nr.fused_stages(sm, x, P):
        st = nr.check_stage(bits, z, mag, act)
        xs.report("%s %s" % (case, tag), st)
        assert st["mismatches"] == 0 and st["max_ulp"] <= 1, (tag, st["mismatches"], st["max_ulp"], st["worst"])
        assert st["wide"] <= xs.WIDE_CAP * st["n"], (tag, st["wide"], st["n"])
        assert st["ambiguous"] <= xs.AMBIGUOUS_CAP * st["n"], (tag, st["ambiguous"], st["n"])
        tags.append(tag)
    assert len(tags) == 4 * P.n
    img64 = nr.image_from_nets(x, sm.net, P)
    terms = nr.image_from_nets(x, sm.net, P, absolute=True)
    tol = 0.25 * (nr.MARGIN * nr.NR_F32_STAGE_FLOOR + 2.0 ** -18) * terms + nr.MARGIN * nr.NR_F32_IMAGE_FLOOR
    got = run(case, "bf16")["img"].astype(np.float64)
    print(case, "image from the stored maps: largest error %.3g, largest error / tolerance %.3g" % (np.abs(got - img64).max(), (np.abs(got - img64) / tol).max()))
    assert np.all(np.abs(got - img64) <= tol)
    assert np.array_equal(sm.img, got)


def bf16_want(case, d_img=None, frozen=False):
    P, x, d_img0, f = cpu(case)
    d_img = d_img0 if d_img is None else d_img
    tape = bf16_maps(case).tape(x)
    want = nr.backward(d_img, P, tape, store=nr.bf16_rne, wq=nr.bf16_rne, path="fused", frozen=frozen)
    return want, nr.scale(d_img, P, tape, path="fused", frozen=frozen)


@pytest.mark.parametrize("case", CASES, ids=str)
def test_bf16_gradients_teacher_forced_on_the_stored_maps(case):
    """the fused bf16 backward against the float64 restatement run on the stored
    activations and gates with store = wq = bf16_rne: every entry within 4 x NR_BF16_FLOOR x S.  (4, 256, 3, 2): the 2-byte-gather
    dW kernels (N3DT_NR_DW_LDS=0, read per call) inside the same bound, and the same d_featmap bit for bit."""
    want, S = bf16_want(case)
    bound = nr.bound_of(nr.NR_BF16_FLOOR[case])
    got = run(case, "bf16")["grads"]
    maxima, lines = nr.compare(got, want, S, bound, tag="bf16 %s" % (case,))
    report("bf16 %s" % (case,), maxima, bound)
    assert not lines, "\n".join(lines)
    if case == PROPERTY_CASE:
        other = call(case, "bf16", env={"N3DT_NR_DW_LDS": "0"})["grads"]
        maxima, lines = nr.compare(other, want, S, bound, tag="bf16 gather dW %s" % (case,))
        report("bf16 gather dW %s" % (case,), maxima, bound)
        assert not lines, "\n".join(lines)
        assert np.array_equal(other["d_featmap"], got["d_featmap"])
        assert any(not np.array_equal(other[k], got[k]) for k in got if k.startswith("w")), "the switch did not change the dW route"


@pytest.mark.parametrize("case", nr.UNBUILT_CASES, ids=str)
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_other_channel_widths_are_refused(case, precision):
    """featmap_nc != 256 is not built: the size query says so, and nothing is launched"""
    from n3dt import _lib, ops
    fs, C, n, nb = case
    geom = ops.make_geom(nb, fs * fs, 1, 384, C, 1, 1, 0, fs, n, 0, 0)
    x = torch.zeros(nb, fs, fs, C, device=dev())
    with pytest.raises(_lib.N3dtError, match="only featmap_nc == 256 is built"):
        ops.neural_render_train_fwd(geom, nb, _lib.RenderParams(), x, {"fp32": _lib.F32, "bf16": _lib.BF16}[precision])


def want_for(precision, case, d_img=None, frozen=False):
    if precision == "bf16":
        return bf16_want(case, d_img=d_img, frozen=frozen)
    P, x, d_img0, f = cpu(case)
    d_img = d_img0 if d_img is None else d_img
    _, tape = exact_tape(case)
    return nr.backward(d_img, P, tape, frozen=frozen), nr.scale(d_img, P, tape, frozen=frozen)


def bound_for(precision, case):
    return nr.bound_of((nr.NR_BF16_FLOOR if precision == "bf16" else nr.NR_F32_FLOOR)[case])


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_gradients_accumulate_and_d_featmap_is_overwritten(precision):
    """pre-filled gradient tensors end as prefill + gradient within the bound; a pre-filled d_featmap is overwritten.  The prefill
    is +-S / 64 per entry: an fp32 addition to it rounds by 2^-24 S / 64, far below any bound."""
    case = PROPERTY_CASE
    want, S = want_for(precision, case)
    rng = np.random.RandomState(5)
    prefill = {k: (np.where(rng.rand(*v.shape) < 0.5, -1.0, 1.0) * S[k] / 64.0).astype(np.float32) for k, v in want.items()}
    got = call(case, precision, prefill=prefill)["grads"]
    moved = {k: got[k] - (0.0 if k == "d_featmap" else prefill[k].astype(np.float64)) for k in got}
    maxima, lines = nr.compare(moved, want, S, bound_for(precision, case), tag="prefilled " + precision)
    report("prefilled " + precision, maxima, bound_for(precision, case))
    assert not lines, "\n".join(lines)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_frozen_renderer_returns_the_same_d_featmap(precision):
    """rgrads = None: d_featmap within the bound, and no other output"""
    case = PROPERTY_CASE
    want, S = want_for(precision, case, frozen=True)
    got = call(case, precision, frozen=True)["grads"]
    assert list(got) == ["d_featmap"]
    maxima, lines = nr.compare(got, want, S, bound_for(precision, case), tag="frozen " + precision)
    report("frozen " + precision, maxima, bound_for(precision, case))
    assert not lines, "\n".join(lines)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_a_map_with_a_zero_cotangent_gets_a_zero_gradient(precision):
    """the second map's cotangent is all zero: its d_featmap is exactly 0, every gradient is within the bound of the restatement,
    and no parameter gradient differs beyond the bound from the same call without that map"""
    case = PROPERTY_CASE
    P, x, d_img, f = cpu(case)
    d0 = d_img.copy()
    d0[1] = 0.0
    want, S = want_for(precision, case, d_img=d0)
    got = call(case, precision, d_img=d0)["grads"]
    assert not np.any(got["d_featmap"][1])
    bound = bound_for(precision, case)
    maxima, lines = nr.compare(got, want, S, bound, tag="zero cotangent " + precision)
    report("zero cotangent " + precision, maxima, bound)
    assert not lines, "\n".join(lines)
    alone = call(case, precision, maps=1)["grads"]
    params = {k: v for k, v in got.items() if k != "d_featmap"}
    maxima, lines = nr.compare({k: alone[k] for k in params}, params, {k: S[k] for k in params}, bound, tag="without the map " + precision)
    report("without the map " + precision, maxima, bound)
    assert not lines, "\n".join(lines)
