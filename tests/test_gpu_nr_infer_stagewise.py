"""The 16-bit INFERENCE renderer (run_x16 in csrc/neural_render_x16.inc, the block kernels of nr_fused_x16.inc / nr_fused_lat_x16.inc,
the blur kernels of nr_blur_mfma.inc and blur_act_rgb_q_kernel) pinned stage by stage, forward only, in both map types (bf16 and
IEEE half), against the float64 restatement of tests/nr_restatement.py -- see its last section for the workspace layout, what a call
leaves there, the rules and the floors, all of which come from the CPU alone (test_nr_restatement_cpu.py).

Through ops.neural_render_fwd / ops.neural_render_fwd16 with a caller-owned, pre-filled `ws` and the parameter structs of
NeuralRenderer._rparams_from.  A call over the first k blocks leaves block k - 1's hid, its stored input, the fp32 plane its
level read and the image: every case runs k = 1 .. n and block k - 1 is pinned from the k-block run.

  case (featmap side, channels, blocks, maps)        x = 0.5 randn, seeds from nr.INFER_CASES
  every entry of nr.GPU_CASES   the latency form of the block kernel; 4 x 4 borders, sides 5 (odd: blur_act_rgb_q_kernel) and 8;
                   (4, 256, 4, 1) ends in the 32 -> 32 block and blur_mfma_last_kernel at H = 32
  (64, 256, 1, 5)  M = 20 480: nr_level_x16_kernel at C = 256, fp32 input; the last level has K = 128: blur_mfma_q_kernel<., false>;
                   also fed as a 16-bit map with feat_to_rgb0's rgb0 (the 16-bit-input instantiation at C = 256)
  (48, 256, 3, 2)  M = 4 608 (latency form), 18 432, 73 728: nr_level_x16_kernel at C = 128 and 64 on 16-bit input;
                   blur_mfma_last_kernel at H = 192; blur_mfma_q_kernel<., true> at K = 128 and 64
  (65, 256, 1, 4)  M = 16 900 = 528 x 32 + 4: a ragged last tile and a partial workgroup; odd side

Not observable, hence not pinned alone: t1 and y of the inference kernels (registers only; held through the chain rule of hid, and
in bf16 through equal bits with the training forward, whose SAVE epilogue stores them), and the last level's net (never stored; its
rounding enters the image bound as a slack term)."""
import functools
import os
import types

import numpy as np
import pytest
import torch

import nr_restatement as nr
import x16_stagewise as xs

pytestmark = pytest.mark.gpu

CASES = list(nr.INFER_CASES)
PATTERN = 0x5A


def dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def inputs(case):
    P, x, _ = nr.case_inputs(case, nr.INFER_CASES[case])
    return P, x


def rparams(case, k):
    from n3dt.headnerf import NeuralRenderer
    P, _ = inputs(case)
    flat = dict(zip(P.names(), P.flat()))
    sub = nr.Params(**{f: getattr(P, f)[:k + 1 if f.startswith("rgb") else k] for f in nr.Params.FIELDS})
    tensors = [torch.from_numpy(np.ascontiguousarray(flat[nm], dtype=np.float32)).to(dev()) for nm in sub.names()]
    return NeuralRenderer._rparams_from(types.SimpleNamespace(n_blocks=k), tensors), tensors


def geom_of(case, k):
    from n3dt import ops
    fs, C, _, nb = case
    return ops.make_geom(nb, fs * fs, 1, 384, C, 1, 1, 0, fs, k, 0, 0)   # NeuralRenderer._geom


def to16(t, fmt):
    """fp32 -> the 16-bit map (round to nearest even), as the bit patterns"""
    return t.to(torch.bfloat16 if fmt == "bf16" else torch.float16).contiguous()


def render(case, fmt, k, x=None, in16=False, env=None):
    """one inference call over the first k blocks into a pre-filled workspace; returns img [nb, P, P, 3], the decoded workspace
    (nr.InferWs) and the number of workspace bytes outside the regions the call writes that lost the pattern"""
    from n3dt import _lib, ops
    P, x0 = inputs(case)
    fs, C, n, nb = case
    ck = (fs, C, k, nb)
    geom = geom_of(case, k)
    rp, keep = rparams(case, k)
    prec = {"bf16": _lib.BF16, "fp16": _lib.F16}[fmt]
    L = nr.infer_ws_layout(ck)
    wbytes = ops.neural_render_workspace_bytes(geom, nb)
    assert wbytes == L["total"], "the restated carve and n3dt_neural_render_workspace_bytes disagree: %d / %d" % (L["total"], wbytes)
    assert L["end"] <= L["packw"], "the 16-bit carve runs into the packed weights"
    ws = torch.full((wbytes,), PATTERN, dtype=torch.uint8, device=dev())
    xd = torch.from_numpy(np.ascontiguousarray(x0 if x is None else x, dtype=np.float32)).to(dev())
    old = {}
    for key, val in (env or {}).items():
        old[key] = os.environ.get(key)
        os.environ[key] = val
    try:
        rgb0 = None
        if in16:
            rgb0 = ops.feat_to_rgb0(xd.reshape(nb, fs * fs, C), keep[0], keep[1])
            ops.neural_render_pack(geom, nb, rp, prec, ws)
            img = ops.neural_render_fwd16(geom, nb, rp, to16(xd, fmt), rgb0, prec, ws=ws)
        else:
            img = ops.neural_render_fwd(geom, nb, rp, xd, prec, ws=ws)
        torch.cuda.synchronize()
    finally:
        for key, val in old.items():
            if val is None:
                del os.environ[key]
            else:
                os.environ[key] = val
    # bytes outside what the call is known to write keep the pattern (compared on the device: the workspace is up to 300 MB)
    written = sorted(nr.infer_written(ck, in16))
    lost, o = 0, 0
    for off, size in written + [(wbytes, 0)]:
        assert off >= o, "the written regions overlap"
        if off > o:
            lost += int((ws[o:off] != PATTERN).sum().item())
        o = off + size
    # read back only what is decoded: everything from hid to the end of the planes
    host = np.full(L["end"], PATTERN, dtype=np.uint8)
    host[L["hid"]:L["end"]] = ws[L["hid"]:L["end"]].cpu().numpy()
    out = {"img": img.cpu().numpy().transpose(0, 2, 3, 1).astype(np.float64), "lost": lost,
           "ws": nr.InferWs(host, ck, None if rgb0 is None else rgb0.cpu().numpy())}
    if rgb0 is not None:
        out["rgb0"] = rgb0.cpu().numpy()
    return out


@functools.lru_cache(maxsize=None)
def run(case, fmt, k):
    return render(case, fmt, k)


def block_input(case, fmt, k):
    """the stored input of block k - 1 as float64: the caller's map for k = 1, net[k - 2] of the k-block run otherwise"""
    return inputs(case)[1] if k == 1 else xs.bits16_to_f64(run(case, fmt, k)["ws"].net_bits, fmt)


def hid_of(case, fmt, k):
    return xs.bits16_to_f64(run(case, fmt, k)["ws"].hid_bits, fmt)


def level_form(case, k, env=None):
    fs, C, n, nb = case
    h = fs << (k - 1)
    return nr.blur_form(nb, h, h, nr.nr_ch(C, k), env)


@pytest.mark.parametrize("fmt", nr.FORMATS16)
@pytest.mark.parametrize("case", CASES, ids=str)
def test_workspace_layout_and_untouched_bytes(case, fmt):
    """the restated carve plus the packed tail is exactly n3dt_neural_render_workspace_bytes (asserted in every call), and no byte
    outside the regions a call writes (nr.infer_written) loses the pre-filled pattern, for every k"""
    for k in range(1, case[2] + 1):
        r = run(case, fmt, k)
        print(case, fmt, "k = %d: bytes outside the written regions that changed: %d" % (k, r["lost"]))
        assert r["lost"] == 0


@pytest.mark.parametrize("case", CASES, ids=str)
def test_rgb0_per_entry(case):
    """rgb0 as to_rgb16_kernel leaves it in the workspace after the one-block call (either map type: the kernel has none), and as
    n3dt_feat_to_rgb0 returns it on the same input: per entry within MARGIN x NR_X16_RGB0_FLOOR x (|b| + sum |w x|), and the same bits"""
    from n3dt import ops
    P, x = inputs(case)
    fs, C, n, nb = case
    want, S = nr.rgb0_stage(x, P)
    bound = nr.MARGIN * nr.NR_X16_RGB0_FLOOR * S
    got = {fmt: run(case, fmt, 1)["ws"].lo for fmt in nr.FORMATS16}
    _, keep = rparams(case, 1)
    xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev())
    alone = ops.feat_to_rgb0(xd.reshape(nb, fs * fs, C), keep[0], keep[1]).cpu().numpy()
    got["feat_to_rgb0"] = alone.reshape(nb, 3, fs, fs).transpose(0, 2, 3, 1).astype(np.float64)
    for tag, g in got.items():
        worst, at = nr.worst_ratio(g, want, bound)
        print(case, tag, "rgb0: largest error %.3g of S (bound %.3g), largest error / bound %.3g at %s" %
              (float((np.abs(g - want) / S).max()), nr.MARGIN * nr.NR_X16_RGB0_FLOOR, worst, at))
        assert worst <= 1.0, (tag, worst, at)
    assert np.array_equal(got["bf16"], got["fp16"]) and np.array_equal(got["bf16"], got["feat_to_rgb0"])


@pytest.mark.parametrize("fmt", nr.FORMATS16)
@pytest.mark.parametrize("case", CASES, ids=str)
def test_hid_from_the_blocks_stored_input(case, fmt):
    """hid[k - 1] of the k-block run under the chain rule (nr.x16_hid_chain): inside [rne16(z - delta_hid), rne16(z + delta_hid)], at most
    one ulp from rne16(z) wherever that interval is not wide; the median of delta_hid / magnitude over the stage <= HID_MEDIAN_CAP"""
    P, _ = inputs(case)
    for k in range(1, P.n + 1):
        st = nr.x16_check_hid(run(case, fmt, k)["ws"].hid_bits, block_input(case, fmt, k), P, k - 1, fmt)
        xs.report("%s %s hid[%d]" % (case, fmt, k - 1), st)
        print("    delta_hid / magnitude: median %.3g, maximum %.3g" % (st["median"], st["max"]))
        assert st["mismatches"] == 0 and st["max_ulp"] <= 1, (k, st["mismatches"], st["max_ulp"], st["worst"])
        assert st["median"] <= nr.HID_MEDIAN_CAP, (k, st["median"])


@pytest.mark.parametrize("fmt", nr.FORMATS16)
@pytest.mark.parametrize("case", [c for c in CASES if c[2] >= 2], ids=str)
def test_net_from_the_stored_hid(case, fmt):
    """net[i] (stored by the (i + 2)-block run) from hid[i] (read after the (i + 1)-block run) under the one-stage bit rule with the
    caps of the format.  First: whatever of block i's input both runs leave observable -- the stored input map for i >= 1, the fp32
    plane level i read -- has equal bits in the two runs."""
    P, _ = inputs(case)
    amb_cap, wide_cap = xs.CAPS[fmt]
    for i in range(P.n - 1):
        a, b = run(case, fmt, i + 1)["ws"], run(case, fmt, i + 2)["ws"]
        assert np.array_equal(a.lo, b.lo_prev), "the plane level %d read differs between the %d- and the %d-block run" % (i, i + 1, i + 2)
        if i >= 1:
            assert np.array_equal(a.net_bits, b.net_prev_bits), "net[%d] differs between the %d- and the %d-block run" % (i - 1, i + 1, i + 2)
        st = nr.x16_check_net(b.net_bits, xs.bits16_to_f64(a.hid_bits, fmt), P, i, fmt)
        xs.report("%s %s net[%d]" % (case, fmt, i), st)
        assert st["mismatches"] == 0 and st["max_ulp"] <= 1, (i, st["mismatches"], st["max_ulp"], st["worst"])
        assert st["wide"] <= wide_cap * st["n"] and st["ambiguous"] <= amb_cap * st["n"], (i, st["wide"], st["ambiguous"], st["n"])


def check_image(tag, r, hid, lo, P, i, fmt, form):
    pre, S, slack = nr.x16_rgb_stage(hid, None, lo, P, i, fmt, form)
    _, bound = nr.x16_rgb_bounds(pre, S, slack)
    worst, at = nr.worst_ratio(r["img"], nr.sigmoid(pre), bound)
    print("%s img (%s form): largest error %.3g, largest error / bound %.3g at %s" % (tag, form, float(np.abs(r["img"] - nr.sigmoid(pre)).max()), worst, at))
    return worst, at


@pytest.mark.parametrize("fmt", nr.FORMATS16)
@pytest.mark.parametrize("case", CASES, ids=str)
def test_pyramid_plane_and_image_from_the_stored_hid(case, fmt):
    """img of every k-block run from hid[k - 1], the plane level k - 1 read, feat_b and to_rgb_k (the last level's net is not stored:
    its rounding slack is part of the bound); the plane a non-last level wrote (read back as the next level's `lo` after the
    (k + 1)-block run) from the STORED net[k - 1] of that run, so without a slack: MARGIN x NR_X16_RGB_FLOOR x S"""
    P, _ = inputs(case)
    for k in range(1, P.n + 1):
        r = run(case, fmt, k)
        form = level_form(case, k)
        worst, at = check_image("%s %s k = %d" % (case, fmt, k), r, hid_of(case, fmt, k), r["ws"].lo, P, k - 1, fmt, form)
        assert worst <= 1.0, (k, worst, at)
        if k < P.n:
            nxt = run(case, fmt, k + 1)["ws"]
            assert np.array_equal(nxt.lo_prev, r["ws"].lo)
            pre, S, _ = nr.x16_rgb_stage(None, xs.bits16_to_f64(nxt.net_bits, fmt), r["ws"].lo, P, k - 1, fmt, form)
            bound, _ = nr.x16_rgb_bounds(pre, S, 0.0)
            worst, at = nr.worst_ratio(nxt.lo, pre, bound)
            print("%s %s plane written by level %d: largest error %.3g of S (bound %.3g) at %s" %
                  (case, fmt, k - 1, float((np.abs(nxt.lo - pre) / S).max()), nr.MARGIN * nr.NR_X16_RGB_FLOOR, at))
            assert worst <= 1.0, (k, worst, at)


@pytest.mark.parametrize("fmt", nr.FORMATS16)
@pytest.mark.parametrize("case", nr.FORM_CASES, ids=str)
def test_all_three_last_level_forms_from_the_same_hid(case, fmt):
    """the last level (K = 32) as blur_mfma_last_kernel, as blur_mfma_q_kernel<., false> (N3DT_NR_BLUR_TILE8=0) and as
    blur_act_rgb_q_kernel (N3DT_NR_BLUR_MFMA=0): every image inside the img rule from the hid and the plane its own call stored.
    N3DT_NR_BLUR_TILE8 touches the last level alone, so that call stores the bits of the default one; N3DT_NR_BLUR_MFMA=0 moves every
    level to the per-output kernel (the switches are per call, not per level), so its plane, and through net[n - 2] its hid, may
    differ in roundings and are judged on their own."""
    P, _ = inputs(case)
    n = P.n
    base = run(case, fmt, n)
    imgs = [base["img"]]
    for env in ({"N3DT_NR_BLUR_TILE8": "0"}, {"N3DT_NR_BLUR_MFMA": "0"}):
        r = render(case, fmt, n, env=env)
        assert r["lost"] == 0
        if "N3DT_NR_BLUR_TILE8" in env:
            assert np.array_equal(r["ws"].hid_bits, base["ws"].hid_bits) and np.array_equal(r["ws"].lo, base["ws"].lo)
        hid = xs.bits16_to_f64(r["ws"].hid_bits, fmt)
        worst, at = check_image("%s %s %s" % (case, fmt, env), r, hid, r["ws"].lo, P, n - 1, fmt, level_form(case, n, env))
        assert worst <= 1.0, (env, worst, at)
        imgs.append(r["img"])
    assert not np.array_equal(imgs[0], imgs[2]), "N3DT_NR_BLUR_MFMA=0 did not change the form"


@pytest.mark.parametrize("fmt", nr.FORMATS16)
def test_the_16_bit_input_form_gives_the_bits_of_the_fp32_input_form(fmt):
    """(64, 256, 1, 5) fed as rne16(x) with feat_to_rgb0's rgb0 through neural_render_fwd16 (the 16-bit-input instantiation of the
    throughput kernel at C = 256): hid and img have the bits of the fp32-input call -- on an x that is representable already (what the
    header promises), and on the case's own x, which the fp32-input kernel rounds the same way; nothing outside the written regions
    changes, and the caller's rgb0 is within the rgb0 rule"""
    case = nr.IN16_CASE
    P, x = inputs(case)
    xr = xs.round16(x, fmt)
    for tag, xv, ref in (("representable x", xr, render(case, fmt, 1, x=xr)), ("the case's x", x, run(case, fmt, 1))):
        got = render(case, fmt, 1, x=xv, in16=True)
        assert got["lost"] == 0
        assert np.array_equal(got["ws"].hid_bits, ref["ws"].hid_bits), tag
        assert np.array_equal(got["img"], ref["img"]), tag
        assert np.array_equal(got["ws"].lo, ref["ws"].lo), tag
        want, S = nr.rgb0_stage(xv, P)
        worst, at = nr.worst_ratio(got["ws"].lo, want, nr.MARGIN * nr.NR_X16_RGB0_FLOOR * S)
        print(fmt, tag, "rgb0: largest error / bound %.3g" % worst)
        assert worst <= 1.0


# ---------------------------------------------------------------------------------------------
# bf16: the training forward is the same block kernels with SAVE
# ---------------------------------------------------------------------------------------------
def train_forward(case, k):
    """the training forward over the first k blocks: SavedMaps with hid[k - 1] from the training workspace (nr_train16.h:62-64, 86)"""
    from n3dt import _lib, ops
    P, x = inputs(case)
    fs, C, n, nb = case
    rp, keep = rparams(case, k)
    xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev())
    img, saved = ops.neural_render_train_fwd(geom_of(case, k), nb, rp, xd, _lib.BF16)
    torch.cuda.synchronize()
    sm = nr.SavedMaps(saved.cpu().numpy(), (fs, C, k, nb), "fused")
    h, co = fs << (k - 1), nr.nr_ch(C, k)
    raw = ops.WORKSPACE.get("nr_train", 1, dev())[:2 * 4 * nb * h * h * co].cpu().numpy().view(np.uint16).reshape(2, 2, nb, h, h, co)
    sm.hid_bits[k - 1] = np.ascontiguousarray(raw.transpose(2, 3, 0, 4, 1, 5)).reshape(nb, 2 * h, 2 * h, co)
    sm.hid[k - 1] = xs.bf16_to_f64(sm.hid_bits[k - 1])
    return sm, img.cpu().numpy().transpose(0, 2, 3, 1).astype(np.float64)


@pytest.mark.parametrize("case", CASES, ids=str)
def test_bf16_inference_has_the_bits_of_the_training_forward(case):
    """k-block inference call against the k-block training forward: hid[k - 1] and every intermediate net map the inference call
    stores are equal bit for bit (SAVE only adds stores; nrf_run_level and nrf_run_level_train select the same form,
    nr_fused_x16.inc:397-422), which carries the training pin's one-stage bit rule for t1, y and hid over to the inference
    instantiations.  On TRAIN_TWIN_CASES the training forward's stored t1, y, hid and net are held to that rule here: the SAVE
    throughput kernels' first pin."""
    P, x = inputs(case)
    for k in range(1, P.n + 1):
        sm, _ = train_forward(case, k)
        w = run(case, "bf16", k)["ws"]
        assert np.array_equal(w.hid_bits, sm.hid_bits[k - 1]), "hid[%d] of the %d-block inference call differs from the training forward's" % (k - 1, k)
        if k >= 2:
            assert np.array_equal(w.net_bits, sm.bits["net"][k - 2]), "net[%d]" % (k - 2)
        if k >= 3:
            assert np.array_equal(w.net_prev_bits, sm.bits["net"][k - 3]), "net[%d]" % (k - 3)
        if case in nr.TRAIN_TWIN_CASES:
            i = k - 1                                                  # block k - 1: its hid is this run's (the stages of fused_stages)
            xin = np.asarray(x, dtype=np.float64) if i == 0 else sm.net[i - 1]
            for tag, (z, mag), act, bits in (("t1[%d]" % i, nr.fused_stage_t1(xin, P, i), True, sm.bits["t1"][i]),
                                             ("y[%d]" % i, nr.fused_stage_y(sm.t1[i], P, i), True, sm.bits["tv"][i]),
                                             ("hid[%d]" % i, nr.fused_stage_hid(sm.tv[i], xin, P, i), False, sm.hid_bits[i]),
                                             ("net[%d]" % i, nr.fused_stage_net(sm.hid[i], P, i), True, sm.bits["net"][i])):
                st = nr.check_stage(bits, z, mag, act)
                xs.report("%s training %s" % (case, tag), st)
                assert st["mismatches"] == 0 and st["max_ulp"] <= 1, (tag, st["mismatches"], st["max_ulp"], st["worst"])
                assert st["wide"] <= xs.WIDE_CAP * st["n"] and st["ambiguous"] <= xs.AMBIGUOUS_CAP * st["n"], (tag, st["wide"], st["ambiguous"], st["n"])
