"""The float64 restatement of the 2-D renderer's training step (tests/nr_restatement.py) pinned on the CPU, before any kernel is
held to it (test_gpu_nr_stagewise.py): against torch's float64 autograd, against the reference's own module (the nr_grad
fixture), the gate condition of every GPU case, the floors, the check_bf16 caps on the CPU emulation of the bf16 forwards, and
the proof that the GPU test's bounds are tight enough to matter -- seven deliberate faults that must all be reported."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nr_restatement as nr
import x16_stagewise as xs

TIGHT = {k: 1e-12 for k in nr.FAMILIES}


def torch_forward(x, flat, n):
    """The renderer in torch ops on float64 tensors: x [nb, C, h, w], flat = [w, b] pairs in Params.flat() order"""
    pairs = [(flat[2 * i], flat[2 * i + 1]) for i in range(len(flat) // 2)]
    rgbp, l1, l2, fe = pairs[:n + 1], pairs[n + 1:2 * n + 1], pairs[2 * n + 1:3 * n + 1], pairs[3 * n + 1:]
    k = torch.tensor([1.0, 2.0, 1.0], dtype=torch.float64)
    k2 = (k[:, None] * k[None, :]) / 16.0

    def conv(t, wb):
        return F.conv2d(t, wb[0][:, :, None, None], wb[1])

    def blur(t):
        C = t.shape[1]
        return F.conv2d(F.pad(t, [1, 1, 1, 1], mode="reflect"), k2.expand(C, 1, 3, 3), groups=C)

    def up(t):
        return blur(F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=False))
    rgb = up(conv(x, rgbp[0]))
    net = x
    for i in range(n):
        o = F.leaky_relu(conv(net, l1[i]), 0.2)
        o = F.leaky_relu(conv(o, l2[i]), 0.2)
        o = blur(F.pixel_shuffle(o + net.repeat(1, 4, 1, 1), 2))
        net = F.leaky_relu(conv(o, fe[i]), 0.2)
        rgb = rgb + conv(net, rgbp[i + 1])
        if i < n - 1:
            rgb = up(rgb)
    return torch.sigmoid(rgb)


def hwc(t):
    return t.detach().numpy().transpose(0, 2, 3, 1)


@pytest.mark.parametrize("case", list(nr.AUTOGRAD_CASES), ids=str)
def test_hand_written_backward_matches_float64_autograd(case):
    """every gradient of the hand-written backward, per entry, within 1e-12 S of torch's autograd through the same forward
    written with F.pixel_shuffle / F.interpolate / F.conv2d / F.pad(reflect); both operator orders ("exact" and "fused", which
    commutes the blur behind feat_layers and sends the residual through R_q) are the same function in exact arithmetic"""
    P, x, d_img = nr.case_inputs(case, nr.AUTOGRAD_CASES[case])
    f = nr.forward(x, P)
    tape = nr.tape_from_forward(f)
    flat = [torch.tensor(a, requires_grad=True) for a in P.flat()]
    xt = torch.tensor(np.ascontiguousarray(x.transpose(0, 3, 1, 2)), requires_grad=True)
    img = torch_forward(xt, flat, P.n)
    (img * torch.tensor(np.ascontiguousarray(d_img.transpose(0, 3, 1, 2)))).sum().backward()
    assert np.abs(hwc(img) - f["img"]).max() <= 1e-14
    want = {"d_featmap": hwc(xt.grad)}
    want.update({nm: t.grad.numpy() for nm, t in zip(P.names(), flat)})
    for path in ("exact", "fused"):
        got = nr.backward(d_img, P, tape, path=path)
        assert set(got) == set(want)
        maxima, lines = nr.compare(got, want, nr.scale(d_img, P, tape, path=path), TIGHT, tag=path)
        print(case, path, maxima)
        assert not lines, "\n".join(lines)
    frozen = nr.backward(d_img, P, tape, frozen=True)
    assert list(frozen) == ["d_featmap"] and np.array_equal(frozen["d_featmap"], nr.backward(d_img, P, tape)["d_featmap"])


def test_restatement_matches_the_reference_fixture(golden):
    """tests/golden/nr_grad (tools/gen_golden_nr_grad.py: the reference's NeuralRenderer in float64): image within 1e-14, d x and
    every parameter gradient per entry within 1e-12 S"""
    from n3dt import synthetic as syn
    data, m = golden("nr_grad")
    ref_name = {"rgb_w": "feat_2_rgb_list.%d.weight", "rgb_b": "feat_2_rgb_list.%d.bias", "w1_": "feat_upsample_list.%d.layer_1.weight",
                "b1_": "feat_upsample_list.%d.layer_1.bias", "w2_": "feat_upsample_list.%d.layer_2.weight", "b2_": "feat_upsample_list.%d.layer_2.bias",
                "wf": "feat_layers.%d.weight", "bf": "feat_layers.%d.bias"}
    assert len(m["cases"]) == len(nr.FIXTURE_CASES)
    for ci, (case, mc) in enumerate(zip(nr.FIXTURE_CASES, m["cases"])):
        assert case == (mc["featmap_size"], mc["featmap_nc"], mc["n_blocks"], mc["maps"])
        sd = syn.make_state_dict(nr.case_options(case), seed=m["seed"], bg_noise=0.1)
        assert np.allclose(syn.state_dict_checksum(sd), mc["weights_checksum"], rtol=1e-9, atol=1e-6), "synthetic weight generator drifted from the fixture"
        P = nr.params_from_state_dict(sd, case[2])
        tag = "c%d_" % ci
        x, d_img = data[tag + "x"].astype(np.float64), data[tag + "d_img"].astype(np.float64)
        f = nr.forward(x, P)
        assert np.abs(f["img"] - data[tag + "img"]).max() <= 1e-14
        tape = nr.tape_from_forward(f)
        got = nr.backward(d_img, P, tape)
        want = {"d_featmap": data[tag + "d_x"]}
        for name in got:
            if name != "d_featmap":
                stem = name.rstrip("0123456789")
                want[name] = data[tag + "g_" + ref_name[stem] % int(name[len(stem):])]
        assert len(want) == len(mc["parameters"]) + 1
        maxima, lines = nr.compare(got, want, nr.scale(d_img, P, tape), TIGHT, tag=str(case))
        print(case, maxima)
        assert not lines, "\n".join(lines)


def test_adjoint_matrices_are_the_transposes_of_the_forward_operators():
    """the closed forms of blur_adj_w3 / bil_adj_taps against the operators they are adjoint to, sizes 2 .. 9 (2: every tap is a border)"""
    for n in range(2, 10):
        assert np.array_equal(nr.blur_adj_matrix(n), nr.blur_matrix(n).T)
        assert np.array_equal(nr.bilinear_adj_matrix(n), nr.bilinear_matrix(n).T)
        assert np.allclose(nr.blur_matrix(n).sum(axis=1), 1.0) and np.allclose(nr.bilinear_matrix(n).sum(axis=1), 1.0)


# ---------------------------------------------------------------------------------------------
# everything below runs on the GPU test's own (geometry, seed) table
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def free64(case):
    P, x, d_img = nr.case_inputs(case, nr.GPU_CASES[case])
    f = nr.forward(x, P)
    tape = nr.tape_from_forward(f)
    return P, x, d_img, f, tape, nr.scale(d_img, P, tape)


@pytest.mark.parametrize("case", list(nr.GPU_CASES), ids=str)
def test_gate_condition(case):
    """Pre-activations within GATE_MARGIN (|b| + sum |w x|) of zero.  A case in STRICT_GATE_CASES has none, and the exact-path GPU
    test demands every gate of it.  The other geometries cannot have none whatever the seed: the share of such entries is about
    12 GATE_MARGIN (the density of z / (|b| + sum |w x|) at zero), 14 to 65 entries of the 4.6e5 to 1.2e6 pre-activations of a
    case, so the chance of a seed without one is e^-14 at best.  There the entries inside the band are counted (at most
    BAND_SHARE_CAP of a case) and listed to the GPU test, which demands every gate OUTSIDE the band and runs the restatement's
    backward on the kernel's own gates."""
    P, x, d_img, f, tape, S = free64(case)
    n_band, total = 0, 0
    for k in ("t1", "tv", "net"):
        for i in range(P.n):
            band = nr.gate_band(f, k, i)
            n_band += int(band.sum())
            total += band.size
    print(case, "entries inside the band: %d of %d; smallest distance %.3g" % (n_band, total, nr.gate_distance(f)))
    if case in nr.STRICT_GATE_CASES:
        assert n_band == 0
    assert n_band <= nr.BAND_SHARE_CAP * total


def f32_runs(case):
    """the free restatement in float32 in two accumulation orders; the float64 backward it is compared with runs on the float32
    run's gates (they may differ inside the gate band only, which is asserted)"""
    P, x, d_img, f64, tape64, S = free64(case)
    P32, x32, d32 = nr.to32(P, x, d_img)
    for tag, mm in (("torch.matmul", nr.mm32_torch), ("16-wide sequential", nr.mm32_seq16)):
        f32 = nr.forward(x32, P32, mm=mm)
        t32 = nr.tape_from_forward(f32)
        g32 = nr.backward(d32, P32, t32, mm=mm)
        forced = nr.tape_from_forward(f64)
        for k in ("t1", "tv", "net"):
            for i in range(P.n):
                flipped = getattr(forced, "g_" + k)[i] != getattr(t32, "g_" + k)[i]
                assert not np.any(flipped & ~nr.gate_band(f64, k, i)), "a float32 gate outside the band differs"
            setattr(forced, "g_" + k, getattr(t32, "g_" + k))
        yield tag, f32, g32, nr.backward(d_img, P, forced)


def test_f32_floors_have_not_moved_up():
    """NR_F32_FLOOR / NR_F32_IMAGE_FLOOR / NR_F32_STAGE_FLOOR re-measured: largest |g32 - g64| / S per case and family over both
    orders, largest |img32 - img64|, largest |a32 - a64| / (|b| + sum |w x|) over the lrelu stages"""
    img_floor = stage_floor = 0.0
    for case in nr.GPU_CASES:
        P, x, d_img, f64, tape64, S = free64(case)
        worst = {}
        for tag, f32, g32, g64 in f32_runs(case):
            maxima, _ = nr.compare(g32, g64, S, {k: np.inf for k in nr.FAMILIES})
            for k, v in maxima.items():
                worst[k] = max(worst.get(k, 0.0), v)
            img_floor = max(img_floor, float(np.abs(f32["img"].astype(np.float64) - f64["img"]).max()))
            stage_floor = max(stage_floor, max(float((np.abs(f32[k][i].astype(np.float64) - f64[k][i]) / f64[k + "_mag"][i]).max())
                                               for k in ("t1", "tv", "net") for i in range(P.n)))
        print(case, {k: "%.3g" % v for k, v in worst.items()})
        for k, v in worst.items():
            assert v <= nr.NR_F32_FLOOR[case][k], (case, k, v)
    print("image %.3g  stage %.3g" % (img_floor, stage_floor))
    assert img_floor <= nr.NR_F32_IMAGE_FLOOR and stage_floor <= nr.NR_F32_STAGE_FLOOR


@functools.lru_cache(maxsize=None)
def emulated(case):
    P, x, d_img, f, tape, S = free64(case)
    sm = nr.emulate_fused(x, P)
    tape16 = sm.tape(x)
    return sm, tape16, nr.scale(d_img, P, tape16, path="fused")


@pytest.mark.parametrize("case", list(nr.GPU_CASES), ids=str)
def test_bf16_forward_stages_stay_inside_the_caps(case):
    """check_bf16 on the CPU emulation of the case's fused bf16 forward: no mismatch (the emulation is one legal fp32 order), and
    every stage inside AMBIGUOUS_CAP and WIDE_CAP"""
    P, x, d_img, f, tape, S = free64(case)
    sm, _, _ = emulated(case)
    for tag, z, mag, act, bits in nr.fused_stages(sm, x, P):
        st = nr.check_stage(bits, z, mag, act)
        xs.report("%s %s" % (case, tag), st)
        assert st["mismatches"] == 0 and st["max_ulp"] <= 1
        assert st["ambiguous"] <= xs.AMBIGUOUS_CAP * st["n"] and st["wide"] <= xs.WIDE_CAP * st["n"], tag


def bf16_orders():
    return [("one k at a time", nr.mm32_seq1), ("16-wide sequential", nr.mm32_seq16e)] + \
        [("permuted %d" % s, nr.mm32_permuted(s)) for s in range(nr.BF16_FLOOR_ORDERS - 2)]


def bf16_spread(case):
    """largest |g32 - g64| / S per family of the teacher-forced backward with store = wq = bf16_rne, over BF16_FLOOR_ORDERS float32
    accumulation orders (all elementwise numpy: the same bits on every machine) x BF16_FLOOR_SEEDS seeds of the geometry"""
    worst = {}
    for seed in range(nr.GPU_CASES[case], nr.GPU_CASES[case] + nr.BF16_FLOOR_SEEDS):
        P, x, d_img = nr.case_inputs(case, seed)
        tape16 = nr.emulate_fused(x, P).tape(x)
        S = nr.scale(d_img, P, tape16, path="fused")
        g64 = nr.backward(d_img, P, tape16, store=nr.bf16_rne, wq=nr.bf16_rne, path="fused")
        P32, d32 = nr.to32(P, d_img)
        t32 = tape16.map(lambda a: a.astype(np.float32))
        t32.img = tape16.img.astype(np.float32)
        for o, (tag, mm) in enumerate(bf16_orders()):
            g32 = nr.backward(d32, P32, t32, mm=mm, store=nr.bf16_rne, wq=nr.bf16_rne, path="fused", rows_first=o % 2 == 0)
            maxima, _ = nr.compare(g32, g64, S, {k: np.inf for k in nr.FAMILIES})
            for k, v in maxima.items():
                worst[k] = max(worst.get(k, 0.0), v)
    return worst


def test_bf16_floors_have_not_moved_up():
    """NR_BF16_FLOOR re-measured"""
    for case in nr.GPU_CASES:
        worst = bf16_spread(case)
        print(case, "bf16", {k: "%.3g" % v for k, v in worst.items()})
        for k, v in worst.items():
            assert v <= nr.NR_BF16_FLOOR[case][k], (case, k, v)


# ---------------------------------------------------------------------------------------------
# mutants: the comparison rule at the GPU test's bound must report each of these faults
# ---------------------------------------------------------------------------------------------
def gate_of_layer_1_from_tv(tape):
    t = nr.Tape(tape.img, **{k: getattr(tape, k) for k in nr.Tape.FIELDS})
    t.g_t1 = [g[..., :g.shape[-1] // 2] for g in tape.g_tv]   # layer_1's gate read from the first 2C channels of tv
    return t


FAULTS = ("blur_border", "bilinear_edge", "residual_three", "db2_plane", "gate_t1_from_tv", "rgb0_branch", "dw_slice")


@pytest.mark.parametrize("fault", FAULTS)
def test_a_deliberate_fault_is_reported_at_the_gpu_bound(fault):
    """The float64 restatement with one fault against itself, at 4 x NR_F32_FLOOR (the exact path's bound) and, on the fused bf16
    path with its stores, at 4 x NR_BF16_FLOOR.  Every fault can show in every case (4 x 4 maps are all border; every map
    has an edge; the smallest product has 64 pixels), so every case must report it, in both precisions."""
    for case in nr.GPU_CASES:
        P, x, d_img, f, tape, S = free64(case)
        good = nr.backward(d_img, P, tape)
        bad = nr.backward(d_img, P, gate_of_layer_1_from_tv(tape) if fault == "gate_t1_from_tv" else tape,
                          fault=None if fault == "gate_t1_from_tv" else fault)
        maxima, lines = nr.compare(bad, good, S, nr.bound_of(nr.NR_F32_FLOOR[case]))
        assert lines, "%s passes the exact path's bound in case %s" % (fault, case)
        sm, tape16, S16 = emulated(case)
        kw = dict(store=nr.bf16_rne, wq=nr.bf16_rne)
        good = nr.backward(d_img, P, tape16, path="fused", **kw)
        bad = nr.backward(d_img, P, gate_of_layer_1_from_tv(tape16) if fault == "gate_t1_from_tv" else tape16, path="fused",
                          fault=None if fault == "gate_t1_from_tv" else fault, **kw)
        maxima16, lines16 = nr.compare(bad, good, S16, nr.bound_of(nr.NR_BF16_FLOOR[case]))
        assert lines16, "%s passes the bf16 bound in case %s" % (fault, case)
        print(fault, case, "exact: %d entries reported, largest %.3g of S; bf16: largest %.3g of S" %
              (len(lines), max(maxima.values()), max(maxima16.values())))


# ---------------------------------------------------------------------------------------------
# the 16-bit INFERENCE renderer, forward only, bf16 and IEEE half (the last section of nr_restatement.py; the GPU side is
# test_gpu_nr_infer_stagewise.py): layout, floors, caps on the CPU emulation, and the five faults the rules must report
# ---------------------------------------------------------------------------------------------
def infer_mm(case):
    """the large cases' emulation takes torch.matmul (their maps are 16-wide-sequential minutes); any float32 order is a legal one"""
    return nr.mm32_torch if case in nr.LARGE_INFER_CASES else nr.mm32_seq16


@functools.lru_cache(maxsize=None)
def infer_inputs(case):
    P, x, _ = nr.case_inputs(case, nr.INFER_CASES[case])
    return P, x


@functools.lru_cache(maxsize=None)
def infer_emulated(case, fmt):
    P, x = infer_inputs(case)
    return nr.emulate_infer(x, P, fmt, mm=infer_mm(case))


def test_16_bit_formats_round_like_the_hardware_types():
    """round16 / bits16 against numpy's IEEE half (subnormals, ties, overflow) and torch's bfloat16 conversion of float32 values; the
    bf16 names are wrappers"""
    rng = np.random.RandomState(3)
    z = np.concatenate([rng.randn(200000) * 10.0 ** rng.uniform(-9, 5, 200000),
                        [0.0, -0.0, 65504.0, 65519.9, 65520.0, 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * 1.0001, 3 * 2.0 ** -25, 2.0 ** -14, 1.0 + 2.0 ** -11]])
    z = z.astype(np.float32).astype(np.float64)
    with np.errstate(over="ignore"):
        half = z.astype(np.float16)
    assert np.array_equal(xs.bits16(z, "fp16"), half.view(np.uint16))
    assert np.array_equal(xs.bits16_to_f64(half.view(np.uint16), "fp16"), half.astype(np.float64))
    bf = torch.from_numpy(z.astype(np.float32)).to(torch.bfloat16)
    assert np.array_equal(xs.bf16_bits(z), bf.view(torch.int16).numpy().view(np.uint16))
    assert np.array_equal(xs.bits16(z, "bf16"), xs.bf16_bits(z)) and np.array_equal(xs.round16(z, "bf16"), xs.bf16_round(z))
    fin = np.abs(z) < 6e4
    assert np.all(np.abs(nr.trunc16(z[fin], "fp16")) <= np.abs(z[fin])) and np.array_equal(nr.trunc16(half.astype(np.float64)[fin], "fp16"), half.astype(np.float64)[fin])


@pytest.mark.parametrize("case", list(nr.INFER_CASES), ids=str)
def test_infer_workspace_layout_is_consistent(case):
    """for every k: the regions a call writes lie inside their carve regions, in order and without overlap, and the 16-bit carve ends
    before the packed tail"""
    fs, C, n, nb = case
    for k in range(1, n + 1):
        ck = (fs, C, k, nb)
        L = nr.infer_ws_layout(ck)
        assert L["t1"] == 0 and L["end"] <= L["packw"] and L["total"] % 4 == 0
        order = ["t1", "ps", "hid", "netA", "netB", "rgbA", "rgbB", "end"]
        assert all(L[a] <= L[b] for a, b in zip(order, order[1:]))
        o = 0
        for off, size in sorted(nr.infer_written(ck)):
            assert off >= o and off % 4 == 0
            o = off + size
        assert o <= L["total"]
        for name, nxt in (("hid", "netA"), ("netA", "netB"), ("netB", "rgbA"), ("rgbA", "rgbB"), ("rgbB", "end")):
            for off, size in nr.infer_written(ck):
                if off == L[name]:
                    assert off + size <= L[nxt], (name, k)


def test_infer_floors_are_in_range():
    """NR_X16_RGB0_FLOOR, NR_X16_RGB_FLOOR, NR_X16_SIGMOID_FLOOR re-measured over every inference case in both formats and both
    float32 orders: measured <= floor < 2 x measured"""
    m = {"rgb0": 0.0, "rgb": 0.0, "sigmoid": 0.0}
    for case in nr.INFER_CASES:
        P, x = infer_inputs(case)
        z64, S = nr.rgb0_stage(x, P)
        for tag, mm, rows_first in nr.RGB_ORDERS:
            z32 = nr.conv(x.astype(np.float32), P.rgb_w[0].astype(np.float32), P.rgb_b[0].astype(np.float32), mm)
            m["rgb0"] = max(m["rgb0"], float((np.abs(z32 - z64) / S).max()))
        for fmt in nr.FORMATS16:
            e = infer_emulated(case, fmt)
            for i in range(P.n):
                net = nr.emu_map(e, "net", i)
                pre, S, _ = nr.x16_rgb_stage(None, net, e["lo"][i], P, i, fmt, "mfma")
                for tag, mm, rows_first in nr.RGB_ORDERS:
                    p32 = nr.rgb_pre32(net, e["lo"][i], nr.hi_lo16(P.rgb_w[i + 1], fmt), P.rgb_b[i + 1], mm, rows_first)
                    m["rgb"] = max(m["rgb"], float((np.abs(p32 - pre) / S).max()))
                    for use_torch in (False, True):
                        err = np.abs(nr.sigmoid32(p32, use_torch).astype(np.float64) - nr.sigmoid(p32.astype(np.float64)))
                        m["sigmoid"] = max(m["sigmoid"], float(err.max()))
        print(case, {k: "%.3g" % v for k, v in m.items()})
    for k, floor in (("rgb0", nr.NR_X16_RGB0_FLOOR), ("rgb", nr.NR_X16_RGB_FLOOR), ("sigmoid", nr.NR_X16_SIGMOID_FLOOR)):
        print("%s: measured %.3g, floor %.3g" % (k, m[k], floor))
        assert m[k] <= floor < 2.0 * m[k], (k, m[k], floor)


@pytest.mark.parametrize("fmt", nr.FORMATS16)
@pytest.mark.parametrize("case", list(nr.INFER_CASES), ids=str)
def test_infer_emulation_passes_every_rule(case, fmt):
    """The CPU emulation (one legal float32 order) of the case in the format: every rounding under the ONE-stage rule with no mismatch
    and inside the caps of the format (bf16: AMBIGUOUS_CAP 5 %, WIDE_CAP 0.5 %; IEEE half: 25 %, 4 %); hid under the chain rule with the
    median of delta_hid / magnitude <= HID_MEDIAN_CAP; the pyramid plane from the stored net and the image from the stored hid inside
    their bounds"""
    P, x = infer_inputs(case)
    e = infer_emulated(case, fmt)
    amb_cap, wide_cap = xs.CAPS[fmt]
    for tag, z, mag, act, bits in nr.x16_one_stage(e, x, P, fmt):
        st = xs.check16(bits, z, xs.U * mag, fmt, act=nr.lrelu64 if act else None)
        xs.report("%s %s %s" % (case, fmt, tag), st)
        assert st["mismatches"] == 0 and st["max_ulp"] <= 1, tag
        assert st["ambiguous"] <= amb_cap * st["n"] and st["wide"] <= wide_cap * st["n"], tag
    xin = x
    for i in range(P.n):
        st = nr.x16_check_hid(e["hid_bits"][i], xin, P, i, fmt)
        print("%s %s hid[%d] chain rule: ambiguous %.1f %%, mismatches %d, delta_hid / magnitude median %.3g maximum %.3g" %
              (case, fmt, i, 100.0 * st["ambiguous"] / st["n"], st["mismatches"], st["median"], st["max"]))
        assert st["mismatches"] == 0 and st["max_ulp"] <= 1 and st["median"] <= nr.HID_MEDIAN_CAP
        hid, net = nr.emu_map(e, "hid", i), nr.emu_map(e, "net", i)
        pre, S, _ = nr.x16_rgb_stage(None, net, e["lo"][i], P, i, fmt, "mfma")
        bound, _ = nr.x16_rgb_bounds(pre, S, 0.0)
        assert nr.worst_ratio(e["pre"][i], pre, bound)[0] <= 1.0
        pre, S, slack = nr.x16_rgb_stage(hid, None, e["lo"][i], P, i, fmt, "mfma")
        _, bound = nr.x16_rgb_bounds(pre, S, slack)
        worst, at = nr.worst_ratio(e["img"][i], nr.sigmoid(pre), bound)
        print("%s %s img after %d blocks: largest error / bound %.3g" % (case, fmt, i + 1, worst))
        assert worst <= 1.0
        xin = net


def infer_verdicts(e, x, P, fmt):
    """which rules report something on an emulation: {"hid", "net", "img", "plane"} -> bool, over all blocks, exactly as the GPU test
    applies them (hid: chain rule; net: bit rule; img: from the stored hid with the slack; plane: from the stored net)"""
    out = {"hid": False, "net": False, "img": False, "plane": False}
    xin = x
    for i in range(P.n):
        st = nr.x16_check_hid(e["hid_bits"][i], xin, P, i, fmt)
        out["hid"] |= st["mismatches"] > 0 or st["max_ulp"] > 1
        hid, net = nr.emu_map(e, "hid", i), nr.emu_map(e, "net", i)
        st = nr.x16_check_net(e["net_bits"][i], hid, P, i, fmt)
        out["net"] |= st["mismatches"] > 0 or st["max_ulp"] > 1
        pre, S, _ = nr.x16_rgb_stage(None, net, e["lo"][i], P, i, fmt, "mfma")
        out["plane"] |= nr.worst_ratio(e["pre"][i], pre, nr.x16_rgb_bounds(pre, S, 0.0)[0])[0] > 1.0
        pre, S, slack = nr.x16_rgb_stage(hid, None, e["lo"][i], P, i, fmt, "mfma")
        out["img"] |= nr.worst_ratio(e["img"][i], nr.sigmoid(pre), nr.x16_rgb_bounds(pre, S, slack)[1])[0] > 1.0
        xin = net
    return out


EXPECTED_REPORTS = {"k_block": ("hid",), "residual_plane": ("hid",), "reflect": ("img",), "bilinear_swap": ("img", "plane"), "net_trunc": ("net",)}


@pytest.mark.parametrize("fmt", nr.FORMATS16)
@pytest.mark.parametrize("fault", nr.INFER_FAULTS)
def test_a_deliberate_inference_fault_is_reported(fault, fmt):
    """The CPU emulation with one deliberate fault, at the bounds the GPU test uses, in every case of GPU_CASES (every fault can show
    in each: the smallest has one 16-pixel tile, 4 x 4 maps are all border, every plane has interior outputs): the rule named for
    the fault reports it; the emulation without a fault reports nothing (test_infer_emulation_passes_every_rule)."""
    for case in nr.GPU_CASES:
        P, x = infer_inputs(case)
        got = infer_verdicts(nr.emulate_infer(x, P, fmt, fault=fault), x, P, fmt)
        print(fault, fmt, case, got)
        for rule in EXPECTED_REPORTS[fault]:
            assert got[rule], "%s passes the %s rule in case %s (%s)" % (fault, rule, case, fmt)
