"""CPU side of the stagewise pins of the fused bf16 training path (tests/x16_stagewise.py): the decoders and bf16 helpers
on exact data, the layout totals, and the conditions the GPU tests rely on -- the fp32 floors the tolerances are four times
of, re-measured on the CPU emulation of every case, and the cap on the share of entries a stage may leave ambiguous."""
import functools

import numpy as np
import pytest
import torch

import x16_stagewise as xs


# ---------------------------------------------------------------------------------------------------------------------
# formats
# ---------------------------------------------------------------------------------------------------------------------
def test_tile_image_round_trip_and_row_order():
    """An integer pattern value = 1000 tile + 32 sample + channel survives encode -> decode, and the encoded row of sample c holds
    the channels in the order [0-3, 8-11, 4-7, 12-15 | 16-19, 24-27, 20-23, 28-31] at byte 64 c (x16_core.h:420-425)."""
    n_tiles = 3
    s, c = np.meshgrid(np.arange(32), np.arange(n_tiles * 32), indexing="ij")
    x = (1000 * (c // 32) + 32 * s + c % 32).astype(np.uint16)[None]
    raw = xs.encode_images(x, n_tiles)
    assert raw.shape == (1, n_tiles * 1024)
    order = [0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15, 16, 17, 18, 19, 24, 25, 26, 27, 20, 21, 22, 23, 28, 29, 30, 31]
    assert list(xs.ROW_CH) == order
    for tile, samp in ((0, 0), (1, 5), (2, 31)):
        row = raw[0, tile * 1024 + samp * 32:tile * 1024 + samp * 32 + 32]
        assert list(row) == [1000 * tile + 32 * samp + ch for ch in order]
    # lane (c, h) writes fragment f_s at byte 64 c + 32 s + 16 h: element j of it is channel 16 s + 8 (j >> 2) + 4 h + (j & 3)
    for cc, h, sfrag, j in ((3, 1, 0, 5), (17, 0, 1, 2), (31, 1, 1, 7)):
        at = (64 * cc + 32 * sfrag + 16 * h) // 2 + j
        assert raw[0, at] == 32 * cc + 16 * sfrag + 8 * (j >> 2) + 4 * h + (j & 3)
    assert np.array_equal(xs.decode_images(raw, n_tiles), x)


def test_fragment_round_trip():
    """lane-linear fragments: piece ks, lane 32 h + c, element j = channel 16 ks + 8 (j >> 2) + 4 h + (j & 3) of sample c"""
    n_ks = 12
    s, c = np.meshgrid(np.arange(32), np.arange(n_ks * 16), indexing="ij")
    x = (256 * s + c).astype(np.uint16)[None]
    raw = xs.encode_frags(x, n_ks)
    for ks, lane, j in ((0, 0, 0), (3, 37, 6), (11, 63, 7), (5, 31, 3)):
        cc, h = lane & 31, lane >> 5
        assert raw[0, ks * 512 + lane * 8 + j] == 256 * cc + 16 * ks + 8 * (j >> 2) + 4 * h + (j & 3)
    assert np.array_equal(xs.decode_frags(raw, n_ks), x)


def test_gate_word_round_trip():
    """word w of a lane: bits 0-15 = tile 2 w, 16-31 = tile 2 w + 1; bit r = accumulator register r = row (r & 3) + 8 (r >> 2) + 4 h"""
    rng = np.random.default_rng(0)
    bits = rng.integers(0, 2, size=(2, 8, 32, 384)).astype(bool)
    raw = xs.encode_gates(bits)
    assert raw.shape == (2, xs.GATE_WORDS) and raw.dtype == np.uint32
    for blk, layer, w, lane, b in ((0, 0, 0, 0, 0), (1, 7, 5, 63, 31), (0, 3, 2, 40, 17), (1, 5, 4, 9, 12)):
        cc, h, r = lane & 31, lane >> 5, b & 15
        ch = 32 * (2 * w + (b >> 4)) + (r & 3) + 8 * (r >> 2) + 4 * h
        assert bool((raw[blk, (layer * 6 + w) * 64 + lane] >> b) & 1) == bits[blk, layer, cc, ch]
    assert np.array_equal(xs.decode_gates(raw), bits)


def test_bf16_helpers_against_torch():
    """ties (to even, both ways), subnormals, negative zero, the largest finite value and the overflow to infinity"""
    vals = [0.0, -0.0, 1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, 1.0 + 2.0 ** -8 - 2.0 ** -20, -(1.0 + 2.0 ** -8),
            2.0 ** -126, 2.0 ** -133, 2.0 ** -134, 3 * 2.0 ** -134, 2.0 ** -134 * 1.0001, -(2.0 ** -130) * 1.3, 3.3e38, 3.39e38, 3.4e38, -3.4e38, 1e-45, 123.456,
            -0.001953125 * 1.00390625]
    rng = np.random.default_rng(1)
    vals = np.concatenate([np.array(vals, dtype=np.float32), rng.standard_normal(4096).astype(np.float32) * np.float32(2.0) ** rng.integers(-140, 120, 4096).astype(np.float32)])
    want = torch.from_numpy(vals).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    got = xs.bf16_bits(vals.astype(np.float64))
    assert np.array_equal(got, want)
    assert np.array_equal(xs.bf16_to_f64(want), torch.from_numpy(vals).to(torch.bfloat16).double().numpy())
    assert xs.bf16_bits(np.array([-0.0]))[0] == 0x8000 and xs.ordinal(np.array([0x8000], dtype=np.uint16))[0] == 0
    # neighbours are 1 apart on the ordinal line, across zero and across a binade
    b = np.array([0x0001, 0x0000, 0x8001, 0x3F7F, 0x3F80], dtype=np.uint16)
    assert list(xs.ordinal(b)) == [1, 0, -1, 0x3F7F, 0x3F80]
    # float64 is rounded once: a value above the tie by less than an fp32 ulp goes up, through float32 it would tie to even
    z = 1.0 + 2.0 ** -8 + 2.0 ** -30
    assert xs.bf16_round(z) == 1.0 + 2.0 ** -7 and float(torch.tensor(np.float32(z)).to(torch.bfloat16)) == 1.0
    hi, lo = xs.split_hi_lo(np.array([0.123456789], dtype=np.float32))
    assert abs(hi[0] + lo[0] - np.float32(0.123456789)) <= 2.0 ** -16 * 0.13 and xs.bf16_round(hi)[0] == hi[0] and xs.bf16_round(lo)[0] == lo[0]


def test_check_bf16_rule():
    """bit-exact away from a boundary, either neighbour next to one, zero or the rounded value next to a ReLU's zero, closed gates zero"""
    ulp = 2.0 ** -7
    z = np.array([1.0 + 0.3 * ulp, 1.0 + 0.5 * ulp + 1e-9, -1e-9, 0.7, 0.7])
    delta = np.full(5, 1e-7)
    exp = xs.bf16_bits(np.maximum(z, 0))
    up = xs.bf16_bits(np.array([1.0 + ulp]))[0]
    one = xs.bf16_bits(np.array([1.0]))[0]
    st = xs.check_bf16(exp, z, delta, relu=True)
    assert st["mismatches"] == 0 and st["ambiguous"] == 2 and st["max_ulp"] == 0
    stored = exp.copy()
    stored[1] = one                                  # the other neighbour of an ambiguous entry
    stored[2] = xs.bf16_bits(np.array([5e-8]))[0]    # a ReLU entry the kernel saw just above zero
    st = xs.check_bf16(stored, z, delta, relu=True)
    # (the ReLU entry is a wide one: between 0 and bf16(z + delta) lie the subnormals; its distance is reported apart, unclamped)
    assert st["mismatches"] == 0 and st["max_ulp"] == 1 and st["wide"] == 1 and st["max_ulp_wide"] > 1
    stored = exp.copy()
    stored[0] = up                                   # not ambiguous: one ulp off is a mismatch
    st = xs.check_bf16(stored, z, delta, relu=True)
    assert st["mismatches"] == 1 and st["max_ulp"] == 1 and st["worst"][0][0] == 0
    stored = exp.copy()
    stored[1] = xs.bf16_bits(np.array([1.0 + 2 * ulp]))[0]   # ambiguous, but two ulps away
    assert xs.check_bf16(stored, z, delta, relu=True)["mismatches"] == 1
    gate = np.array([True, True, True, False, True])
    assert xs.check_bf16(exp, z, delta, gate=gate)["mismatches"] == 1          # a closed gate must store zero
    stored = exp.copy()
    stored[3] = 0
    assert xs.check_bf16(stored, z, delta, relu=True, gate=gate)["mismatches"] == 0


def test_layout_totals_against_the_library_and_by_hand():
    """The Python restatement of saved16_layout / ws16_layout against the library's own totals, and the totals of the GPU
    shapes against sizes computed by hand."""
    from n3dt import ops
    for name, c in xs.CASES.items():
        S = 179 + (64 if c["kw"].get("include_gaze") else 0)
        U = c["kw"].get("audio_dim", 64)
        geom = ops.make_geom(c["B"], c["n_rays"], c["n_samples"], 384, 256, S, 127, U, 8, 2, 2.5, -3.5)
        sv, ws = xs.library_totals(geom)
        assert sv == xs.saved_layout(c["B"], c["n_rays"], c["n_samples"])["total"], name
        assert ws == xs.ws_layout(c["B"], c["n_rays"], c["n_samples"])["total"], name
    geom = ops.make_geom(2, 16, 24, 384, 256, 179, 127, 64, 8, 2, 2.5, -3.5, vd_dim=27)
    assert xs.library_totals(geom)[0] == xs.saved_layout(2, 16, 24, vd_dim=27)["total"]

    def up(n):
        return -(-n // 256) * 256
    fixed_ws = up(2280 * 1024) + up(4 * 224 * 384) + 4 * 10 * 8 * 384 * 384 + 4 * 10 * 4096
    # (a) 2 x 16 x 24: 32 blocks, 32 rays
    assert xs.saved_layout(2, 16, 24)["total"] == up(4 * 2 * 4064) + 33 * 98 * 2048 + 33 * 12 * 1024 + 32 * 256 + 32 * 24 * 4 + 32 * 196 * 4 + 33 * 3072 * 4 + 4 * 192 * 384
    assert xs.ws_layout(2, 16, 24)["total"] == (32 * 196 * 4 + 32 * 128 + 33 * 103 * 2048 + 2 * 32 * 128 + 2 * 32 * 32 * 64 * 4 + 32 * 256 * 4 + 32 * 192 * 4 +
                                                 up(32 * 4) + up(4 * 2 * 4064) + up(4 * 2 * 224) + fixed_ws)
    # (b) 1 x 9 x 40: 18 blocks, 9 rays
    assert xs.saved_layout(1, 9, 40)["total"] == up(4 * 4064) + 19 * 98 * 2048 + 19 * 12 * 1024 + 18 * 256 + up(9 * 40 * 4) + up(9 * 196 * 4) + 19 * 3072 * 4 + 4 * 192 * 384
    # (c) 2 x 25 x 40: 100 blocks, 50 rays
    assert xs.saved_layout(2, 25, 40)["total"] == up(4 * 2 * 4064) + 101 * 98 * 2048 + 101 * 12 * 1024 + 100 * 256 + up(50 * 40 * 4) + up(50 * 196 * 4) + 101 * 3072 * 4 + 4 * 192 * 384
    assert xs.ws_layout(2, 25, 40)["total"] == (up(100 * 196 * 4) + 100 * 128 + 101 * 103 * 2048 + 2 * 100 * 128 + 2 * 100 * 32 * 64 * 4 + 50 * 256 * 4 + 50 * 192 * 4 +
                                                 up(50 * 4) + up(4 * 2 * 4064) + up(4 * 2 * 224) + fixed_ws)


def test_weight_gradient_slices_of_the_gpu_shapes():
    """50 blocks per frame (case c) in the slice counts both planners pick: 6 slices of ceil(50 / 6) = 9 blocks, the last one 5."""
    assert xs.dw_slices(50, 2) == (6, 9) and xs.dw_slices(50, 2, 7, 2) == (6, 9) and xs.dw_slices(50, 2, 2, 1) == (6, 9)
    assert xs.dw_slices(16, 2) == (2, 8) and xs.dw_slices(16, 2, 7, 2) == (2, 8)
    assert xs.dw_slices(18, 1) == (2, 9) and xs.dw_slices(18, 1, 7, 2) == (2, 9)


# ---------------------------------------------------------------------------------------------------------------------
# the floors and the ambiguity cap, on the CPU emulation of every case
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def emulation(name):
    return xs.Emulation(name)


@pytest.mark.parametrize("name", list(xs.CASES))
def test_fp32_floor_and_ambiguous_share(name):
    """Every forward and dX stage of the case: the three float32 summation orders against float64, in units of
    |b| + sum |w x| -- none above the recorded floor U_FLOOR, of which U is four times -- and under that U at most 5 % of a
    stage's entries ambiguous.  (A cap on the emulation, not a measurement of a kernel.)"""
    em = emulation(name)
    sv, ws, W = em.saved, em.ws, em.W
    floor, shares, wides = 0.0, {}, {}
    frame = sv.frame_of_point()
    stages = []
    for l in range(8):
        stages.append(("H%d" % l, xs.forward_input(sv.x_bits, l), W.fwd[l], xs.bias_rows(sv.fold, frame, l, 384), True, None))
    h7 = xs.bf16_to_f64(sv.h_bits(7))
    stages.append(("sigma", h7, W.den[None, :], xs.bias_rows(sv.fold, frame, 8, 1), None, None))
    stages.append(("gS", h7, W.wm, xs.bias_rows(sv.fold, frame, 10, 192), True, None))
    for l in range(7, -1, -1):
        stages.append(("dZ%d" % l, xs.dx_input(ws, l), W.bwd[l].T, None, False, sv.gates[l]))
    for tag, X, Wq, b, relu, gate in stages:
        z, mag = xs.linear64(X, Wq, b)
        worst = 0.0
        for _, fn in xs.LIN32:
            z32 = fn(X, Wq, b).astype(np.float64)
            sel = xs.pairwise_rows(z.shape[0]) if z32.shape[0] != z.shape[0] else slice(None)
            ok = mag[sel] > 0
            worst = max(worst, float((np.abs(z32 - z[sel])[ok] / mag[sel][ok]).max()))
        floor = max(floor, worst)
        if relu is not None:
            shares[tag], wides[tag] = xs.ambiguous_share(z, xs.U * mag, relu=relu, gate=gate)
        print("%-10s %-6s floor %.3e%s" % (name, tag, worst, "" if relu is None else "  ambiguous %.3f %%" % (100 * shares[tag])))
    print("%s: floor %.3e (recorded %.3e), largest ambiguous share %.3f %%" % (name, floor, xs.U_FLOOR, 100 * max(shares.values())))
    assert floor <= xs.U_FLOOR
    assert max(shares.values()) <= xs.AMBIGUOUS_CAP, shares
    print("%s: largest share of wide-delta entries %.4f %% (cap %.3f %%)" % (name, 100 * max(wides.values()), 100 * xs.WIDE_CAP))
    assert max(wides.values()) <= xs.WIDE_CAP, wides


def test_the_emulation_passes_its_own_stage_checks():
    """The comparison rule on data with a known answer: the emulation stores bf16 of its sequential fp32 sums, so every stage
    must pass under U with no mismatch -- and fail once one stored value moves to a neighbour, one gate bit flips, or two
    k-slots of a weight are swapped."""
    em = emulation("b")
    sv, ws, W = em.saved, em.ws, em.W
    for tag, z, mag, relu, bits in xs.forward_stages(sv, W):
        st = xs.check_bf16(bits, z, xs.U * mag, relu=relu)
        assert st["mismatches"] == 0 and st["max_ulp"] <= 1, (tag, st)
    for tag, z, mag, gate, bits in xs.dx_stages(sv, ws, W):
        st = xs.check_bf16(bits, z, xs.U * mag, gate=gate)
        assert st["mismatches"] == 0 and st["max_ulp"] <= 1, (tag, st)
    # one stored activation one ulp up
    z, mag = xs.hidden_stage64(sv, W, 3)
    bits = sv.h_bits(3).copy()
    i = np.unravel_index(np.argmax(xs.bf16_to_f64(bits)), bits.shape)
    bits[i] += 1
    assert xs.check_bf16(bits, z, xs.U * mag, relu=True)["mismatches"] == 1
    # two k-slots of one weight row swapped
    Wb = W.fwd[2].copy()
    Wb[7, [16, 17]] = Wb[7, [17, 16]]
    zb, mb = xs.linear64(xs.forward_input(sv.x_bits, 2), Wb, xs.bias_rows(sv.fold, sv.frame_of_point(), 2, 384))
    assert xs.check_bf16(sv.h_bits(2), zb, xs.U * mb, relu=True)["mismatches"] > 0
    # a gate word paired with the wrong tile: the gates of layer 4 applied to dZ5
    z, mag = xs.dx_stage64(xs.dx_input(ws, 5), W, 5)
    assert xs.check_bf16(ws.dz_bits(5), z, xs.U * mag, gate=sv.gates[4])["mismatches"] > 0


@pytest.mark.parametrize("name", list(xs.CASES))
def test_weight_gradient_floors(name):
    """The weight-gradient families in float32 -- 16 points at a time inside the kernel's slices, numpy's and torch's products, the
    small products behind them in float32 as well -- against float64, per entry in units of sum |dz| |x|: none above the recorded
    floors, of which the GPU bounds are four times."""
    em = emulation(name)
    c = xs.CASES[name]
    ref = xs.grads64(em.saved, em.ws, em.W, em.codes)
    per = xs.dw_slices(c["n_rays"] * ((c["n_samples"] + 31) // 32), c["B"])[1]
    floors = {}
    for tag, mm in (("seq", xs.dw32_seq(per)), ("numpy", xs.dw32_numpy), ("torch", xs.dw32_torch)):
        got = xs.grads64(em.saved, em.ws, em.W, em.codes, matmul=mm, cast=np.float32, post=np.float32)
        for k, (v, mag, fam) in ref.items():
            floors[fam] = max(floors.get(fam, 0.0), xs.grad_error(got[k][0], v, mag, em.saved.nb * 32 * xs.UNDERFLOW_TERMS))
    print("%s: weight-gradient floors %s" % (name, {k: "%.3e" % v for k, v in floors.items()}))
    for fam, v in floors.items():
        assert v <= xs.dw_floor(name, fam), (fam, v)
        if c.get("hier") and fam in xs.DW_FLOOR_GIVEN:   # an entry of its own only where the table does not hold, and no wider than measured
            assert xs.DW_FLOOR[fam] < v and xs.DW_FLOOR_GIVEN[fam] <= 1.25 * v, (fam, v)


@pytest.mark.parametrize("name", list(xs.CASES))
def test_weight_floor(name):
    """per-sample weights: float32 compositing against float64 on the emulation's sigma and dist, in units of weight_tolerance"""
    em = emulation(name)
    c = xs.CASES[name]
    R, bpr = c["B"] * c["n_rays"], (c["n_samples"] + 31) // 32
    w64, T64 = xs.composite64(em.saved.sigma_pre, em.saved.dist, R, bpr, c["n_samples"])
    w32 = xs.composite32(em.saved.sigma_pre, em.saved.dist, R, bpr, c["n_samples"])
    worst = float((np.abs(w32 - w64) / xs.weight_tolerance(w64, T64)).max())
    print("%s: weight floor %.3f of weight_tolerance (recorded %.2f)" % (name, worst, xs.W_FLOOR))
    assert worst <= xs.W_FLOOR


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_bias_route_spread(name):
    """The inference kernel differs from the training forward only by the bias route (exact fp32 C operand against hi + lo through
    an MFMA): the spread of the two free-running emulations on per-sample weights, fg_feat and bg_alpha, none above the recorded
    floor, of which the GPU bound is four times."""
    em = emulation(name)
    w2, b2 = em.ws_[11], em.bs_[11]
    got = xs.route_spread(xs.free_forward(em.saved, em.W, w2, b2, True), xs.free_forward(em.saved, em.W, w2, b2, False))
    print("%s: bias-route spread %s" % (name, {k: "%.3e" % v for k, v in got.items()}))
    for k, v in got.items():
        assert v <= xs.ROUTE_FLOOR[k], (k, v)
