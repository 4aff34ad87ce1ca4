"""CPU side of the pin of the kernels around the fused MLP kernel in the inference forward (tests/head_stagewise.py):
  * every floor of head_stagewise.FLOOR re-measured from the float32-ordered emulations (a floor that moved up fails);
  * the float64 restatement of the whole chain fold -> MLP -> part -> head against the project's oracle at 1e-5;
  * each deliberate fault applied to the float64 reference must move an entry of its stage beyond the bound, measured against the
    float32 emulation of the CORRECT stage -- or be listed in INDISTINGUISHABLE with the reason it cannot be told from rounding.
No GPU: `part` comes from head_stagewise.cpu_part (the oracle's sample points through the restated matrices in float64)."""
import functools

import numpy as np
import pytest

import head_stagewise as hs

ALL = list(hs.CASES)
WEIGHT_SETS = ("ragged", "contrast", "gaze", "vd")   # the four distinct state dicts
BLOCKS = (16, 32)


@functools.lru_cache(maxsize=None)
def head_stages(name, bs):
    """every head stage of a case: float64 reference and the float32 emulations"""
    ci = hs.case_inputs(name)
    part, wlocal = hs.cpu_part(name, bs)
    R = part.shape[0]
    W2, b2 = ci["ws"][11], ci["bs"][11]
    bg = hs.bg_rows(ci["bg_hwc"], R, ci["n_rays"])
    ref = hs.head_ref(part, W2, b2, bg)
    pref, ws, ds = hs.head_chain32(part)
    G32 = hs.head_G32(part, pref)
    e = {"pref": pref, "ws": ws, "ds": ds, "G": G32, "fg_fma": hs.head_fma32(G32, ws, W2, b2), "fg_mfma": hs.head_mfma32(G32, ws, W2, b2)}
    e["merge_fma"], e["merge_mfma"] = hs.merge32(e["fg_fma"], ws, bg), hs.merge32(e["fg_mfma"], ws, bg)
    e["rgb0"] = hs.rgb0_emul(e["merge_mfma"], ci["w3"], ci["b3"])
    e["block"] = hs.block_sum32(wlocal, bs)
    return {"ci": ci, "part": part, "wlocal": wlocal, "ref": ref, "emu": e, "bg": bg, "W2": W2, "b2": b2}


@functools.lru_cache(maxsize=None)
def measured():
    """family -> (largest |emulation32 - ref64| / magnitude, where)"""
    out = {}

    def put(family, r, where):
        if family not in out or r > out[family][0]:
            out[family] = (r, where)

    for name in WEIGHT_SETS:
        ci = hs.case_inputs(name)
        ref, mag = hs.merged_matrix64(ci["ws"])
        put("wm", hs.ratio(hs.merged_matrix32(ci["ws"]), ref, mag), name)
    for name in ALL:
        ci = hs.case_inputs(name)
        for merged in (False, True):
            ref, mag, exact = hs.fold_ref(ci["ws"], ci["bs"], ci["codes"], ci["S"], ci["A"], ci["U"], merged)
            emu = hs.fold_emul(ci["ws"], ci["bs"], ci["codes"], ci["S"], ci["A"], ci["U"], merged)
            put("fold", hs.ratio(emu[:, ~exact], ref[:, ~exact], mag[:, ~exact]), "%s merged=%d" % (name, merged))
        d = hs.directions32(ci)
        w_vd = hs.case_inputs("vd")["w_vd"]
        ref, mag = hs.vd_ref(w_vd, d)
        put("vd", hs.ratio(hs.vd_emul(w_vd, d), ref, mag), name)
        for bs in BLOCKS:
            st = head_stages(name, bs)
            ref, e, where = st["ref"], st["emu"], "%s bs=%d" % (name, bs)
            put("block", hs.ratio(e["block"], hs.f64(st["wlocal"]).sum(2).reshape(-1), np.abs(hs.f64(st["wlocal"])).sum(2).reshape(-1)), where)
            put("chain", hs.ratio(e["ws"], ref["wsum"], ref["mag_chain_w"]), where)
            put("chain", hs.ratio(e["ds"], ref["dsum"], ref["mag_chain_d"]), where)
            put("G", hs.ratio(e["G"], ref["G"], ref["mag_G"]), where)
            for form in ("fma", "mfma"):
                put(hs.family_of(name, "fg_" + form), hs.ratio(e["fg_" + form], ref["fg"], ref["mag_fg"]), where)
                put("merge_" + form, hs.ratio(e["merge_" + form], ref["merge"], ref["mag_merge"]), where)
            r0, m0 = hs.rgb0_ref(e["merge_mfma"], st["ci"]["w3"], st["ci"]["b3"])
            put("rgb0", hs.ratio(e["rgb0"], r0, m0), where)
    return out


@pytest.mark.parametrize("family", sorted(hs.FLOOR))
def test_floor_is_not_above_its_recorded_constant(family):
    r, where = measured()[family]
    print("%-10s measured floor %.3e (%s), recorded %.3e, unit %.3e" % (family, r, where, hs.FLOOR[family], hs.unit(family)))
    assert 0.0 < r <= hs.FLOOR[family]
    assert hs.FLOOR[family] <= 1.25 * r, "the recorded constant is the measured floor rounded up, not a wider number"


def test_bg_alpha_and_weight_of_the_emulation_are_inside_their_rules():
    """bg_alpha = 1 - wsum of the float32 chain inside bound_bg_alpha; weight is a single float32 multiply (nothing to measure)"""
    for name in ALL:
        for bs in BLOCKS:
            st = head_stages(name, bs)
            ba = np.float32(1) - st["emu"]["ws"]
            assert np.all(np.abs(hs.f64(ba) - st["ref"]["bg_alpha"]) <= hs.bound_bg_alpha(st["ref"]["mag_chain_w"])), (name, bs)
            w = hs.weight_expected(st["part"], st["wlocal"], st["ci"]["Ns"], bs)
            assert w.shape == (st["part"].shape[0], st["ci"]["Ns"]) and np.isfinite(w).all()


def test_the_cases_reach_the_branches_they_are_there_for():
    bpr = {n: {bs: (hs.CASES[n]["n_samples"] + bs - 1) // bs for bs in BLOCKS} for n in ALL}
    assert bpr["ragged"] == {16: 3, 32: 2} and bpr["span"] == {16: 5, 32: 3} and bpr["full"] == {16: 2, 32: 1}
    assert bpr["deep"] == {16: hs.HEAD_MAX_BPR, 32: 32} and bpr["one"] == {16: 2, 32: 1}
    total = {n: hs.CASES[n]["B"] * hs.CASES[n]["n_rays"] for n in ALL}
    assert total["one"] < hs.HEAD_RAYS and total["ragged"] % hs.HEAD_RAYS and total["ragged"] < hs.RH_RAYS
    assert total["span"] == 4 * 32 + 7 and hs.CASES["span"]["n_rays"] % hs.RH_RAYS and total["full"] % hs.RH_RAYS == 0
    # deep: the seeded weights are translucent, so pref only falls to 0.44 .. 0.78 over the 64 blocks (measured); what the case pins is
    # the 64-entry pref row and the 64-term chains.  pref that underflows is case contrast's: 1e-57 at 16-sample blocks, 0 at 32.
    deep = head_stages("deep", 16)["ref"]["pref"]
    assert deep.shape[1] == hs.HEAD_MAX_BPR and np.all(np.diff(deep, axis=1) <= 0) and deep[:, -1].max() < 0.8
    st = head_stages("contrast", 32)
    t = hs.f64(st["part"])[:, :, hs.G + 2]
    assert t.min() < 1e-9 and t.max() > 0.5, "saturated and transparent blocks side by side"
    assert 0.0 < head_stages("contrast", 16)["ref"]["pref"].min() < 2.0 ** -126, "pref below the smallest normal float32"


def test_workspace_carve_and_packed_size_against_the_library():
    """render_carve == n3dt_render_workspace_bytes and packed_bytes == n3dt_mlp_packed_bytes, every case and precision (host code only)"""
    import ctypes
    from n3dt import ops
    from n3dt._lib import lib
    for name in ALL:
        ci = hs.case_inputs(name)
        geom = ops.make_geom(ci["B"], ci["n_rays"], ci["Ns"], 384, 256, ci["S"], ci["A"], ci["U"], hs.FEATMAP_SIZE, 2, 2.5, -3.5, vd_dim=ci["vd"])
        for p in hs.PRECS.values():
            c = hs.render_carve(ci["B"], ci["n_rays"], ci["Ns"], p, ci["vd"])
            assert c["total"] == ops.render_workspace_bytes(geom, p), (name, p)
            assert hs.packed_bytes(p) == lib().n3dt_mlp_packed_bytes(ctypes.byref(geom), p), (name, p)
            assert all(c[k] % 256 == 0 for k in ("part", "wlocal", "bghwc", "total"))


def test_index_maps_are_bijections_and_pack_writes_what_it_says():
    for p in hs.PRECS.values():
        for s in range(hs.NSTAGE):
            N, K, _ = hs.stage_dims(s)
            row, col = hs.pack_index_map(N, K, p)
            assert np.array_equal(np.sort(row * K + col), np.arange(N * K)), (p, s)
    ci = hs.case_inputs("ragged")
    wm = hs.merged_matrix32(ci["ws"])
    for p in hs.PRECS.values():
        a, n = hs.pack_expected(ci["ws"], ci["bs"], ci["S"], p, wm, 0xA5)
        b, _ = hs.pack_expected(ci["ws"], ci["bs"], ci["S"], p, wm, 0x5A)
        assert int((a != b).sum()) == a.size - n, "the bytes that follow the prefill are exactly the ones no kernel writes"


@pytest.mark.parametrize("name", ALL)
def test_restatement_against_the_oracle(name):
    """fold -> MLP -> part -> head in float64 (restated layouts and column selections all the way) against oracle.forward,
    skip_neural_render=True (include_vd for case vd): fg_feat and bg_alpha at 1e-5; both block sizes give the same rays."""
    from oracle import oracle as orc
    ci = hs.case_inputs(name)
    if ci["planes"] is not None:   # the hierarchical cases: the oracle's fine pass on the case's planes (oracle.forward_hier's second half)
        inp = ci["inp"]
        f = orc.sample_planes(inp["batch_xy"].numpy(), inp["batch_Rmats"].numpy(), inp["batch_Tvecs"].numpy(), inp["batch_inv_inmats"].numpy(), ci["planes"])
        rgb, dens = orc.mlp(ci["sd"], orc.embed(f["pts"]), ci["codes"][0], ci["codes"][1], ci["codes"][2])
        fg, ba, _, _ = orc.composite(rgb, dens, f["z_dists"], f["zvals"])
        ref = {"fg_feat": fg, "bg_alpha": ba}
    else:
        ref = orc.forward(ci["sd"], ci["opt"], ci["inp"], skip_neural_render=True, include_vd=bool(ci["vd"]))
    fg_o, ba_o = np.moveaxis(ref["fg_feat"], 1, 2).reshape(-1, hs.C), ref["bg_alpha"].reshape(-1)
    pt = hs.cpu_points(name)
    e_s = float((np.abs(np.maximum(pt["sigma64"], 0.0) - pt["sigma"]) / pt["sigma_mag"]).max())
    print("%s: restated density against the oracle's per-sample density, largest |d| / (|b| + sum |w h|) = %.3e" % (name, e_s))
    assert e_s <= 1e-5
    for bs in BLOCKS:
        st = head_stages(name, bs)["ref"]
        e_fg, e_ba = float(np.abs(st["fg"] - fg_o).max()), float(np.abs(st["bg_alpha"] - ba_o).max())
        print("%s bs=%d: max|fg - oracle| %.3e (max|fg| %.2f), max|bg_alpha - oracle| %.3e" % (name, bs, e_fg, np.abs(fg_o).max(), e_ba))
        assert e_fg <= 1e-5 and e_ba <= 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# strength: deliberate faults
# ---------------------------------------------------------------------------------------------------------------------
# faults that no comparison can see at these shapes, with the reason (asserted below to be invisible, so the list cannot rot)
INDISTINGUISHABLE = {
    "bg_prev_frame": "the background map has one row per ray index and none per frame: the same ray index one frame earlier IS the same row "
                     "(bit-identical, not merely inside rounding).  The fault that exists here -- the row index not wrapped at a frame "
                     "boundary inside a workgroup -- is `bg_no_wrap`, which is detected.",
}


def beyond(emu, ref, mag, family, extra=0.0):
    """the largest (|emulation of the correct stage - faulty reference| - extra) / (unit x magnitude): > 1 means detected"""
    return hs.ratio(emu, ref, mag, extra) / hs.unit(family)


def head_fault(fault, stage, families, cases=ALL):
    worst = 0.0
    for name in cases:
        for bs in BLOCKS:
            st = head_stages(name, bs)
            if fault in ("bg_prev_frame", "bg_no_wrap"):
                bad = hs.head_ref(st["part"], st["W2"], st["b2"], hs.bg_rows(st["ci"]["bg_hwc"], st["part"].shape[0], st["ci"]["n_rays"], fault[3:]))
            else:
                bad = hs.head_ref(st["part"], st["W2"], st["b2"], st["bg"], fault)
            mag = np.maximum(bad["mag_" + stage], st["ref"]["mag_" + stage]) if "mag_" + stage in bad else None
            for form, family in families:
                worst = max(worst, beyond(st["emu"][form], bad[stage], mag, family))
    return worst


HEAD_FAULTS = {
    "pref_prev": ("G", (("G", "G"),)),
    "lost_block": ("G", (("G", "G"),)),
    "no_b2": ("fg", (("fg_fma", "fg_fma"), ("fg_mfma", "fg_mfma"))),
    "bg_prev_frame": ("merge", (("merge_fma", "merge_fma"), ("merge_mfma", "merge_mfma"))),
    "bg_no_wrap": ("merge", (("merge_mfma", "merge_mfma"),)),
    "lane_half": ("fg", (("fg_mfma", "fg_mfma"),)),
}


@pytest.mark.parametrize("fault", sorted(HEAD_FAULTS))
def test_head_fault_is_beyond_the_bound(fault):
    stage, families = HEAD_FAULTS[fault]
    w = head_fault(fault, stage, families)
    print("fault %-14s stage %-6s largest deviation = %.3g x bound" % (fault, stage, w))
    if fault in INDISTINGUISHABLE:
        print("  cannot be told from rounding: " + INDISTINGUISHABLE[fault])
        assert w <= 1.0
    else:
        assert w > 1.0


def test_pref_prev_also_moves_the_chain():
    """wsum / depth see the shifted pref as well (family chain), at every case with more than one block"""
    for name in ("ragged", "span", "deep", "contrast"):
        st = head_stages(name, 32)
        bad = hs.head_ref(st["part"], st["W2"], st["b2"], st["bg"], "pref_prev")
        assert beyond(st["emu"]["ws"], bad["wsum"], bad["mag_chain_w"], "chain") > 1.0, name


@pytest.mark.parametrize("drop", ["a_lo_b_hi", "a_hi_b_lo"])
def test_dropped_mfma_product_is_beyond_the_bound(drop):
    """the reference without one of the three products, against the emulation with all three"""
    worst = 0.0
    for name in ALL:
        st = head_stages(name, 32)
        bad = st["ref"]["fg"] - hs.mfma_terms64(st["emu"]["G"], st["W2"])[drop]
        worst = max(worst, beyond(st["emu"]["fg_mfma"], bad, st["ref"]["mag_fg"], "fg_mfma"))
    print("fault %s: largest deviation = %.3g x bound" % (drop, worst))
    assert worst > 1.0


def test_rgb0_label_fault_is_beyond_the_bound():
    worst = 0.0
    for name in ALL:
        st = head_stages(name, 32)
        ref, mag = hs.rgb0_ref(st["emu"]["merge_mfma"], st["ci"]["w3"], st["ci"]["b3"], "label")
        worst = max(worst, beyond(st["emu"]["rgb0"], ref, mag, "rgb0"))
    print("fault rgb0 label: largest deviation = %.3g x bound" % worst)
    assert worst > 1.0


def test_fold_without_br0_is_beyond_the_bound():
    worst = 0.0
    for name in WEIGHT_SETS:
        ci = hs.case_inputs(name)
        a = (ci["ws"], ci["bs"], ci["codes"], ci["S"], ci["A"], ci["U"], True)
        bad, _, exact = hs.fold_ref(*a, fault="no_br0")
        _, mag, _ = hs.fold_ref(*a)
        worst = max(worst, beyond(hs.fold_emul(*a)[:, ~exact], bad[:, ~exact], mag[:, ~exact], "fold"))
    print("fault merged fold without Wr1[:, :384] . br0: largest deviation = %.3g x bound" % worst)
    assert worst > 1.0


@pytest.mark.parametrize("fault,precisions", [("zero63", ("fp32", "bf16", "fp16", "bf16x3")), ("skip", ("fp32", "bf16", "fp16", "bf16x3")),
                                              ("swap", ("bf16x3",))])
def test_pack_fault_changes_bits(fault, precisions):
    """the packed weights are held bit for bit, so a fault is detected as soon as it changes one byte -- and it changes thousands"""
    for name in ("ragged", "gaze"):
        ci = hs.case_inputs(name)
        wm = hs.merged_matrix32(ci["ws"])
        for prec in precisions:
            good, _ = hs.pack_expected(ci["ws"], ci["bs"], ci["S"], hs.PRECS[prec], wm, 0xA5)
            bad, _ = hs.pack_expected(ci["ws"], ci["bs"], ci["S"], hs.PRECS[prec], wm, 0xA5, fault)
            n = int((good != bad).sum())
            print("fault %s %s %s: %d bytes differ" % (fault, name, prec, n))
            assert n >= 384
