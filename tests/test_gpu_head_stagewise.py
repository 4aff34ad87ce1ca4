"""The kernels around the fused MLP kernel in the inference forward (csrc/nerf_aux.hip: pack_mlp / pack_tail / small_gemm, fold_latents,
rayfold, ray_vd_bias, chw_to_hwc and the three per-ray heads) pinned per entry from what they leave in the caller-owned workspace and
the packed buffer -- see tests/head_stagewise.py for the layouts, the comparison rule and the floors, all of which come from the CPU
alone (test_head_stagewise_cpu.py re-measures them).  Every bound here is 4 x one of those floors; nothing is taken from a GPU run.

One synchronised call per (case, precision, output set, background layout, prefill) through ops.pack_mlp and ops.render_fwd with
`ws=` a prefilled buffer; merge_out / weight_out / merge16_out / rgb0_out are prefilled too (fg_feat, bg_alpha and depth are
allocated inside ops.render_fwd: every float of theirs is compared with a reference instead).  Cached per process.

Cases (free ray sets of an 8 x 8 grid, `batch_xy[:, :, rays]`; B x rays x samples):
  one       1 x  1 x   32   fewer rays than either workgroup (8 / 32): min(ray0 + rr, total - 1) clamps everywhere
  ragged    3 x  7 x   40   21 rays: ragged last workgroup; 16-bit bpr = 2 with 8 live samples in block 2; fp32 bpr = 3; three frames
                            with different codes inside one 32-ray workgroup
  span      3 x 45 x   65   135 = 4 x 32 + 7 rays: workgroups that begin mid-frame (background row rg % n_rays); 16-bit bpr = 3 (the
                            general loop, one live sample in the last block); fp32 bpr = 5
  full      2 x 32 x   32   whole workgroups; bpr = 1; fp32 bpr = 2
  deep      1 x  2 x 1024   fp32 bpr = 64 = HEAD_MAX_BPR; 16-bit bpr = 32
  contrast  ragged with contrast_state_dict: saturating alpha, tprod down to 1e-32 (0 over a 32-sample block), pref underflowing
  gaze      ragged with include_gaze, eye_gaze_dim = 64, audio_dim = 0: other fold offsets and logical_weight columns
  vd        ragged with include_vd: ray_vd_bias, rayfold, the per-ray table behind the fold table
Output sets: fg | merge | all (fg + merge + depth + weight + bg_alpha) | map16 (merge16 + rgb0 alone, the inference forward's call) |
both (merge16 + rgb0 + merge_out + fg + depth + weight: both instantiations in one call); bf16x3 takes the f16 map type."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import head_stagewise as hs

pytestmark = pytest.mark.gpu

ALL = list(hs.CASES)
PRECISIONS = ["fp32", "bf16", "fp16", "bf16x3"]
SETS32 = ("fg", "merge", "all")
SETS16 = ("fg", "merge", "all", "map16", "both")
WORST = {}   # family -> (worst / bound, where): filled by every comparison, printed by test_report


def dev():
    return torch.device("cuda:0")


def sets_of(prec):
    return SETS32 if prec == "fp32" else SETS16


def filled(shape, dtype, fill):
    n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    return torch.full((n,), fill, dtype=torch.uint8, device=dev()).view(dtype).view(shape)


@functools.lru_cache(maxsize=None)
def device_inputs(name):
    from n3dt import ops
    ci = hs.case_inputs(name)
    inp = ci["inp"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev())
    d = {"xy": inp["batch_xy"].to(dev()).contiguous(), "R": ops._f32c(inp["batch_Rmats"].to(dev())),
         "T": ops._f32c(inp["batch_Tvecs"].to(dev())).view(ci["B"], 3), "Kinv": ops._f32c(inp["batch_inv_inmats"].to(dev())),
         "shape": t(ci["codes"][0]), "appea": t(ci["codes"][1]), "audio": t(ci["codes"][2]) if ci["U"] > 0 else None,
         "ws": [t(w) for w in ci["ws"]], "bs": [t(b) for b in ci["bs"]], "w10_full": t(ci["w10_full"]),
         "bg": {0: t(ci["bg_chw"]), 1: t(ci["bg_hwc"])}, "w3": t(ci["w3"]), "b3": t(ci["b3"]),
         "planes": t(ci["planes"]) if ci["planes"] is not None else None}   # the hierarchical cases: z_planes_given, passed as t_rand
    d["params"] = ops.mlp_params(d["ws"], d["bs"])
    return d


def make_geom(ci, d, hwc):
    from n3dt import ops
    return ops.make_geom(ci["B"], ci["n_rays"], ci["Ns"], 384, 256, ci["S"], ci["A"], ci["U"], hs.FEATMAP_SIZE, 2, ci["opt"].world_z1,
                         ci["opt"].world_z2, d["xy"].stride(), int(ci["planes"] is not None), hwc, vd_dim=ci["vd"])


@functools.lru_cache(maxsize=None)
def packed(name, prec, fill=0xA5):
    """(device buffer, its bytes) of n3dt_mlp_pack over a prefilled buffer of exactly n3dt_mlp_packed_bytes"""
    from n3dt import ops
    from n3dt._lib import lib
    ci, d, p = hs.case_inputs(name), device_inputs(name), hs.PRECS[prec]
    geom = make_geom(ci, d, 1)
    n = hs.packed_bytes(p)
    assert n == lib().n3dt_mlp_packed_bytes(ctypes.byref(geom), p)
    buf = torch.full((n,), fill, dtype=torch.uint8, device=dev())
    out = ops.pack_mlp(geom, p, d["params"], dev(), out=buf)
    torch.cuda.synchronize()
    assert out.data_ptr() == buf.data_ptr()
    return buf, buf.cpu().numpy()


@functools.lru_cache(maxsize=None)
def run(name, prec, outset, hwc=1, fill=0x00, rep=0):
    """one render call; returns the workspace bytes, its carved regions and every output as numpy"""
    from n3dt import ops
    ci, d, p = hs.case_inputs(name), device_inputs(name), hs.PRECS[prec]
    B, n_rays, Ns = ci["B"], ci["n_rays"], ci["Ns"]
    geom = make_geom(ci, d, hwc)
    carve = hs.render_carve(B, n_rays, Ns, p, ci["vd"])
    assert carve["total"] == ops.render_workspace_bytes(geom, p)
    ws = torch.full((carve["total"],), fill, dtype=torch.uint8, device=dev())
    ray_bias = sample = None
    if ci["vd"]:
        ray_bias = ops.ray_vd_bias(geom, d["w10_full"], d["xy"], d["R"], d["Kinv"], out=filled((B, n_rays, hs.G), torch.float32, fill))
        sample = ops.sample_points(geom, d["xy"], d["R"], d["T"], d["Kinv"])["ray_d"]
    kw = dict(want_fg=outset in ("fg", "all", "both"), want_merge=outset != "fg", want_depth=outset in ("all", "both"),
              want_weight=outset in ("all", "both"))
    if kw["want_merge"] and outset != "map16":
        kw["merge_out"] = filled((B, n_rays, hs.C), torch.float32, fill)
    if kw["want_weight"]:
        kw["weight_out"] = filled((B, n_rays, Ns), torch.float32, fill)
    if outset in ("map16", "both"):
        dt16 = torch.bfloat16 if hs.MAP16[p] == "bf16" else torch.float16
        kw.update(merge16_out=filled((B, n_rays, hs.C), dt16, fill), rgb0_out=filled((B, 3, n_rays), torch.float32, fill), rgb0_wb=(d["w3"], d["b3"]))
    out = ops.render_fwd(geom, p, packed(name, prec)[0], d["params"], d["xy"], d["R"], d["T"], d["Kinv"], d["shape"], d["appea"], d["audio"], d["planes"],
                         d["bg"][hwc] if kw["want_merge"] else None, ws=ws, ray_bias=ray_bias, **kw)
    torch.cuda.synchronize()
    raw = ws.cpu().numpy()
    R = B * n_rays
    r = {"carve": carve, "raw": raw, "ci": ci, "p": p, "R": R,
         "fold": raw[:B * hs.FOLD_STRIDE * 4].view(np.float32).reshape(B, hs.FOLD_STRIDE),
         "part": raw[carve["part"]:carve["part"] + carve["part_used"]].view(np.float32).reshape(R, carve["bpr"], hs.PART_STRIDE),
         "wlocal": raw[carve["wlocal"]:carve["wlocal"] + carve["wlocal_used"]].view(np.float32).reshape(R, carve["bpr"], carve["bs"]),
         "bghwc": raw[carve["bghwc"]:carve["bghwc"] + carve["bghwc_used"]].view(np.float32).reshape(n_rays, hs.C)}
    if ci["vd"]:
        o = 4 * hs.rayfold_offset(B)
        r["rayfold"] = raw[o:o + R * hs.RAYFOLD_STRIDE * 4].view(np.float32).reshape(R, hs.RAYFOLD_STRIDE)
        r["ray_bias"] = ray_bias.cpu().numpy().reshape(R, hs.G)
        r["ray_d"] = np.moveaxis(sample.cpu().numpy(), 1, 2).reshape(R, 3)
    for k, v in out.items():
        if v is None or k == "merge_feat16":
            continue
        r[k] = v.cpu().numpy().reshape((R, -1) if k in ("fg_feat", "merge_feat", "weight") else (B, 3, n_rays) if k == "rgb0" else (R,))
    if out.get("merge_feat16") is not None:
        r["merge16"] = out["merge_feat16"].contiguous().view(torch.int16).cpu().numpy().view(np.uint16).reshape(R, hs.C)
    return r


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else a.dtype)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def held(tag, family, got, ref, mag, extra=0.0):
    """prints the figure, records it for the report, then judges it"""
    q = hs.report(tag, family, hs.ratio(got, ref, mag, extra))
    if family not in WORST or q > WORST[family][0]:
        WORST[family] = (q, tag)
    assert q <= 1.0, (tag, family, q)


def pattern(n, fill):
    return np.full(n, fill, dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------------------------
# packed weights
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("name", ["ragged", "gaze", "vd"])
def test_packed_weights(name, prec):
    """Every byte of the n3dt_mlp_pack buffer: each stage's element decoded through the restated index map holds the logical weight
    (fp32), its RNE bf16 / IEEE half rounding, or bf16(W) and bf16(W - bf16(W)) in pieces 2P and 2P + 1; the merged stage is the same
    rounding of the tail's own float32 W_m; W2^T, b2 and the hi / lo fragments likewise; stage 10's slot of the 16-bit buffers and the
    unused second half of their stage-9 slot, the fp32 buffer's W_m slot and every padding byte keep the prefill.  W_m itself is held per entry to U_wm sum |a b|."""
    ci, p = hs.case_inputs(name), hs.PRECS[prec]
    got = packed(name, prec)[1]
    region = hs.packed_region_bytes(p)
    wm = got[region + 4 * hs.TAIL_WM:region + 4 * hs.TAIL_FRAGS].view(np.float32).reshape(hs.G, hs.HID)
    exp, written = hs.pack_expected(ci["ws"], ci["bs"], ci["S"], p, wm, 0xA5)
    bad = np.flatnonzero(got != exp)
    print("%s %s: %d bytes, %d written by the kernels, %d keep the prefill, %d differ" % (name, prec, got.size, written, got.size - written, bad.size))
    assert bad.size == 0, "first differing byte %d (matrix region ends at %d)" % (bad[0], region)
    if p != hs.F32:
        ref, mag = hs.merged_matrix64(ci["ws"])
        held("%s %s W_m" % (name, prec), "wm", wm, ref, mag)
        # the density stage: rows 1..31 and column 63 of L0 / L5 are zero in the decoded logical matrices
        mat = got[:region].view(np.uint16)
        if p == hs.BF16X3:
            mat = mat.reshape(-1, 2, 512)[:, 0].reshape(-1)     # the hi pieces
        for s, rows, cols in ((8, slice(1, 32), slice(0, 384)), (0, slice(0, 384), slice(63, 64)), (5, slice(0, 384), slice(63, 64))):
            N, K, _ = hs.stage_dims(s)
            row, col = hs.pack_index_map(N, K, p)
            W = np.zeros((N, K), dtype=np.uint16)
            W[row, col] = mat[hs.stage_offset(s):hs.stage_offset(s) + N * K]
            assert not W[rows, cols].any(), "stage %d" % s
    else:
        assert np.array_equal(got[region + 4 * hs.TAIL_WM:region + 4 * hs.TAIL_FRAGS], pattern(4 * hs.G * hs.HID, 0xA5)), "fp32 forms no W_m"


# ---------------------------------------------------------------------------------------------------------------------
# fold table, view-direction bias, rayfold, background transpose
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("name", ALL)
def test_fold_table(name, prec):
    """every float of every frame's row: folded entries per entry (merged form in the 16-bit precisions), copies and the density tile
    bitwise, the unused end of the row and the region's padding untouched"""
    r = run(name, prec, "all")
    ci, p = r["ci"], r["p"]
    ref, mag, exact = hs.fold_ref(ci["ws"], ci["bs"], ci["codes"], ci["S"], ci["A"], ci["U"], merged=p != hs.F32)
    got = r["fold"]
    held("%s %s fold" % (name, prec), "fold", got[:, :hs.FOLD_USED][:, ~exact], ref[:, ~exact], mag[:, ~exact])
    assert same_bits(got[:, :hs.FOLD_USED][:, exact], np.broadcast_to(ref[0, exact].astype(np.float32), (ci["B"], int(exact.sum()))))
    assert not bits(got[:, hs.FOLD_USED:]).any(), "the end of a row is never written (zero prefill)"


@pytest.mark.parametrize("prec", PRECISIONS)
def test_view_direction_bias_and_rayfold(prec):
    r = run("vd", prec, "all")
    ci = r["ci"]
    ref, mag = hs.vd_ref(ci["w_vd"], r["ray_d"])
    held("vd %s ray_vd_bias" % prec, "vd", r["ray_bias"], ref, mag)
    frame = np.arange(r["R"]) // ci["n_rays"]
    o = hs.bias_offset(10)
    assert same_bits(r["rayfold"], r["fold"][frame, o:o + hs.G] + r["ray_bias"]), "rayfold = fold entry + ray_bias, one float32 add"
    # ... and the directions the kernel used are the ones the CPU forms (a cross-check of the reference's own input)
    d_cpu = hs.directions32(ci).reshape(-1, 3)
    print("vd %s: max |ray_d(GPU) - ray_d(CPU float32)| = %.3e" % (prec, np.abs(r["ray_d"] - d_cpu).max()))
    assert np.abs(r["ray_d"] - d_cpu).max() <= 2.0 ** -22


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("name", ["ragged", "span"])
def test_background_transpose(name, prec):
    """bghwc = the [C][N_r] parameter transposed, bit for bit; untouched when the caller's map is ray-major already or nothing merges"""
    ci = hs.case_inputs(name)
    for outset in ("merge", "all") + (("map16",) if prec != "fp32" else ()):
        assert same_bits(run(name, prec, outset, hwc=0)["bghwc"], ci["bg_hwc"]), outset
    for outset, hwc in (("fg", 0), ("fg", 1), ("all", 1), ("merge", 1)):
        assert not bits(run(name, prec, outset, hwc=hwc)["bghwc"]).any(), (outset, hwc)


# ---------------------------------------------------------------------------------------------------------------------
# what the fused kernels leave for the head
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("name", ALL)
def test_part_and_wlocal_invariants(name, prec):
    r = run(name, prec, "all")
    part, wl, c, Ns = r["part"], r["wlocal"], r["carve"], r["ci"]["Ns"]
    assert np.isfinite(part).all() and np.isfinite(wl).all()
    assert not bits(part[:, :, hs.G + 3]).any(), "part[G + 3] == 0"
    lanes = np.arange(c["bpr"] * c["bs"]).reshape(c["bpr"], c["bs"])
    assert not bits(wl[:, lanes >= Ns]).any(), "wlocal beyond n_samples is exactly 0"
    held("%s %s part[G + 0] vs sum wlocal" % (name, prec), "block", part[:, :, hs.G], hs.f64(wl).sum(2), np.abs(hs.f64(wl)).sum(2))
    assert np.all(part[:, :, hs.G + 2] >= 0) and np.all(part[:, :, hs.G + 2] <= 1.0)
    # weight not requested: wlocal keeps the prefill, part is the same
    q = run(name, prec, "merge")
    assert not bits(q["wlocal"]).any() and same_bits(q["part"], part)


# ---------------------------------------------------------------------------------------------------------------------
# the head, every form
# ---------------------------------------------------------------------------------------------------------------------
def check_head(tag, r, form):
    """every requested output of one call against float64 of the call's own part / wlocal / background rows"""
    ci = r["ci"]
    bg = hs.bg_rows(ci["bg_hwc"], r["R"], ci["n_rays"])
    ref = hs.head_ref(r["part"], ci["ws"][11], ci["bs"][11], bg)
    if "fg_feat" in r:
        held(tag + " fg_feat", hs.family_of(ci["name"], "fg_" + form), r["fg_feat"], ref["fg"], ref["mag_fg"])
    if "merge_feat" in r:
        held(tag + " merge_feat", "merge_" + form, r["merge_feat"], ref["merge"], ref["mag_merge"])
    if "bg_alpha" in r:
        held(tag + " bg_alpha", "chain", r["bg_alpha"], ref["bg_alpha"], ref["mag_chain_w"], extra=hs.ONE_ULP)
        assert np.all(np.abs(hs.f64(r["bg_alpha"]) - ref["bg_alpha"]) <= hs.bound_bg_alpha(ref["mag_chain_w"]))
    if "depth" in r:
        held(tag + " depth", "chain", r["depth"], ref["dsum"], ref["mag_chain_d"])
    if "weight" in r:
        assert same_bits(r["weight"], hs.weight_expected(r["part"], r["wlocal"], ci["Ns"], r["carve"]["bs"])), tag + " weight"
    for k in ("fg_feat", "merge_feat", "bg_alpha", "depth", "weight", "rgb0"):
        assert k not in r or np.isfinite(r[k]).all(), (tag, k)
    if "merge16" in r and "merge_feat" in r:
        assert np.array_equal(r["merge16"], hs.round_bits(r["merge_feat"], hs.MAP16[r["p"]])), tag + " merge16 = 16-bit rounding of merge_out"
    if "rgb0" in r and "merge_feat" in r:
        rr, mag = hs.rgb0_ref(r["merge_feat"], ci["w3"], ci["b3"])
        got = np.moveaxis(r["rgb0"], 1, 2).reshape(r["R"], 3)
        held(tag + " rgb0", "rgb0", got, rr, mag)


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("name", ALL)
def test_head_per_entry(name, prec):
    form = "fma" if prec == "fp32" else "mfma"
    for outset in sets_of(prec):
        check_head("%s %s %s" % (name, prec, outset), run(name, prec, outset), form)
    if prec != "fp32":
        alone, both = run(name, prec, "map16"), run(name, prec, "both")
        assert "merge_feat" not in alone and "fg_feat" not in alone
        assert np.array_equal(alone["merge16"], both["merge16"]) and same_bits(alone["rgb0"], both["rgb0"]), "map16 alone = map16 with the fp32 maps"


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("name", ["ragged", "span"])
def test_head_with_the_channel_major_background(name, prec):
    """bg_is_hwc = 0: the head reads the transposed copy and gives the bits of the ray-major call"""
    form = "fma" if prec == "fp32" else "mfma"
    for outset in [s for s in sets_of(prec) if s != "fg"]:
        a, b = run(name, prec, outset, hwc=0), run(name, prec, outset, hwc=1)
        check_head("%s %s %s chw" % (name, prec, outset), a, form)
        for k in ("merge_feat", "merge16", "rgb0", "fg_feat", "bg_alpha", "depth", "weight"):
            assert (k in a) == (k in b) and (k not in a or same_bits(a[k], b[k])), (outset, k)


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("name", ALL)
def test_same_bits_across_output_sets(name, prec):
    full = run(name, prec, "all")
    assert same_bits(run(name, prec, "fg")["fg_feat"], full["fg_feat"]) and same_bits(run(name, prec, "fg")["bg_alpha"], full["bg_alpha"])
    assert same_bits(run(name, prec, "merge")["merge_feat"], full["merge_feat"])
    if prec != "fp32":
        both = run(name, prec, "both")
        for k in ("fg_feat", "merge_feat", "bg_alpha", "depth", "weight"):
            assert same_bits(both[k], full[k]), k


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("name", ALL)
def test_prefill_and_rerun(name, prec):
    """0xFF prefill of the workspace and the caller-owned outputs: the bits of the run over zeros, every requested float finite, every
    workspace byte outside the four regions still 0xFF; and a second run over zeros repeats the first bit for bit (nothing is atomic)"""
    outset = "all" if prec == "fp32" else "both"
    a, f, again = run(name, prec, outset), run(name, prec, outset, fill=0xFF), run(name, prec, outset, rep=1)
    c, ci = a["carve"], a["ci"]
    keys = [k for k in ("fg_feat", "merge_feat", "bg_alpha", "depth", "weight", "rgb0", "merge16", "part", "wlocal") if k in a]
    for k in keys:
        assert same_bits(a[k], f[k]), "0xFF prefill: " + k
        assert same_bits(a[k], again[k]), "second run: " + k
        assert k == "merge16" or np.isfinite(f[k]).all(), k
    assert same_bits(a["fold"][:, :hs.FOLD_USED], f["fold"][:, :hs.FOLD_USED]) and same_bits(a["raw"], again["raw"])
    keep = np.ones(c["total"], dtype=bool)
    fold_rows = (np.arange(ci["B"])[:, None] * hs.FOLD_STRIDE + np.arange(hs.FOLD_USED)[None, :]).reshape(-1)
    keep[(4 * fold_rows[:, None] + np.arange(4)[None, :]).reshape(-1)] = False
    if ci["vd"]:
        keep[4 * hs.rayfold_offset(ci["B"]):c["fold_used"]] = False
    keep[c["part"]:c["part"] + c["part_used"]] = False
    keep[c["wlocal"]:c["wlocal"] + c["wlocal_used"]] = False
    # (bghwc: the caller's map is ray-major in this call, so the region is not written either)
    assert np.all(f["raw"][keep] == 0xFF), "%d bytes outside the regions changed" % int((f["raw"][keep] != 0xFF).sum())
    assert not np.any(np.all(f["raw"][~keep].reshape(-1, 4) == 0xFF, axis=1)), "a float inside a region was left unwritten"


def test_every_laid_out_float_is_compared():
    """Coverage accounting, case span / bf16 / `both` and its packed buffer: every float of the fold region, part, wlocal, bghwc, the
    packed buffer and every requested output is compared by a test above or asserted to hold the prefill."""
    r = run("span", "bf16", "both")
    c, ci = r["carve"], r["ci"]
    B, R = ci["B"], r["R"]
    fold_cmp, fold_pre = B * hs.FOLD_USED, B * (hs.FOLD_STRIDE - hs.FOLD_USED)
    assert fold_cmp + fold_pre == c["fold_used"] // 4                                        # test_fold_table, every entry or prefill
    part_cmp = {"G -> fg / merge (head_ref)": R * c["bpr"] * hs.G, "wsum, depth, tprod (chain) and the zero": R * c["bpr"] * 4}
    assert sum(part_cmp.values()) == c["part_used"] // 4                                     # test_head_per_entry + invariants
    assert R * c["bpr"] * c["bs"] == c["wlocal_used"] // 4                                   # weight bitwise + invariants
    assert ci["n_rays"] * hs.C == c["bghwc_used"] // 4                                       # test_background_transpose / prefill
    pad = c["total"] - (c["fold_used"] + c["part_used"] + c["wlocal_used"] + c["bghwc_used"])
    assert 0 <= pad < 4 * 256                                                                # test_prefill_and_rerun
    _, written = hs.pack_expected(ci["ws"], ci["bs"], ci["S"], hs.BF16, np.zeros((hs.G, hs.HID), np.float32), 0)
    total = hs.packed_bytes(hs.BF16)
    # 16-bit buffers: the merged 192 x 384 matrix fills half of stage 9's 384 x 384 slot; its other half and stage 10's slot are unused
    unused = 2 * (hs.HID * hs.HID - hs.G * hs.HID) + 2 * hs.G * hs.HID + (hs.packed_region_bytes(hs.BF16) - 2 * hs.MATRIX_ELEMS)
    assert written + unused == total                                                         # test_packed_weights, bitwise or prefill
    outs = {"fg_feat": R * hs.C, "merge_feat": R * hs.C, "bg_alpha": R, "depth": R, "weight": R * ci["Ns"], "rgb0": 3 * R, "merge16": R * hs.C}
    assert all(r[k].size == n for k, n in outs.items())
    print("span bf16 both: fold %d compared + %d prefill, part %d, wlocal %d, bghwc %d, padding %d bytes, packed %d bytes (%d written), outputs %d"
          % (fold_cmp, fold_pre, c["part_used"] // 4, c["wlocal_used"] // 4, c["bghwc_used"] // 4, pad, total, written, sum(outs.values())))


def test_report():
    """the largest error per family in units of its bound, over everything compared in this process (run last; prints only)"""
    for family in sorted(WORST):
        print("%-12s worst / bound = %.3f   (%s)" % (family, WORST[family][0], WORST[family][1]))
