"""CPU side of the stagewise pin of the exact fp32 volumetric training path (tests/f32_stagewise.py): the restatement against
torch float64 autograd of the same function written plainly, the layouts and the split planner, the floors every GPU bound is
four times of -- re-measured here on the float32 emulation -- and the deliberate faults the GPU bounds must report."""
import functools

import numpy as np
import pytest
import torch

import f32_stagewise as fs

SEEDS = (0, 1, 2)
ALL = list(fs.CASES)


@functools.lru_cache(maxsize=None)
def emulated(name, seed=0, variant="full"):
    inp = fs.case_inputs(name, seed, variant)
    return inp, fs.run_path(inp, np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# layout and planner
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_layout_totals_against_the_library(name):
    from n3dt import ops
    c = fs.CASES[name]
    opt = fs.case_options()
    S = opt.iden_code_dims + opt.expr_code_dims + (c["kw"].get("eye_gaze_dim", 0) if c["kw"].get("include_gaze") else 0)
    geom = ops.make_geom(c["B"], c["n_rays"], c["n_samples"], 384, 256, S, opt.text_code_dims + opt.illu_code_dims, c["kw"].get("audio_dim", 64),
                         fs.FEATMAP_SIZE, 2, opt.world_z1, opt.world_z2, vd_dim=c["vd"])
    saved, ws, saved_bytes = fs.library_totals(geom)
    assert saved == fs.saved_layout(c["B"], c["n_rays"], c["n_samples"], c["vd"])["total"]
    assert ws == fs.ws_layout(c["B"], c["n_rays"], c["n_samples"])["total"]
    assert saved_bytes >= 4 * saved


def test_the_cases_reach_what_they_are_there_for():
    """the derived numbers of every case from a restatement of split_for and the slice length: a change of planner cannot
    silently empty a case"""
    P = {k: c["B"] * c["n_rays"] * c["n_samples"] for k, c in fs.CASES.items()}
    ppf = {k: c["n_rays"] * c["n_samples"] for k, c in fs.CASES.items()}
    assert P["a"] == 768 and P["a"] % 128 == 0 and ppf["a"] % 128 == 0 and fs.split_for(P["a"]) == 1
    assert P["tail"] == 360 and P["tail"] % 128 == 104
    assert P["frames"] == 2000 and ppf["frames"] == 1000 and ppf["frames"] % 128 != 0 and fs.split_for(P["frames"]) == 1
    assert P["split"] == 4830 and ppf["split"] == 2415
    split = fs.split_for(P["split"])
    per = fs.slice_rows(P["split"], split)
    assert (split, per) == (2, 2416) and per % 16 == 0
    assert [min(P["split"], (z + 1) * per) - z * per for z in range(split)] == [2416, 2414] and 2414 % 16 == 14
    assert per - ppf["split"] == 1                                   # the slice boundary is one row off the frame boundary
    assert [min(64, 105 - s0) for s0 in range(0, 105, 64)] == [64, 41]
    assert [min(64, 130 - s0) for s0 in range(0, 130, 64)] == [64, 64, 2]
    assert fs.CASES["vd"]["n_samples"] == 40 and 128 % 40 != 0 and fs.CASES["vd"]["vd"] > 0
    assert fs.split_for(2047) == 1 and fs.split_for(2048) == 1 and fs.split_for(4096) == 2 and fs.split_for(10 ** 9) == 128


# ---------------------------------------------------------------------------------------------------------------------
# the restatement against torch float64 autograd of the function written plainly
# ---------------------------------------------------------------------------------------------------------------------
def autograd_reference(inp):
    """MLP with skip and latent concatenation, compositing, merge -- float64 torch, gradients by autograd of
    sum(d_merge merge) + sum(d_fg fg) + sum(d_ba bg_alpha)."""
    t = lambda a, g=True: torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=g)  # noqa: E731
    B, n_rays, Ns = inp["B"], inp["n_rays"], inp["Ns"]
    W, b = [t(w) for w in inp["W"]], [t(v) for v in inp["b"]]
    shape, appea = t(inp["shape"]), t(inp["appea"])
    audio = t(inp["audio"]) if inp["audio"] is not None else None
    xy, R, T, Kinv, bg = t(inp["xy"]), t(inp["R"]), t(inp["T"]), t(inp["Kinv"]), t(inp["bg"])
    rb = t(inp["ray_bias"]) if inp["ray_bias"] is not None else None
    t_rand = t(inp["t_rand"], False) if inp["t_rand"] is not None else torch.zeros(B, n_rays, Ns + 1, dtype=torch.float64)
    h = torch.cat([xy, torch.ones(B, 1, n_rays, dtype=torch.float64)], dim=1)
    w = R @ (Kinv @ h)
    d = w / w.norm(dim=1, keepdim=True)                                      # [B, 3, rays]
    l = -1.0 / d[:, 2]
    lin = torch.linspace(0.0, 1.0, Ns + 1, dtype=torch.float64)
    zv = (T[:, 2:3] - inp["z1"]) * (1.0 - lin)[None] + (T[:, 2:3] - inp["z2"]) * lin[None]
    mid = 0.5 * (zv[:, 1:] + zv[:, :-1])
    lower, upper = torch.cat([zv[:, :1], mid], dim=1), torch.cat([mid, zv[:, -1:]], dim=1)
    z = lower[:, None] + (upper - lower)[:, None] * t_rand                   # [B, rays, Ns + 1]
    if inp.get("planes") is not None:   # the hierarchical pass: the planes are data that move with T_z (d plane / d T_z = 1, train_mlp.hip:401-411)
        z = t(inp["planes"], False) + (T[:, 2] - T[:, 2].detach())[:, None, None]
    dist = (z[..., 1:] - z[..., :-1]) * l[..., None]
    pts = T[:, None, None, :] + (d.transpose(1, 2) * l[..., None])[:, :, None, :] * z[..., :-1, None]
    pe = torch.cat([pts] + [f(pts * 2.0 ** k) for k in range(10) for f in (torch.sin, torch.cos)], dim=-1)   # [B, rays, Ns, 63]
    ex = lambda c: c[:, None, None, :].expand(B, n_rays, Ns, c.shape[1])  # noqa: E731
    vp = torch.cat([pe, ex(shape)], dim=-1)
    x = torch.cat([vp, ex(audio)], dim=-1) if audio is not None else vp
    for i in range(8):
        if i == 5:
            x = torch.cat([vp, x], dim=-1)
        x = torch.relu(x @ W[i].T + b[i])
    sigma = torch.relu(x @ W[8].T + b[8])[..., 0]
    r0 = x @ W[9].T + b[9]
    pre = r0 @ W[10][:, :384].T + ex(appea) @ W[10][:, 384:].T + b[10]
    if rb is not None:
        pre = pre + rb[:, :, None, :]
    feat = torch.relu(pre) @ W[11].T + b[11]                                # [B, rays, Ns, 256]
    alpha = 1.0 - torch.exp(-sigma * dist)
    xx = 1.0 - alpha + 1e-10
    Tt = torch.cat([torch.ones(B, n_rays, 1, dtype=torch.float64), torch.cumprod(xx, dim=-1)[..., :-1]], dim=-1)
    wgt = alpha * Tt
    fg = (wgt[..., None] * feat).sum(dim=2)
    ba = 1.0 - wgt.sum(dim=2)
    merge = fg + ba[..., None] * bg.T[None]
    loss = (merge * t(inp["d_merge"], False)).sum()
    if inp["d_fg"] is not None:
        loss = loss + (fg * t(inp["d_fg"], False)).sum() + (ba * t(inp["d_ba"], False)).sum()
    loss.backward()
    g = lambda v: None if v is None else (v.grad.numpy() if v.grad is not None else np.zeros(v.shape))  # noqa: E731
    return {"fg_feat": fg.detach().numpy(), "bg_alpha": ba.detach().numpy(), "merge_feat": merge.detach().numpy(), "gw": [g(v) for v in W], "gb": [g(v) for v in b],
            "d_shape": g(shape), "d_appea": g(appea), "d_audio": g(audio), "d_bg": g(bg), "d_ray_bias": g(rb), "d_R": g(R), "d_T": g(T), "d_Kinv": g(Kinv),
            "d_xy": g(xy)}


E2E = [(n, "full") for n in ALL] + [("a", "dfg"), ("tail", "dfg")]


@pytest.mark.parametrize("name,variant", E2E)
def test_restatement_end_to_end_against_torch_autograd(name, variant):
    """The path of f32_stagewise.run_path in float64 (the same code the float32 emulation runs) against autograd: every output and
    gradient within 1e-12 of S per entry, S the magnitude the stage check of that entry carries."""
    inp = fs.case_inputs(name, 0, variant)
    rec = fs.run_path(inp, np.float64)
    ref = autograd_reference(inp)
    S_of = {}
    for c in fs.stages(inp, rec):
        e = fs.evaluate(c, u=1e-12)
        assert e["bad"] == 0, (c["tag"], e["ratio"])        # the restatement agrees with itself stage by stage
        S_of[c["tag"]] = np.broadcast_to(c["S"] if c["Sc"] is None else c["Sc"], c["z"].shape)
    S_ = inp["S"]
    pairs = [("fg_feat", rec["out"]["fg_feat"], ref["fg_feat"], S_of["fg_feat"]), ("merge_feat", rec["out"]["merge_feat"], ref["merge_feat"], S_of["merge_feat"]),
             ("bg_alpha", rec["out"]["bg_alpha"], ref["bg_alpha"], S_of["bg_alpha"])]
    for k in ("d_shape", "d_appea", "d_audio", "d_R", "d_T", "d_Kinv", "d_xy", "d_ray_bias"):
        if rec["res"][k] is None:
            assert ref[k] is None or k == "d_ray_bias"
            continue
        pairs.append((k, rec["res"][k], ref[k], S_of[k]))
    pairs.append(("d_bg_featmap", rec["res"]["d_bg"], ref["d_bg"], S_of["d_bg_featmap"]))
    gw, gb = rec["gw"], rec["gb"]
    for l in (1, 2, 3, 4, 6, 7):
        pairs += [("dW%d" % l, gw[l], ref["gw"][l], S_of["dW%d" % l]), ("db%d" % l, gb[l], ref["gb"][l], S_of["db%d" % l])]
    pairs += [("dW0 PE", gw[0][:, :63], ref["gw"][0][:, :63], S_of["dW0[:, PE]"]), ("dW0 latent", gw[0][:, 63:], ref["gw"][0][:, 63:], S_of["dW0[:, latent]"]),
              ("dW5 PE", gw[5][:, :63], ref["gw"][5][:, :63], S_of["dW5[:, PE]"]), ("dW5 latent", gw[5][:, 63:63 + S_], ref["gw"][5][:, 63:63 + S_], S_of["dW5[:, latent]"]),
              ("dW5 H4", gw[5][:, 63 + S_:], ref["gw"][5][:, 63 + S_:], S_of["dW5[:, H4]"]),
              ("dWd", gw[8], ref["gw"][8], S_of["dWc"][384:385]), ("dWr0", gw[9], ref["gw"][9], S_of["dWc"][:384]),
              ("dbd", gb[8], ref["gb"][8], S_of["dbc"][384:385]), ("dbr0", gb[9], ref["gb"][9], S_of["dbc"][:384]),
              ("dWr1", gw[10][:, :384], ref["gw"][10][:, :384], S_of["dWr1[:, 0:384]"]), ("dWr1 latent", gw[10][:, 384:], ref["gw"][10][:, 384:], S_of["dWr1[:, latent]"]),
              ("dW_rgb2", gw[11], ref["gw"][11], S_of["dW_rgb2"]), ("db_rgb2", gb[11], ref["gb"][11], S_of["db_rgb2"]),
              ("db0", gb[0], ref["gb"][0], S_of["db0"]), ("db5", gb[5], ref["gb"][5], S_of["db5"]), ("db10", gb[10], ref["gb"][10], S_of["db10"])]
    worst = 0.0
    for tag, got, want, S in pairs:
        got, want, S = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64).reshape(np.shape(got)), np.asarray(S).reshape(np.shape(got))
        err = np.abs(got - want)
        assert np.all(err <= 1e-12 * S + fs.ABS_SLACK), (tag, float((err / np.maximum(S, 1e-300)).max()))
        assert np.abs(want).max() > 0, tag
        worst = max(worst, float((err / np.maximum(S, 1e-300)).max()))
    print("%s %s: %d tensors, worst |restatement - autograd| / S = %.2e" % (name, variant, len(pairs), worst))


# ---------------------------------------------------------------------------------------------------------------------
# the floors
# ---------------------------------------------------------------------------------------------------------------------
def _ratio(got, z, S):
    err = np.abs(np.asarray(got, dtype=np.float64) - z)
    assert not np.any(err[S == 0] != 0)
    return float((err[S > 0] / S[S > 0]).max())


def fma_chain_floors(inp, rec, rows=48):
    """The single-fmaf chain of the fp32 MFMA, teacher-forced on sampled rows (products over the channels) and sampled output
    rows (products over the points, one slice, two and three slices added in either order), per family."""
    sv, wk = rec["saved"], rec["ws"]
    P = sv.P
    sel = np.arange(0, P, max(1, P // rows) | 1)[:rows]
    W = inp["W"]
    frame = np.arange(P) // (inp["n_rays"] * inp["Ns"])
    out = {}

    def put(fam, r):
        out[fam] = max(out.get(fam, 0.0), r)

    def rows_product(fam, X, Wm, bias=None):
        X, Wm = np.ascontiguousarray(X[sel]), np.ascontiguousarray(Wm)
        z32 = fs.mm_fma_chain(X, Wm)
        if bias is not None:
            z32 = z32 + bias[sel].astype(np.float32)
        z, S = fs.prod64(X, Wm, None if bias is None else bias[sel])
        put(fam, _ratio(z32, z, S))
    fold = np.asarray(sv.fold)
    rows_product("k63", sv.cat5[:, :63], W[0][:, :63], fold[frame, 0:384])
    rows_product("k384", sv.h[0], W[1], fold[frame, 384:768])
    rows_product("k448", sv.cat5, wk.w5p, fold[frame, fs.bias_offset(5):fs.bias_offset(5) + 384])
    rows_product("k192", wk.dg, W[10][:, :384].T)
    rows_product("k384", wk.dha, W[1].T)
    if rec["gw"] is not None:
        cols = np.arange(0, 384, 384 // 12)[:12]
        a, b = np.ascontiguousarray(np.asarray(wk.dha)[:, cols]), np.ascontiguousarray(sv.h[0])
        z, S = a.astype(np.float64).T @ b.astype(np.float64), np.abs(a.astype(np.float64)).T @ np.abs(b.astype(np.float64))
        for split in (1, 2, 3):
            per = fs.slice_rows(P, split) if split > 1 else P
            parts = [fs.mm_fma_chain(a[k0:k0 + per].T, b[k0:k0 + per].T) for k0 in range(0, P, per)]
            orders = [list(range(len(parts))), list(range(len(parts)))[::-1]] + ([[1, 0, 2]] if len(parts) == 3 else [])
            for o in orders:
                tot = np.zeros_like(parts[0])
                for i in o:
                    tot = tot + parts[i]
                put("dw", _ratio(tot, z, S))
    return out


@functools.lru_cache(maxsize=None)
def measured_floors():
    """{family: largest ratio} and the largest ambiguous share, over every case (and the extra runs of a and tail) and SEEDS"""
    from oracle import oracle as orc
    worst, amb_share = {}, 0.0
    runs = [(n, s, "full") for n in ALL for s in SEEDS] + [(n, 0, v) for n in ("a", "tail") for v in ("frozen", "dfg")]
    for name, seed, variant in runs:
        inp, rec = emulated(name, seed, variant)
        orders = [None] if fs.split_for(rec["saved"].P) == 1 else [None, [1, 0]]
        for order in orders:
            r = rec if order is None else fs.run_path(inp, np.float32, order=order)
            for c in fs.stages(inp, r):
                e = fs.evaluate(c)
                if e["exact"]:
                    assert e["bad"] == 0, (name, seed, variant, e["tag"])
                    continue
                assert np.isfinite(e["ratio"]), (name, seed, variant, e["tag"])
                worst[e["family"]] = max(worst.get(e["family"], 0.0), e["ratio"])
                if name == "hier" and e["tag"] in ("d sigma", "d dist"):
                    # the four samples between the five planes one float32 step apart have alpha below ALPHA_EDGE by construction: of
                    # 1280 samples they are 0.31 %, inside AMBIGUOUS_CAP but not a tenth of it; nothing else of the case is ambiguous here
                    assert e["ambiguous"] <= 4 and e["ambiguous"] <= fs.AMBIGUOUS_CAP * e["n"], (seed, e["tag"], e["ambiguous"])
                    continue
                amb_share = max(amb_share, e["ambiguous"] / e["n"])
        if variant == "full" and seed == 0:
            for fam, v in fma_chain_floors(inp, rec).items():
                worst[fam] = max(worst.get(fam, 0.0), v)
        if variant == "full":   # geometry: the fp32 oracle's sampler against float64
            o = orc.sample(inp["xy"], inp["R"], inp["T"], inp["Kinv"], inp["Ns"], inp["z1"], inp["z2"], inp["t_rand"])
            if inp["planes"] is not None:
                o = orc.sample_planes(inp["xy"], inp["R"], inp["T"], inp["Kinv"], inp["planes"])
            (pts, dist, zval), (S_p, S_d, S_z) = fs.sample(np.float64, inp)
            P = pts.shape[0]
            g = max(_ratio(np.moveaxis(o["pts"], 1, 3).reshape(P, 3), pts, S_p), _ratio(o["z_dists"][:, 0].reshape(P), dist, S_d),
                    _ratio(o["zvals"][:, 0].reshape(P), zval, S_z))
            worst["geo"] = max(worst.get("geo", 0.0), g)
    return worst, amb_share


def test_floors():
    """Every recorded floor is at least the measured one and less than twice it; the emulation leaves at most a tenth of the
    ambiguity cap on every stage of every case."""
    worst, amb_share = measured_floors()
    for fam in sorted(fs.FLOOR):
        print("%-16s measured %.3e  recorded floor %.3e  bound %.3e" % (fam, worst.get(fam, float("nan")), fs.FLOOR[fam], fs.bound(fam)))
    print("largest ambiguous share of a stage: %.5f %% (cap %.3f %%)" % (100 * amb_share, 100 * fs.AMBIGUOUS_CAP))
    assert set(worst) == set(fs.FLOOR), set(worst) ^ set(fs.FLOOR)
    for fam, v in worst.items():
        assert v <= fs.FLOOR[fam] < 2.0 * v, (fam, v, fs.FLOOR[fam])
    assert fs.FACTOR == 4.0
    assert amb_share <= 0.1 * fs.AMBIGUOUS_CAP


# ---------------------------------------------------------------------------------------------------------------------
# deliberate faults at the GPU bounds
# ---------------------------------------------------------------------------------------------------------------------
FAULTS = [("carry", "chunks3"), ("carry", "split"), ("trun", "split"), ("bias_row_tile", "frames"), ("slice_tail", "split"),
          ("colsum_last_row", "frames"), ("ddist_sign", "a"), ("raybias_ppf", "vd")] + [("unpack_off", n) for n in ALL]


@pytest.mark.parametrize("name", ALL)
def test_the_clean_emulation_passes_at_the_gpu_bounds(name):
    inp, rec = emulated(name)
    bad, worst, _ = fs.failures(inp, rec, name)
    assert bad == []


@pytest.mark.parametrize("fault,name", FAULTS)
def test_a_deliberate_fault_is_reported_at_the_gpu_bounds(fault, name):
    """carry dropped; Trun not carried across chunks; the bias row of a tile taken from its first row; the second K slice short by its
    14-wide tail; the un-pack's 63 + S off by one; a column sum missing a frame's last row; d dist with the wrong sign (seen by
    the camera gradients); the per-ray bias indexed by m / ppf."""
    inp = fs.case_inputs(name, 0)
    rec = fs.run_path(inp, np.float32, fault=fault)
    bad, _, evs = fs.failures(inp, rec, quiet=True)
    print("%s on %s: reported by %s" % (fault, name, bad))
    expect = {"carry": {"d sigma"}, "trun": {"w", "ray Trun"}, "bias_row_tile": {"H0", "H5", "g"}, "slice_tail": {"dW1", "dWc", "dW7"},
              "unpack_off": {"unpack W5 H4", "dW5[:, H4]"}, "colsum_last_row": {"dfold0", "dfold5", "dfold10"}, "ddist_sign": {"d dist"},
              "raybias_ppf": {"g"}}[fault]
    assert expect <= set(bad), (fault, name, bad)
    if fault == "ddist_sign":   # with the faulty d dist taken as given, the camera gradients of the emulation follow it: the sign shows there
        good = fs.run_path(inp, np.float32)
        rec["ws"].dxr[:, 385] = good["ws"].dxr[:, 385]
        bad2, _, _ = fs.failures(inp, rec, quiet=True)
        assert {"d_R", "d_Kinv", "d_xy"} <= set(bad2), bad2


HIER_VISIBLE = {"unpack_off": {"unpack W5 H4", "dW5[:, H4]"}, "ddist_sign": {"d dist"}, "no_gtz": {"d_T"}}
HIER_INVISIBLE = {
    "carry": "40 samples are one 64-wide chunk: no carry exists",
    "slice_tail": "P = 1280 points are one K slice (split_for(1280) = 1)",
    "bias_row_tile": "a frame is 640 = 5 x 128 rows: no tile spans two frames",
}


@pytest.mark.parametrize("fault", sorted(HIER_VISIBLE) + sorted(HIER_INVISIBLE))
def test_the_mutants_on_the_given_plane_case(fault):
    """DESIGN's five mutants re-run on case hier (z_planes_given), and the new one: the g_tz term of d_T dropped when the planes are given.
    Three of the five cannot show at this shape, for the reason listed, and are asserted to stay invisible."""
    inp = fs.case_inputs("hier", 0)
    assert inp["planes"] is not None and inp["t_rand"] is None
    rec = fs.run_path(inp, np.float32, fault=fault)
    bad, _, _ = fs.failures(inp, rec, quiet=True)
    print("%s on hier: reported by %s" % (fault, bad))
    if fault in HIER_INVISIBLE:
        print("    cannot show at this shape: " + HIER_INVISIBLE[fault])
        assert bad == []
    else:
        assert HIER_VISIBLE[fault] <= set(bad), (fault, bad)
        if fault == "no_gtz":
            assert set(bad) == {"d_T"}, "the other three camera gradients do not take g_tz"


def test_a_bias_added_by_every_slice_is_reported():
    """No split product of this path carries a bias (gemm32.hip adds it in the first slice only), so this fault is injected into
    the emulation's product itself: case split's dW1 with a bias row, two slices, the bias added by both."""
    inp, rec = emulated("split")
    a, b = np.asarray(rec["ws"].dha), np.asarray(rec["saved"].h[0])
    bias = inp["b"][1].astype(np.float32)[None, :]
    z = a.astype(np.float64).T @ b.astype(np.float64) + bias
    S = np.abs(a.astype(np.float64)).T @ np.abs(b.astype(np.float64)) + np.abs(bias)
    good = fs.mm_points(np.float32, a, b, 2, prior=np.broadcast_to(bias, z.shape))
    assert _ratio(good, z, S) <= fs.bound("dw")
    assert _ratio(good + bias, z, S) > fs.bound("dw")


# ---------------------------------------------------------------------------------------------------------------------
# the restatement against the committed fixtures (the reference's own fp32 forward and autograd, tests/golden/tiny_*.npz)
# ---------------------------------------------------------------------------------------------------------------------
FIXTURE_SEAM_TOL = 1e-5   # of the largest |entry| of a seam: the reference computed it in float32 through up to eleven layers
FIXTURE_GRAD_TOL = 1e-4   # of the largest |entry| of a gradient tensor: float32 autograd through the renderer and the MLP


@pytest.mark.parametrize("name", ["tiny_test", "tiny_train"])
def test_restatement_reproduces_the_committed_fixtures(name):
    """Float64 run of the restatement on the fixture's inputs: the seams (PE, density, weights, fg_feat, bg_alpha, depth, merged
    map), then -- with d_merge from the float64 renderer restatement (nr_restatement.py) under the fixture's loss -- the gradients
    of the codes, R, T and every MLP parameter the fixture sampled."""
    import nr_restatement as nr
    from conftest import load_golden, synthetic_case
    from n3dt import _lib, synthetic as syn
    from n3dt.train import data_losses, disk_mask
    g, m = load_golden(name)
    opt, sd, inp = synthetic_case(m)
    B, side, Ns = m["batch"], opt.featmap_size, opt.num_sample_coarse
    n_rays = side * side
    t_rand = syn.stratified_noise(B, n_rays, Ns, m["t_rand_seed"]).numpy() if m["mode"] == "train" else None
    x = fs.pack_inputs(opt, sd, inp, np.arange(n_rays), Ns, t_rand, np.zeros((B, n_rays, 256), dtype=np.float32))
    per_pt = lambda a, c: np.moveaxis(np.asarray(a).reshape(B, n_rays, Ns, c), 3, 1)  # noqa: E731
    (pts, dist, zval), _ = fs.sample(np.float64, x)
    for k, got in (("pts", per_pt(pts, 3)), ("z_dists", per_pt(dist, 1)), ("zvals", per_pt(zval, 1))):
        assert np.abs(got - g[k]).max() <= 1e-6 * np.abs(g[k]).max(), k
    # the encoding multiplies a point by up to 512: everything behind it is reproduced from the fixture's own fp32 sample points
    unpt = lambda a: np.moveaxis(a.astype(np.float64), 1, 3).reshape(B * n_rays * Ns, -1)  # noqa: E731
    x["geo"] = (unpt(g["pts"]), unpt(g["z_dists"])[:, 0], unpt(g["zvals"])[:, 0])
    rec = fs.run_path(x, np.float64)
    sv = rec["saved"]
    W2, b2 = x["W"][11].astype(np.float64), x["b"][11].astype(np.float64)
    seams = [("pe", per_pt(sv.cat5[:, :63], 63)), ("density", per_pt(np.maximum(sv.xr[:, 384], 0.0), 1)), ("feat", per_pt(np.asarray(sv.g) @ W2.T + b2, 256)),
             ("weight", np.asarray(sv.w).reshape(B, 1, n_rays, Ns)), ("fg_feat", np.moveaxis(rec["out"]["fg_feat"], 2, 1)),
             ("bg_alpha", rec["out"]["bg_alpha"].reshape(B, 1, n_rays)), ("depth", np.asarray(sv.ray[:, fs.G + 1]).reshape(B, 1, n_rays)),
             ("merge_featmap", np.moveaxis(rec["out"]["merge_feat"], 2, 1).reshape(B, 256, side, side))]
    for k, got in seams:
        ref = g[k].astype(np.float64)
        err = np.abs(got - ref).max() / np.abs(ref).max()
        print("%s %-14s largest |restatement - fixture| = %.2e of the largest entry" % (name, k, err))
        assert got.shape == ref.shape and err <= FIXTURE_SEAM_TOL, (k, err)
    # the renderer and the loss in float64, d_merge by the renderer restatement
    P = nr.params_from_state_dict(sd, 2)
    f = nr.forward(np.moveaxis(g["merge_featmap"].astype(np.float64), 1, 3) * 0 + rec["out"]["merge_feat"].reshape(B, side, side, 256), P)
    img = torch.tensor(np.moveaxis(f["img"], 3, 1), requires_grad=True)
    assert np.abs(img.detach().numpy() - g["merge_img"]).max() <= 1e-5
    terms = data_losses({"merge_img": img, "bg_img": torch.tensor(g["bg_img"].astype(np.float64))}, torch.full_like(img, 0.5), disk_mask(B, opt.pred_img_size).double())
    np.testing.assert_allclose([float(terms[k].detach()) for k in ("bg_loss", "head_loss", "nonhead_loss")], g["loss_terms"], atol=1e-6)
    (terms["bg_loss"] + terms["head_loss"] + terms["nonhead_loss"]).backward()
    d_feat = nr.backward(np.moveaxis(img.grad.numpy(), 1, 3), P, nr.tape_from_forward(f))["d_featmap"]
    x["d_merge"] = d_feat.reshape(B, n_rays, 256)
    # A ReLU whose float64 pre-activation lies within 2^-23 S of zero went either way in the reference's float32 forward (the seams
    # cannot tell: the activation is ~1e-7 either way).  The gradients are reproduced for the float64 gates or with ONE such gate flipped.
    near = []
    for c in fs.stages(x, rec):
        if c["tag"] in ["H%d" % l for l in range(8)]:
            pt, ch = np.nonzero(np.abs(c["z"]) < 2.0 ** -23 * c["S"])
            near += [(int(c["tag"][1]), int(a), int(b)) for a, b in zip(pt, ch)]
    assert len(near) <= 8, near
    best = None
    for flip in [()] + [(n,) for n in near]:
        x["flip"] = flip
        r = fs.run_path(x, np.float64)
        e = np.abs(r["res"]["d_shape"] - g["grad_in.shape_code"]).max()
        if best is None or e < best[0]:
            best = (e, flip, r)
    print("%s: %d gates within 2^-23 S of zero; the fixture is reproduced with %s flipped" % (name, len(near), list(best[1]) or "none"))
    rec = best[2]
    res = rec["res"]
    pairs = [("grad_in.shape_code", res["d_shape"]), ("grad_in.appea_code", res["d_appea"]), ("grad_in.audiostyle", res["d_audio"]),
             ("grad_in.batch_Rmats", res["d_R"]), ("grad_in.batch_Tvecs", res["d_T"].reshape(B, 3, 1))]
    for k, got in pairs:
        ref = g[k].astype(np.float64)
        err = np.abs(got - ref).max() / np.abs(ref).max()
        print("%s %-22s largest |restatement - fixture| = %.2e of the largest entry" % (name, k, err))
        assert got.shape == ref.shape and err <= FIXTURE_GRAD_TOL, (k, err)
    worst = 0.0
    for l, mod in enumerate(_lib.MLP_ORDER):
        for kind, got in (("weight", rec["gw"][l]), ("bias", rec["gb"][l])):
            key = "grad_p.fg_CD_predictor.%s.%s" % (mod, kind)
            idx, val = g[key + ".idx"], g[key + ".val"].astype(np.float64)
            err = np.abs(got.reshape(-1)[idx] - val).max() / (np.abs(val).max() + 1e-12)
            serr = abs(got.sum() - float(g[key + ".sum"])) / float(g[key + ".abs"])
            worst = max(worst, err, serr)
            assert err <= FIXTURE_GRAD_TOL and serr <= FIXTURE_GRAD_TOL, (key, err, serr)
    print("%s: 24 parameter gradients, largest sampled-entry / sum error %.2e of the tensor's scale" % (name, worst))
