"""The fused bf16 training path (nerf_fwd_x16_train_kernel, nerf_bwd_x16_kernel, the dw_x16 launches, dw_reduce,
train16_finish / _unmerge) pinned one linear stage at a time from the tiles it leaves in HBM -- see tests/x16_stagewise.py for
the formats, the comparison rule (check_bf16), U and the floors, all of which come from the CPU alone.

One synchronised forward + backward per case through ops.render_train_fwd / ops.render_bwd with precision = bf16 (run
twice, for the reproducibility test), `saved` and the training workspace read back, every stage recomputed in float64 from
the decoded tiles of the stage before it.

Cases (free ray sets of an 8 x 8 grid; B x rays x samples):
  a           2 x 16 x 24   one partial block per ray; 32 blocks = whole workgroups of the forward (8 waves) and the dX chain (4)
  b           1 x  9 x 40   18 blocks: the last workgroup of either kernel has dead waves, which write the dump record; the second
                            block of each ray is a quarter full
  c           2 x 25 x 40   50 blocks per frame.  Both weight-gradient planners pick 6 slices per frame here (dw_plan_slices:
                            min(ceil(256 / 2), 50 / 8) = 6; launch_dw_multi's loop: one round of workgroups whatever the count up to
                            50 / 8 = 6, so the most slices win), and a slice is ceil(50 / 6) = 9 blocks: five slices of 9 and a last
                            one of 5 -- 50 is no multiple of 6, nor of 9.  100 blocks are 3 short of a multiple of the forward's
                            8-wave workgroups (104), so dead waves run here too.
  d_contrast  case a with contrast_state_dict: saturating alpha, zero weights behind it
  d_gaze      case a with include_gaze (shape code 179 + 64) and audio_dim = 0: other fold offsets, other in0 / in5

Lanes of a partial block beyond n_samples: the sampler hands them the point (0, 0, 0) with dist = 0 (n3dt_device.h:101-105), so
they are real samples of the padded block in the forward -- PE(0), then the MLP on it -- and are checked like every other
lane; their weight is zero, so every dZ entry of theirs must be exactly zero, or it would leak into the weight gradients."""
import functools

import numpy as np
import pytest
import torch

import x16_stagewise as xs

pytestmark = pytest.mark.gpu

ALL = list(xs.CASES)


def dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def run(name):
    from n3dt import HeadNeRFNet, _lib, ops
    c = xs.CASES[name]
    B, n_rays, Ns = c["B"], c["n_rays"], c["n_samples"]
    opt, sd, inp, rays, t_rand, d_merge = xs.case_inputs(name)
    net = HeadNeRFNet(opt, False, False, train_precision="bf16", **c["kw"]).to(dev())
    net.load_state_dict(sd, strict=True)
    prec = _lib.BF16
    xy = inp["batch_xy"].to(dev()).contiguous()
    geom = net._geom(B, n_rays, xy, n_samples=Ns, z_planes_given=int(bool(c.get("hier"))))   # (hier: t_rand below holds the planes)
    params, ws, bs = net._mlp_params()
    packed = net._packed(geom, prec, params, ws, bs)
    R, T, Kinv = (ops._f32c(inp[k].to(dev())) for k in ("batch_Rmats", "batch_Tvecs", "batch_inv_inmats"))
    T = T.view(B, 3)
    shape, appea = ops._f32c(inp["shape_code"].to(dev())), ops._f32c(inp["appea_code"].to(dev()))
    audio = ops._f32c(inp["audiostyle"].to(dev())) if geom.audio_dim > 0 else None
    tr = t_rand.to(dev()).contiguous()
    bg = net.neural_render.bg_featmap.detach().reshape(opt.featmap_nc, -1)[:, rays.to(dev())].contiguous()
    dm = d_merge.to(dev()).contiguous()
    Ls, Lw = xs.saved_layout(B, n_rays, Ns), xs.ws_layout(B, n_rays, Ns)
    assert xs.library_totals(geom) == (Ls["total"], Lw["total"])
    runs = []
    for _ in range(2):
        out, saved = ops.render_train_fwd(geom, packed, params, xy, R, T, Kinv, shape, appea, audio, tr, bg, prec)
        assert saved.numel() >= Ls["total"]  # (the size query covers the fp32 path's layout too)
        gws, gbs = [torch.zeros_like(w) for w in ws], [torch.zeros_like(b) for b in bs]
        res = ops.render_bwd(geom, params, ops.mlp_params(gws, gbs), shape, appea, audio, bg, dm, saved, precision=prec)
        torch.cuda.synchronize()
        wsbuf = ops.WORKSPACE.get("train", Lw["total"], dev())
        runs.append({"saved": saved.cpu().numpy(), "ws": wsbuf[:Lw["dwpart"]].cpu().numpy(),
                     "gw": [g.cpu().numpy() for g in gws], "gb": [g.cpu().numpy() for g in gbs],
                     "codes": [None if r is None else r.cpu().numpy() for r in res[1:4]],
                     "out": {k: v.cpu().numpy() for k, v in out.items()}})
    r0 = runs[0]
    sv = xs.Saved(r0["saved"], B, n_rays, Ns)
    wk = xs.Workspace(r0["ws"], B, n_rays, Ns)
    W = xs.Weights([w.cpu().numpy() for w in ws], [b.cpu().numpy() for b in bs], geom.shape_dim, geom.audio_dim, sv.wm)
    codes = (inp["shape_code"].numpy(), inp["appea_code"].numpy(), inp["audiostyle"].numpy() if geom.audio_dim > 0 else None)
    infer = None
    if name in ("a", "b", "c"):
        # the inference kernel (nerf_fwd_x16_kernel<bf16>) on the same rays, planes and codes
        net.num_sample_coarse = Ns
        with torch.no_grad():
            o = net.render_features(xy, inp["audiostyle"].to(dev()), shape, appea, R, T, Kinv, t_rand=tr, want_weight=True, want_merge=False,
                                    precision="bf16")
        torch.cuda.synchronize()
        infer = {k: o[k].cpu().numpy() for k in ("weight", "fg_feat", "bg_alpha")}
    return {"c": c, "sv": sv, "wk": wk, "W": W, "codes": codes, "runs": runs, "inp": inp, "t_rand": t_rand, "opt": opt, "S": geom.shape_dim,
            "infer": infer}


def assert_stage(tag, st):
    xs.report(tag, st)
    assert st["mismatches"] == 0 and st["max_ulp"] <= 1, (tag, st["mismatches"], st["max_ulp"], st["worst"])
    assert st["ambiguous"] <= xs.AMBIGUOUS_CAP * st["n"], (tag, st["ambiguous"], st["n"])
    assert st["wide"] <= xs.WIDE_CAP * st["n"], (tag, st["wide"], st["n"])


@pytest.mark.parametrize("name", ALL)
def test_forward_stages_teacher_forced(name):
    """H_0 .. H_7 and relu(RGB_layer_1) from the decoded inputs of each stage under check_bf16; sigma (kept in fp32) within
    U (|b| + sum |w x|) of the float64 row; every gate bit = "stored activation != 0" of its tile, lane and register."""
    r = run(name)
    sv, W = r["sv"], r["W"]
    for tag, z, mag, relu, bits in xs.forward_stages(sv, W):
        assert_stage("%s %s" % (name, tag), xs.check_bf16(bits, z, xs.U * mag, relu=relu))
    z, mag = xs.density_stage64(sv, W)
    err = np.abs(sv.sigma_pre.astype(np.float64) - z) / mag
    print("%s sigma: entries %d, largest |s - s64| / (|b| + sum |w x|) = %.3e (bound %.3e)" % (name, z.size, err.max(), xs.U))
    assert err.max() <= xs.U
    for l in range(8):
        assert np.array_equal(sv.gates[l], sv.h_bits(l) != 0), "gate bits of layer %d" % l
        assert not np.any(sv.h_bits(l) == 0x8000)  # the ReLU on the packed value clears negative zero as well
    assert sv.gates.any(axis=(1, 2)).all()


def _oracle_points(r):
    """the oracle's fp32 sample points and plane distances in padded-block order (lanes beyond n_samples: point 0, dist 0)"""
    from oracle import oracle as orc
    sv, c, inp, opt = r["sv"], r["c"], r["inp"], r["opt"]
    B, n_rays, Ns = c["B"], c["n_rays"], c["n_samples"]
    o = orc.sample(inp["batch_xy"].numpy(), inp["batch_Rmats"].numpy(), inp["batch_Tvecs"].numpy(), inp["batch_inv_inmats"].numpy(), Ns,
                   opt.world_z1, opt.world_z2, r["t_rand"].numpy())
    if c.get("hier"):   # the oracle's FineSample._calc_sample_points_by_zvals on the given planes
        o = orc.sample_planes(inp["batch_xy"].numpy(), inp["batch_Rmats"].numpy(), inp["batch_Tvecs"].numpy(), inp["batch_inv_inmats"].numpy(),
                              r["t_rand"].numpy())
    pts = np.zeros((B, n_rays, sv.bpr * 32, 3))
    pts[:, :, :Ns] = np.moveaxis(o["pts"].astype(np.float64), 1, 3)
    dist = np.zeros((B, n_rays, sv.bpr * 32))
    dist[:, :, :Ns] = o["z_dists"][:, 0]
    return pts.reshape(-1, 3), dist.reshape(-1)


@pytest.mark.parametrize("name", ALL)
def test_pe_tiles_against_the_oracle_points(name):
    """The PE tiles against bf16 of the float64 encoding of the oracle's fp32 sample points: never more than one bf16 ulp.
    (The sample points are the oracle's bit for bit -- geo's dist matches it exactly, test below -- so the distance is the
    encoder's own.  This test found two defects of pe_fast, fixed with it: the low part of the 1/(2 pi) split was 2.0e-10 off,
    and the phase was rounded at the scale of 1/2 .. 1 revolution ahead of v_sin_f32; together up to 2e-7 in the sine, three bf16
    ulps of one entry of 1.2e-5 in the 16-ray cases.  docs/tuning_log.md has the figures before and after.)"""
    r = run(name)
    sv = r["sv"]
    pts, _ = _oracle_points(r)
    pe64 = xs.embed64(pts)
    want = xs.bf16_bits(pe64)
    d = np.abs(xs.ordinal(sv.pe_bits()) - xs.ordinal(want))
    print("%s PE: entries %d, off by one ulp %d, by more %d, largest distance %d" % (name, d.size, int((d == 1).sum()), int((d > 1).sum()), int(d.max())))
    for i in np.argwhere(d > 1)[:8]:
        got = float(xs.bf16_to_f64(sv.pe_bits()[i[0], i[1]:i[1] + 1])[0])
        print("    point %d channel %d: stored %.9g, float64 %.12g (|difference| %.3g), %d ulps" % (i[0], i[1], got, pe64[i[0], i[1]], abs(got - pe64[i[0], i[1]]), d[i[0], i[1]]))
    assert d.max() <= 1


@pytest.mark.parametrize("name", ALL)
def test_plane_distances_and_weights(name):
    """geo's plane distance against the oracle's (relative 1e-5) and the saved per-sample weights against the float64 compositing
    of the decoded sigma and dist (relative 1e-5 plus 2^-21: weight_tolerance; the fp32 CPU emulation holds it four times over)."""
    r = run(name)
    sv, c = r["sv"], r["c"]
    B, n_rays, Ns = c["B"], c["n_rays"], c["n_samples"]
    _, dist = _oracle_points(r)
    derr = np.abs(sv.dist - dist)
    print("%s dist: largest relative error %.3e" % (name, (derr / np.maximum(np.abs(dist), 1e-30)).max()))
    assert np.all(derr <= 1e-5 * np.abs(dist))
    w64, T64 = xs.composite64(sv.sigma_pre, sv.dist, B * n_rays, sv.bpr, Ns)
    werr = np.abs(sv.weight - w64) / xs.weight_tolerance(w64, T64)
    print("%s weight: entries %d, largest error %.3f of the tolerance (1e-5 w + 2^-21)" % (name, w64.size, werr.max()))
    assert werr.max() <= 1.0


@pytest.mark.parametrize("name", ALL)
def test_dx_chain_teacher_forced(name):
    """dG from the saved weights and the workspace's d Gray, the d sigma row, then dZ_7 .. dZ_0 each from the decoded dZ_{l+1}
    (or [dG | d sigma]) and the gate words, under check_bf16; samples beyond n_samples are exactly zero in every tile."""
    r = run(name)
    sv, wk, W, c = r["sv"], r["wk"], r["W"], r["c"]
    ray_of_point = np.repeat(np.arange(sv.nb) // sv.bpr, 32)
    z, mag = xs.dg_stage64(sv.point_weight(), wk.dgray[ray_of_point])
    assert_stage("%s dG" % name, xs.check_bf16(wk.dg_bits(), z, xs.U * mag, gate=sv.gs_bits != 0))
    row = wk.dsig_row_bits()
    assert np.array_equal(row[:, 0], xs.bf16_bits(wk.dsig.astype(np.float64))) and not row[:, 1:].any()
    for tag, z, mag, gate, bits in xs.dx_stages(sv, wk, W):
        assert_stage("%s %s" % (name, tag), xs.check_bf16(bits, z, xs.U * mag, gate=gate))
    dead = sv.sample_of_point() >= c["n_samples"]
    assert dead.sum() == sv.nb * 32 - c["B"] * c["n_rays"] * c["n_samples"]
    assert not np.any(xs.bf16_to_f64(wk.dz_all[dead]) != 0), "a sample beyond n_samples carries a gradient"
    assert np.any(xs.bf16_to_f64(wk.dz_bits(0)[~dead]) != 0)


def _family_errors(got, val, mag, fams, fam_of_col, n_points):
    out = {}
    for i, fam in enumerate(fams):
        cols = fam_of_col == i
        out[fam] = max(out.get(fam, 0.0), xs.grad_error(got[:, cols], val[:, cols], mag[:, cols], n_points))
    return out


@pytest.mark.parametrize("name", ALL)
def test_weight_bias_and_code_gradients(name):
    """Every `grads` tensor of the MLP (FeaExt_module_0..7, density, the un-merged RGB_layer_0 / _1) and d_shape / d_appea /
    d_audio against the float64 products of the decoded tiles (un-merge and folding adjoint in float64), per entry relative to
    sum_points |dz| |x| of that entry, bound 4 x the CPU floor of the product family."""
    r = run(name)
    ref = xs.grads64(r["sv"], r["wk"], r["W"], r["codes"])
    full = xs.assemble_grads(ref, r["S"])
    worst = {}
    n_terms = r["sv"].nb * 32 * xs.UNDERFLOW_TERMS  # (grad_error: underflow allowance)
    for k, (val, mag, fams, fam_of_col) in sorted(full.items()):
        l = int(k[1:])
        got = r["runs"][0]["gw"][l] if k[0] == "w" else r["runs"][0]["gb"][l].reshape(1, -1)
        assert got.shape == val.shape, (k, got.shape, val.shape)
        e = _family_errors(got.astype(np.float64), val, mag, fams, fam_of_col, n_terms)
        print("%s %-4s %s" % (name, k, "  ".join("%s %.3e (bound %.3e)" % (f, v, 4 * xs.dw_floor(name, f)) for f, v in e.items())))
        for f, v in e.items():
            worst[f] = max(worst.get(f, 0.0), v)
            assert v <= 4 * xs.dw_floor(name, f), (k, f, v)
    # per frame, as the weight-gradient kernels leave them: dfold[f][bias_offset(l)] = row sums of dZ_l (dw_x16_body's rowsum,
    # train_x16.inc:846-851), rs_rgb[f] = [db_m (192) | d b_density], copied to dfold[f][bias_offset(10)] (train16_finish_kernel, :1009-1014);
    # train_fold_bwd_kernel only reads them, so they survive the backward
    wk, B = r["wk"], r["c"]["B"]
    per_frame = [("rs%d" % l, wk.dfold[:, xs.bias_offset(l):xs.bias_offset(l) + 384]) for l in range(8)]
    per_frame += [("rs_m", wk.rsrgb[:, :193]), ("rs_m", np.concatenate([wk.dfold[:, xs.bias_offset(10):xs.bias_offset(10) + 192], wk.rsrgb[:, 192:193]], axis=1))]
    for k, got in per_frame:
        assert got.shape == ref[k][0].shape == (B, got.shape[1])
        v = xs.grad_error(got, ref[k][0], ref[k][1], n_terms)
        print("%s %-5s per frame: bias %.3e (bound %.3e)" % (name, k, v, 4 * xs.dw_floor(name, "bias")))
        assert v <= 4 * xs.dw_floor(name, "bias"), (k, v)
    for k, got in zip(("d_shape", "d_appea", "d_audio"), r["runs"][0]["codes"]):
        if k not in ref:
            assert got is None
            continue
        v = xs.grad_error(got, ref[k][0], ref[k][1], n_terms)
        print("%s %-8s latent %.3e (bound %.3e)" % (name, k, v, 4 * xs.dw_floor(name, "latent")))
        assert v <= 4 * xs.dw_floor(name, "latent"), (k, v)
    print("%s: largest error per family %s" % (name, {f: "%.3e" % v for f, v in worst.items()}))


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_inference_kernel_against_the_training_forward(name):
    """nerf_fwd_x16_kernel<bf16> (render_features, want_weight=True) against the training forward on the same inputs: per-sample
    weights, fg_feat and bg_alpha.  The two kernels differ only by the bias route -- the exact fp32 bias as the C operand against
    its hi + lo halves through an MFMA -- so they are held to 4 x the spread of two free-running CPU emulations that differ in
    exactly that (ROUTE_FLOOR; weights and bg_alpha absolute, fg_feat relative to its largest entry).  FEAT_TOL stays where it is."""
    r = run(name)
    train = {"weight": r["sv"].weight.reshape(r["infer"]["weight"].shape), "fg_feat": r["runs"][0]["out"]["fg_feat"],
             "bg_alpha": r["runs"][0]["out"]["bg_alpha"]}
    got = xs.route_spread(r["infer"], train)
    print("%s inference against training forward: %s" % (name, "  ".join("%s %.3e (bound %.3e)" % (k, v, 4 * xs.ROUTE_FLOOR[k]) for k, v in got.items())))
    for k, v in got.items():
        assert r["infer"][k].shape == train[k].shape and np.abs(train[k]).max() > 0
        assert v <= 4 * xs.ROUTE_FLOOR[k], (k, v)


def test_a_lost_block_or_slice_cannot_pass():
    """Strength of the bound, on the decoded-tile reference of case c: taking any single 32-sample block, or any single slice
    of the planners' 9-block slices, out of the float64 sum of any product moves at least one entry of it beyond the bound.
    (A block whose dZ is identically zero -- sigma <= 0 on all its samples: no weight, no d sigma -- adds exactly nothing and
    cannot be lost; such blocks are a small minority and no slice consists of them.)"""
    r = run("c")
    sv, wk, c = r["sv"], r["wk"], r["c"]
    bpf = c["n_rays"] * sv.bpr
    spf, per = xs.dw_slices(bpf, c["B"])
    assert (spf, per) == (6, 9) and xs.dw_slices(bpf, c["B"], 7, 2) == (6, 9) and xs.dw_slices(bpf, c["B"], 2, 1) == (6, 9) and bpf % spf != 0 and bpf % per != 0
    f = xs.bf16_to_f64
    pe = f(sv.pe_bits())[:, :63]
    dgs = np.concatenate([f(wk.dg_bits()), f(wk.dsig_row_bits()[:, :1])], axis=1)
    products = [("w%d" % l, f(wk.dz_bits(l)), f(sv.h_bits(4 if l == 5 else l - 1)), "hidden") for l in range(1, 8)]
    products += [("w0_pe", f(wk.dz_bits(0)), pe, "pe"), ("w5_pe", f(wk.dz_bits(5)), pe, "pe"), ("dwm", dgs, f(sv.h_bits(7)), "rgb")]
    for tag, a, b, fam in products:
        mag = np.abs(a).T @ np.abs(b)
        per_block = np.einsum("bsi,bsj->bij", a.reshape(sv.nb, 32, -1), b.reshape(sv.nb, 32, -1))
        lim = 4 * xs.DW_FLOOR[fam] * mag
        moved = (np.abs(per_block) > lim[None]).any(axis=(1, 2))
        live = (a.reshape(sv.nb, -1) != 0).any(axis=1)
        assert moved[live].all() and live.sum() >= 0.9 * sv.nb, (tag, "blocks", np.flatnonzero(live & ~moved), int(live.sum()))
        n_slices = 0
        for fr in range(c["B"]):
            for s0 in range(0, bpf, per):
                sl = per_block[fr * bpf + s0:fr * bpf + min(s0 + per, bpf)].sum(axis=0)
                assert (np.abs(sl) > lim).any(), (tag, "slice", fr, s0)
                n_slices += 1
        assert n_slices == spf * c["B"]
        print("c %-6s every one of %d live blocks and %d slices moves an entry beyond the bound (weakest block: %.1f x the bound)" %
              (tag, int(live.sum()), n_slices, np.where(lim[None] > 0, np.abs(per_block) / np.maximum(lim[None], 1e-300), 0.0).max(axis=(1, 2))[live].min()))


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_two_runs_are_bit_identical_where_nothing_is_atomic(name):
    """xT, gS, geo, gates and dzT of two runs of the same shape are bit-identical (live records; the dump record is not
    compared): no atomics on those.  NOT bit-stable, because they are reduced with fp32 atomics in an order the hardware picks:
    every weight gradient (per-XCD partials, dw_x16_body's epilogue), the row sums behind the bias gradients and the per-frame
    folded biases (dfold, rs_rgb), RGB_layer_0's bias (train16_unmerge_bias_kernel), the latent columns and d_shape / d_appea /
    d_audio (train_fold_bwd_kernel) -- those are held to the float64 reference above instead, and printed here."""
    r = run(name)
    c = r["c"]
    a, b = r["runs"]
    s0, s1 = (xs.Saved(x["saved"], c["B"], c["n_rays"], c["n_samples"]) for x in (a, b))
    for k in ("xT", "gS", "geo", "gates"):
        assert np.array_equal(s0.raw[k], s1.raw[k]), k
    w0, w1 = (xs.Workspace(x["ws"], c["B"], c["n_rays"], c["n_samples"]) for x in (a, b))
    assert np.array_equal(w0.raw_dzT, w1.raw_dzT)
    assert np.array_equal(s0.weight, s1.weight) and np.array_equal(w0.dsig, w1.dsig)
    same = sum(int(np.array_equal(x, y)) for x, y in zip(a["gw"][:11] + a["gb"][:11], b["gw"][:11] + b["gb"][:11]))
    print("%s: %d of 22 gradient tensors happened to be bit-identical between the two runs" % (name, same))
