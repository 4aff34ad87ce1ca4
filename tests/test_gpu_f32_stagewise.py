"""The exact fp32 volumetric training path (n3dt_launch_train_fwd / _bwd, the fp32 kernel of gemm32.hip, the fold, ray-head,
colsum, compositing and camera kernels) pinned one stage at a time from what it leaves in `saved`, the training workspace and
the gradient tensors -- see tests/f32_stagewise.py for the layouts, the comparison rule and the bounds, all of which come from
the CPU alone (every bound is 4 x a floor test_f32_stagewise_cpu.py re-measures).

One synchronised forward + backward per case through ops.render_train_fwd / ops.render_bwd with precision = F32 and camera
gradients through n3dt_render_bwd_cam (R, T, Kinv, xy).  Cases (free ray sets of an 8 x 8 grid; B x rays x samples):
  a         2 x 16 x  24   P = 768: whole 128-row tiles, no split, no tile straddles a frame (384 points per frame): the baseline
  tail      1 x  9 x  40   P = 360: a tile tail of 104 rows in M, and in the k-major staging of every dW product
  frames    2 x 25 x  40   P = 2000, 1000 per frame: tiles straddle the frame boundary (per-frame bias rows, per-frame column sums)
  split     2 x 23 x 105   P = 4830: split_k = 2, slices of 2416 and 2414 rows (a K tail of 14, the slice boundary one row off the
                           frame boundary), two compositing chunks per ray (64 + 41)
  chunks3   1 x  9 x 130   three chunks, the last holding 2 samples
  contrast  case a with contrast_state_dict: saturated alpha (x = 1e-10), zero weights behind it, the alpha > 0 branch
  gaze      case a with include_gaze and audio_dim = 0: other fold offsets, other in0 / in5, d_audio is None
  vd        case tail with vd_dim = 27 and a seeded ray_bias: the per-ray bias (40 rows per bias row against 128-row tiles), d_ray_bias
Cases a and tail run three more times: frozen (grads = None), with d_fg and d_bg_alpha cotangents beside d_merge, and with an
all-zero d_merge."""
import functools

import numpy as np
import pytest
import torch

import f32_stagewise as fs

pytestmark = pytest.mark.gpu

ALL = list(fs.CASES)
EXTRA = [(n, v) for n in ("a", "tail") for v in ("frozen", "dfg", "zero")]


def dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def run(name, variant="full"):
    from n3dt import _lib, ops
    inp = fs.case_inputs(name, 0, variant)
    B, n_rays, Ns, vd = inp["B"], inp["n_rays"], inp["Ns"], inp["vd"]
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev())  # noqa: E731
    xy = t(inp["xy"])
    geom = ops.make_geom(B, n_rays, Ns, 384, 256, inp["S"], inp["A"], inp["U"], fs.FEATMAP_SIZE, 2, inp["z1"], inp["z2"], xy.stride(), int(inp["planes"] is not None), vd_dim=vd)
    Ls, Lw = fs.saved_layout(B, n_rays, Ns, vd), fs.ws_layout(B, n_rays, Ns)
    saved_floats, ws_floats, saved_bytes = fs.library_totals(geom)
    assert (saved_floats, ws_floats) == (Ls["total"], Lw["total"]) and saved_bytes >= 4 * saved_floats
    ws_, bs_ = [t(w) for w in inp["W"]], [t(b) for b in inp["b"]]
    params = ops.mlp_params(ws_, bs_)
    packed = ops.pack_mlp(geom, _lib.F32, params, dev())
    R, T, Kinv, shape, appea, audio, tr, bg, rb = (t(inp[k]) for k in ("R", "T", "Kinv", "shape", "appea", "audio", "t_rand", "bg", "ray_bias"))
    if inp["planes"] is not None:   # the hierarchical pass: z_planes_given, the planes go where t_rand goes
        tr = t(inp["planes"])
    dm, dfg, dba = t(inp["d_merge"]), t(inp["d_fg"]), t(inp["d_ba"])
    runs = []
    for _ in range(2 if variant == "full" else 1):
        out, saved = ops.render_train_fwd(geom, packed, params, xy, R, T, Kinv, shape, appea, audio, tr, bg, _lib.F32, ray_bias=rb)
        gws = gbs = grads = None
        if not inp["frozen"]:
            gws, gbs = [torch.zeros_like(w) for w in ws_], [torch.zeros_like(b) for b in bs_]
            grads = ops.mlp_params(gws, gbs)
        res = ops.render_bwd(geom, params, grads, shape, appea, audio, bg, dm, saved, cam=(xy, R, T, Kinv, tr), precision=_lib.F32,
                             frozen=inp["frozen"], cam_grads=("R", "T", "Kinv", "xy"), d_fg=dfg, d_ba=dba)
        torch.cuda.synchronize()
        wsbuf = ops.WORKSPACE.get("train", 4 * Lw["total"], dev())
        n = lambda x: None if x is None else x.cpu().numpy()  # noqa: E731
        res = list(res)
        d_ray = res.pop(6) if vd else None
        names = ("d_bg", "d_shape", "d_appea", "d_audio", "d_R", "d_T", "d_Kinv", "d_xy")
        rec = {"saved": fs.Saved(saved.cpu().numpy().view(np.float32), B, n_rays, Ns, vd),
               "ws": fs.Workspace(wsbuf[:4 * Lw["total"]].cpu().numpy().view(np.float32), B, n_rays, Ns),
               "gw": None if gws is None else [n(g) for g in gws], "gb": None if gbs is None else [n(g) for g in gbs],
               "out": {k: n(v) for k, v in out.items()}, "res": dict(zip(names, (n(x) for x in res)), d_ray_bias=n(d_ray))}
        runs.append(rec)
    return inp, runs


def check(name, variant):
    inp, runs = run(name, variant)
    bad, worst, evs = fs.failures(inp, runs[0], "%s%s" % (name, "" if variant == "full" else "/" + variant))
    print("%s %s: largest error per family, in units of its bound: %s" % (name, variant, "  ".join("%s %.3f (%.2e)" % (f, v / fs.bound(f), v) for f, v in sorted(worst.items()))))
    assert bad == [], bad
    return inp, runs[0]


@pytest.mark.parametrize("name", ALL)
def test_every_stage_within_four_times_its_cpu_floor(name):
    """fold, PE and geometry, H_0 .. H_7, xr, g, the weights and the ray record, fg_feat / bg_alpha / merge_feat; dgray, dwsum, dg, d sigma,
    d dist, dxr, dH_1 and dH_0 at the end of the float64 chain, dfold, dpe; all twelve weight and bias gradients, the un-pack, the
    latent columns and code gradients, dW2 / db2 / d_bg_featmap, d_ray_bias, d_R / d_T / d_Kinv / d_xy."""
    inp, rec = check(name, "full")
    assert np.abs(rec["gw"][0]).max() > 0 and np.abs(rec["res"]["d_xy"]).max() > 0
    if name == "contrast":   # the case is there for saturated samples (alpha = 1 in fp32: x = 1e-10), vanishing weights behind them, and alpha = 0
        sig, dist, w = rec["saved"].xr[:, 384], rec["saved"].geo[:, 0], rec["saved"].w
        alpha = np.float32(1) - np.exp(-np.maximum(sig, np.float32(0)) * dist)
        assert (alpha == 1).any() and (alpha == 0).any() and ((w > 0) & (w < 1e-9)).any() and (w == 0).any()


@pytest.mark.parametrize("name,variant", EXTRA)
def test_frozen_extra_cotangents_and_zero_cotangent(name, variant):
    """frozen: no parameter gradient is formed, the code and camera gradients are those of the full run's rule; dfg: the d_fg and
    d_bg_alpha routes of train_head_bwd_kernel; zero: an all-zero d_merge gives exactly zero everywhere."""
    inp, rec = check(name, variant)
    if variant == "frozen":
        assert rec["gw"] is None and rec["res"]["d_bg"] is None
    if variant == "dfg":
        assert np.abs(inp["d_fg"]).max() > 0 and np.abs(inp["d_ba"]).max() > 0
    if variant == "zero":
        for k, v in rec["res"].items():
            assert v is None or not np.any(v != 0), k
        for g in rec["gw"] + rec["gb"]:
            assert not np.any(g != 0)
        wk = rec["ws"]
        for a in (wk.dg, wk.dxr[:, :386], wk.dha, wk.dhb, wk.dpe[:, :63], wk.dfold, wk.dw5p, wk.dwc, wk.dbc):
            assert not np.any(a != 0)


@pytest.mark.parametrize("name", ALL)
def test_two_runs_are_bit_identical_where_nothing_is_atomic(name):
    """`saved`, dg, dxr, the surviving dH, dpe and d_xy of two runs agree bit for bit.  Everything accumulated with fp32 atomics
    (split-K weight gradients, column sums, dfold, the code and camera sums) is held to the float64 reference instead."""
    _, (a, b) = run(name, "full")
    for x, y in zip(a["saved"].live + a["ws"].live, b["saved"].live + b["ws"].live):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint32), np.ascontiguousarray(y).view(np.uint32))
    assert np.array_equal(a["res"]["d_xy"].view(np.uint32), b["res"]["d_xy"].view(np.uint32))
    for k in ("fg_feat", "bg_alpha", "merge_feat"):
        assert np.array_equal(a["out"][k].view(np.uint32), b["out"][k].view(np.uint32))


@pytest.mark.parametrize("name", ["a", "split", "chunks3"])
def test_sample_points_against_the_oracle(name):
    """cat5[:, 0:3] and geo against the fp32 oracle's sampler (the CPU floor of family "geo" is the oracle's own distance from
    float64, so the two fp32 evaluations are at most floor + bound apart), and the PE columns against the float64 encoding of the
    oracle's points, wider by what 2^k times that distance allows."""
    from oracle import oracle as orc
    inp, runs = run(name, "full")
    sv = runs[0]["saved"]
    o = orc.sample(inp["xy"], inp["R"], inp["T"], inp["Kinv"], inp["Ns"], inp["z1"], inp["z2"], inp["t_rand"])
    P = sv.P
    pts, dist, zval = np.moveaxis(o["pts"], 1, 3).reshape(P, 3), o["z_dists"][:, 0].reshape(P), o["zvals"][:, 0].reshape(P)
    _, (S_p, S_d, S_z) = fs.sample(np.float64, inp)
    u = fs.FLOOR["geo"] + fs.bound("geo")
    same = int(np.sum(sv.cat5[:, :3] == pts))
    print("%s: %d of %d point coordinates bit-identical to the oracle's; largest distance %.3e of S (allowed %.3e)" %
          (name, same, pts.size, float((np.abs(sv.cat5[:, :3].astype(np.float64) - pts) / np.maximum(S_p, 1e-300)).max()), u))
    assert np.all(np.abs(sv.cat5[:, :3].astype(np.float64) - pts) <= u * S_p)
    assert np.all(np.abs(sv.geo[:, 0].astype(np.float64) - dist) <= u * S_d) and np.all(np.abs(sv.geo[:, 1].astype(np.float64) - zval) <= u * S_z)
    pe64 = fs.embed(np.float64, pts.astype(np.float64))[:, 3:63]
    scale = np.repeat(2.0 ** np.arange(10), 6)[None, :]
    allowed = fs.bound("pe") + scale * np.tile(u * S_p, (1, 20))
    assert np.all(np.abs(sv.cat5[:, 3:63].astype(np.float64) - pe64) <= allowed)
