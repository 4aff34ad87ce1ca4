"""The fused MLP inference kernels -- nerf_fwd_x16_kernel<bf16 | f16>, nerf_fwd_x16s_kernel (bf16x3) and nerf_fwd_f32_kernel -- pinned per
entry at their only outputs, `part` and `wlocal` in the caller-owned workspace, against the format-following float64 chain of the
kernel's own inputs: the bytes of the n3dt_mlp_pack buffer, the fold table (and rayfold) of the same call's workspace, the float32
points / plane distances / z values of ops.sample_points (the one device function the fused kernels call), and for the 16-bit kernels
the kernel's own PE fragments (n3dt_x16_pe_probe, form 0).  The rules, the units and their floors are in tests/mlp_stagewise.py; every
bound is 4 x a floor that test_mlp_stagewise_cpu.py re-measures on the CPU, nothing is taken from a GPU run.

Every case of head_stagewise.CASES at every precision (the calls are test_gpu_head_stagewise.run's, cached per process): the ragged
second block, workgroups spanning frames, bpr = 1, 64 blocks a ray in fp32, saturating alpha, gaze offsets, the per-ray vd table.
The bitwise properties of the seam (rays reversed, one frame alone, 0xFF prefill) on cases ragged and span."""
import functools

import numpy as np
import pytest
import torch

import head_stagewise as hs
import mlp_stagewise as ms
import x16_stagewise as xs
from test_gpu_head_stagewise import dev, device_inputs, make_geom, packed, run, same_bits

pytestmark = pytest.mark.gpu

ALL = list(hs.CASES)
WORST = {}   # (rule, precision) -> (share of the bound, where): filled by test_rules, printed by test_report


@functools.lru_cache(maxsize=None)
def geometry(name):
    """the float32 points [R, Ns, 3], plane distances and z values [R, Ns] of ops.sample_points for the case's geometry"""
    from n3dt import ops
    ci, d = hs.case_inputs(name), device_inputs(name)
    s = ops.sample_points(make_geom(ci, d, 1), d["xy"], d["R"], d["T"], d["Kinv"], d["planes"])
    torch.cuda.synchronize()
    R, Ns = ci["B"] * ci["n_rays"], ci["Ns"]
    pts = s["pts"].permute(0, 2, 3, 1).reshape(R, Ns, 3).contiguous()
    return pts, s["z_dists"].reshape(R, Ns).cpu().numpy(), s["zvals"].reshape(R, Ns).cpu().numpy()


@functools.lru_cache(maxsize=None)
def fragments(name, fmt):
    """the kernel's own 16-bit encoding of those points, [R Ns, 64] as float64 (pe_encode through the probe; the decoding of test_gpu_pe_pairs.py)"""
    from n3dt import ops
    pts = geometry(name)[0].reshape(-1, 3)
    n = pts.shape[0]
    pad = torch.zeros(((-n) % 32, 3), dtype=torch.float32, device=pts.device)
    out = ops.x16_pe_probe(torch.cat([pts, pad]), fmt, 0)
    torch.cuda.synchronize()
    raw = out.view(torch.int16).cpu().numpy().view(np.uint16)
    return xs.bits16_to_f64(ms.pe_channels(raw)[:n], fmt)


@functools.lru_cache(maxsize=None)
def judged(name, prec):
    """the stored part / wlocal of the case's call, the reference of all its rays and the figures of every rule"""
    r = run(name, prec, "all")
    ci, p = r["ci"], r["p"]
    W = ms.decode_packed(packed(name, prec)[1], p)
    o = hs.bias_offset(10)
    b10 = r["rayfold"] if ci["vd"] else np.repeat(r["fold"][:, o:o + hs.G], ci["n_rays"], axis=0)
    pts, dist, zval = geometry(name)
    pts = pts.cpu().numpy()
    pe16 = fragments(name, hs.FMT16[p]) if p != hs.F32 else None
    src = ms.make_source(name, prec, W, r["fold"], np.ascontiguousarray(b10), pts, dist, zval, ms.pe_inputs(p, pts.reshape(-1, 3), pe16))
    ref = ms.reference(src, np.arange(r["R"]))
    return r, ms.judge(ref, r["part"], r["wlocal"], prec)


@pytest.mark.parametrize("prec", ms.PRECISIONS)
@pytest.mark.parametrize("name", ALL)
def test_rules(name, prec):
    """rules 1 - 7 of mlp_stagewise on every block of the case: the density read back through wlocal per sample and as a block's rms, every
    live weight inside its interval, part[:192] teacher-forced on the stored weights per entry and as a block's rms, part[G + 1],
    part[G + 2], the zero of part[G + 3] and of the dead lanes"""
    r, f = judged(name, prec)
    assert np.isfinite(r["part"]).all() and np.isfinite(r["wlocal"]).all()
    v = ms.show("%s %s" % (name, prec), f, prec)
    for k, q in v.items():
        if (k, prec) not in WORST or q > WORST[(k, prec)][0]:
            WORST[(k, prec)] = (q, name)
    assert ms.failing(v) == [], (name, prec, {k: v[k] for k in ms.failing(v)})


@pytest.mark.parametrize("prec", ms.PRECISIONS)
@pytest.mark.parametrize("name", ALL)
def test_rule_1_judges_nine_tenths_of_the_positive_densities(name, prec):
    """a condition of rule 1, not a measurement; cases deep (alpha near 1e-5) and contrast (saturating alpha) print their share only"""
    share = judged(name, prec)[1]["share"]
    print("%s %s: %.3f of the live samples with a positive reference density are judged" % (name, prec, share))
    if name in ms.SHARE_CASES:
        assert share >= ms.SHARE_MIN, (name, prec, share)


# ---------------------------------------------------------------------------------------------------------------------
# bitwise properties at the seam
# ---------------------------------------------------------------------------------------------------------------------
def render(name, prec, frames=None, reverse=False, fill=0x00):
    """part [R, bpr, 196] and wlocal [R, bpr, bs] of a call on the case's inputs: the frames `frames` only, the rays of every frame in
    reversed order"""
    from n3dt import ops
    ci, d, p = hs.case_inputs(name), device_inputs(name), hs.PRECS[prec]
    assert not ci["vd"]
    f = slice(None) if frames is None else frames
    xy = d["xy"][f]
    if reverse:
        xy = xy.flip(2)
    xy = xy.contiguous()
    B, n_rays, Ns = xy.shape[0], ci["n_rays"], ci["Ns"]
    geom = ops.make_geom(B, n_rays, Ns, 384, 256, ci["S"], ci["A"], ci["U"], hs.FEATMAP_SIZE, 2, ci["opt"].world_z1, ci["opt"].world_z2,
                         xy.stride(), 0, 1, vd_dim=0)
    carve = hs.render_carve(B, n_rays, Ns, p, 0)
    assert carve["total"] == ops.render_workspace_bytes(geom, p)
    ws = torch.full((carve["total"],), fill, dtype=torch.uint8, device=dev())
    audio = d["audio"][f].contiguous() if d["audio"] is not None else None
    ops.render_fwd(geom, p, packed(name, prec)[0], d["params"], xy, d["R"][f].contiguous(), d["T"][f].contiguous(), d["Kinv"][f].contiguous(),
                   d["shape"][f].contiguous(), d["appea"][f].contiguous(), audio, None, None, ws=ws, want_fg=True, want_merge=False,
                   want_depth=True, want_weight=True)
    torch.cuda.synchronize()
    raw = ws.cpu().numpy()
    R = B * n_rays
    part = raw[carve["part"]:carve["part"] + carve["part_used"]].view(np.float32).reshape(R, carve["bpr"], hs.PART_STRIDE)
    wlocal = raw[carve["wlocal"]:carve["wlocal"] + carve["wlocal_used"]].view(np.float32).reshape(R, carve["bpr"], carve["bs"])
    return part, wlocal


@pytest.mark.parametrize("prec", ms.PRECISIONS)
@pytest.mark.parametrize("name", ["ragged", "span"])
def test_a_block_does_not_depend_on_where_it_runs(name, prec):
    """The rays of every frame in reversed order give the rows of part and wlocal permuted, bit for bit: a block's result depends on
    neither its wave, its workgroup nor its place in the weight stream; one frame rendered alone gives the bits it has inside the
    batch; a 0xFF prefill of part and wlocal gives the bits of a zero prefill; wlocal beyond n_samples is exactly 0 in all of them."""
    ci = hs.case_inputs(name)
    B, n_rays = ci["B"], ci["n_rays"]
    base = run(name, prec, "all")
    part, wl = render(name, prec)
    assert same_bits(part, base["part"]) and same_bits(wl, base["wlocal"]), "the call without a background = the call of test_rules"
    rp, rw = render(name, prec, reverse=True)
    perm = (np.arange(B)[:, None] * n_rays + np.arange(n_rays)[::-1][None, :]).reshape(-1)
    assert same_bits(rp[perm], part), "%d rows of part differ" % int((rp[perm] != part).any(axis=(1, 2)).sum())
    assert same_bits(rw[perm], wl)
    for f in range(B):
        p1, w1 = render(name, prec, frames=slice(f, f + 1))
        assert same_bits(p1, part[f * n_rays:(f + 1) * n_rays]) and same_bits(w1, wl[f * n_rays:(f + 1) * n_rays]), "frame %d alone" % f
    fp, fw = render(name, prec, fill=0xFF)
    assert same_bits(fp, part) and same_bits(fw, wl), "0xFF prefill"
    lanes = np.arange(wl.shape[1] * wl.shape[2]).reshape(wl.shape[1:])
    for w in (wl, rw, fw):
        assert not w[:, lanes >= ci["Ns"]].view(np.uint32).any(), "wlocal beyond n_samples is exactly 0"


def test_report():
    """the largest figure per rule and precision in units of its bound, over everything test_rules compared in this process (run last;
    prints only)"""
    for (k, prec) in sorted(WORST):
        print("rule %-20s %-7s worst / bound = %.3f   (%s)" % (ms.RULES[k], prec, WORST[(k, prec)][0], WORST[(k, prec)][1]))
