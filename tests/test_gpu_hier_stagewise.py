"""The hierarchical pass on the device, per entry: fine_sample_kernel (n3dt_fine_sample) in every case of hier_stagewise.case_names() --
six shapes from the smallest legal call (3, 0) to the cap (1024, 1023: 2 rays x 2048 planes), each with the caller's u and the default
linspace, with the coarse planes recomputed (with and without t_rand) and given by the caller unevenly spaced, and the hand-made weight
patterns -- against the float64 restatement of the kernel's own float32 inputs, and the given-plane branch of n3dt_sample_point through
ops.sample_points.  The rules, the units and their floors are in tests/hier_stagewise.py; every bound is 4 x a floor that
test_hier_stagewise_cpu.py re-measures on the CPU, nothing is taken from a GPU run.  Every figure is printed before it is judged."""
import functools

import numpy as np
import pytest
import torch

import hier_stagewise as hh

pytestmark = pytest.mark.gpu

WORST = {}   # rule -> (share of the bound, where): filled by the tests, printed by test_report


def dev():
    return torch.device("cuda:0")


def t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def geom_of(cam, n_samples, given):
    from n3dt import ops
    xy = t(cam["xy"])
    return ops.make_geom(cam["B"], cam["n_rays"], n_samples, 384, 256, 179, 127, 64, 32, 2, cam["z1"], cam["z2"], xy.stride(), given), xy


def record(v, where):
    for k, q in v.items():
        if k not in WORST or q > WORST[k][0]:
            WORST[k] = (q, where)


@functools.lru_cache(maxsize=None)
def device_planes(name):
    """z_out [R, Nc + Nu] of one n3dt_fine_sample call into a 0xFF-prefilled buffer, and the Nc coarse planes [R, Nc] the kernel worked from:
    the caller's, or n3dt_sample_points' zvals for the same geometry and t_rand"""
    from n3dt import ops
    c = hh.case(name)
    cam, Nc, Nf, B, n_rays = c["cam"], c["Nc"], c["Nf"], c["B"], c["n_rays"]
    R, Nall = B * n_rays, Nc + Nf + 1
    given = c["mode"] == "given"
    geom, xy = geom_of(cam, Nc, int(given))
    T, t_rand = t(cam["T"]), t(c["t_rand"])
    if given:
        zc = c["t_rand"].reshape(R, Nc + 1)[:, :Nc].copy()
    else:
        s = ops.sample_points(geom, xy, t(cam["R"]), T, t(cam["Kinv"]), t_rand)
        zc = s["zvals"].reshape(R, Nc).cpu().numpy()
    out = torch.full((B * n_rays * Nall * 4,), 0xFF, dtype=torch.uint8, device=dev()).view(torch.float32).view(B, n_rays, Nall)
    z = ops.fine_sample(geom, Nf, t(c["weight"]).view(B, n_rays, Nc), T, t_rand=t_rand, u=t(c["u"]), out=out)
    torch.cuda.synchronize()
    assert z.data_ptr() == out.data_ptr()
    return z.cpu().numpy().reshape(R, Nall), zc


@pytest.mark.parametrize("name", hh.case_names())
def test_rules(name):
    """coarse, order, decided and undecided on every stored float of z_out"""
    c = hh.case(name)
    z_out, zc = device_planes(name)
    if c["mode"] != "given":
        d = np.abs(zc.astype(np.float64) - hh.coarse_planes32(c)).max()
        print("%s: coarse planes of n3dt_sample_points against the CPU stand-in, max |difference| %.3e" % (name, d))
        assert d <= 4 * 2.0 ** -24 * 16.0, "a plane of magnitude < 16 restated in float32: a few roundings"
    ref = hh.restate(c["weight"], zc, hh.draw_u(c))
    f = hh.judge(z_out, zc, ref, c["Nc"])
    v = hh.show(name, f)
    record(v, name)
    assert hh.failing(v) == [], (name, {k: v[k] for k in hh.failing(v)})
    if hh.is_random(name):
        assert f["undecided"] <= hh.UNDECIDED_MAX, (name, f["undecided"])


def test_a_ray_does_not_depend_on_its_prefill_or_its_neighbours():
    """the planes of one frame computed alone are the bits it has inside the batch, whatever the buffer held before"""
    from n3dt import ops
    name = "rand_66_64_jitter_caller"
    c = hh.case(name)
    base, _ = device_planes(name)
    cam, Nc, Nf, n_rays = c["cam"], c["Nc"], c["Nf"], c["n_rays"]
    for b in range(c["B"]):
        one = {k: (v[b:b + 1] if isinstance(v, np.ndarray) else v) for k, v in cam.items()}
        one["B"] = 1
        geom, _ = geom_of(one, Nc, 0)
        z = ops.fine_sample(geom, Nf, t(c["weight"][b * n_rays:(b + 1) * n_rays]).view(1, n_rays, Nc), t(one["T"]), t_rand=t(c["t_rand"][b:b + 1]),
                            u=t(c["u"][b * n_rays:(b + 1) * n_rays]))
        torch.cuda.synchronize()
        got = z.cpu().numpy().reshape(n_rays, -1)
        assert np.array_equal(got.view(np.uint32), base[b * n_rays:(b + 1) * n_rays].view(np.uint32)), "frame %d alone" % b


def test_invalid_calls_return_einval_without_a_launch():
    """more than 2048 planes a ray, fewer than three coarse samples, and z_planes_given without planes: N3DT_EINVAL (-1), and the output
    buffer keeps its prefill"""
    from n3dt import ops
    from n3dt._lib import N3dtError
    cam = hh.cameras(1, 2)
    T = t(cam["T"])

    def call(Nc, Nf, given, planes):
        geom, _ = geom_of(cam, Nc, given)
        w = torch.rand(1, 2, Nc, device=dev())
        out = torch.full((2 * (Nc + Nf + 1) * 4,), 0xFF, dtype=torch.uint8, device=dev()).view(torch.float32).view(1, 2, Nc + Nf + 1)
        tr = torch.rand(1, 2, Nc + 1, device=dev()) if planes else None
        with pytest.raises(N3dtError, match=r"\(-1\)"):
            ops.fine_sample(geom, Nf, w, T, t_rand=tr, out=out)
        torch.cuda.synchronize()
        assert bool((out.view(torch.int32) == -1).all()), "nothing was launched"

    call(1024, 1024, 0, False)   # Nall = 2049
    call(2, 4, 0, False)         # Nc = 2
    call(16, 24, 1, False)       # z_planes_given = 1 without planes


@pytest.mark.parametrize("name", ["p40", "p65", "p3"])
def test_given_planes_through_sample_points(name):
    """zvals bit for bit the given planes, dist from the pair (s, s + 1) of the ray's own Ns + 1 planes -- exactly 0 between equal planes, the last
    sample reading plane Ns, the widest interval -- and pts, per entry against float64 of the same float32 planes"""
    from n3dt import ops
    c = hh.point_case(name)
    geom, xy = geom_of(c, c["Ns"], 1)
    s = ops.sample_points(geom, xy, t(c["R"]), t(c["T"]), t(c["Kinv"]), t(c["planes"]))
    torch.cuda.synchronize()
    pts = s["pts"].permute(0, 2, 3, 1).cpu().numpy()
    f = hh.judge_points(c, pts, s["z_dists"][:, 0].cpu().numpy(), s["zvals"][:, 0].cpu().numpy())
    v = hh.show_points(name, f)
    record({"points " + k: q for k, q in v.items()}, name)
    assert hh.failing(v) == [], (name, {k: v[k] for k in hh.failing(v)})


def test_report():
    """the largest figure per rule in units of its bound, over everything compared in this process (run last; prints only)"""
    names = dict(hh.RULES, **{"points " + k: "points: " + r for k, r in hh.POINT_RULES.items()})
    for k in sorted(WORST):
        print("rule %-40s worst / bound = %.3f   (%s)" % (names[k], WORST[k][0], WORST[k][1]))
