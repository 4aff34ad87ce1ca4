"""The hierarchical pass pinned per entry: fine_sample_kernel (csrc/nerf_aux.hip:746-819) and the given-plane branch of
n3dt_sample_point (csrc/n3dt_device.h:90-93) through ops.sample_points, for tests/test_hier_stagewise_cpu.py and
tests/test_gpu_hier_stagewise.py.  A helper module, not a test file: CPU only.

fine_sample_kernel is a discontinuous function of its input (an upper bound into a float32 cumulative sum, a threshold on a difference
of two of its entries, two clamps, a stable rank sort), so a flat tolerance either hides a wrong decision or fails on a right one.
The reference is restate(): the kernel's arithmetic in float64 from the kernel's own float32 inputs -- the weights [R, Nc], the Nc
coarse planes as float32 values (the caller's, or what n3dt_sample_points stores as zvals for the same geometry and t_rand), and u (the
caller's, or linspace01(float32): its three operations are single IEEE roundings, so the float32 u is reproduced bit for bit).  The two
constants 1e-5f are the float32 value.  emulate() is the same chain in float32, in the orders of VARIANTS (the kernel's strided partial
sums and xor butterfly, the butterfly in the other direction, numpy's pairwise sum; z in two roundings and as one fma); it is the source
of the floors and the stand-in of the kernel on a machine without a GPU.

A defect this pin found (rule order: a slot keeps its prefill): with n_fine = 0 the kernel's default u was n3dt_linspace01(0, 1) = 1 - (1 / 0) 0,
a NaN, where torch.linspace(0, 1, 1) is [0]; the NaN took rank 0 in the sort together with the nearest plane and one output slot stayed
unwritten.  emulate(fault="linspace_nu1") is that kernel.

Every stored float of z_out [R, Nc + Nu], Nu = n_fine + 1, is judged by one of the rules (judge()):
  coarse     the Nc coarse planes appear in the output bit for bit (as a multiset: figure `coarse` counts those missing).
  order      the output is non-decreasing (`order`), no slot keeps the 0xFF prefill written before the call and nothing is NaN
             (`prefill`), and what is left after the coarse planes are taken out is exactly Nu values (`count`).
  decided    a draw is decided if (a) for every cdf entry j, |u - cdf_j| > delta_c(j), or delta_c(j) = 0 (then the float32 entry is
             the float64 one: a sum of exact zeros), and (b) |denom - 1e-5f| > 2 delta_c(above).  Its device value must be within
                 U_z cond,   cond = |b1 - b0| ((1 + 2 t) delta_c(above) / denom + 2 t u32) + u32 (|b0| + |b1| + |z|),   t = |u - c0| / denom
             of the float64 value: c0 moves by delta_c and the subtraction u - c0 rounds (u32 |u - c0|, inside 2 t u32); denom moves by 2 delta_c,
             which t multiplies; the division rounds (t u32); the midpoints b0, b1 round twice each and b1 - b0, the product and the
             sum once each, all inside u32 (|b0| + |b1| + |z|) with the factor 4 of the unit.  denom is the kept difference or the 1 that
             replaces it.  u32 = 2^-24.
  undecided  every other draw must lie inside the hull of the float64 values of every decision its float32 cdf could take: every
             inds between #{cdf_j + delta_c(j) <= u} and #{cdf_j - delta_c(j) <= u} (inds +- 1 and beyond, where several entries lie
             within delta_c of u), either side of the denom switch where |denom - 1e-5f| <= 2 delta_c, widened by U_z cond of that decision.
             Cap, a condition and not a measurement: at most UNDECIDED_MAX of the draws of any random case are undecided.
  delta_c(j) = U_cdf growth(j),  growth(j) = u32 (sqrt(sum_{2 <= k <= j} cdf_k^2) + (NTOT + 2) cdf_j): every addition of the sequential sum
             rounds at the size of its result, cdf_k, and the roundings of a sum of positive terms are independent in sign, so they add in
             quadrature (the worst case, sum_k cdf_k, is nearly 30 times larger at entry 1000 and left up to 3.8 % of the draws of
             (1024, 1023) undecided when it was tried; the measured floor times 4 is what makes the quadrature a bound: the emulations' worst entry is 0.38 of it); every
             pdf carries its division's rounding and the relative error of the normaliser, which are common to all terms and add
             linearly: NTOT = 8 + ceil((Nc - 2) / 64) roundings (+1e-5f, the strided partial sums, six butterfly steps).
             Where below == above (u before the first or past the last entry) denom is exactly 0 in any precision and the switch certain.
How ties are matched.  The sort scrambles positions, so the Nu device values (ascending, coarse planes removed) meet the reference draws
as ORDER STATISTICS: with [L_i, H_i] the interval of draw i (decided: z_i -+ U_z cond_i; undecided: its widened hull), the k-th smallest
device value must be >= the k-th smallest L and <= the k-th smallest H.  That is necessary for ANY assignment of values to draws, so a
right kernel never fails it, and it is no weaker than judging each value of a tie cluster by the cluster's largest tolerance: at most
k - 1 draws have L_i below (z - tau_max)_(k).  The figure `z` is the smallest scale s of all the tolerances at which the condition holds
(s <= 1 passes): the worst share of the bound.

Given planes through n3dt_sample_points (judge_points()): zvals equal planes[..., :-1] bit for bit; dist within U_dist |z_hi - z_lo| |l| of
the float64 (z_hi - z_lo) l of the float32 planes and exactly 0 where two planes are equal -- the difference of two given planes is the
kernel's only subtraction, so the bound scales with the distance itself (the floor carries the rounding of l); pts within
f32_stagewise.bound("geo") S_pts, S_pts = |T| + |d l| max |plane|, as f32_stagewise.sample judges them.

Units: U_family = FACTOR x FLOOR[family]; a floor is the largest figure of the float32 emulations against the float64 restatement over
all CASES; test_hier_stagewise_cpu.py re-measures every one.  No number comes from a GPU run.
"""
import functools

import numpy as np

import f32_stagewise as fs

U32 = 2.0 ** -24
EPS32 = float(np.float32(1e-5))      # the kernel's 1e-5f, in the normaliser and in the denom switch
FACTOR = 4.0
UNDECIDED_MAX = 0.02
WORLD_Z1, WORLD_Z2 = 2.5, -3.5
PREFILL = np.uint32(0xFFFFFFFF)

# ---- the measured floors (test_hier_stagewise_cpu.py prints each beside its constant and fails unless measured <= recorded <= 1.25 x)
FLOOR = {
    "cdf": 0.39,     # measured 0.382 (rand_16_24_geom_linspace, pairwise_fma)
    "z": 0.66,       # measured 0.651 (rand_16_24_given_linspace, every variant: the roundings of a midpoint near a power of two)
    "dist": 1.25e-7,  # measured 1.241e-7 (p40)
}
FAMILIES = tuple(FLOOR)
VARIANTS = ("lanes", "lanes_fma", "lanes_up", "pairwise_fma")


def unit(family):
    return FACTOR * FLOOR[family]


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
SHAPES = {   # (Nc, Nf) -> (B, rays per frame)
    (3, 0): (2, 2), (16, 24): (2, 3), (64, 128): (2, 2), (66, 64): (2, 2), (130, 70): (1, 3), (1024, 1023): (2, 1),
}
PLANE_MODES = ("geom", "jitter", "given")   # z_planes_given 0 without t_rand, 0 with t_rand, 1 with the caller's planes
U_MODES = ("linspace", "caller")
PATTERNS = ("zero", "onehot", "switch", "uedge", "ends")
PATTERN_SHAPES = ((16, 24), (66, 64))


def case_names():
    names = ["rand_%d_%d_%s_%s" % (nc, nf, pm, um) for (nc, nf) in SHAPES for pm in PLANE_MODES for um in U_MODES]
    return names + ["%s_%d_%d" % (p, nc, nf) for p in PATTERNS for (nc, nf) in PATTERN_SHAPES]


def is_random(name):
    return name.startswith("rand_")


def cameras(B, n_rays):
    """a camera per frame with its own T (so that T[b] and rayg / n_rays matter) and integer pixel rays, float32"""
    T = np.array([[0.10, -0.20, 12.0], [-0.30, 0.25, 11.5], [0.05, 0.15, 12.25]], dtype=np.float32)[:B]
    R = np.zeros((B, 3, 3), dtype=np.float32)
    for b in range(B):
        a = 0.2 * b - 0.1
        R[b] = np.array([[np.cos(a), 0, np.sin(a)], [0, -1, 0], [np.sin(a), 0, -np.cos(a)]], dtype=np.float32)
    Kinv = np.tile(np.array([[1 / 75.0, 0, -16 / 75.0], [0, 1 / 75.0, -16 / 75.0], [0, 0, 1]], dtype=np.float32), (B, 1, 1))
    px = (np.arange(n_rays) * 37 + 5) % 32
    py = (np.arange(n_rays) * 11 + 3) % 32
    xy = np.tile(np.stack([px, py]).astype(np.float32)[None], (B, 1, 1))
    xy[1:, 0] += 1.0
    return {"B": B, "n_rays": n_rays, "xy": xy, "R": R, "T": T, "Kinv": Kinv, "z1": WORLD_Z1, "z2": WORLD_Z2}


def uneven_planes(rng, R, n, lo=8.0, hi=16.0):
    """[R, n] ascending float32 planes that are NOT uniformly spaced: sorted draws, per ray"""
    return np.sort(lo + (hi - lo) * rng.random((R, n)) ** 2, axis=1).astype(np.float32)


def random_weights(rng, R, Nc):
    """compositing-like weights: a peak or two over a small noisy floor, some exact zeros, the end weights live"""
    j = np.arange(Nc)[None, :]
    c = rng.random((R, 1)) * Nc
    s = 1.0 + rng.random((R, 1)) * Nc / 6
    w = 0.6 * np.exp(-((j - c) / s) ** 2) + 0.02 * rng.random((R, Nc)) ** 3
    w[rng.random((R, Nc)) < 0.1] = 0.0
    w[:, 0], w[:, -1] = 0.3, 0.2
    return w.astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(name):
    """name -> dict(Nc, Nf, B, n_rays, weight [R, Nc] f32, u [R, Nu] f32 or None, mode, t_rand [B, n_rays, Nc + 1] f32 or None, cam)
    In mode "given" t_rand holds the caller's planes (the far edge is not read: it is set to NaN bits so that a read would show)."""
    parts = name.split("_")
    Nc, Nf = (int(parts[1]), int(parts[2])) if is_random(name) else (int(parts[-2]), int(parts[-1]))
    B, n_rays = SHAPES[(Nc, Nf)]
    R, Nu = B * n_rays, Nf + 1
    rng = np.random.default_rng(abs(hash_name(name)))
    c = {"name": name, "Nc": Nc, "Nf": Nf, "B": B, "n_rays": n_rays, "cam": cameras(B, n_rays)}
    mode, umode = (parts[3], parts[4]) if is_random(name) else ("given", "caller")
    w = random_weights(rng, R, Nc)
    u = rng.random((R, Nu)).astype(np.float32) if umode == "caller" else None
    if mode == "given":
        t_rand = np.full((R, Nc + 1), np.nan, dtype=np.float32)
        t_rand[:, :Nc] = uneven_planes(rng, R, Nc)
    elif mode == "jitter":
        t_rand = rng.random((R, Nc + 1)).astype(np.float32)
    else:
        t_rand = None
    if not is_random(name):
        w, u = pattern(parts[0], rng, w, u, t_rand[:, :Nc])
    c.update(weight=w, u=u, mode=mode, t_rand=None if t_rand is None else t_rand.reshape(B, n_rays, Nc + 1))
    return c


def hash_name(name):
    h = 2166136261
    for ch in name.encode():
        h = ((h ^ ch) * 16777619) & 0xFFFFFFFF
    return h


def pattern(kind, rng, w, u, zc):
    """the hand-made weight patterns (ISSUE: cases); u is the caller's [R, Nu]"""
    R, Nc = w.shape
    Nu = u.shape[1]
    if kind == "zero":          # cdf all zero: every draw takes inds = Nc - 1, denom -> 1, all Nu values equal bins[Nc - 2]
        w[:, 1:-1] = 0.0
    elif kind == "onehot":      # flat cdf runs on both sides: right=True must step over the whole run
        w[:, 1:-1] = 0.0
        for r in range(R):
            w[r, 1 + (3 + 5 * r) % (Nc - 4) + 1] = 0.7
        u[:, 0], u[:, -1] = 0.0, 1.0
    elif kind == "switch":      # one denom just under and one just over 1e-5, early in the sum where delta_c is smallest
        w[:, 1:-1] = (0.2 + 0.8 * rng.random((R, Nc - 2))).astype(np.float32)
        tot = (w[:, 3:-1].astype(np.float64) + EPS32).sum(1)
        w[:, 1], w[:, 2] = (0.8e-5 * tot).astype(np.float32), (1.2e-5 * tot).astype(np.float32)
        u[:, 0], u[:, 1], u[:, 2] = 0.4e-5, 1.4e-5, 1.9e-5
    elif kind == "uedge":       # u exactly 0, exactly 1, exactly a float32 cdf entry and one float32 step either side of it
        cdf32 = emulate(w, zc, u, "lanes")["cdf"]
        for r in range(R):
            j = 2 + (3 * r) % (Nc - 4)
            e = cdf32[r, j]
            u[r, :5] = [0.0, 1.0, e, np.nextafter(e, np.float32(0)), np.nextafter(e, np.float32(2))]
    elif kind == "ends":        # the end weights must not enter the pdf
        w[:, 0], w[:, -1] = 3.0e4, 7.0e4
    else:
        raise ValueError(kind)
    return w, u


def coarse_planes32(c):
    """the Nc coarse planes [R, Nc] in float32 as the CPU stand-in forms them (on the GPU: n3dt_sample_points' zvals)"""
    Nc, R = c["Nc"], c["B"] * c["n_rays"]
    if c["mode"] == "given":
        return c["t_rand"].reshape(R, Nc + 1)[:, :Nc].copy()
    z, _ = fs.edges(np.float32, c["cam"]["T"][:, 2], WORLD_Z1, WORLD_Z2, Nc, c["t_rand"])
    return np.ascontiguousarray(np.broadcast_to(z, (c["B"], c["n_rays"], Nc + 1)).reshape(R, Nc + 1)[:, :Nc])


# ---------------------------------------------------------------------------------------------------------------------
# the restatement (float64) and the emulation (float32)
# ---------------------------------------------------------------------------------------------------------------------
def linspace01(dt, n):
    """n3dt_linspace01 (n3dt_device.h:27) in dtype dt; torch.linspace(0, 1, 1) is [0]"""
    if n == 1:
        return np.zeros(1, dtype=dt)
    step = dt(1) / dt(n - 1)
    i = np.arange(n)
    return np.where(i < n // 2, step * i.astype(dt), dt(1) - step * (n - 1 - i).astype(dt)).astype(dt)


def draw_u(c):
    """the float32 u [R, Nu] the kernel works from"""
    R, Nu = c["B"] * c["n_rays"], c["Nf"] + 1
    return c["u"] if c["u"] is not None else np.ascontiguousarray(np.broadcast_to(linspace01(np.float32, Nu), (R, Nu)))


def decisions(cdf, u, Nc):
    inds = (cdf[:, None, :] <= u[:, :, None]).sum(-1)
    return inds, np.maximum(inds - 1, 0), np.minimum(inds, Nc - 2)


def take(a, idx):
    return np.take_along_axis(a, idx, axis=1)


def restate(weight, zc, u):
    """fine_sample_kernel in float64 from float32 weight [R, Nc], coarse planes zc [R, Nc], u [R, Nu] -> the draws z [R, Nu], every
    intermediate, and planes [R, Nc + Nu] (stable sort of coarse ++ draws)"""
    w, zc, u = (np.asarray(a, dtype=np.float64) for a in (weight, zc, u))
    Nc = w.shape[1]
    total = (w[:, 1:Nc - 1] + EPS32).sum(1)
    cdf = np.concatenate([np.zeros((w.shape[0], 1)), np.cumsum(w[:, 1:Nc - 1] / total[:, None], axis=1)], axis=1)   # [R, Nc - 1]
    bins = 0.5 * (zc[:, 1:] + zc[:, :-1])                                                                       # [R, Nc - 1]
    inds, below, above = decisions(cdf, u, Nc)
    out = value64(cdf, bins, u, below, above)
    out.update(total=total, cdf=cdf, bins=bins, inds=inds, u=u, planes=np.sort(np.concatenate([zc, out["z"]], axis=1), axis=1, kind="stable"))
    return out


def value64(cdf, bins, u, below, above, switch=None):
    """the float64 value of a draw under the decision (below, above) and the denom switch (None: decided by denom itself)"""
    c0, c1, b0, b1 = take(cdf, below), take(cdf, above), take(bins, below), take(bins, above)
    raw = c1 - c0
    sw = (raw < EPS32) if switch is None else switch
    denom = np.where(sw, 1.0, raw)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (u - c0) / denom
        z = b0 + t * (b1 - b0)
    return {"z": z, "c0": c0, "b0": b0, "b1": b1, "raw": raw, "denom": denom, "t": t, "below": below, "above": above}


def f32sum_lanes(x, up=False):
    """[R, n] float32 -> the kernel's sum: lane l adds x[l], x[l + 64], ... in sequence, then the xor butterfly 32, 16, .., 1
    (up: 1, 2, .., 32, the other tree of the same depth)"""
    R, n = x.shape
    pad = np.zeros((R, (-n) % 64), dtype=np.float32)
    rows = np.concatenate([x, pad], axis=1).reshape(R, -1, 64)
    part = np.zeros((R, 64), dtype=np.float32)
    for k in range(rows.shape[1]):
        live = (k * 64 + np.arange(64)) < n
        part = np.where(live[None], part + rows[:, k], part)
    lanes = np.arange(64)
    for off in ((1, 2, 4, 8, 16, 32) if up else (32, 16, 8, 4, 2, 1)):
        part = part + part[:, lanes ^ off]
    return part[:, 0]


def rank_sort(vals, tie_break=True):
    """the kernel's rank sort of [R, N] float32 into a 0xFF-prefilled output: out[rank] = v, rank = #{o < v} + #{o == v, j < i}"""
    R, N = vals.shape
    out = np.full((R, N), PREFILL, dtype=np.uint32).view(np.float32)
    idx = np.arange(N)
    for r in range(R):
        v = vals[r]
        with np.errstate(invalid="ignore"):
            less = (v[None, :] < v[:, None]).sum(1)
            if tie_break:
                less = less + ((v[None, :] == v[:, None]) & (idx[None, :] < idx[:, None])).sum(1)
        out[r, less] = v
    return out


FAULTS = ("right_false", "above_nc1", "switch_le", "no_switch", "eps_numerator", "cumsum_w0", "bins_lower", "u_over_nu", "no_tie_break",
          "draws_ge_64", "T_frame0", "u_stride_nc", "linspace_nu1")


def emulate(weight, zc, u, variant="lanes", fault=None, c=None):
    """fine_sample_kernel in float32.  variant: "lanes" the kernel's normaliser (strided partial sums, xor butterfly) and z in two roundings;
    "lanes_fma" the same with z as one fma; "seq" a sequential normaliser (the oracle's order); "pairwise_fma" numpy's pairwise sum and fma.
    The cumulative sum is sequential and the division float32 in all of them.  fault: one of FAULTS (c: the case, for the faults of the
    launch geometry).  -> z_out [R, Nc + Nu] float32 (rank sort into a 0xFF prefill), the draws, cdf, inds and the switch."""
    f1, eps = np.float32(1), np.float32(1e-5)
    w = np.ascontiguousarray(weight, dtype=np.float32)
    zc = np.ascontiguousarray(zc, dtype=np.float32)
    u = np.ascontiguousarray(u, dtype=np.float32)
    R, Nc = w.shape
    Nu = u.shape[1]
    if fault == "T_frame0" and c is not None and c["mode"] != "given":     # every frame takes T of frame 0
        c0 = dict(c, cam=dict(c["cam"], T=np.repeat(c["cam"]["T"][:1], c["B"], axis=0)))
        zc = coarse_planes32(c0)
    if fault == "u_over_nu" and c is not None and c["u"] is None:
        u = np.ascontiguousarray(np.broadcast_to((np.arange(Nu, dtype=np.float32) / np.float32(Nu)).astype(np.float32), (R, Nu)))
    if fault == "linspace_nu1" and c is not None and c["u"] is None and Nu == 1:
        u = np.full((R, 1), np.nan, dtype=np.float32)    # n3dt_linspace01(0, 1): step = 1 / 0, 1 - inf * 0 (the kernel before the n_fine = 0 fix)
    if fault == "u_stride_nc" and c is not None and c["u"] is not None:   # u_in[rayg * Nc + i]
        flat = np.concatenate([u.reshape(-1), np.zeros(R * max(Nc - Nu, 0) + Nc, dtype=np.float32)])
        u = np.stack([flat[r * Nc:r * Nc + Nu] for r in range(R)])
    x = w[:, 1:Nc - 1] + eps
    if variant in ("lanes", "lanes_fma", "lanes_up"):
        total = f32sum_lanes(x, up=variant == "lanes_up")
    else:
        total = x.sum(1, dtype=np.float32)
    num = x if fault == "eps_numerator" else w[:, 1:Nc - 1]
    pdf = (num / total[:, None]).astype(np.float32)
    cdf = np.zeros((R, Nc - 1), dtype=np.float32)
    run = (w[:, 0] / total).astype(np.float32) if fault == "cumsum_w0" else np.zeros(R, dtype=np.float32)
    cdf[:, 0] = run if fault == "cumsum_w0" else 0
    for j in range(Nc - 2):
        run = run + pdf[:, j]
        cdf[:, j + 1] = run
    if fault == "right_false":
        inds = (cdf[:, None, :] < u[:, :, None]).sum(-1)
    else:
        inds = (cdf[:, None, :] <= u[:, :, None]).sum(-1)
    below = np.maximum(inds - 1, 0)
    above = np.minimum(inds, Nc - 1 if fault == "above_nc1" else Nc - 2)
    # the kernel's LDS: zc [Nc], cdf [Nc - 1], all [Nall] -- an index past an array reads its neighbour (fault above_nc1)
    lds_zc = np.concatenate([zc, cdf, zc], axis=1)
    lds_cdf = np.concatenate([cdf, zc], axis=1)
    c0, c1 = take(lds_cdf, below), take(lds_cdf, above)
    if fault == "bins_lower":
        b0, b1 = take(lds_zc, below), take(lds_zc, above)
    else:
        b0 = np.float32(0.5) * (take(lds_zc, below + 1) + take(lds_zc, below))
        b1 = np.float32(0.5) * (take(lds_zc, above + 1) + take(lds_zc, above))
    raw = c1 - c0
    if fault == "no_switch":
        sw = np.zeros(raw.shape, dtype=bool)
    elif fault == "switch_le":
        sw = raw <= eps
    else:
        sw = raw < eps
    denom = np.where(sw, f1, raw)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = ((u - c0) / denom).astype(np.float32)
        if variant.endswith("fma"):
            z = (b0.astype(np.float64) + t.astype(np.float64) * (b1 - b0).astype(np.float64)).astype(np.float32)   # 24 x 24 bits: exact in float64
        else:
            z = b0 + t * (b1 - b0)
    if fault == "draws_ge_64":
        z = z.copy()
        z[:, 64:] = np.full(z[:, 64:].shape, PREFILL, dtype=np.uint32).view(np.float32)   # LDS never written: whatever it held
    z_out = rank_sort(np.concatenate([zc, z], axis=1), tie_break=fault != "no_tie_break")
    return {"z_out": z_out, "z": z, "cdf": cdf, "inds": inds, "switch": sw, "raw": raw, "total": total, "zc": zc}


# ---------------------------------------------------------------------------------------------------------------------
# the rules
# ---------------------------------------------------------------------------------------------------------------------
def growth(cdf64, Nc):
    """[R, Nc - 1]: what one unit of float32 rounding does to cdf entry j along the sequential sum (module docstring)"""
    ntot = 8 + (Nc - 2 + 63) // 64
    tail = np.cumsum(cdf64 ** 2, axis=1) - (cdf64[:, :2] ** 2).sum(1, keepdims=True)       # sum_{2 <= k <= j} cdf_k^2
    return U32 * (np.sqrt(np.maximum(tail, 0.0)) + (ntot + 2) * cdf64)


def cond_of(v, dc):
    """the decided rule's conditioning of a draw under the decision of v (value64), dc = delta_c(above)"""
    with np.errstate(invalid="ignore", divide="ignore"):
        t = np.abs(v["t"])
        return np.abs(v["b1"] - v["b0"]) * ((1 + 2 * t) * dc / v["denom"] + 2 * t * U32) + U32 * (np.abs(v["b0"]) + np.abs(v["b1"]) + np.abs(v["z"]))


def intervals(ref, Nc, u_cdf=None):
    """per draw: decided?, and the interval ends lo, hi [R, Nu] with the tolerance tol [R, Nu] that widens them (scaled by s in judge())"""
    u_cdf = unit("cdf") if u_cdf is None else u_cdf
    cdf, bins, u = ref["cdf"], ref["bins"], ref["u"]
    delta = u_cdf * growth(cdf, Nc)                                            # [R, Nc - 1]
    near = (np.abs(u[:, :, None] - cdf[:, None, :]) <= delta[:, None, :]) & (delta[:, None, :] > 0)
    i_min = ((cdf + delta)[:, None, :] <= u[:, :, None]).sum(-1)
    i_max = ((cdf - delta)[:, None, :] <= u[:, :, None]).sum(-1)
    i_min, i_max = np.minimum(i_min, ref["inds"]), np.maximum(i_max, ref["inds"])
    dc = take(delta, ref["above"])
    # (below == above, past the last entry or before the first: the difference is exactly 0 in any precision, the switch certain)
    sw_open = (np.abs(ref["raw"] - EPS32) <= 2 * dc) & (ref["below"] != ref["above"])
    decided = ~near.any(-1) & ~sw_open
    lo, hi = ref["z"].copy(), ref["z"].copy()
    tol = unit("z") * cond_of(ref, dc)
    span = int((i_max - i_min).max())
    for k in range(span + 1):
        inds = np.minimum(i_min + k, i_max)
        below, above = np.maximum(inds - 1, 0), np.minimum(inds, Nc - 2)
        dck = take(delta, above)
        raw = take(cdf, above) - take(cdf, below)
        for sw in (False, True):
            ok = ~decided & (((np.abs(raw - EPS32) <= 2 * dck) & (below != above)) | ((raw < EPS32) == sw))
            if not ok.any():
                continue
            v = value64(cdf, bins, u, below, above, np.full(raw.shape, sw))
            tk = unit("z") * cond_of(v, dck)
            lo, hi = np.where(ok, np.minimum(lo, v["z"]), lo), np.where(ok, np.maximum(hi, v["z"]), hi)
            tol = np.where(ok, np.maximum(tol, tk), tol)
    return {"decided": decided, "lo": lo, "hi": hi, "tol": tol, "delta": delta, "span": span}


def split_coarse(z_out, zc):
    """per ray: the device values left after the Nc coarse planes are taken out bit for bit (ascending order kept), and how many coarse
    planes were not found"""
    rest, missing = [], 0
    ob, cb = np.ascontiguousarray(z_out, dtype=np.float32).view(np.uint32), np.ascontiguousarray(zc, dtype=np.float32).view(np.uint32)
    for r in range(ob.shape[0]):
        need = {}
        for b in cb[r].tolist():
            need[b] = need.get(b, 0) + 1
        keep = np.ones(ob.shape[1], dtype=bool)
        for i, b in enumerate(ob[r].tolist()):
            if need.get(b, 0) > 0:
                need[b] -= 1
                keep[i] = False
        missing += sum(need.values())
        rest.append(z_out[r][keep])
    return rest, missing


def order_stat_share(d, iv):
    """the smallest scale s of the tolerances at which the sorted device values d [Nu] meet the order statistics of the intervals"""
    def holds(s):
        L, H = np.sort(iv["lo"] - s * iv["tol"]), np.sort(iv["hi"] + s * iv["tol"])
        return bool(np.all(d >= L) and np.all(d <= H))
    if holds(0.0):
        return 0.0
    hi = 1.0
    while not holds(hi):
        hi *= 4.0
        if hi > 1e12:
            return float("inf")
    lo = 0.0
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        lo, hi = (lo, mid) if holds(mid) else (mid, hi)
    return hi


def judge(z_out, zc, ref, Nc):
    """every rule on z_out [R, Nc + Nu] float32 -> figures: exact rules as violation counts (`coarse`, `order`, `prefill`, `count`), `z`
    as the worst share of the decided / undecided bound, and the undecided share of the draws"""
    z_out = np.ascontiguousarray(z_out, dtype=np.float32)
    Nu = ref["u"].shape[1]
    f = {}
    f["prefill"] = int((z_out.view(np.uint32) == PREFILL).sum() + np.isnan(z_out).sum())
    with np.errstate(invalid="ignore"):
        f["order"] = int((~(z_out[:, 1:] >= z_out[:, :-1])).sum())
    rest, f["coarse"] = split_coarse(z_out, zc)
    f["count"] = int(sum(abs(len(v) - Nu) for v in rest))
    iv = intervals(ref, Nc)
    f["undecided"] = float((~iv["decided"]).mean())
    f["span"] = iv["span"]
    worst = 0.0
    for r, d in enumerate(rest):
        if len(d) != Nu or np.isnan(d).any():
            worst = float("inf")
            continue
        worst = max(worst, order_stat_share(np.sort(d.astype(np.float64)), {k: iv[k][r] for k in ("lo", "hi", "tol")}))
    f["z"] = worst
    return f


RULES = {"coarse": "coarse", "order": "order (non-decreasing)", "prefill": "order (no prefill, no NaN)", "count": "order (multiset)", "z": "decided / undecided"}


def verdict(f):
    """figure -> its share of the bound (<= 1 passes); the exact rules count violations (0 passes)"""
    v = {k: (float("inf") if f[k] else 0.0) for k in ("coarse", "order", "prefill", "count")}
    v["z"] = f["z"]
    return v


def failing(v):
    return sorted(k for k, r in v.items() if not r <= 1.0)


def show(tag, f):
    """prints every figure of one judged call before it is asserted"""
    v = verdict(f)
    print("%-44s z %.3f of its bound | violations: coarse %d order %d prefill %d count %d | undecided %.4f of the draws (inds span %d)"
          % (tag, v["z"], f["coarse"], f["order"], f["prefill"], f["count"], f["undecided"], f["span"]))
    return v


def floors_of(em, ref, Nc):
    """the float32 emulation's own error in the units of the rules: cdf entries against growth(), and the draws it decided as the reference
    did against cond (with delta_c at the committed unit)"""
    g = growth(ref["cdf"], Nc)
    e = np.abs(em["cdf"].astype(np.float64) - ref["cdf"])
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(e == 0, 0.0, e / g)
    iv = intervals(ref, Nc)
    same = iv["decided"] & (em["inds"] == ref["inds"]) & (em["switch"] == (ref["raw"] < EPS32))
    dc = take(iv["delta"], ref["above"])
    cz = cond_of(ref, dc)
    ez = np.abs(em["z"].astype(np.float64) - ref["z"])
    with np.errstate(divide="ignore", invalid="ignore"):
        qz = np.where(same & (ez > 0), ez / cz, 0.0)
    return {"cdf": float(q.max()), "z": float(qz.max()), "wrongly_decided": int((iv["decided"] & ~same).sum())}


# ---------------------------------------------------------------------------------------------------------------------
# given planes for the other pins (head_stagewise, mlp_stagewise, f32_stagewise, x16_stagewise)
# ---------------------------------------------------------------------------------------------------------------------
EDGE_RAY = 1   # the ray (of frame 0) whose planes are overwritten by hand


def given_planes(Tz, n_rays, Nc, Nf, seed=0, z1=WORLD_Z1, z2=WORLD_Z2):
    """[B, n_rays, Nc + Nf + 1] float32 fine planes of a hierarchical pass, made by restate() -- seeded peaked coarse weights over the
    uniform coarse planes of each frame's T_z, the default linspace u -- and rounded ONCE to float32 (so a pin that takes them does not
    depend on fine_sample_kernel).  Ray EDGE_RAY of frame 0 is overwritten by hand: all its fine planes inside one coarse bin, among them
    two pairs of equal planes and a run of five planes one float32 step apart; the far plane (the last coarse one) is not repeated, so
    the last sample's distance is not 0."""
    Tz = np.asarray(Tz, dtype=np.float32)
    B, R, Nu = len(Tz), len(Tz) * n_rays, Nf + 1
    rng = np.random.default_rng(1000 + seed)
    z, _ = fs.edges(np.float32, Tz, z1, z2, Nc, None)
    zc = np.ascontiguousarray(np.broadcast_to(z, (B, n_rays, Nc + 1)).reshape(R, Nc + 1)[:, :Nc])
    u = np.broadcast_to(linspace01(np.float32, Nu), (R, Nu))
    planes = restate(random_weights(rng, R, Nc), zc, u)["planes"].astype(np.float32)
    assert Nu >= 12 and Nc >= 8
    lo, hi = zc[EDGE_RAY, Nc // 2], zc[EDGE_RAY, Nc // 2 + 1]
    fine = np.sort((lo + (hi - lo) * (0.05 + 0.9 * rng.random(Nu))).astype(np.float32))
    fine[1], fine[4] = fine[0], fine[3]                        # two pairs of equal planes
    for k in range(1, 5):                                      # a run of five planes one float32 step apart
        fine[6 + k] = np.nextafter(fine[6 + k - 1], np.float32(np.inf))
    planes[EDGE_RAY] = np.sort(np.concatenate([zc[EDGE_RAY], fine]), kind="stable")
    p = planes[EDGE_RAY]
    assert (np.diff(planes, axis=1) >= 0).all() and (np.diff(p) == 0).sum() == 2 and p[-1] > p[-2] and lo < fine.min() and fine.max() < hi
    return planes.reshape(B, n_rays, Nc + Nu)


# ---------------------------------------------------------------------------------------------------------------------
# given planes through n3dt_sample_points
# ---------------------------------------------------------------------------------------------------------------------
POINT_FAULTS = ("stride_ns", "zhi_next_ray", "dist_prev_pair")


@functools.lru_cache(maxsize=None)
def point_case(name):
    """given-plane geometry: B = 2, planes [B, n_rays, Ns + 1] ascending and uneven with the LAST interval the widest (so that a sample
    Ns - 1 that did not read plane Ns shows), two pairs of equal planes and a run of five planes one float32 step apart in ray 1"""
    B, n_rays, Ns = {"p40": (2, 5, 40), "p65": (2, 3, 65), "p3": (2, 2, 3)}[name]
    rng = np.random.default_rng(hash_name(name))
    R = B * n_rays
    p = uneven_planes(rng, R, Ns + 1, 8.0, 14.0)
    p[:, -1] = p[:, -2] + np.float32(2.0) * (p[:, 1:-1] - p[:, :-2]).max(1) + np.float32(0.5)
    if Ns >= 40:
        p[1, 3], p[1, 20] = p[1, 4], p[1, 21]
        for k in range(1, 5):
            p[1, 10 + k] = np.nextafter(p[1, 10 + k - 1], np.float32(100))
        assert (np.diff(p[1]) >= 0).all()
    cam = cameras(B, n_rays)
    return dict(cam, name=name, Ns=Ns, planes=p.reshape(B, n_rays, Ns + 1), t_rand=None)


def sample_given(dt, c, fault=None):
    """pts [B, r, Ns, 3], dist, zval [B, r, Ns] of n3dt_sample_point with the planes given, in dtype dt (float32: no contraction, the
    library is built with -ffp-contract=off), and the magnitudes S_pts; fault: one of POINT_FAULTS"""
    B, n_rays, Ns = c["B"], c["n_rays"], c["Ns"]
    _, _, _, _, dh, l = fs.ray_setup(dt, c["xy"], c["R"], c["Kinv"])
    p = np.asarray(c["planes"]).astype(dt)
    flat = np.concatenate([p.reshape(-1), np.zeros(Ns + 2, dtype=dt)])
    if fault == "stride_ns":
        p = np.stack([flat[r * Ns:r * Ns + Ns + 1] for r in range(B * n_rays)]).reshape(B, n_rays, Ns + 1)
    z_lo, z_hi = p[..., :-1], p[..., 1:].copy()
    if fault == "zhi_next_ray":
        z_hi[..., -1] = np.stack([flat[(r + 1) * (Ns + 1) + Ns] for r in range(B * n_rays)]).reshape(B, n_rays)
    T = np.asarray(c["T"]).astype(dt)
    dl = dh * l[..., None]
    dist = (z_hi - z_lo) * l[..., None]
    if fault == "dist_prev_pair":
        dist = np.concatenate([dist[..., :1], dist[..., :-1]], axis=-1)
    pts = T[:, None, None, :] + dl[:, :, None, :] * z_lo[..., None]
    sz = np.abs(np.asarray(c["planes"], dtype=np.float64)).max()
    S_pts = (np.abs(T)[:, None, None, :] + np.abs(dl)[:, :, None, :] * sz) * np.ones_like(pts)
    return {"pts": pts, "dist": dist, "zval": z_lo, "S_pts": S_pts, "l": l}


def judge_points(c, pts, dist, zval):
    """pts [B, r, Ns, 3], dist, zval [B, r, Ns] float32 against float64 of the same float32 planes -> figures"""
    r64 = sample_given(np.float64, c)
    p32 = np.ascontiguousarray(c["planes"], dtype=np.float32)
    f = {}
    f["zval_bits"] = int((np.ascontiguousarray(zval, dtype=np.float32).view(np.uint32) != np.ascontiguousarray(p32[..., :-1]).view(np.uint32)).sum())
    equal = p32[..., 1:] == p32[..., :-1]
    f["equal_planes"] = int(equal.sum())
    f["dist_nonzero"] = int((np.asarray(dist)[equal] != 0).sum())
    scale = np.abs(r64["dist"])        # |z_hi - z_lo| |l|
    e = np.abs(np.asarray(dist, dtype=np.float64) - r64["dist"])
    with np.errstate(divide="ignore", invalid="ignore"):
        f["dist"] = float(np.where(e == 0, 0.0, e / scale).max())
    f["pts"] = float((np.abs(np.asarray(pts, dtype=np.float64) - r64["pts"]) / r64["S_pts"]).max())
    return f


POINT_RULES = {"zval_bits": "zvals bit for bit", "dist_nonzero": "dist exactly 0 between equal planes", "dist": "dist", "pts": "pts (S_pts)"}


def verdict_points(f):
    return {"zval_bits": float("inf") if f["zval_bits"] else 0.0, "dist_nonzero": float("inf") if f["dist_nonzero"] else 0.0,
            "dist": f["dist"] / unit("dist"), "pts": f["pts"] / fs.bound("geo")}


def show_points(tag, f):
    v = verdict_points(f)
    print("%-28s dist %.3f  pts %.3f of their bounds | zvals differing %d | %d equal plane pairs, %d with a non-zero dist"
          % (tag, v["dist"], v["pts"], f["zval_bits"], f["equal_planes"], f["dist_nonzero"]))
    return v
