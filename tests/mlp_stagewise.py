"""The fused MLP inference kernels pinned per entry at what they leave in the caller-owned workspace: `part` (196 floats per block of
32 / 16 samples) and `wlocal`, for tests/test_mlp_stagewise_cpu.py and tests/test_gpu_mlp_stagewise.py.  A helper module, not
a test file: CPU only.

The kernels: nerf_fwd_x16_kernel<bf16 | f16> (csrc/nerf_fwd_x16.hip), nerf_fwd_x16s_kernel (bf16x3, csrc/nerf_fwd_x16s.hip) and
nerf_fwd_f32_kernel (csrc/nerf_fwd_f32.hip).  Nothing per sample ever leaves them, so the reference is a free-running, format-following
float64 chain from the kernel's own bit-exact inputs (chain(), mode "ref"):
  weights   decoded from the bytes of the n3dt_mlp_pack buffer (held byte for byte by test_gpu_head_stagewise.py): the 16-bit roundings,
            pieces 2P / 2P + 1 of bf16x3, fp32 as it is; the merged W_m from its packed slot (decode_packed)
  biases    the float32 fold table of the same call's workspace; the merged RGB stage's per-ray table `rayfold` under include_vd
  geometry  the float32 points, plane distances and z values of ops.sample_points.  They are bit-identical to the fused kernels' own:
            all four kernels and seam_sample_kernel (csrc/seams.hip:27) form them with the one device function n3dt_sample_point
            (csrc/n3dt_device.h:74-106; nerf_fwd_x16.hip:314, nerf_fwd_x16s.hip:131, nerf_fwd_f32.hip:85), the library is built with
            -ffp-contract=off, and the function has no input but the geometry.  So no float32 geometry enters the floors
  encoder   16-bit kernels: the kernel's own PE fragments of those points (n3dt_x16_pe_probe form 0 = pe_encode, x16_core.h:558).
            bf16x3: hi = those bf16 fragments (pe_fast rounded by the same pack, nerf_fwd_x16s.hip:146-149, and form 1 == form 0 bit
            for bit, test_gpu_pe_pairs.py), lo = bf16(v - hi) with v the float64 sine / cosine of the float32 point: the kernel's v is
            pe_fast's float32 value, below 1e-6 away (test_gpu_x16_stagewise.py), against the 2^-17 spacing of hi + lo.
            fp32: float64 sin / cos of the float32 point
  roundings 16-bit: H_l = round16(relu(z_l)) at every hidden stage (nerf_fwd_x16.hip:138-145), sigma and the RGB stage stay float32;
            bf16x3: hi = bf16(x), lo = bf16(x - hi) of every activation, the products W_hi x_hi + W_hi x_lo + W_lo x_hi
            (nerf_fwd_x16s.hip:72-74), no lo lo term; fp32: none
Without a GPU the same chain runs from the CPU stand-ins of those inputs (cpu_source: head_stagewise.pack_expected, fold_emul, vd_emul,
f32_stagewise.sample / embed in float32), which is where every floor below comes from.

The rules (judge()); everything downstream of a stored value is judged from the stored value:
  1  density through wlocal.  Per block, in float64:  alpha_s = wlocal_s / Tl_s,  Tl_s = prod_{t<s} (1 - alpha_t + 1e-10),
     sigma_rec = -log1p(-alpha_s) / dist_s.  The recovery's own conditioning, first order, with u = 2^-24 (one float32 rounding):
         e_s    = alpha_s (u + sum_{t<s} (u + ulp(x_t) / x_t + e_t / x_t)) + 2^-149 (1 + alpha_s) / Tl_s
                  the error of the recovered alpha_s.  Per earlier factor: one product of the scan (u, whatever its order: s factors
                  meet in s - 1 products), the two roundings of x = (1 - alpha) + 1e-10f (half a spacing each: ulp(x) / x together)
                  and the earlier recovered alpha entering x_t = 1 - alpha_t + 1e-10 (e_t / x_t); then the product alpha Tl (u); and
                  gradual underflow of the stored weight and of the in-block product, which lose up to 2^-149 absolutely (case
                  contrast: products of 1e-10 transmittances)
         dalpha = e_s + ulp(x) / 2 + x a u + [alpha > 1/2] ulp(alpha) / 2,     a = sigma dist,  x = e = 1 - alpha
                  the roundings of the kernel's alpha = 1 - expf(-(sigma dist)): e as ONE correctly rounded float32 value (half a
                  spacing, ABSOLUTE: 2^-25 for e in [1/2, 1), whatever alpha is -- a float32 alpha of 0.01 is a multiple of 2^-24 and
                  carries 17 bits), the product sigma dist, and the subtraction, which is exact while e >= 1/2.  What expf adds beyond
                  a correct rounding is not a rounding of alpha, x or the scan: it is part of the emulation's error and so of the
                  floor of family sigma (below), which the factor 4 then carries to a device expf of one ulp
         cond_s = dalpha / (x_s dist_s) / (1 - 2 E_s),  E_s = sum_{t<s} e_t / x_t     d sigma / d alpha = 1 / ((1 - alpha) dist); E_s is the
                  relative error of the recovered Tl_s, and the first-order step is taken only where E_s <= 2^-7 (the last factor
                  covers its second order); behind a sample whose x_t is lost in its own error the recovery is not judged at all
     A sample is judged if sigma_ref > dsigma = U_sigma magnitude, every earlier alpha of its block is below 1 - 2^-10, E_s <= 2^-7 and
     cond <= dsigma / 2.  (a) |sigma_rec - sigma_ref| <= dsigma + cond per judged sample; (b) per block the rms of (sigma_rec - sigma_ref) /
     magnitude over its judged samples <= U_sigma_rms + the rms of cond / magnitude over the same samples (the triangle inequality of
     the rms: what the recovery itself may add to every sample; below 1e-3 of the unit in the 16-bit precisions).  Where sigma_ref < -dsigma the stored weight is exactly 0.
  2  every live wlocal inside the interval the density band allows (rigorous, no first-order step), +- x16_stagewise.weight_tolerance
  3  part[:192] against sum_s wlocal_s g_ref_s, M = sum_s wlocal_s mag(g)_s: (a) per entry U_g M, (b) per block rms over the channels
  4  part[G + 1] against sum wlocal zval (family zsum)
  5  part[G + 2] inside [prod x_lo (1 - eps), prod x_hi (1 + eps)] +- 2^-116.  Each factor's band is widened by what float32 itself
     does to it: x = (1 - alpha) + 1e-10f with alpha = 1 - e rounded at the scale of 1, so x carries an ABSOLUTE error of up to 2^-25
     (and 4 u relative from expf and the product sigma dist), and is never below 1e-10f.  Without that term the float32 emulation
     itself leaves the band behind a nearly saturated sample of case contrast (x ~ 1e-7, 30 % off), at every unit a rounding argument
     could give; x16_stagewise.weight_tolerance carries the same term for the weights, for the same reason.  eps is the scan alone.
     (A block without a live sample would have to give exactly 1; there is none: bpr = ceil(n_samples / block), so every block's
     lane 0 is live.  Dead lanes carry dist = 0, alpha = 0 and x = 1 + 1e-10f = 1 exactly, n3dt_device.h:101-105.)
  6  part[G + 3] is exactly 0;   7  wlocal beyond n_samples is exactly 0 (the other bitwise properties need a second call: GPU test)
Rule 7's bitwise properties hold by construction: a wave's arithmetic depends on nothing but its block's own samples, tables and the
shared weight stream (nerf_fwd_x16.hip:300-323: blk -> ray, frame; every wave reads the same pieces), and nothing is atomic.

Given planes (cases hier and hier_span of head_stagewise.CASES: z_planes_given, the planes of hier_stagewise.given_planes passed as t_rand)
go through the same rules, with two additions: a sample between two equal planes (dist == 0) stores a weight of exactly 0 (figure
zero_dist_nonzero, under rule 1) and rule 5 runs across it (x = 1 + 1e-10f); and rule 1's dalpha carries an expf of one ulp (see judge()).
Where their measured floor is above the table's they have their own entry (FLOOR_GIVEN).

Units: U_family = 4 x FLOOR[family][precision]; a floor is the largest figure of the float32-ordered CPU emulations (chain() modes
"asc", "desc", "torch", and "fma" for fp32: the k order nerf_fwd_f32.hip walks) through the sequential float32 compositing
(composite32) against this reference over all CASES; test_mlp_stagewise_cpu.py re-measures every one.  No number comes from a GPU run.
Families sigma and sigma_rms are floored twice over and take the larger: the emulation's float32 sigma against the reference's, and
its density read back through its own float32 wlocal by rule 1 (the error beyond cond, over the samples rule 1 judges).  The second
depends on the unit through the set of judged samples; the recorded constants are its fixed point (reached in one step: the worst
sample is judged at either unit), and the CPU test's measured <= recorded <= 1.25 x measured holds them there.  In fp32 and bf16x3
the second is the larger (numpy's float32 exp against the exact one), in bf16 and fp16 the first.
"""
import functools

import numpy as np
import torch

import f32_stagewise as fs
import head_stagewise as hs
import x16_stagewise as xs

F32, BF16, F16, BF16X3 = hs.F32, hs.BF16, hs.F16, hs.BF16X3
PRECISIONS = ["fp32", "bf16", "fp16", "bf16x3"]
G = hs.G
U32 = 2.0 ** -24
ALPHA_EDGE = 1.0 - 2.0 ** -10
SUBNORMAL = 2.0 ** -149    # the spacing of float32 below 2^-126: what a stored weight or an in-block product may lose absolutely
TL_ERR_MAX = 2.0 ** -7      # rule 1: the first-order propagation is trusted while the recovered in-block product is this accurate
X_ABS = 2.0 ** -25          # rule 5: the float32 resolution of x = 1 - alpha + 1e-10 (alpha rounded in [0.5, 1))
X_MIN = 1e-10 * (1 - 2.0 ** -23)
SHARE_CASES = ("one", "ragged", "span", "full", "gaze", "vd")
SHARE_MIN = 0.9
MODES = ("asc", "desc", "torch")

# ---- the measured floors (test_mlp_stagewise_cpu.py prints each beside its constant and fails unless measured <= recorded <= 1.25 x)
FLOOR = {
    "sigma": {"fp32": 4.45e-7, "bf16": 9.6e-4, "fp16": 1.52e-4, "bf16x3": 8.8e-6},
    "sigma_rms": {"fp32": 2.55e-7, "bf16": 2.25e-4, "fp16": 7.2e-5, "bf16x3": 2.6e-6},
    "g": {"fp32": 1.85e-7, "bf16": 2.05e-4, "fp16": 1.47e-4, "bf16x3": 3.2e-6},
    "g_rms": {"fp32": 3.7e-8, "bf16": 5.6e-5, "fp16": 3.15e-5, "bf16x3": 7.1e-7},
    "zsum": {"fp32": 1.27e-7, "bf16": 1.16e-7, "fp16": 1.2e-7, "bf16x3": 1.23e-7},
    "eps": {"fp32": 2.05e-7, "bf16": 3.1e-7, "fp16": 4.0e-7, "bf16x3": 3.2e-7},
}
# The given-plane cases (hier, hier_span: z_planes_given) where their measured floor is above the table's: their own entries, the table
# above stays.  Fine planes cluster: neighbouring samples are nearly the same point, so their 16-bit encodings and hence their errors are the
# same and do not average out over a block (g, g_rms), and the plane distances are a tenth of a uniform slab's, so what float32 exp adds
# beyond a correct rounding of e -- an error of alpha that the conditioning term does not carry -- is ten times larger in sigma = a / dist.
FLOOR_GIVEN = {
    "sigma": {"fp16": 1.6e-4, "bf16x3": 1.0e-5},              # measured 1.715e-4 at the table's unit (hier_span asc), 9.77e-6 (hier_span asc)
    "sigma_rms": {"bf16": 4.6e-4, "fp16": 8.3e-5},            # measured 4.51e-4 (hier_span asc), 8.03e-5 (hier_span torch)
    "g": {"fp32": 1.9e-7, "bf16": 1.0e-3},                    # measured 1.874e-7 (hier_span torch), 9.99e-4 (hier_span asc)
    "g_rms": {"bf16": 2.4e-4},                                # measured 2.35e-4 (hier_span asc)
}
GIVEN_CASES = tuple(n for n, c in hs.CASES.items() if c.get("hier"))
FACTOR = 4.0
FAMILIES = tuple(FLOOR)


def floor_of(family, prec, name=None):
    own = FLOOR_GIVEN.get(family, {}) if name in GIVEN_CASES else {}
    return own.get(prec, FLOOR[family][prec])


def unit(family, prec, name=None):
    """name: the case; a given-plane case takes its own entry where it has one"""
    return FACTOR * floor_of(family, prec, name)


# ---------------------------------------------------------------------------------------------------------------------
# the kernel's inputs
# ---------------------------------------------------------------------------------------------------------------------
def decode_packed(buf, p):
    """the bytes of the n3dt_mlp_pack buffer -> stage -> logical matrix [N, K] in float64 (bf16x3: the pair (hi, lo)); the inverse of
    head_stagewise.pack_expected.  The 16-bit buffers hold the merged 192 x 384 matrix in stage 9's slot and nothing in stage 10's."""
    mat = np.ascontiguousarray(buf[:hs.packed_region_bytes(p)]).view(np.float32 if p == F32 else np.uint16)
    out = {}
    for s in range(hs.NSTAGE):
        if p != F32 and s == 10:
            continue
        N, K, _ = hs.stage_dims(10 if (p != F32 and s == 9) else s)
        row, col = hs.pack_index_map(N, K, p)
        at = hs.stage_offset(s) + np.arange(N * K)

        def put(v):
            W = np.zeros((N, K))
            W[row, col] = v
            return W

        if p == F32:
            out[s] = put(mat[at].astype(np.float64))
        elif p == BF16X3:
            P, inn = at >> 9, at & 511
            out[s] = (put(xs.bits16_to_f64(mat[2 * P * 512 + inn], "bf16")), put(xs.bits16_to_f64(mat[(2 * P + 1) * 512 + inn], "bf16")))
        else:
            out[s] = put(xs.bits16_to_f64(mat[at], hs.FMT16[p]))
    return out


def pe_channels(frags):
    """n3dt_x16_pe_probe's [waves, 4, 64, 8] fragments -> [points, 64] channels: piece ks, lane (c, h), element j is channel
    16 ks + 8 (j >> 2) + 4 h + (j & 3) of the wave's point c (x16_core.h:543-545)"""
    w = frags.shape[0]
    return frags.reshape(w, 4, 2, 32, 2, 4).transpose(0, 3, 1, 4, 2, 5).reshape(w * 32, 64)


def make_source(name, prec, W, fold, b10, pts, dist, zval, pe):
    ci = hs.case_inputs(name)
    return {"name": name, "prec": prec, "p": hs.PRECS[prec], "W": W, "fold": fold, "b10": b10, "pts": pts, "dist": dist, "zval": zval,
            "pe": pe, "B": ci["B"], "n_rays": ci["n_rays"], "Ns": ci["Ns"], "R": ci["B"] * ci["n_rays"], "bs": hs.block_samples(hs.PRECS[prec])}


def pe_inputs(p, pts, pe16=None):
    """the encoder's output as the chain takes it, from the float32 points [P, 3]: 16-bit values (pe16 [P, 64] float64: the kernel's own
    fragments; None: the rounding of the float32 encoding, the CPU stand-in), the bf16x3 pair, or None (fp32: chain() encodes)"""
    if p == F32:
        return None
    fmt = hs.FMT16[p]
    hi = pe16 if pe16 is not None else xs.round16(fs.embed(np.float32, pts).astype(np.float64), fmt)
    if p != BF16X3:
        return hi
    v = fs.embed(np.float64, pts) if pe16 is not None else fs.embed(np.float32, pts).astype(np.float64)
    return hi, xs.round16(v - hi, "bf16")


@functools.lru_cache(maxsize=None)
def _wm32(weights_of):
    return hs.merged_matrix32(hs.case_inputs(weights_of)["ws"])


@functools.lru_cache(maxsize=None)
def cpu_geometry(name):
    ci = hs.case_inputs(name)
    inp, opt = ci["inp"], ci["opt"]
    B = ci["B"]
    g = {"B": B, "n_rays": ci["n_rays"], "Ns": ci["Ns"], "xy": inp["batch_xy"].numpy(), "R": inp["batch_Rmats"].numpy().reshape(B, 3, 3),
         "Kinv": inp["batch_inv_inmats"].numpy().reshape(B, 3, 3), "T": inp["batch_Tvecs"].numpy().reshape(B, 3), "z1": opt.world_z1,
         "z2": opt.world_z2, "t_rand": None, "planes": ci["planes"]}
    (pts, dist, zval), _ = fs.sample(np.float32, g)
    R, Ns = B * ci["n_rays"], ci["Ns"]
    return pts.reshape(R, Ns, 3), dist.reshape(R, Ns), zval.reshape(R, Ns)


@functools.lru_cache(maxsize=None)
def cpu_tables(name, merged):
    """the float32 fold table [B, FOLD_STRIDE] (fold_emul + the copied biases) and the RGB stage's bias of every ray [R, 192]"""
    ci = hs.case_inputs(name)
    ws, bs, B = ci["ws"], ci["bs"], ci["B"]
    fold = np.zeros((B, hs.FOLD_STRIDE), dtype=np.float32)
    fold[:, :hs.FOLD_USED] = hs.fold_emul(ws, bs, ci["codes"], ci["S"], ci["A"], ci["U"], merged)
    for s in (1, 2, 3, 4, 6, 7, 9):
        fold[:, hs.bias_offset(s):hs.bias_offset(s) + 384] = bs[s]
    fold[:, hs.bias_offset(8)] = bs[8][0]
    o = hs.bias_offset(10)
    b10 = np.repeat(fold[:, o:o + G], ci["n_rays"], axis=0)
    if ci["vd"]:
        b10 = b10 + hs.vd_emul(ci["w_vd"], hs.directions32(ci)).reshape(-1, G)   # rayfold: one float32 add
    return fold, b10.astype(np.float32)


@functools.lru_cache(maxsize=None)
def cpu_source(name, prec, pack_fault=None):
    """the stand-in of the kernel's inputs on a machine without a GPU.  pack_fault "trunc": the pack truncates to 16 bits."""
    ci, p = hs.case_inputs(name), hs.PRECS[prec]
    weights_of = name if name in ("contrast", "gaze", "vd") else "ragged"
    buf, _ = hs.pack_expected(ci["ws"], ci["bs"], ci["S"], p, _wm32(weights_of), 0)
    W = decode_packed(buf, p)
    if pack_fault == "trunc" and p != F32:
        W = {s: truncated(ci, s, p, _wm32(weights_of)) for s in W}
    fold, b10 = cpu_tables(name, p != F32)
    pts, dist, zval = cpu_geometry(name)
    return make_source(name, prec, W, fold, b10, pts, dist, zval, pe_inputs(p, pts.reshape(-1, 3)))


def toward_zero16(v32, fmt):
    """float32 -> the 16-bit value next to it toward zero, as float64 (the deliberate fault of a pack that truncates)"""
    v = np.asarray(v32, dtype=np.float32)
    if fmt == "bf16":
        return (np.ascontiguousarray(v).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32).astype(np.float64)
    r = v.astype(np.float16)
    over = np.abs(r.astype(np.float32)) > np.abs(v)
    return np.where(over, np.nextafter(r, np.float16(0)), r).astype(np.float64)


def truncated(ci, s, p, wm32):
    fmt = hs.FMT16[p]
    v = np.asarray(wm32, dtype=np.float32) if s == 9 else hs.logical_weight(ci["ws"], s, ci["S"])
    hi = toward_zero16(v, fmt)
    if p != BF16X3:
        return hi
    return hi, toward_zero16((v - hi.astype(np.float32)).astype(np.float32), fmt)


# ---------------------------------------------------------------------------------------------------------------------
# the chain
# ---------------------------------------------------------------------------------------------------------------------
def point_index(Ns, rays):
    return (np.asarray(rays)[:, None] * Ns + np.arange(Ns)[None, :]).reshape(-1)


def _cat(a, b):
    return tuple(np.concatenate([x, y], axis=1) for x, y in zip(a, b)) if isinstance(a, tuple) else np.concatenate([a, b], axis=1)


def _cols(a, sl, value=0.0):
    def one(x):
        x = x.copy()
        x[:, sl] = value
        return x
    return tuple(one(x) for x in a) if isinstance(a, tuple) else one(a)


def linear(p, mode, X, W, b, no_wlo_xhi=False, want_mag=False):
    """z = b + W X per point, X [P, K] (bf16x3: the pair (hi, lo)), W [N, K] (likewise), b [P, N] float32.
    "ref": every product and sum in float64 (with want_mag also |b| + sum |w x|).  The float32 orders: "asc" / "desc" 16-wide k-steps
    in sequence on an accumulator that starts as the bias (the C operand, nerf_fwd_x16.hip:154; bf16x3: the bias as bf16 hi + lo through
    one MFMA, nerf_fwd_x16s.hip:53-57, and the two correction products in an accumulator of their own, :72-77); "torch": torch's matmul;
    "fma": one fmaf per k in ascending order, the chain v_mfma_f32_16x16x4_f32 walks (nerf_fwd_f32.hip:36-48; packed column 16 k4 + 4 j
    + (lane >> 4), head_stagewise.pack_index_map)."""
    if p == BF16X3:
        (xh, xl), (wh, wl) = X, W
        main, cor = [(xh, wh)], [(xl, wh)] + ([] if no_wlo_xhi else [(xh, wl)])
    else:
        main, cor = [(X, W)], []
    if mode == "ref":
        z = np.asarray(b, dtype=np.float64) + sum(x @ w.T for x, w in main + cor)
        if not want_mag:
            return z
        x1, w1 = (np.abs(X[0] + X[1]), np.abs(W[0] + W[1])) if p == BF16X3 else (np.abs(X), np.abs(W))
        return z, np.abs(np.asarray(b, dtype=np.float64)) + x1 @ w1.T
    b0 = np.asarray(b, dtype=np.float32)
    if p == BF16X3:
        hi, lo = xs.split_hi_lo(b0)
        b0 = (hi + lo).astype(np.float32)
    f = lambda t: [(np.ascontiguousarray(x, dtype=np.float32), np.ascontiguousarray(w, dtype=np.float32)) for x, w in t]
    main, cor = f(main), f(cor)
    n, N, K = main[0][0].shape[0], main[0][1].shape[0], main[0][0].shape[1]
    acc = np.broadcast_to(b0, (n, N)).astype(np.float32)
    c = np.zeros((n, N), dtype=np.float32)
    if mode in ("asc", "desc"):
        steps = range(0, K, 16) if mode == "asc" else range(K - 16, -1, -16)
        for k0 in steps:
            for x, w in main:
                acc = acc + x[:, k0:k0 + 16] @ w[:, k0:k0 + 16].T
            for x, w in cor:
                c = c + x[:, k0:k0 + 16] @ w[:, k0:k0 + 16].T
    elif mode == "torch":
        mm = lambda x, w: torch.matmul(torch.from_numpy(x), torch.from_numpy(w).T).numpy()
        for x, w in main:
            acc = acc + mm(x, w)
        for x, w in cor:
            c = c + mm(x, w)
    elif mode == "fma":
        for x, w in main + cor:
            x64, w64 = x.astype(np.float64), w.astype(np.float64)
            for k in range(K):
                acc = (acc.astype(np.float64) + x64[:, k:k + 1] * w64[None, :, k]).astype(np.float32)
    else:
        raise ValueError(mode)
    return acc + c if cor else acc


def activation(p, z):
    """what a hidden stage hands to the next one"""
    v = np.maximum(np.asarray(z, dtype=np.float64), 0.0)
    if p == F32:
        return v
    if p == BF16X3:
        hi = xs.round16(v, "bf16")
        return hi, xs.round16(v - hi, "bf16")
    return xs.round16(v, hs.FMT16[p])


RGB = "rgb"   # the stage key of the RGB stage in a fault: the merged stage (16-bit) or RGB_layer_1 (fp32)


def chain(src, mode, idx, fault=None):
    """sigma (pre-activation) and g = relu(RGB stage) of the points idx (flat indices into [R, Ns]); "ref" adds the magnitudes.
    fault: None or (name, ...) -- the deliberate faults of the MLP chain (test_mlp_stagewise_cpu.py: FAULTS)."""
    p, Ns, n_rays, B = src["p"], src["Ns"], src["n_rays"], src["B"]
    ref = mode == "ref"
    fname = fault[0] if fault else None
    ray = idx // Ns
    frame = ray // n_rays
    tab = src["fold"][(frame + B - 1) % B if fname == "neighbour_bias" else frame]
    W = dict(src["W"])
    if fname == "col63":
        for s in (0, 5):
            W[s] = _cols(W[s], slice(63, 64), 1.0)
    pts = src["pts"].reshape(-1, 3)[idx]
    if p == F32:
        x = fs.embed(np.float64, pts) if ref else fs.embed(np.float32, pts).astype(np.float64)
    else:
        x = tuple(a[idx] for a in src["pe"]) if p == BF16X3 else src["pe"][idx]
    if fname == "no_xlo":
        x = (x[0], np.zeros_like(x[1]))
    kw = {"no_wlo_xhi": fname == "no_wlo_xhi"}

    def bias(stage, n):
        o = hs.bias_offset(stage)
        return tab[:, o:o + n]

    def L(key, s, X, b, rows=None, **more):
        Ws = W[s] if rows is None else (tuple(w[rows] for w in W[s]) if p == BF16X3 else W[s][rows])
        z = linear(p, mode, X, Ws, b, **kw, **more)
        if fname == "drop" and fault[1] == key:
            ks, tile = fault[2], fault[3]
            z2 = linear(p, mode, _cols(X, slice(16 * ks, 16 * ks + 16)), Ws, b, **kw)
            z = np.array(z[0] if isinstance(z, tuple) else z)
            cols = slice(None) if tile is None else slice(32 * tile, 32 * tile + 32)
            z[:, cols] = z2[:, cols]
        return z

    def act(z):
        h = activation(p, z)
        return (h[0], np.zeros_like(h[1])) if fname == "no_xlo" else h

    h = act(L(0, 0, x, bias(0, 384)))
    for l in range(1, 8):
        X = _cat(_cols(x, slice(0, 64)) if fname == "no_pe_L5" else x, h) if l == 5 else h
        h = act(L(l, l, X, bias(l, 384)))
    row = 1 if fname == "density_row1" else 0
    b8 = bias(8, 32)[:, row:row + 1]
    if fname == "no_density_bias":
        b8 = np.zeros_like(b8)
    out = {}
    if ref:
        z, m = L(8, 8, h, b8, rows=slice(row, row + 1), want_mag=True)
        out["sigma"], out["mag_sigma"] = z[:, 0], m[:, 0]
    else:
        out["sigma"] = L(8, 8, h, b8, rows=slice(row, row + 1))[:, 0]
    b10 = src["b10"][(ray + src["R"] - n_rays) % src["R"] if fname == "neighbour_bias" else ray]
    if p == F32:
        t = np.asarray(L(9, 9, h, bias(9, 384)), dtype=np.float64)
        s10 = 10
    else:
        t, s10 = h, 9
    if ref:
        z, out["mag_g"] = L(RGB, s10, t, b10, want_mag=True)
    else:
        z = L(RGB, s10, t, b10)
    out["g"] = np.maximum(z, 0)
    return out


def reference(src, rays):
    """the float64 chain of whole rays -> sigma, mag_sigma [n, Ns], g, mag_g [n, Ns, 192], dist, zval [n, Ns]"""
    Ns = src["Ns"]
    o = chain(src, "ref", point_index(Ns, rays))
    n = len(rays)
    return {"name": src["name"], "rays": np.asarray(rays), "sigma": o["sigma"].reshape(n, Ns), "mag_sigma": o["mag_sigma"].reshape(n, Ns), "g": o["g"].reshape(n, Ns, G),
            "mag_g": o["mag_g"].reshape(n, Ns, G), "dist": src["dist"][rays].astype(np.float64), "zval": src["zval"][rays].astype(np.float64)}


# ---------------------------------------------------------------------------------------------------------------------
# the compositing in float32 (the emulation) and the rules
# ---------------------------------------------------------------------------------------------------------------------
def blocks(v, bs, fill=0.0):
    """[n, Ns, ...] -> [n, bpr, bs, ...], the lanes beyond n_samples filled"""
    n, Ns = v.shape[:2]
    bpr = (Ns + bs - 1) // bs
    pad = np.full((n, bpr * bs - Ns) + v.shape[2:], fill, dtype=v.dtype)
    return np.concatenate([v, pad], axis=1).reshape((n, bpr, bs) + v.shape[2:])


def composite32(sigma, g, dist, zval, bs, fault=None):
    """part [n, bpr, 196] and wlocal [n, bpr, bs] in float32 as the kernels' epilogues form them (nerf_fwd_x16.hip:391-421 and :229-246,
    nerf_fwd_f32.hip:109-141) with the SEQUENTIAL in-block product, from float32 sigma [n, Ns], g [n, Ns, 192], dist and zval; and the
    float32 factors x.  Block size 32: the samples of a channel meet in a halving butterfly; 16: one sum in ascending sample order.
    fault: the deliberate faults of the compositing and the stored outputs."""
    one = np.float32(1)
    s, gd = blocks(np.asarray(sigma, dtype=np.float32), bs), blocks(np.asarray(g, dtype=np.float32), bs)
    d, zv = blocks(np.asarray(dist, dtype=np.float32), bs), blocks(np.asarray(zval, dtype=np.float32), bs)
    live = blocks(np.ones(sigma.shape, dtype=bool), bs, False)
    if fault == "min_dist":      # a live sample's distance is never taken as 0 (given planes: two equal planes)
        d = np.where(live, np.maximum(d, np.float32(1e-4)), d)
    if fault == "dead_dist":     # the dead lanes take the block's last live sample, its distance included
        li = np.maximum(live.sum(2) - 1, 0)
        take = lambda a: np.where(live if a.ndim == 3 else live[..., None], a, np.take_along_axis(a, li.reshape(li.shape + (1,) * (a.ndim - 2)), axis=2))
        s, d, gd = take(s), take(d), take(gd)
    alpha = one - np.exp(-np.maximum(s, np.float32(0)) * d).astype(np.float32)
    x = one - alpha if fault == "no_eps" else (one - alpha) + np.float32(1e-10)
    Tl = np.ones_like(x)
    for i in range(1, bs):
        Tl[..., i] = Tl[..., i - 1] * x[..., i - 1]
    if fault == "inclusive":
        Tl = Tl * x
    w = alpha * Tl
    last = bs - 2 if fault == "tprod_lane30" else bs - 1
    prev = lambda a: np.concatenate([np.zeros_like(a[..., :1]), a[..., :-1]], axis=-1)
    part = np.zeros(w.shape[:2] + (hs.PART_STRIDE,), dtype=np.float32)
    wg = prev(w) if fault == "g_prev_weight" else w
    if bs == 32:
        part[..., :G] = hs.halving_sum(np.moveaxis(np.maximum(gd, np.float32(0)) * wg[..., None], 2, 3))
    else:
        acc = np.zeros(w.shape[:2] + (G,), dtype=np.float32)
        for i in range(bs):
            acc = acc + wg[..., i, None] * gd[..., i, :]
        part[..., :G] = acc
    part[..., G] = hs.halving_sum(w)
    part[..., G + 1] = hs.halving_sum(w * (prev(zv) if fault == "zval_shift" else zv))
    part[..., G + 2] = Tl[..., last] * (one if fault == "inclusive" else x[..., last])
    return part, w, x


def ulp32(v):
    """the spacing of float32 at v > 0 (2^-149 below the normal range)"""
    _, e = np.frexp(np.asarray(v, dtype=np.float64))
    return np.ldexp(1.0, np.maximum(e, -125) - 24)


def judge(ref, part, wlocal, prec):
    """every rule on the stored part [n, bpr, 196] / wlocal [n, bpr, bs] of the reference's rays -> figures: for each family the largest
    error in units of its magnitude (to be divided by unit()), the counts of the exact rules, the shares and the widths"""
    p = hs.PRECS[prec]
    bs = hs.block_samples(p)
    name = ref.get("name")
    f = {"name": name}
    sig, mag = blocks(ref["sigma"], bs), blocks(ref["mag_sigma"], bs, 1.0)
    d, zv = blocks(ref["dist"], bs), blocks(ref["zval"], bs)
    live = blocks(np.ones(ref["sigma"].shape, dtype=bool), bs, False)
    w = np.asarray(wlocal, dtype=np.float64)
    wbits = np.ascontiguousarray(wlocal, dtype=np.float32).view(np.uint32)
    pt = np.asarray(part, dtype=np.float64)
    dsig = unit("sigma", prec, name) * mag
    # ---- rule 1
    alpha, dal, early, tl_err = np.zeros_like(w), np.zeros_like(w), np.zeros(w.shape, dtype=bool), np.zeros_like(w)
    Tl, acc, ok, scan = np.ones(w.shape[:2]), np.zeros(w.shape[:2]), np.ones(w.shape[:2], dtype=bool), np.zeros(w.shape[:2])
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for s in range(bs):
            a = np.where(Tl > 0, w[..., s] / Tl, np.inf)
            alpha[..., s], early[..., s], tl_err[..., s] = a, ok, acc
            dal[..., s] = a * (scan + U32 + acc) + SUBNORMAL * (1.0 + a) / Tl
            xs_ = 1.0 - a + 1e-10
            scan = scan + U32 + ulp32(xs_) / xs_
            acc = acc + dal[..., s] / xs_
            ok = ok & (a < ALPHA_EDGE)
            Tl = Tl * np.maximum(xs_, 0.0)
        x1 = 1.0 - alpha
        a_arg = -np.log1p(-alpha)
        srec = a_arg / d
        dalpha = dal + 0.5 * ulp32(x1) + x1 * a_arg * U32 + np.where(alpha > 0.5, 0.5 * ulp32(alpha), 0.0)
        if name in GIVEN_CASES:
            # given planes: an expf of ONE ulp, not a correct rounding of e, enters the conditioning -- half a spacing of x more.  With
            # uniform planes that excess is part of the floor of family sigma (above); with fine planes it cannot be: dist spans three
            # decades, the excess grows as 1 / dist like cond itself, and a unit that carried it would admit samples (cond <= dsigma / 2)
            # whose excess is larger again -- measured: the floor tripled at every step and had no fixed point
            dalpha = dalpha + 0.5 * ulp32(x1)
        cond = dalpha / (x1 * d) / (1.0 - 2.0 * np.minimum(tl_err, TL_ERR_MAX))
        eligible = live & (d > 0) & early & (alpha < 1.0) & (tl_err <= TL_ERR_MAX) & np.isfinite(srec) & np.isfinite(cond)
        judged = eligible & (sig > dsig) & (cond <= 0.5 * dsig)
        e1 = np.maximum(np.abs(srec - np.maximum(sig, 0.0)) - cond, 0.0) / mag
        rel, crel = np.where(judged, (srec - sig) / mag, 0.0), np.where(judged, cond / mag, 0.0)
    f["sigma"] = float(e1[judged].max()) if judged.any() else 0.0
    nj = judged.sum(2)
    rms = lambda v: np.sqrt((v ** 2).sum(2)[nj > 0] / nj[nj > 0])
    f["sigma_rms"] = float(np.maximum(rms(rel) - rms(crel), 0.0).max()) if (nj > 0).any() else 0.0
    f["neg_nonzero"] = int((live & (sig < -dsig) & (wbits != 0)).sum())
    # (given planes: a sample between two equal planes has dist = 0, alpha = 1 - expf(-(sigma 0)) = 0 and a stored weight of exactly 0, so
    #  it adds exactly nothing to part[:192], which rule 3 then judges from the stored weights; its x is 1 + 1e-10f in rule 5)
    f["zero_dist"] = int((live & (d == 0)).sum())
    f["zero_dist_nonzero"] = int((live & (d == 0) & (wbits != 0)).sum())
    positive = live & (sig > 0)
    f["share"] = float(judged.sum()) / max(int(positive.sum()), 1)
    # ---- rule 2
    a_lo = -np.expm1(-np.maximum(sig - dsig, 0.0) * d)
    a_hi = -np.expm1(-np.maximum(sig + dsig, 0.0) * d)
    x_lo, x_hi = np.where(live, 1.0 - a_hi + 1e-10, 1.0), np.where(live, 1.0 - a_lo + 1e-10, 1.0)
    excl = lambda v: np.concatenate([np.ones(v.shape[:2] + (1,)), np.cumprod(v, axis=2)[..., :-1]], axis=2)
    lo, hi = a_lo * excl(x_lo), a_hi * excl(x_hi)
    out = np.maximum((lo - w) / xs.weight_tolerance(lo), (w - hi) / xs.weight_tolerance(hi))
    f["interval"] = float(out[live].max())
    big = live & (w > 1e-4)
    f["width"] = [float(q) for q in np.quantile((hi - lo)[big] / w[big], (0.5, 0.9, 0.99))] if big.any() else [0.0, 0.0, 0.0]
    # ---- rule 3
    r3 = np.einsum("rks,rksj->rkj", w, blocks(ref["g"], bs))
    M = np.einsum("rks,rksj->rkj", w, blocks(ref["mag_g"], bs))
    err = np.maximum(np.abs(pt[..., :G] - r3) - hs.ABS_SLACK, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0.0, 0.0, err / M)
    f["g"] = float(q.max())
    f["g_rms"] = float(np.sqrt((q ** 2).mean(-1)).max())
    # ---- rule 4
    f["zsum"] = hs.ratio(pt[..., G + 1], (w * zv).sum(2), np.abs(w * zv).sum(2))
    # ---- rule 5
    eps = unit("eps", prec, name)
    T_lo = np.prod(np.where(live, np.maximum(x_lo * (1 - 4 * U32) - X_ABS, X_MIN), 1.0), axis=2)
    T_hi = np.prod(np.where(live, x_hi * (1 + 4 * U32) + X_ABS, 1.0), axis=2)
    t = pt[..., G + 2]
    f["tprod"] = float(np.maximum((T_lo - t) / (eps * T_lo + hs.ABS_SLACK), (t - T_hi) / (eps * T_hi + hs.ABS_SLACK)).max())
    # ---- rules 6 and 7
    f["pad_nonzero"] = int((np.ascontiguousarray(np.asarray(part, dtype=np.float32)[..., G + 3]).view(np.uint32) != 0).sum())
    f["dead_nonzero"] = int((~live & (wbits != 0)).sum())
    return f


RULES = {"sigma": "1a", "sigma_rms": "1b", "neg_nonzero": "1 (negative density)", "interval": "2", "g": "3a", "g_rms": "3b", "zsum": "4", "tprod": "5",
         "pad_nonzero": "6", "dead_nonzero": "7 (dead lanes)", "zero_dist_nonzero": "1 (zero-width sample)"}


def verdict(f, prec):
    """figure -> its share of the bound (<= 1 passes); the exact rules count violations (0 passes)"""
    v = {k: f[k] / unit(k, prec, f.get("name")) for k in ("sigma", "sigma_rms", "g", "g_rms", "zsum")}
    v["interval"], v["tprod"] = f["interval"], f["tprod"]
    for k in ("neg_nonzero", "pad_nonzero", "dead_nonzero", "zero_dist_nonzero"):
        v[k] = float("inf") if f[k] else 0.0
    return v


def failing(v):
    return sorted(k for k, r in v.items() if not r <= 1.0)


def show(tag, f, prec):
    """prints every figure of one judged call before it is asserted"""
    v = verdict(f, prec)
    print("%-30s 1a %.3f  1b %.3f  2 %.3f  3a %.3f  3b %.3f  4 %.3f  5 %.3f | exact-rule violations %d %d %d, %d of %d zero-width samples | judged share %.3f | width q50 %.2e q90 %.2e q99 %.2e"
          % (tag, v["sigma"], v["sigma_rms"], v["interval"], v["g"], v["g_rms"], v["zsum"], v["tprod"], f["neg_nonzero"], f["pad_nonzero"],
             f["dead_nonzero"], f["zero_dist_nonzero"], f["zero_dist"], f["share"], f["width"][0], f["width"][1], f["width"][2]))
    return v
