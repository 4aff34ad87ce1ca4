"""Stage-by-stage float64 restatement of the exact fp32 volumetric training path (n3dt_launch_train_fwd / _bwd in
csrc/train_mlp.hip, the fp32 kernel of csrc/gemm32.hip and the fold, ray-head, colsum and camera kernels they call), for the
tests that pin it (test_f32_stagewise_cpu.py, test_gpu_f32_stagewise.py).  A helper module, not a test file: CPU only, numpy.

The path keeps every forward intermediate in `saved` (TrainSaved) and most backward intermediates in the training workspace
(TrainWs), all fp32, point-major ([P][C], point = (frame * n_rays + ray) * n_samples + sample).  Every stage is recomputed in
float64 from the kernel's own stored inputs ("teacher-forced") and compared per entry:

    |got - z64| <= u_family * S          S = float64 sum of the absolute terms of that entry (|b| + sum |w x| for a product)

ReLU gates of the backward are READ from `saved` (H_l > 0, g > 0, sigma_pre > 0), never recomputed, so the backward is a fixed
linear map of the cotangents and no gate flip can widen a band.  A forward entry behind a ReLU whose |z64| <= u S may be stored as
0 or as the value (both lie within u S of relu(z64)); such entries are counted and printed, and a stage may have at most
AMBIGUOUS_CAP of them.  The one gate that is not stored is the compositing backward's `alpha > 0`: it is taken as the float32
evaluation of 1 - exp(-sigma dist) > 0, and a sample whose float64 alpha is below ALPHA_EDGE (where one ulp of expf decides it)
may hold 0 or the value -- counted as ambiguous too.

What survives the backward, and what is chained.  dcur / dnext swap seven times, so after n3dt_render_bwd returns dH_1 is in
`dha`, dH_0 in `dhb`; dH_7 .. dH_2 are overwritten.  They are chained in float64 from the stored dxr through the forced gates
(S carried: S_{l-1} = gate . (S_l |W_l|)); dH_1 and dH_0 are compared at the end of that chain (families "chain1", "chain0"),
dH_0 also directly from the stored dH_1.  Weight gradients, column sums and d PE that consume a chained dH_L use the chained S
and have families of their own, one per layer because the carried S grows about tenfold per level ("dw_chainL",
"colsum_chainL", "dpe_chain"); those whose operands are both stored use "dw" / "colsum".

Compositing.  The reference value uses T_s = prod_{t<s} x_t in float64 (the kernel recovers the same T as w / alpha from the
weight the forward stored); S follows the formulas as the kernel writes them: alpha = 1 - e, x = e + 1e-10 are rounded at the
scale of 1, so x_t carries an absolute error of u (e (1 + |sigma dist|) + alpha + 2 x), T = w / alpha the relative sum of those
over the samples in front, and the suffix sums sum_{t>s} |dw_t w_t|.

Bounds.  Every u_family is FACTOR = 4 times a floor measured on the CPU alone (FLOOR below, re-measured by
test_f32_stagewise_cpu.py, which fails if a recorded floor is below the measured one or more than twice it): the largest
|z32 - z64| / S of a float32 emulation of the kernels' arithmetic -- products summed over k in sequence (16-wide blocks for the
free-running emulation that produces realistic buffers, the single-fmaf chain of v_mfma_f32_32x32x2_f32 on sampled rows and
columns), K slices added in either order, the wave butterflies of the compositing kernels, numpy's float32 exp / sin / cos for
expf / sinf / cosf -- against the float64 restatement, over all cases and three seeds.  No bound comes from a GPU run.  The
factor 4 separates rounding from a dropped term, as in the earlier pins (x16_stagewise.py, nr_restatement.py).
"""
import ctypes

import numpy as np
import torch

PE_DIM, HID, G, C = 63, 384, 192, 256
XR_LD = 388                          # train_mlp.hip:23
PART_STRIDE = G + 4                  # n3dt_device.h: N3DT_PART_STRIDE
FOLD_STRIDE = 384 * 10 + 32 + 192    # n3dt_layout.h: N3DT_FOLD_STRIDE
RAYFOLD_STRIDE = 192
FOLD_USED = 384 * 9 + 32 + 192       # the table's last entry ends here; the rest of a row is never written
FOLDB_ROWGROUPS = 16                 # train_mlp.hip:539
FEATMAP_SIZE = 8

FACTOR = 4.0
AMBIGUOUS_CAP = 5e-3                 # the WIDE cap of the x16 pin; the CPU emulation must stay under a tenth of it
ALPHA_EDGE = 2.0 ** -21
ABS_SLACK = 2.0 ** -100              # fp32 underflow of products (case contrast: weights of 1e-30 behind a saturated sample)

# measured floors: largest |z32 - z64| / S of the float32 emulation per family (test_f32_stagewise_cpu.py::test_floors)
FLOOR = {
    # families "chainL", "dw_chainL", "colsum_chainL": what consumes the float64 chain at dH_L (see the module docstring)
    "fold": 1.1e-07,   # measured 7.57e-08
    "geo": 2.7e-07,   # measured 1.91e-07
    "pe": 9.5e-08,   # measured 6.81e-08
    "k63": 2.8e-07,   # measured 2.00e-07
    "k384": 4.0e-07,   # measured 2.87e-07
    "k448": 9.2e-07,   # measured 6.59e-07
    "k192": 3.9e-07,   # measured 2.81e-07
    "k256": 8.7e-08,   # measured 6.21e-08
    "head": 1.6e-07,   # measured 1.16e-07
    "chain1": 9.3e-13,   # measured 6.61e-13
    "chain0": 7.8e-14,   # measured 5.55e-14
    "dw": 1.0e-06,   # measured 7.26e-07
    "colsum": 4.7e-07,   # measured 3.33e-07
    "dpe_chain": 9.4e-10,   # measured 6.70e-10
    "comp_w": 1.5e-07,   # measured 1.06e-07
    "comp": 1.1e-06,   # measured 7.78e-07
    "dcomp": 2.4e-07,   # measured 1.72e-07
    "code": 1.6e-07,   # measured 1.15e-07
    "cam": 3.4e-07,   # measured 2.40e-07
    "dw_chain2": 7.4e-12,   # measured 5.31e-12
    "dw_chain3": 8.1e-11,   # measured 5.79e-11
    "dw_chain4": 8.1e-10,   # measured 5.80e-10
    "dw_chain5": 1.0e-08,   # measured 7.22e-09
    "dw_chain6": 9.9e-08,   # measured 7.08e-08
    "dw_chain7": 5.1e-07,   # measured 3.67e-07
    "colsum_chain2": 4.4e-12,   # measured 3.16e-12
    "colsum_chain3": 6.0e-11,   # measured 4.27e-11
    "colsum_chain4": 4.4e-10,   # measured 3.15e-10
    "colsum_chain5": 4.2e-09,   # measured 3.03e-09
    "colsum_chain6": 4.2e-08,   # measured 3.01e-08
    "colsum_chain7": 1.6e-07,   # measured 1.13e-07
}


def bound(family):
    return FACTOR * FLOOR[family]


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
CASES = {
    "a": dict(B=2, n_rays=16, n_samples=24, weights="seed", kw={}, vd=0),
    "tail": dict(B=1, n_rays=9, n_samples=40, weights="seed", kw={}, vd=0),
    "frames": dict(B=2, n_rays=25, n_samples=40, weights="seed", kw={}, vd=0),
    "split": dict(B=2, n_rays=23, n_samples=105, weights="seed", kw={}, vd=0),
    "chunks3": dict(B=1, n_rays=9, n_samples=130, weights="seed", kw={}, vd=0),
    "contrast": dict(B=2, n_rays=16, n_samples=24, weights="contrast", kw={}, vd=0),
    "gaze": dict(B=2, n_rays=16, n_samples=24, weights="seed", kw={"include_gaze": True, "eye_gaze_dim": 64, "audio_dim": 0}, vd=0),
    "vd": dict(B=1, n_rays=9, n_samples=40, weights="seed", kw={}, vd=27),
    # the hierarchical pass: z_planes_given = 1, the 16 + 24 + 1 planes of hier_stagewise.given_planes passed as t_rand
    "hier": dict(B=2, n_rays=16, n_samples=40, weights="seed", kw={}, vd=0, hier=(16, 24)),
}
VARIANTS = ("full", "frozen", "dfg", "zero")   # the three extra runs of cases a and tail


def split_for(K):  # train_mlp.hip:655-660
    return int(min(max(K // 2048, 1), 128))


def slice_rows(K, split):  # gemm32.hip:70: rows per K slice, a multiple of the 16-wide staging step
    return ((K + split - 1) // split + 15) // 16 * 16


def case_options():
    from n3dt import BaseOptions
    return BaseOptions({"featmap_size": FEATMAP_SIZE, "featmap_nc": 256, "pred_img_size": 4 * FEATMAP_SIZE, "num_sample_coarse": 32})


def case_rays(n_rays):
    r = np.unique(np.round(np.linspace(0, FEATMAP_SIZE * FEATMAP_SIZE - 1, n_rays)).astype(np.int64))
    assert len(r) == n_rays
    return r


def pack_inputs(opt, sd, inp, rays, Ns, t_rand, d_merge, vd=0, ray_bias=None, name="", variant="full", kw=None):
    """the dict every function here takes, from a state dict, synthetic.frame_inputs() and the chosen rays: float32 numpy arrays"""
    from n3dt import _lib
    p = "fg_CD_predictor."
    W = [sd[p + n + ".weight"].reshape(sd[p + n + ".weight"].shape[0], -1).numpy().copy() for n in _lib.MLP_ORDER]
    b = [sd[p + n + ".bias"].numpy().copy() for n in _lib.MLP_ORDER]
    B, n_rays = inp["shape_code"].shape[0], len(rays)
    audio = inp["audiostyle"].numpy() if inp["audiostyle"].shape[1] > 0 else None
    r = torch.from_numpy(np.asarray(rays))
    return dict(name=name, variant=variant, B=B, n_rays=n_rays, Ns=Ns, vd=vd, S=inp["shape_code"].shape[1], A=inp["appea_code"].shape[1],
                U=0 if audio is None else audio.shape[1], z1=float(opt.world_z1), z2=float(opt.world_z2), W=W, b=b, rays=np.asarray(rays), sd=sd, opt=opt, kw=kw or {},
                shape=inp["shape_code"].numpy().copy(), appea=inp["appea_code"].numpy().copy(), audio=None if audio is None else audio.copy(),
                xy=inp["batch_xy"][:, :, r].contiguous().numpy(), R=inp["batch_Rmats"].numpy().copy(),
                T=inp["batch_Tvecs"].numpy().reshape(B, 3).copy(), Kinv=inp["batch_inv_inmats"].numpy().copy(),
                t_rand=None if t_rand is None else np.asarray(t_rand),
                bg=sd["neural_render.bg_featmap"].reshape(256, -1)[:, r].contiguous().numpy(),
                ray_bias=ray_bias, d_merge=d_merge, d_fg=None, d_ba=None, frozen=False)


def case_inputs(name, seed=0, variant="full"):
    """Everything a run of a case takes, seeded.  variant: see VARIANTS."""
    from n3dt import synthetic as syn
    c = CASES[name]
    B, n_rays, Ns = c["B"], c["n_rays"], c["n_samples"]
    opt = case_options()
    sd = syn.contrast_state_dict(opt, seed=seed) if c["weights"] == "contrast" else syn.make_state_dict(opt, seed=seed, bg_noise=0.1, **c["kw"])
    inp = syn.frame_inputs(opt, B, **c["kw"])
    gen = torch.Generator().manual_seed(9 + 100 * seed)
    d_merge = torch.randn(B, n_rays, 256, generator=gen).numpy()
    d_fg = torch.randn(B, n_rays, 256, generator=gen).numpy()
    d_ba = torch.randn(B, n_rays, generator=gen).numpy()
    ray_bias = 0.2 * torch.randn(B, n_rays, 192, generator=gen).numpy() if c["vd"] else None
    out = pack_inputs(opt, sd, inp, case_rays(n_rays), Ns, syn.stratified_noise(B, n_rays, Ns, 7 + seed).numpy(), d_merge, c["vd"], ray_bias, name, variant, c["kw"])
    out["planes"] = None
    if c.get("hier"):
        import hier_stagewise as hh   # (imports this module)
        out["planes"] = hh.given_planes(out["T"][:, 2], n_rays, c["hier"][0], c["hier"][1], seed, out["z1"], out["z2"])
        out["t_rand"] = None
        assert out["planes"].shape == (B, n_rays, Ns + 1)
    if variant == "frozen":
        out["frozen"] = True
    elif variant == "dfg":
        out["d_fg"], out["d_ba"] = d_fg, d_ba
    elif variant == "zero":
        out["d_merge"] = np.zeros_like(d_merge)
    else:
        assert variant == "full"
    return out


# ---------------------------------------------------------------------------------------------------------------------
# layouts (train_mlp.hip:25-73), float offsets
# ---------------------------------------------------------------------------------------------------------------------
def al64(n):
    return (n + 63) & ~63


def bias_offset(stage):  # n3dt_layout.h: n3dt_bias_offset
    return 384 * stage if stage <= 8 else (384 * 8 + 32 if stage == 9 else 384 * 9 + 32)


def rayfold_offset(B):
    return al64(B * FOLD_STRIDE)


def fold_region_floats(B, n_rays, vd):
    return rayfold_offset(B) + B * n_rays * RAYFOLD_STRIDE if vd > 0 else B * FOLD_STRIDE


def _offsets(sizes):
    out, o = {}, 0
    for name, n in sizes:
        if n is None:            # an alias: H4 lives inside cat5
            out[name] = out["cat5"]
            continue
        out[name] = o
        o += al64(n)
    out["total"] = o
    return out


def saved_layout(B, n_rays, Ns, vd=0):
    P, R = B * n_rays * Ns, B * n_rays
    sizes = [("cat5", P * 448), ("geo", P * 2)] + [("h%d" % l, None if l == 4 else P * 384) for l in range(8)]
    sizes += [("xr", P * XR_LD), ("g", P * 192), ("w", P), ("ray", R * PART_STRIDE), ("fold", fold_region_floats(B, n_rays, vd))]
    return _offsets(sizes)


def ws_layout(B, n_rays, Ns):
    P, R = B * n_rays * Ns, B * n_rays
    return _offsets([("w5p", 384 * 448), ("wc", 385 * 384), ("bc", 385), ("dha", P * 384), ("dhb", P * 384), ("dxr", P * XR_LD), ("dg", P * 192),
                     ("dgray", R * 192), ("dwsum", R), ("dw5p", 384 * 448), ("dwc", 385 * 384), ("dfold", B * FOLD_STRIDE), ("dpe", P * 64)])


def library_totals(geom):
    """(n3dt_train_saved_floats, n3dt_train_ws_floats, n3dt_render_train_saved_bytes) of the built library"""
    from n3dt import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    out = []
    for name in ("n3dt_train_saved_floats", "n3dt_train_ws_floats", "n3dt_render_train_saved_bytes"):
        fn = getattr(L, name)
        fn.restype = ctypes.c_size_t
        fn.argtypes = [ctypes.POINTER(_lib.Geom)]
        out.append(int(fn(ctypes.byref(geom))))
    return tuple(out)


class Saved:
    def __init__(self, buf, B, n_rays, Ns, vd=0):
        buf = np.asarray(buf).reshape(-1)
        L = saved_layout(B, n_rays, Ns, vd)
        assert buf.size >= L["total"]
        P, R = B * n_rays * Ns, B * n_rays
        self.L, self.P, self.R = L, P, R
        v = lambda k, n, shape: buf[L[k]:L[k] + n].reshape(shape)  # noqa: E731
        self.cat5 = v("cat5", P * 448, (P, 448))
        self.geo = v("geo", P * 2, (P, 2))
        self.h = [self.cat5[:, 64:] if l == 4 else v("h%d" % l, P * 384, (P, 384)) for l in range(8)]
        self.xr = v("xr", P * XR_LD, (P, XR_LD))
        self.g = v("g", P * 192, (P, 192))
        self.w = v("w", P, (R, Ns))
        self.ray = v("ray", R * PART_STRIDE, (R, PART_STRIDE))
        self.fold = v("fold", B * FOLD_STRIDE, (B, FOLD_STRIDE))
        self.rayfold = buf[L["fold"] + rayfold_offset(B):L["fold"] + rayfold_offset(B) + R * 192].reshape(R, 192) if vd > 0 else None
        # everything no atomic touches, for the bit-for-bit comparison of two runs
        self.live = [self.cat5, self.geo] + [self.h[l] for l in range(8) if l != 4] + [self.xr[:, :385], self.g, self.w, self.ray[:, :G + 3], self.fold[:, :FOLD_USED]] + ([self.rayfold] if vd > 0 else [])


class Workspace:
    def __init__(self, buf, B, n_rays, Ns):
        buf = np.asarray(buf).reshape(-1)
        L = ws_layout(B, n_rays, Ns)
        assert buf.size >= L["total"]
        P, R = B * n_rays * Ns, B * n_rays
        self.L = L
        v = lambda k, n, shape: buf[L[k]:L[k] + n].reshape(shape)  # noqa: E731
        self.w5p, self.wc, self.dbc = v("w5p", 384 * 448, (384, 448)), v("wc", 385 * 384, (385, 384)), v("bc", 385, (385,))
        self.dha, self.dhb = v("dha", P * 384, (P, 384)), v("dhb", P * 384, (P, 384))
        self.dxr, self.dg = v("dxr", P * XR_LD, (P, XR_LD)), v("dg", P * 192, (P, 192))
        self.dgray, self.dwsum = v("dgray", R * 192, (R, 192)), v("dwsum", R, (R,))
        self.dw5p, self.dwc = v("dw5p", 384 * 448, (384, 448)), v("dwc", 385 * 384, (385, 384))
        self.dfold = v("dfold", B * FOLD_STRIDE, (B, FOLD_STRIDE))
        self.dpe = v("dpe", P * 64, (P, 64))
        self.live = [self.dg, self.dxr[:, :386], self.dha, self.dhb, self.dpe[:, :63], self.dgray, self.dwsum]


# ---------------------------------------------------------------------------------------------------------------------
# geometry (n3dt_device.h:25-106) in any dtype
# ---------------------------------------------------------------------------------------------------------------------
def ray_setup(dt, xy, R, Kinv):
    """c = Kinv [x, y, 1], w = R c, n = |w|, dh = w / n, l = -1 / dh_z: all [B, rays, ...]"""
    xy, R, Kinv = (np.asarray(a).astype(dt) for a in (xy, R, Kinv))
    B, _, n_rays = xy.shape
    h = np.stack([xy[:, 0], xy[:, 1], np.ones((B, n_rays), dtype=dt)], axis=-1)            # [B, r, 3]
    c = np.einsum("bij,brj->bri", Kinv, h)
    w = np.einsum("bij,brj->bri", R, c)
    n = np.sqrt((w * w).sum(axis=-1))
    dh = w / n[..., None]
    l = -dt(1) / dh[..., 2]
    return h, c, w, n, dh, l


def edges(dt, Tz, z1, z2, Ns, t_rand, planes=None):
    """stratified plane edges [B, rays, Ns + 1] (n3dt_edge_z) and the magnitude |rz1| + |rz2| their roundings scale with.
    planes [B, rays, Ns + 1] (z_planes_given, the hierarchical pass): the planes themselves in dt -- they are data, nothing is computed --
    and the largest |plane| of each frame as their magnitude"""
    if planes is not None:
        p = np.asarray(planes).astype(dt)
        assert p.shape[-1] == Ns + 1
        return p, np.abs(np.asarray(planes, dtype=np.float64)).reshape(p.shape[0], -1).max(axis=1)
    Tz = np.asarray(Tz).astype(dt)
    rz1, rz2 = Tz - dt(z1), Tz - dt(z2)
    t = np.linspace(0.0, 1.0, Ns + 1).astype(dt)
    zv = rz1[:, None] * (dt(1) - t)[None] + rz2[:, None] * t[None]
    mid = dt(0.5) * (zv[:, 1:] + zv[:, :-1])
    lower = np.concatenate([zv[:, :1], mid], axis=1)
    upper = np.concatenate([mid, zv[:, -1:]], axis=1)
    if t_rand is None:   # no jitter: the planes themselves
        return zv[:, None, :], (np.abs(rz1) + np.abs(rz2))
    z = lower[:, None, :] + (upper - lower)[:, None, :] * np.asarray(t_rand).astype(dt)
    return z, (np.abs(rz1) + np.abs(rz2))


def sample(dt, inp):
    """points [P, 3], dist [P], zval [P] and their magnitudes"""
    B, n_rays, Ns = inp["B"], inp["n_rays"], inp["Ns"]
    h, c, w, n, dh, l = ray_setup(dt, inp["xy"], inp["R"], inp["Kinv"])
    z, sz = edges(dt, inp["T"][:, 2], inp["z1"], inp["z2"], Ns, inp["t_rand"], inp.get("planes"))
    z = np.broadcast_to(z, (B, n_rays, Ns + 1))
    T = np.asarray(inp["T"]).astype(dt)
    dl = dh * l[..., None]
    pts = T[:, None, None, :] + dl[:, :, None, :] * z[..., :-1, None]
    dist = (z[..., 1:] - z[..., :-1]) * l[..., None]
    S_pts = (np.abs(T)[:, None, None, :] + np.abs(dl)[:, :, None, :] * sz[:, None, None, None]) * np.ones_like(pts)
    S_dist = 2.0 * sz[:, None, None] * np.abs(l)[..., None] * np.ones_like(dist)
    S_z = sz[:, None, None] * np.ones_like(dist)
    P = B * n_rays * Ns
    return (pts.reshape(P, 3), dist.reshape(P), z[..., :-1].reshape(P)), (S_pts.reshape(P, 3), S_dist.reshape(P), S_z.reshape(P))


def embed(dt, p):
    """[P, 3] -> [P, 64]: p, sin(2^k p), cos(2^k p), k = 0 .. 9, channel 63 zero; sin / cos of the dtype"""
    p = np.asarray(p).astype(dt)
    feats = [p]
    for k in range(10):
        a = p * dt(2.0 ** k)
        feats += [np.sin(a), np.cos(a)]
    return np.concatenate(feats + [np.zeros((p.shape[0], 1), dtype=dt)], axis=1)


# ---------------------------------------------------------------------------------------------------------------------
# products in float32 order / float64
# ---------------------------------------------------------------------------------------------------------------------
def mm_rows(dt, X, Wm):
    """X [M, K] Wm[N, K]^T: float64 exactly, float32 as 16-wide k blocks in sequence (the staging steps of gemm32_kernel)"""
    if dt is np.float64:
        return X @ Wm.T
    acc = np.zeros((X.shape[0], Wm.shape[0]), dtype=np.float32)
    for k0 in range(0, X.shape[1], 16):
        acc = acc + X[:, k0:k0 + 16] @ Wm[:, k0:k0 + 16].T
    return acc


def mm_fma_chain(X, Wm):
    """the single-fmaf chain of v_mfma_f32_32x32x2_f32: one product at a time in ascending k, each step rounded once to float32
    (the product of two float32 values is exact in float64)"""
    X, Wm = np.asarray(X, dtype=np.float32).astype(np.float64), np.asarray(Wm, dtype=np.float32).astype(np.float64)
    acc = np.zeros((X.shape[0], Wm.shape[0]), dtype=np.float32)
    for k in range(X.shape[1]):
        acc = (acc.astype(np.float64) + X[:, k:k + 1] * Wm[None, :, k]).astype(np.float32)
    return acc


def mm_points(dt, a, b, split=1, order=None, fault=None, prior=None):
    """a[K, M]^T b[K, N] over the points (both operands k-major), K slices of slice_rows() added into the destination in `order`
    (atomics), a single slice with `+=`.  prior: what the destination held.  fault "slice_tail": the second slice stops at its
    last whole staging step."""
    K = a.shape[0]
    if dt is np.float64 and fault is None:
        out = a.T @ b
        return out if prior is None else out + prior
    per = slice_rows(K, split) if split > 1 else K
    parts = []
    for z in range(split):
        k0, k1 = z * per, min(K, (z + 1) * per)
        if fault == "slice_tail" and z == 1:
            k1 = k0 + (k1 - k0) // 16 * 16
        acc = np.zeros((a.shape[1], b.shape[1]), dtype=dt)
        for kk in range(k0, k1, 16):
            acc = acc + a[kk:min(kk + 16, k1)].T @ b[kk:min(kk + 16, k1)]
        parts.append(acc)
    out = np.zeros_like(parts[0]) if prior is None else prior.astype(dt)
    for z in (order if order is not None and len(order) == split else range(split)):
        out = out + parts[z]
    return out


def butterfly_sum(v):
    """__shfl_xor butterfly over the last axis (64 lanes): every lane ends with the same sum"""
    lanes = np.arange(v.shape[-1])
    off = v.shape[-1] // 2
    while off > 0:
        v = v + v[..., lanes ^ off]
        off >>= 1
    return v


def colsum(dt, X, rows_per_frame, frames, N, fault=None):
    """train_colsum_kernel: out[f][n] = sum of the rows of frame f; row lanes in turn, chunks of rows added with atomics"""
    if dt is np.float64 and fault is None:
        return X[:frames * rows_per_frame, :N].reshape(frames, rows_per_frame, N).sum(axis=1)
    chunk = max(256, (rows_per_frame * frames + 383) // 384)
    lanes = 256 // ((N + 3) // 4)
    out = np.zeros((frames, N), dtype=dt)
    for f in range(frames):
        n_rows = rows_per_frame - 1 if fault == "colsum_last_row" else rows_per_frame
        for r0 in range(0, n_rows, chunk):
            blk = X[f * rows_per_frame + r0:f * rows_per_frame + min(n_rows, r0 + chunk), :N]
            part = np.zeros((lanes, N), dtype=dt)
            for i in range(0, blk.shape[0], lanes):
                rows = blk[i:i + lanes]
                part[:rows.shape[0]] = part[:rows.shape[0]] + rows
            s = part[0]
            for l in range(1, lanes):
                s = s + part[l]
            out[f] = out[f] + s
    return out


# ---------------------------------------------------------------------------------------------------------------------
# compositing (train_composite_fwd_kernel / _bwd_kernel) in any dtype, chunk by chunk as the kernels walk a ray
# ---------------------------------------------------------------------------------------------------------------------
def composite_fwd(dt, sig_pre, dist, zv, g, fault=None):
    """sig_pre, dist, zv [R, Ns], g [R, Ns, 192] -> w [R, Ns], record (G sums [R, 192], wsum, dsum, Trun [R])"""
    R, Ns = sig_pre.shape
    one = dt(1)
    Trun, wsum, dsum = np.ones(R, dtype=dt), np.zeros(R, dtype=dt), np.zeros(R, dtype=dt)
    acc, w_out = np.zeros((R, 192), dtype=dt), np.zeros((R, Ns), dtype=dt)
    for s0 in range(0, Ns, 64):
        n = min(64, Ns - s0)
        alpha, zvv = np.zeros((R, 64), dtype=dt), np.zeros((R, 64), dtype=dt)
        sigma = np.maximum(sig_pre[:, s0:s0 + n], dt(0))
        alpha[:, :n] = one - np.exp(-sigma * dist[:, s0:s0 + n])
        zvv[:, :n] = zv[:, s0:s0 + n]
        x = one - alpha + dt(1e-10)
        x[:, n:] = one   # lanes beyond the ray: alpha = 0, and 1 + 1e-10 is 1 in fp32
        incl = x.copy()
        for off in (1, 2, 4, 8, 16, 32):
            nxt = incl.copy()
            nxt[:, off:] = incl[:, off:] * incl[:, :-off]
            incl = nxt
        excl = np.concatenate([np.ones((R, 1), dtype=dt), incl[:, :-1]], axis=1)
        w = alpha * Trun[:, None] * excl
        w_out[:, s0:s0 + n] = w[:, :n]
        wsum = wsum + butterfly_sum(w)[:, 0]
        dsum = dsum + butterfly_sum(w * zvv)[:, 0]
        for k in range(n):
            acc = acc + w[:, k:k + 1] * g[:, s0 + k]
        if fault != "trun":
            Trun = Trun * incl[:, 63]
    return w_out, acc, wsum, dsum, Trun


def composite_bwd(dt, sig_pre, dist, w_in, g, dgray, dwsum, fault=None):
    """-> d sigma [R, Ns], d dist [R, Ns], dG [R, Ns, 192] (gated by g > 0), and the alpha > 0 gate the dtype evaluates"""
    R, Ns = sig_pre.shape
    dsig_o, ddist_o, gate_o = np.zeros((R, Ns), dtype=dt), np.zeros((R, Ns), dtype=dt), np.zeros((R, Ns), dtype=bool)
    dgr = dgray.reshape(R, 3, 64)
    carry = np.zeros(R, dtype=dt)
    for s0 in range((Ns - 1) // 64 * 64, -1, -64):
        n = min(64, Ns - s0)
        gr = g[:, s0:s0 + n].reshape(R, n, 3, 64)
        part = (dgr[:, None, 0] * gr[:, :, 0] + dgr[:, None, 1] * gr[:, :, 1]) + dgr[:, None, 2] * gr[:, :, 2]
        dw = np.zeros((R, 64), dtype=dt)
        dw[:, :n] = butterfly_sum(part)[..., 0] + dwsum[:, None]
        w, sig, dist_ = (np.zeros((R, 64), dtype=dt) for _ in range(3))
        w[:, :n], sig[:, :n], dist_[:, :n] = w_in[:, s0:s0 + n], sig_pre[:, s0:s0 + n], dist[:, s0:s0 + n]
        sigma = np.maximum(sig, dt(0))
        e = np.exp(-sigma * dist_)
        alpha = dt(1) - e
        x = e + dt(1e-10)
        v = dw * w
        incl = v.copy()
        for off in (1, 2, 4, 8, 16, 32):
            nxt = incl.copy()
            nxt[:, :64 - off] = incl[:, :64 - off] + incl[:, off:]
            incl = nxt
        suf = incl - v + (dt(0) if fault == "carry" else carry[:, None])
        pos = alpha > 0
        with np.errstate(divide="ignore", invalid="ignore"):
            T = np.where(pos, w / alpha, dt(0))
        dalpha = np.where(pos, dw * T - suf / x, dt(0))
        dsig = np.where(sig > 0, dalpha * dist_ * e, dt(0))
        dd = dalpha * sigma * e
        dsig_o[:, s0:s0 + n], ddist_o[:, s0:s0 + n], gate_o[:, s0:s0 + n] = dsig[:, :n], (-dd if fault == "ddist_sign" else dd)[:, :n], pos[:, :n]
        carry = carry + incl[:, 0]
    dG = np.where(g > 0, w_in[:, :, None] * dgray[:, None, :], dt(0))
    return dsig_o, ddist_o, dG, gate_o


# ---------------------------------------------------------------------------------------------------------------------
# camera backward (train_camera_bwd_kernel) in any dtype, with the magnitude every sum carries
# ---------------------------------------------------------------------------------------------------------------------
def camera_bwd(dt, inp, cat5, dpe, ddist, S_dq=None, fault=None):
    """-> (d_R [B,3,3], d_T [B,3], d_Kinv [B,3,3], d_xy [B,2,rays]) and the same four as sums of absolute terms.
    With given planes (the hierarchical pass) the planes are data, but d plane / d T_z = 1 as in the coarse pass (train_mlp.hip:401-411:
    they are affine combinations of the coarse planes T_z + const), so g_tz is formed exactly as without them and g_l comes from the
    differences z_hi - z_lo of the given planes.  fault "no_gtz": the g_tz term dropped when the planes are given."""
    B, n_rays, Ns = inp["B"], inp["n_rays"], inp["Ns"]
    h, c, w, n, dh, l = ray_setup(dt, inp["xy"], inp["R"], inp["Kinv"])
    z, sz = edges(dt, inp["T"][:, 2], inp["z1"], inp["z2"], Ns, inp["t_rand"], inp.get("planes"))
    z = np.broadcast_to(z, (B, n_rays, Ns + 1))
    Rm, Km = np.asarray(inp["R"]).astype(dt), np.asarray(inp["Kinv"]).astype(dt)
    pe = np.asarray(cat5)[:, :64].astype(dt).reshape(B, n_rays, Ns, 64)
    dq = np.asarray(dpe).astype(dt).reshape(B, n_rays, Ns, 64)
    dd = np.asarray(ddist).astype(dt).reshape(B, n_rays, Ns)
    aq = np.abs(dq) if S_dq is None else np.asarray(S_dq, dtype=np.float64).reshape(dq.shape)
    dp, S_dp = dq[..., 0:3].copy(), aq[..., 0:3]
    for k in range(10):
        sn, cs = pe[..., 3 + 6 * k:6 + 6 * k], pe[..., 6 + 6 * k:9 + 6 * k]
        dsn, dcs = dq[..., 3 + 6 * k:6 + 6 * k], dq[..., 6 + 6 * k:9 + 6 * k]
        dp = dp + dt(2.0 ** k) * (cs * dsn - sn * dcs)
        S_dp = S_dp + 2.0 ** k * (np.abs(cs) * aq[..., 3 + 6 * k:6 + 6 * k] + np.abs(sn) * aq[..., 6 + 6 * k:9 + 6 * k])
    z_lo, z_hi = z[..., :-1], z[..., 1:]
    dl = dh * l[..., None]
    g_dl, S_gdl = (dp * z_lo[..., None]).sum(axis=2), (S_dp * np.abs(z_lo)[..., None]).sum(axis=2)
    g_T, S_gT = dp.sum(axis=2), S_dp.sum(axis=2)
    g_tz, S_gtz = (dp * dl[:, :, None, :]).sum(axis=(2, 3)), (S_dp * np.abs(dl)[:, :, None, :]).sum(axis=(2, 3))
    if fault == "no_gtz" and inp.get("planes") is not None:
        g_tz = np.zeros_like(g_tz)
    g_l, S_gl = (dd * (z_hi - z_lo)).sum(axis=2), (np.abs(dd) * 2.0 * sz[:, None, None]).sum(axis=2)
    gl, S_glt = g_l + (g_dl * dh).sum(axis=-1), S_gl + (S_gdl * np.abs(dh)).sum(axis=-1)
    ez = np.array([0, 0, 1], dtype=dt)
    g_dh = g_dl * l[..., None] + ez * (gl * l * l)[..., None]
    S_gdh = S_gdl * np.abs(l)[..., None] + ez * (S_glt * l * l)[..., None]
    dot, S_dot = (g_dh * dh).sum(axis=-1), (S_gdh * np.abs(dh)).sum(axis=-1)
    gw = (g_dh - dh * dot[..., None]) / n[..., None]
    S_gw = (S_gdh + np.abs(dh) * S_dot[..., None]) / n[..., None]
    d_R, S_R = np.einsum("bri,brj->bij", gw, c), np.einsum("bri,brj->bij", S_gw, np.abs(c))
    gc, S_gc = np.einsum("bij,bri->brj", Rm, gw), np.einsum("bij,bri->brj", np.abs(Rm), S_gw)
    d_K, S_K = np.einsum("bri,brj->bij", gc, h), np.einsum("bri,brj->bij", S_gc, np.abs(h))
    d_xy = np.stack([np.einsum("bri,bi->br", gc, Km[:, :, 0]), np.einsum("bri,bi->br", gc, Km[:, :, 1])], axis=1)
    S_xy = np.stack([np.einsum("bri,bi->br", S_gc, np.abs(Km[:, :, 0])), np.einsum("bri,bi->br", S_gc, np.abs(Km[:, :, 1]))], axis=1)
    d_T, S_T = (g_T + ez * g_tz[..., None]).sum(axis=1), (S_gT + ez * S_gtz[..., None]).sum(axis=1)
    return (d_R, d_T, d_K, d_xy), tuple(np.asarray(s, dtype=np.float64) for s in (S_R, S_T, S_K, S_xy))


# ---------------------------------------------------------------------------------------------------------------------
# the whole path in one dtype: float32 = the free-running CPU emulation, float64 = the restatement run end to end
# ---------------------------------------------------------------------------------------------------------------------
def latent_code(inp):
    su = inp["shape"] if inp["audio"] is None else np.concatenate([inp["shape"], inp["audio"]], axis=1)
    return su


def fold_dot(dt, code, Wlat):
    """fold_latents_kernel: 64 lanes stride over the code, a butterfly adds them: [B, n] x [N, n] -> [B, N]"""
    if dt is np.float64:
        return code @ Wlat.T
    n = code.shape[1]
    pad = (-n) % 64
    cp = np.concatenate([code, np.zeros((code.shape[0], pad), dtype=dt)], axis=1).reshape(code.shape[0], -1, 64)
    wp = np.concatenate([Wlat, np.zeros((Wlat.shape[0], pad), dtype=dt)], axis=1).reshape(Wlat.shape[0], -1, 64)
    acc = np.zeros((code.shape[0], Wlat.shape[0], 64), dtype=dt)
    for i in range(cp.shape[1]):
        acc = acc + cp[:, None, i, :] * wp[None, :, i, :]
    return butterfly_sum(acc)[..., 0]


def run_path(inp, dt=np.float32, fault=None, order=None):
    """-> record dict(saved=Saved, ws=Workspace, gw, gb (None when frozen), out, res): what a synchronised forward + backward
    through ops.render_train_fwd / ops.render_bwd leaves behind, computed in `dt`.  fault: one of the deliberate faults of
    test_f32_stagewise_cpu.py.  order: the order the K slices of every split product reach their destination."""
    B, n_rays, Ns, S, A, U, vd = (inp[k] for k in ("B", "n_rays", "Ns", "S", "A", "U", "vd"))
    P, R, ppf = B * n_rays * Ns, B * n_rays, n_rays * Ns
    W = [np.asarray(w).astype(dt) for w in inp["W"]]
    b = [np.asarray(v).astype(dt) for v in inp["b"]]
    shape, appea = inp["shape"].astype(dt), inp["appea"].astype(dt)
    su = latent_code(inp).astype(dt)
    Ls, Lw = saved_layout(B, n_rays, Ns, vd), ws_layout(B, n_rays, Ns)
    sv, wk = Saved(np.zeros(Ls["total"], dtype=dt), B, n_rays, Ns, vd), Workspace(np.zeros(Lw["total"], dtype=dt), B, n_rays, Ns)
    frame = np.arange(P) // ppf
    # ---- forward
    for l in range(8):
        sv.fold[:, bias_offset(l):bias_offset(l) + 384] = b[l]
    sv.fold[:, 0:384] = b[0] + fold_dot(dt, su, W[0][:, 63:])
    sv.fold[:, bias_offset(5):bias_offset(5) + 384] = b[5] + fold_dot(dt, shape, W[5][:, 63:63 + S])
    sv.fold[:, bias_offset(8)] = b[8][0]
    sv.fold[:, bias_offset(9):bias_offset(9) + 384] = b[9]
    sv.fold[:, bias_offset(10):bias_offset(10) + 192] = b[10] + fold_dot(dt, appea, W[10][:, 384:])
    if vd:
        sv.rayfold[:] = sv.fold[np.arange(R) // n_rays, bias_offset(10):bias_offset(10) + 192] + inp["ray_bias"].reshape(R, 192).astype(dt)
    wk.w5p[:, :63], wk.w5p[:, 64:] = W[5][:, :63], W[5][:, 63 + S:63 + S + 384]
    wk.wc[:384], wk.wc[384] = W[9], W[8][0]
    (pts, dist, zval), _ = sample(np.float64, inp)
    if inp.get("geo") is not None:   # sample points, plane distances and z values given (a fixture's fp32 ones): [P, 3], [P], [P]
        pts, dist, zval = inp["geo"]
    sv.cat5[:, :64] = embed(dt, pts.astype(dt))
    sv.geo[:, 0], sv.geo[:, 1] = dist.astype(dt), zval.astype(dt)
    brow = frame if fault != "bias_row_tile" else (np.arange(P) // 128 * 128) // ppf

    def fbias(l, n):
        return sv.fold[brow, bias_offset(l):bias_offset(l) + n]
    for l in range(8):
        X, Wl = (sv.cat5[:, :63], W[0][:, :63]) if l == 0 else ((sv.cat5, wk.w5p) if l == 5 else (sv.h[l - 1], W[l]))
        sv.h[l][:] = np.maximum(mm_rows(dt, np.ascontiguousarray(X), np.ascontiguousarray(Wl)) + fbias(l, 384), dt(0))
        for fl, fp, fc in inp.get("flip", ()):   # a gate taken the other way (an fp32 forward that landed on the other side of zero)
            if fl == l:
                sv.h[l][fp, fc] = dt(0) if sv.h[l][fp, fc] > 0 else np.finfo(dt).tiny
    bc = np.concatenate([b[9], b[8]])
    sv.xr[:, :385] = mm_rows(dt, sv.h[7], wk.wc) + bc
    if vd:
        rb = sv.rayfold[(np.arange(P) // ppf) if fault == "raybias_ppf" else (np.arange(P) // Ns)]
    else:
        rb = fbias(10, 192)
    sv.g[:] = np.maximum(mm_rows(dt, np.ascontiguousarray(sv.xr[:, :384]), np.ascontiguousarray(W[10][:, :384])) + rb, dt(0))
    sig, dst, zv = sv.xr[:, 384].reshape(R, Ns), sv.geo[:, 0].reshape(R, Ns), sv.geo[:, 1].reshape(R, Ns)
    w, gsum, wsum, dsum, trun = composite_fwd(dt, sig, dst, zv, sv.g.reshape(R, Ns, 192), fault)
    sv.w[:] = w
    sv.ray[:, :G], sv.ray[:, G], sv.ray[:, G + 1], sv.ray[:, G + 2] = gsum, wsum, dsum, trun
    bg = inp["bg"].astype(dt)                                                    # [256, n_rays]
    bg_r = np.tile(bg.T, (B, 1))                                                 # [R, 256]
    fg = mm_rows(dt, gsum, W[11]) + b[11][None, :] * wsum[:, None]
    ba = dt(1) - wsum
    out = {"fg_feat": fg.reshape(B, n_rays, 256), "bg_alpha": ba.reshape(B, n_rays), "merge_feat": (fg + ba[:, None] * bg_r).reshape(B, n_rays, 256)}
    # ---- backward
    frozen = inp["frozen"]
    dm = inp["d_merge"].reshape(R, 256).astype(dt)
    dfg = dm + (inp["d_fg"].reshape(R, 256).astype(dt) if inp["d_fg"] is not None else dt(0))
    part = b[11][None, :] * dfg - dm * bg_r
    red = butterfly_sum(part.reshape(R, 4, 64))[..., 0]
    wk.dwsum[:] = (red[:, 0] + red[:, 1]) + (red[:, 2] + red[:, 3]) - (inp["d_ba"].reshape(R).astype(dt) if inp["d_ba"] is not None else dt(0))
    wk.dgray[:] = mm_rows(dt, dfg, np.ascontiguousarray(W[11].T))
    gw = gb = d_bg = None
    if not frozen:
        gw, gb = [np.zeros_like(x) for x in W], [np.zeros_like(x) for x in b]
        d_bg = ((dt(1) - wsum)[:, None] * dm).reshape(B, n_rays, 256).sum(axis=0).T.astype(dt)
        gb[11] = (wsum[:, None] * dfg).sum(axis=0).astype(dt)
        gw[11] = mm_points(dt, dfg, gsum, split_for(R), order)

    def dwp(a_, b_, K=P):
        return mm_points(dt, np.ascontiguousarray(a_), np.ascontiguousarray(b_), split_for(K), order, fault if fault == "slice_tail" else None)
    cs_fault = fault if fault == "colsum_last_row" else None
    dsig, ddist, dG, _ = composite_bwd(dt, sig, dst, w, sv.g.reshape(R, Ns, 192), wk.dgray, wk.dwsum, fault)
    wk.dg[:] = dG.reshape(P, 192)
    wk.dxr[:, 384], wk.dxr[:, 385] = dsig.reshape(P), ddist.reshape(P)
    wk.dxr[:, :384] = mm_rows(dt, wk.dg, np.ascontiguousarray(W[10][:, :384].T))
    if not frozen:
        gw[10][:, :384] = dwp(wk.dg, sv.xr[:, :384])
    wk.dfold[:, bias_offset(10):bias_offset(10) + 192] = colsum(dt, wk.dg, ppf, B, 192, cs_fault)
    d_ray = colsum(dt, wk.dg, Ns, R, 192).reshape(B, n_rays, 192) if vd else None
    dcur = np.where(sv.h[7] > 0, mm_rows(dt, np.ascontiguousarray(wk.dxr[:, :385]), np.ascontiguousarray(wk.wc.T)), dt(0))
    if not frozen:
        wk.dwc[:] = dwp(wk.dxr[:, :385], sv.h[7])
        wk.dbc[:] = colsum(dt, wk.dxr, P, 1, 385)[0]
    dH = {7: dcur}
    for l in range(7, -1, -1):
        dcur = dH[l]
        if not frozen:
            if l == 5:
                wk.dw5p[:] = dwp(dcur, sv.cat5)
            elif l == 0:
                gw[0][:, :63] = dwp(dcur, sv.cat5[:, :63])
            else:
                gw[l][:] = dwp(dcur, sv.h[l - 1])
        if l in (0, 5):
            wk.dfold[:, bias_offset(l):bias_offset(l) + 384] = colsum(dt, dcur, ppf, B, 384, cs_fault)
        elif not frozen:
            gb[l] = colsum(dt, dcur, P, 1, 384)[0]
        if l == 5:
            wk.dpe[:] = mm_rows(dt, dcur, np.ascontiguousarray(wk.w5p[:, :64].T))
        if l == 0:
            wk.dpe[:, :63] = wk.dpe[:, :63] + mm_rows(dt, dcur, np.ascontiguousarray(W[0][:, :63].T))
            break
        Wl = wk.w5p[:, 64:] if l == 5 else W[l]
        dH[l - 1] = np.where(sv.h[l - 1] > 0, mm_rows(dt, dcur, np.ascontiguousarray(Wl.T)), dt(0))
    wk.dha[:], wk.dhb[:] = dH[1], dH[0]
    (d_R, d_T, d_K, d_xy), _ = camera_bwd(dt, inp, sv.cat5, wk.dpe, wk.dxr[:, 385], fault=fault)
    if not frozen:   # train_unpack_grads_kernel
        off = 63 + S + (1 if fault == "unpack_off" else 0)
        gw[5][:, :63] += wk.dw5p[:, :63]
        gw[5][:, off:off + 384 - (1 if fault == "unpack_off" else 0)] += wk.dw5p[:, 64:448 - (1 if fault == "unpack_off" else 0)]
        gw[9] += wk.dwc[:384]
        gw[8] += wk.dwc[384:385]
        gb[9] += wk.dbc[:384]
        gb[8] += wk.dbc[384:385]
    # train_fold_bwd_kernel: rows in FOLDB_ROWGROUPS groups, the groups (and the two tables of d_shape) added with atomics
    tables = ((0, 0, su, W[0][:, 63:], 63), (5, 5, shape, W[5][:, 63:63 + S], 63), (10, 10, appea, W[10][:, 384:], 384))
    dcode = {}
    for layer, st, code, Wlat, col0 in tables:
        db = wk.dfold[:, bias_offset(st):bias_offset(st) + Wlat.shape[0]]               # [B, nout]
        per = (Wlat.shape[0] + FOLDB_ROWGROUPS - 1) // FOLDB_ROWGROUPS
        acc = np.zeros((B, Wlat.shape[1]), dtype=dt)
        for o0 in range(0, Wlat.shape[0], per):
            acc = acc + mm_rows(dt, np.ascontiguousarray(db[:, o0:o0 + per]), np.ascontiguousarray(Wlat[o0:o0 + per].T))
        dcode[layer] = acc
        if not frozen:
            for f in range(B):
                gb[layer] = gb[layer] + db[f]
                gw[layer][:, col0:col0 + Wlat.shape[1]] += db[f][:, None] * code[f][None, :]
    d_shape = dcode[0][:, :S] + dcode[5]
    res = {"d_bg": d_bg, "d_shape": d_shape, "d_appea": dcode[10], "d_audio": dcode[0][:, S:] if U > 0 else None, "d_R": d_R, "d_T": d_T,
           "d_Kinv": d_K, "d_xy": d_xy, "d_ray_bias": d_ray}
    return {"saved": sv, "ws": wk, "gw": gw, "gb": gb, "out": out, "res": res, "dH": dH}


# ---------------------------------------------------------------------------------------------------------------------
# the teacher-forced stage checks
# ---------------------------------------------------------------------------------------------------------------------
def f64(a):
    return np.asarray(a).astype(np.float64)


def prod64(X, Wm, bias=None):
    """z = X Wm^T (+ bias) and S = |bias| + |X| |Wm|^T"""
    X, Wm = f64(X), f64(Wm)
    z, S = X @ Wm.T, np.abs(X) @ np.abs(Wm).T
    if bias is not None:
        z, S = z + f64(bias), S + np.abs(f64(bias))
    return z, S


def comp_terms(sig_pre, dist):
    """float64 compositing terms of stored sigma_pre, dist [R, Ns]: alpha, e, x, T, and the absolute error units of alpha and x
    (in u): eps_a = e (1 + |arg|) + alpha, eps_x = eps_a + 2 x; rel_T = sum_{t<s} eps_x / x + s"""
    sig, d = f64(sig_pre), f64(dist)
    sigma = np.maximum(sig, 0.0)
    arg = sigma * d
    e = np.exp(-arg)
    alpha = 1.0 - e
    x = 1.0 - alpha + 1e-10
    T = np.concatenate([np.ones((sig.shape[0], 1)), np.cumprod(x, axis=1)[:, :-1]], axis=1)
    eps_a = e * (1.0 + np.abs(arg)) + np.abs(alpha)
    eps_x = eps_a + 2.0 * x
    rel = eps_x / x + 1.0
    rel_T = np.concatenate([np.zeros((sig.shape[0], 1)), np.cumsum(rel, axis=1)[:, :-1]], axis=1)
    return dict(sigma=sigma, arg=arg, e=e, alpha=alpha, x=x, T=T, eps_a=eps_a, eps_x=eps_x, rel_T=rel_T, rel_all=rel.sum(axis=1))


def chk(tag, family, got, z, S, relu=False, amb=None, exact=False, Sc=None):
    """Sc: the magnitude of the same entry carried through the float64 chain (for entries computed from the stored dH_1 / dH_0, whose
    S is the teacher-forced one): what a free-running float64 evaluation of the whole path can be held to"""
    return dict(tag=tag, family=family, got=np.asarray(got), z=np.asarray(z, dtype=np.float64), S=np.asarray(S, dtype=np.float64), relu=relu, amb=amb,
                exact=exact, Sc=None if Sc is None else np.asarray(Sc, dtype=np.float64))


def stages(inp, rec):
    """Every check of a run, as dicts of chk().  inp: case_inputs(); rec: a record as run_path() / the GPU run leaves it.
    (The CPU floor of family "geo" comes from the fp32 oracle's sampler, test_f32_stagewise_cpu.py.)"""
    B, n_rays, Ns, S_, A, U, vd = (inp[k] for k in ("B", "n_rays", "Ns", "S", "A", "U", "vd"))
    P, R, ppf = B * n_rays * Ns, B * n_rays, n_rays * Ns
    sv, wk = rec["saved"], rec["ws"]
    W, b = [f64(w) for w in inp["W"]], [f64(v) for v in inp["b"]]
    frame = np.arange(P) // ppf
    su, shape, appea = f64(latent_code(inp)), f64(inp["shape"]), f64(inp["appea"])
    out = []
    # ---- fold
    for st, code, Wlat in ((0, su, W[0][:, 63:]), (5, shape, W[5][:, 63:63 + S_]), (10, appea, W[10][:, 384:])):
        n = Wlat.shape[0]
        out.append(chk("fold%d" % st, "fold", sv.fold[:, bias_offset(st):bias_offset(st) + n], b[st] + code @ Wlat.T, np.abs(b[st]) + np.abs(code) @ np.abs(Wlat).T))
    plain = np.zeros((B, FOLD_STRIDE))
    for l in (1, 2, 3, 4, 6, 7, 9):
        plain[:, bias_offset(l):bias_offset(l) + 384] = b[l]
    plain[:, bias_offset(8)] = b[8][0]
    keep = np.arange(FOLD_STRIDE) < FOLD_USED
    for st, n in ((0, 384), (5, 384), (10, 192)):
        keep[bias_offset(st):bias_offset(st) + n] = False
    out.append(chk("fold copies", "fold", sv.fold[:, keep], plain[:, keep], 0.0, exact=True))
    if vd:
        want = np.asarray(sv.fold)[np.arange(R) // n_rays, bias_offset(10):bias_offset(10) + 192] + inp["ray_bias"].reshape(R, 192).astype(np.asarray(sv.fold).dtype)
        out.append(chk("rayfold", "fold", sv.rayfold, want, 0.0, exact=True))
    # ---- geometry and PE
    (pts, dist, zval), (S_p, S_d, S_z) = sample(np.float64, inp)
    out.append(chk("points", "geo", sv.cat5[:, :3], pts, S_p))
    out.append(chk("dist", "geo", sv.geo[:, 0], dist, S_d))
    out.append(chk("zval", "geo", sv.geo[:, 1], zval, S_z))
    out.append(chk("PE", "pe", sv.cat5[:, 3:63], embed(np.float64, f64(sv.cat5[:, :3]))[:, 3:63], 1.0))
    out.append(chk("cat5[:, 63]", "pe", sv.cat5[:, 63], np.zeros(P), 0.0, exact=True))
    # ---- pack
    w5p = np.zeros((384, 448))
    w5p[:, :63], w5p[:, 64:] = W[5][:, :63], W[5][:, 63 + S_:63 + S_ + 384]
    wc = np.concatenate([W[9], W[8]], axis=0)
    out.append(chk("W5'", "fold", wk.w5p, w5p, 0.0, exact=True))
    out.append(chk("Wc", "fold", wk.wc, wc, 0.0, exact=True))
    # ---- trunk
    fold64 = f64(sv.fold)
    for l in range(8):
        if l == 0:
            z, S = prod64(sv.cat5[:, :63], W[0][:, :63], fold64[frame, 0:384])
        elif l == 5:
            z, S = prod64(sv.cat5, w5p, fold64[frame, bias_offset(5):bias_offset(5) + 384])
        else:
            z, S = prod64(sv.h[l - 1], W[l], fold64[frame, bias_offset(l):bias_offset(l) + 384])
        out.append(chk("H%d" % l, "k63" if l == 0 else ("k448" if l == 5 else "k384"), sv.h[l], z, S, relu=True))
    z, S = prod64(sv.h[7], wc, np.concatenate([b[9], b[8]])[None, :])
    out.append(chk("xr", "k384", sv.xr[:, :385], z, S))
    rb = f64(sv.rayfold)[np.arange(P) // Ns] if vd else fold64[frame, bias_offset(10):bias_offset(10) + 192]
    z, S = prod64(sv.xr[:, :384], W[10][:, :384], rb)
    out.append(chk("g", "k384", sv.g, z, S, relu=True))
    # ---- compositing
    sig32, dist32 = np.asarray(sv.xr[:, 384]).reshape(R, Ns), np.asarray(sv.geo[:, 0]).reshape(R, Ns)
    ct = comp_terms(sig32, dist32)
    w64 = ct["alpha"] * ct["T"]
    S_w = ct["T"] * ct["eps_a"] + np.abs(w64) * (ct["rel_T"] + 2.0)
    out.append(chk("w", "comp_w", sv.w, w64, S_w))
    ws_, g_, zv_ = f64(sv.w), f64(sv.g).reshape(R, Ns, 192), f64(sv.geo[:, 1]).reshape(R, Ns)
    out.append(chk("ray G", "comp", sv.ray[:, :G], np.einsum("rs,rsc->rc", ws_, g_), np.einsum("rs,rsc->rc", np.abs(ws_), np.abs(g_))))
    out.append(chk("ray wsum", "comp", sv.ray[:, G], ws_.sum(axis=1), np.abs(ws_).sum(axis=1)))
    out.append(chk("ray dsum", "comp", sv.ray[:, G + 1], (ws_ * zv_).sum(axis=1), np.abs(ws_ * zv_).sum(axis=1)))
    trun = np.prod(ct["x"], axis=1)
    out.append(chk("ray Trun", "comp_w", sv.ray[:, G + 2], trun, trun * (ct["rel_all"] + 1.0)))
    # ---- head
    gray, wsum = f64(sv.ray[:, :G]), f64(sv.ray[:, G])
    bg_r = np.tile(f64(inp["bg"]).T, (B, 1))
    fg = f64(rec["out"]["fg_feat"]).reshape(R, 256)
    ba = f64(rec["out"]["bg_alpha"]).reshape(R)
    out.append(chk("fg_feat", "k192", fg, gray @ W[11].T + b[11][None, :] * wsum[:, None], np.abs(gray) @ np.abs(W[11]).T + np.abs(b[11][None, :] * wsum[:, None])))
    out.append(chk("bg_alpha", "head", ba, 1.0 - wsum, 1.0 + np.abs(wsum)))
    out.append(chk("merge_feat", "head", f64(rec["out"]["merge_feat"]).reshape(R, 256), fg + ba[:, None] * bg_r, np.abs(fg) + np.abs(ba[:, None] * bg_r)))
    # ---- head backward
    rdt = np.asarray(wk.dgray).dtype   # single operations are restated in the record's own type: exact for the fp32 kernels
    dm32 = inp["d_merge"].reshape(R, 256).astype(rdt)
    dfg32 = dm32 + inp["d_fg"].reshape(R, 256).astype(rdt) if inp["d_fg"] is not None else dm32
    dm, dfg = f64(dm32), f64(dfg32)
    dba = f64(inp["d_ba"]).reshape(R) if inp["d_ba"] is not None else np.zeros(R)
    S_dgray = np.abs(dfg) @ np.abs(W[11])
    out.append(chk("dgray", "k256", wk.dgray, dfg @ W[11], S_dgray))
    out.append(chk("dwsum", "k256", wk.dwsum, (b[11][None, :] * dfg - dm * bg_r).sum(axis=1) - dba,
                   (np.abs(b[11][None, :] * dfg) + np.abs(dm * bg_r)).sum(axis=1) + np.abs(dba)))
    # ---- compositing backward
    gate_g = np.asarray(sv.g) > 0
    w32, dgray32 = np.asarray(sv.w).reshape(P), np.asarray(wk.dgray)
    ray_of = np.arange(P) // Ns
    out.append(chk("dg", "head", wk.dg, np.where(gate_g, w32[:, None] * dgray32[ray_of], rdt.type(0)), 0.0, exact=True))
    dgray64, dwsum64 = f64(wk.dgray), f64(wk.dwsum)
    dw = np.einsum("rc,rsc->rs", dgray64, g_) + dwsum64[:, None]
    S_dw = np.einsum("rc,rsc->rs", np.abs(dgray64), np.abs(g_)) + np.abs(dwsum64)[:, None]
    v, S_v = dw * ws_, 2.0 * S_dw * np.abs(ws_)
    suf = np.concatenate([np.cumsum(v[:, ::-1], axis=1)[:, ::-1][:, 1:], np.zeros((R, 1))], axis=1)
    S_suf = np.concatenate([np.cumsum(S_v[:, ::-1], axis=1)[:, ::-1][:, 1:], np.zeros((R, 1))], axis=1)
    pos32 = (np.float32(1) - np.exp(-np.maximum(sig32.astype(np.float32), np.float32(0)) * dist32.astype(np.float32))) > 0
    edge = ((ct["alpha"] > 0) | pos32) & (ct["alpha"] < ALPHA_EDGE)
    dalpha = np.where(pos32 | edge, dw * ct["T"] - suf / ct["x"], 0.0)
    S_da = S_dw * ct["T"] + np.abs(dw) * ct["T"] * (ct["rel_T"] + 2.0) + S_suf / ct["x"] + np.abs(suf) * (ct["eps_x"] + ct["x"]) / ct["x"] ** 2
    d64 = f64(dist32)
    dsig = np.where(sig32 > 0, dalpha * d64 * ct["e"], 0.0)
    ddist = dalpha * ct["sigma"] * ct["e"]
    S_dsig = (S_da * np.abs(d64) + np.abs(dalpha * d64) * (2.0 + ct["arg"])) * ct["e"]
    out.append(chk("d sigma", "dcomp", np.asarray(wk.dxr[:, 384]).reshape(R, Ns), dsig, S_dsig, amb=edge))
    out.append(chk("d dist", "dcomp", np.asarray(wk.dxr[:, 385]).reshape(R, Ns), ddist, (S_da + np.abs(dalpha) * (2.0 + ct["arg"])) * ct["sigma"] * ct["e"], amb=edge))
    # ---- MLP backward
    z, S = prod64(wk.dg, W[10][:, :384].T)
    out.append(chk("dxr[:, 0:384]", "k192", wk.dxr[:, :384], z, S))
    S_dg = np.where(gate_g, S_w.reshape(P, 1) * np.abs(dgray64)[ray_of] + np.abs(ws_).reshape(P, 1) * S_dgray[ray_of], 0.0)
    S_dxr = np.concatenate([S_dg @ np.abs(W[10][:, :384]), S_dsig.reshape(P, 1)], axis=1)
    gates = [np.asarray(sv.h[l]) > 0 for l in range(8)]
    dxr = f64(wk.dxr[:, :385])
    dH, SH = {}, {}
    SHc = {}   # the chain's magnitude started from the magnitude of dxr itself: what a free-running evaluation is held to (chk: Sc)
    dH[7], SH[7], SHc[7] = np.where(gates[7], dxr @ wc, 0.0), np.where(gates[7], np.abs(dxr) @ np.abs(wc), 0.0), np.where(gates[7], S_dxr @ np.abs(wc), 0.0)
    for l in range(7, 0, -1):
        Wl = w5p[:, 64:] if l == 5 else W[l]
        dH[l - 1], SH[l - 1] = np.where(gates[l - 1], dH[l] @ Wl, 0.0), np.where(gates[l - 1], SH[l] @ np.abs(Wl), 0.0)
        SHc[l - 1] = np.where(gates[l - 1], SHc[l] @ np.abs(Wl), 0.0)
    out.append(chk("dH1 (chain)", "chain1", wk.dha, dH[1], SH[1]))
    out.append(chk("dH0 (chain)", "chain0", wk.dhb, dH[0], SH[0]))
    dh1, dh0 = f64(wk.dha), f64(wk.dhb)
    out.append(chk("dH0 from dH1", "k384", wk.dhb, np.where(gates[0], dh1 @ W[1], 0.0), np.where(gates[0], np.abs(dh1) @ np.abs(W[1]), 0.0)))
    onehot = (frame[:, None] == np.arange(B)[None, :]).astype(np.float64)
    dg64 = f64(wk.dg)
    Sdb0, Sdb5 = onehot.T @ SHc[0], onehot.T @ SHc[5]
    out.append(chk("dfold0", "colsum", wk.dfold[:, 0:384], onehot.T @ dh0, onehot.T @ np.abs(dh0), Sc=Sdb0))
    out.append(chk("dfold5", "colsum_chain5", wk.dfold[:, bias_offset(5):bias_offset(5) + 384], onehot.T @ dH[5], onehot.T @ SH[5], Sc=Sdb5))
    out.append(chk("dfold10", "colsum", wk.dfold[:, bias_offset(10):bias_offset(10) + 192], onehot.T @ dg64, onehot.T @ np.abs(dg64), Sc=onehot.T @ S_dg))
    Sdb10 = onehot.T @ S_dg
    cat5 = f64(sv.cat5)
    out.append(chk("dpe", "dpe_chain", wk.dpe[:, :63], dH[5] @ w5p[:, :63] + dh0 @ W[0][:, :63], SH[5] @ np.abs(w5p[:, :63]) + np.abs(dh0) @ np.abs(W[0][:, :63])))
    res = rec["res"]
    if vd:
        out.append(chk("d_ray_bias", "colsum", f64(res["d_ray_bias"]).reshape(R, 192), dg64.reshape(R, Ns, 192).sum(axis=1), np.abs(dg64).reshape(R, Ns, 192).sum(axis=1),
                       Sc=S_dg.reshape(R, Ns, 192).sum(axis=1)))
    else:
        assert res.get("d_ray_bias") is None
    # ---- camera
    (cR, cT, cK, cxy), (sR, sT, sK, sxy) = camera_bwd(np.float64, inp, sv.cat5, wk.dpe, wk.dxr[:, 385])
    S_dq = np.zeros((P, 64))
    S_dq[:, :63] = SHc[5] @ np.abs(w5p[:, :63]) + SHc[0] @ np.abs(W[0][:, :63])
    _, chained = camera_bwd(np.float64, inp, sv.cat5, wk.dpe, wk.dxr[:, 385], S_dq)
    for k, zc, sc, cc in (("d_R", cR, sR, chained[0]), ("d_T", cT, sT, chained[1]), ("d_Kinv", cK, sK, chained[2]), ("d_xy", cxy, sxy, chained[3])):
        if res.get(k) is not None:
            out.append(chk(k, "cam", f64(res[k]).reshape(zc.shape), zc, sc, Sc=cc))
    # ---- code gradients
    dfold = f64(wk.dfold)
    db0, db5, db10 = dfold[:, 0:384], dfold[:, bias_offset(5):bias_offset(5) + 384], dfold[:, bias_offset(10):bias_offset(10) + 192]
    w0l, w5l, w10l = W[0][:, 63:], W[5][:, 63:63 + S_], W[10][:, 384:]
    d_su, S_su = db0 @ w0l, np.abs(db0) @ np.abs(w0l)
    Sc_su = Sdb0 @ np.abs(w0l)
    out.append(chk("d_shape", "code", res["d_shape"], d_su[:, :S_] + db5 @ w5l, S_su[:, :S_] + np.abs(db5) @ np.abs(w5l), Sc=Sc_su[:, :S_] + Sdb5 @ np.abs(w5l)))
    out.append(chk("d_appea", "code", res["d_appea"], db10 @ w10l, np.abs(db10) @ np.abs(w10l), Sc=Sdb10 @ np.abs(w10l)))
    if U > 0:
        out.append(chk("d_audio", "code", res["d_audio"], d_su[:, S_:], S_su[:, S_:], Sc=Sc_su[:, S_:]))
    else:
        assert res["d_audio"] is None
    if rec["gw"] is None:
        assert res["d_bg"] is None
        return out
    # ---- parameter gradients
    gw, gb = rec["gw"], rec["gb"]

    def dwchk(tag, fam, got, a, bm, Sa=None, Sca=None):
        a, bm = f64(a), f64(bm)
        out.append(chk(tag, fam, got, a.T @ bm, (np.abs(a) if Sa is None else Sa).T @ np.abs(bm), Sc=None if Sca is None else Sca.T @ np.abs(bm)))
    dwchk("dW0[:, PE]", "dw", gw[0][:, :63], dh0, cat5[:, :63], Sca=SHc[0])
    dwchk("dW1", "dw", gw[1], dh1, sv.h[0], Sca=SHc[1])
    for l in (2, 3, 4, 6, 7):
        dwchk("dW%d" % l, "dw_chain%d" % l, gw[l], dH[l], sv.h[l - 1], SH[l], SHc[l])
        out.append(chk("db%d" % l, "colsum_chain%d" % l, gb[l], dH[l].sum(axis=0), SH[l].sum(axis=0), Sc=SHc[l].sum(axis=0)))
    out.append(chk("db1", "colsum", gb[1], dh1.sum(axis=0), np.abs(dh1).sum(axis=0), Sc=SHc[1].sum(axis=0)))
    dwchk("dW5'", "dw_chain5", wk.dw5p, dH[5], cat5, SH[5], SHc[5])
    dwchk("dW5[:, PE]", "dw_chain5", gw[5][:, :63], dH[5], cat5[:, :63], SH[5], SHc[5])
    dwchk("dW5[:, H4]", "dw_chain5", gw[5][:, 63 + S_:], dH[5], cat5[:, 64:], SH[5], SHc[5])
    dwchk("dWc", "dw", wk.dwc, dxr, sv.h[7], Sca=S_dxr)
    out.append(chk("dbc", "colsum", wk.dbc, dxr.sum(axis=0), np.abs(dxr).sum(axis=0), Sc=S_dxr.sum(axis=0)))
    dwchk("dWr1[:, 0:384]", "dw", gw[10][:, :384], dg64, sv.xr[:, :384], Sca=S_dg)
    S_gray, S_wsum = np.einsum("rs,rsc->rc", S_w, np.abs(g_)), S_w.sum(axis=1)
    out.append(chk("dW_rgb2", "dw", gw[11], dfg.T @ gray, np.abs(dfg).T @ np.abs(gray), Sc=np.abs(dfg).T @ S_gray))
    out.append(chk("db_rgb2", "colsum", gb[11], (wsum[:, None] * dfg).sum(axis=0), np.abs(wsum[:, None] * dfg).sum(axis=0), Sc=(S_wsum[:, None] * np.abs(dfg)).sum(axis=0)))
    # the un-pack: plain copies of the packed gradients into zeroed tensors (0 + x = x), column 63 of dW5' never leaves
    out.append(chk("unpack W5 PE", "dw", gw[5][:, :63], wk.dw5p[:, :63], 0.0, exact=True))
    out.append(chk("unpack W5 H4", "dw", gw[5][:, 63 + S_:], wk.dw5p[:, 64:], 0.0, exact=True))
    out.append(chk("unpack Wr0", "dw", gw[9], wk.dwc[:384], 0.0, exact=True))
    out.append(chk("unpack wd", "dw", gw[8], wk.dwc[384:385], 0.0, exact=True))
    out.append(chk("unpack br0", "dw", gb[9], wk.dbc[:384], 0.0, exact=True))
    out.append(chk("unpack bd", "dw", gb[8], wk.dbc[384:385], 0.0, exact=True))
    # folding adjoint
    for layer, db, sc in ((0, db0, Sdb0), (5, db5, Sdb5), (10, db10, Sdb10)):
        out.append(chk("db%d" % layer, "code", gb[layer], db.sum(axis=0), np.abs(db).sum(axis=0), Sc=None if sc is None else sc.sum(axis=0)))
    out.append(chk("dW0[:, latent]", "code", gw[0][:, 63:], db0.T @ su, np.abs(db0).T @ np.abs(su), Sc=Sdb0.T @ np.abs(su)))
    out.append(chk("dW5[:, latent]", "code", gw[5][:, 63:63 + S_], db5.T @ shape, np.abs(db5).T @ np.abs(shape), Sc=Sdb5.T @ np.abs(shape)))
    out.append(chk("dWr1[:, latent]", "code", gw[10][:, 384:], db10.T @ appea, np.abs(db10).T @ np.abs(appea), Sc=Sdb10.T @ np.abs(appea)))
    # background map
    dmb, wsb = dm.reshape(B, n_rays, 256), wsum.reshape(B, n_rays)
    out.append(chk("d_bg_featmap", "colsum", res["d_bg"], ((1.0 - wsb)[..., None] * dmb).sum(axis=0).T, ((1.0 + np.abs(wsb))[..., None] * np.abs(dmb)).sum(axis=0).T,
                   Sc=((1.0 + S_wsum.reshape(B, n_rays))[..., None] * np.abs(dmb)).sum(axis=0).T))
    return out


def evaluate(c, u=None):
    """-> dict(tag, family, n, ratio = largest |got - z64| / S, ambiguous, bad): `bad` counts entries beyond u S (u: the family's
    bound unless given; exact checks: any difference).  Entries with S = 0 must be equal."""
    got, z, S = f64(c["got"]).reshape(-1), c["z"].reshape(-1), np.broadcast_to(c["S"], c["z"].shape).reshape(-1)
    assert got.shape == z.shape, (c["tag"], c["got"].shape, c["z"].shape)
    u = bound(c["family"]) if u is None else u
    if c["exact"]:
        bad = int(np.sum(~((got == z) & np.isfinite(got))))
        return dict(tag=c["tag"], family=c["family"], n=z.size, ratio=0.0, ambiguous=0, bad=bad, exact=True)
    ref = np.maximum(z, 0.0) if c["relu"] else z
    err = np.maximum(np.abs(got - ref) - ABS_SLACK, 0.0)
    err = np.where(np.isfinite(got), err, np.inf)
    ok_alt = np.zeros(z.size, dtype=bool)
    amb = np.zeros(z.size, dtype=bool)
    if c["relu"]:
        amb = np.abs(z) <= u * S
    if c["amb"] is not None:
        amb = amb | c["amb"].reshape(-1)
        ok_alt = c["amb"].reshape(-1) & ((got == 0) | (np.abs(got - z) <= u * S))
    zero = S == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(zero, np.where(err == 0, 0.0, np.inf), err / np.where(zero, 1.0, S))
    ratio = np.where(ok_alt, 0.0, ratio)
    return dict(tag=c["tag"], family=c["family"], n=z.size, ratio=float(ratio.max()) if ratio.size else 0.0, ambiguous=int(amb.sum()),
                bad=int((ratio > u).sum()), exact=False)


def report(prefix, e):
    if e["exact"]:
        print("%-34s entries %9d  exact, differing %d" % (prefix + " " + e["tag"], e["n"], e["bad"]))
    else:
        print("%-34s entries %9d  worst %.3e of S = %.3f of the bound (%s: floor %.1e x %g)  ambiguous %d  beyond %d" %
              (prefix + " " + e["tag"], e["n"], e["ratio"], e["ratio"] / bound(e["family"]), e["family"], FLOOR[e["family"]], FACTOR, e["ambiguous"], e["bad"]))


def failures(inp, rec, prefix="", quiet=False):
    """run every check at the GPU bounds; -> (list of failing tags, {family: worst ratio}, evaluations)"""
    bad, worst, evs = [], {}, []
    for c in stages(inp, rec):
        e = evaluate(c)
        evs.append(e)
        if not quiet:
            report(prefix, e)
        if not e["exact"]:
            worst[e["family"]] = max(worst.get(e["family"], 0.0), e["ratio"])
        if e["bad"] or e["ambiguous"] > AMBIGUOUS_CAP * e["n"]:
            bad.append(e["tag"])
    return bad, worst, evs
