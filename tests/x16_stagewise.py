"""Stage-by-stage float64 restatement of the fused bf16 training path, for the tests that pin it
(test_x16_stagewise_cpu.py, test_gpu_x16_stagewise.py).  A helper module, not a test file: CPU only, numpy / torch.

The path leaves every intermediate in HBM in a documented format (`saved`, the training workspace), so every linear stage can
be recomputed alone from the kernel's own bit-exact inputs ("teacher-forced").  The only thing a float64 recomputation leaves
open is the order of the fp32 accumulation, which matters for an entry only when its exact value lies next to a bf16
rounding boundary.  `check_bf16` is the one comparison rule of every stage test:

    expected = bf16_rne(act(z64));  an entry is AMBIGUOUS when bf16_rne(act(z64 - delta)) != bf16_rne(act(z64 + delta)),
    i.e. z64 is within delta of a rounding boundary (a midpoint of two neighbouring bf16 values, or 0 under a ReLU);
    an ambiguous entry may hold any value of that closed range (its two neighbours), every other entry matches bit for
    bit, and no entry is more than one bf16 ulp from the expected value.
    delta = U * (|b| + sum_k |w_k x_k|), per entry.

Where cancellation makes delta itself wider than the spacing of the result (|z| << sum |w x|, or z within delta of a ReLU's
zero, where the neighbours of 0 are subnormal) the range [bf16(z - delta), bf16(z + delta)] holds more than two values, all of
which a correct fp32 accumulation can produce.  Such WIDE entries are counted apart: the one-ulp rule and the printed "max ulp" are
over all other entries and are never clamped; a wide entry must lie in its range (|stored - z64| <= delta + half a ulp), its
true distance is printed next to the count, and a stage may have at most WIDE_CAP of them (measured on the CPU emulation:
<= 0.23 % of a stage, nearly all of them
next to a ReLU's zero; cap 0.5 %).

U comes from the CPU alone, never from a kernel: the same bf16 x bf16 products summed in float32 in three orders (16-wide
k-steps in sequence with the bias first as its hi + lo bf16 halves, the way the MFMA stream walks them; numpy's pairwise sum;
torch.matmul), against float64, over every forward and dX stage of the five cases below.

    measured floor  max |z32 - z64| / (|b| + sum |w x|)  = 2.91e-7, recorded as U_FLOOR = 3.0e-7 (re-measured by
                    test_x16_stagewise_cpu.py; the pairwise order on 128 points spread over all frames, blocks and lanes)
    U = 4 x U_FLOOR = 1.2e-6                                         (the margin of DESIGN 3.12: "bound 4 x the floor";
                                                                      it covers the MFMA's unspecified internal order)
    ambiguous share under U: at most 5 % of any stage of any case (asserted on the CPU emulation; measured <= 1.3 %)

The rule is written once for both 16-bit map types (`check16`, `ambiguous_share16`, `bits16`, `round16`: "bf16", or "fp16" = IEEE
half with its subnormals); `check_bf16`, `ambiguous_share`, `bf16_bits`, `bf16_round` are the bf16 wrappers.  IEEE half has 8 x finer
spacing under the same U, so its caps are wider (CAPS; used by the 2-D renderer's inference pin, nr_restatement.py).

The weight-gradient products (fp32 sums of exact bf16 x bf16 products over blocks, slices, XCD partials and atomics) are
bounded per entry relative to sum_points |dz| |x| of that entry, one bound per product family (DW_FLOOR), 4 x the largest
error of the fp32-ordered CPU sums.  Per-sample weights: W_FLOOR in the measure of `weight_tolerance`.
"""
import ctypes

import numpy as np
import torch

PIECE = 1024            # x16_core.h: X16_PIECE
XT_TILES = 98           # x16_core.h: X16_XT_TILES (PE 2 + 8 hidden layers x 12)
DZ_TILES = 103          # train_x16.inc: T16_DZ_TILES ([dG 6 | d sigma 1] | dZ0 .. dZ7, 12 each)
GATE_WORDS = 8 * 6 * 64  # train_x16.inc: T16_GATE_WORDS
PART_STRIDE = 192 + 4   # n3dt_device.h: N3DT_PART_STRIDE
FOLD_STRIDE = 384 * 10 + 32 + 192  # n3dt_layout.h: N3DT_FOLD_STRIDE
RAYFOLD_STRIDE = 192
PE_DIM, HID, G = 63, 384, 192
DW_XCDS, DW_PACE_SLOTS, DW_MAX_LAUNCHES = 8, 4096, 10
BWD_PIECES_CAM = 168 + 7 * 288 + 2 * 48  # train_x16.inc: T16_BWD_PIECES_CAM

# ---- the measured units (see the module docstring; test_x16_stagewise_cpu.py re-measures every floor and fails if one moved up)
U_FLOOR = 3.0e-7
U = 4.0 * U_FLOOR
AMBIGUOUS_CAP = 0.05
WIDE_CAP = 5e-3           # share of a stage's entries whose delta exceeds the spacing of the result (see the docstring)
# IEEE half has 8 x finer spacing under the same U: the float64 reference alone (nr_restatement's inference stages, cases (4, 256, 1, 1)
# and (4, 256, 3, 2)) shows ambiguous <= 15.4 % (y of block 0) and wide <= 2.4 % (t1 of block 0)
AMBIGUOUS_CAP_FP16 = 0.25
WIDE_CAP_FP16 = 0.04
CAPS = {"bf16": (AMBIGUOUS_CAP, WIDE_CAP), "fp16": (AMBIGUOUS_CAP_FP16, WIDE_CAP_FP16)}
# weight-gradient families: largest |sum32 - sum64| / sum |dz| |x| of the fp32-ordered CPU sums
DW_FLOOR = {
    "hidden": 4.5e-7,    # dW_1..7 (module 5: its H4 columns), 384 x 384
    "pe": 2.6e-7,        # the PE columns of FeaExt_module_0 and _5
    "rgb": 6.0e-7,       # dW_m [192 x 384] and the density row
    "unmerge": 2.8e-7,   # RGB_layer_0 / RGB_layer_1[:, :384] and their biases: two fp32 products on top of dW_m
    "bias": 1.3e-7,      # row sums of dZ_l (bias gradients, per-frame folded biases)
    "latent": 1.7e-7,    # latent columns of modules 0, 5, RGB_layer_1 and d_shape / d_appea / d_audio, from the per-frame sums
}
# the given-plane case e_hier where its measured floor is above the table's: its own entries, the table stays
DW_FLOOR_GIVEN = {"pe": 2.7e-7, "bias": 1.5e-7, "latent": 1.9e-7}   # measured 2.617e-7, 1.471e-7, 1.830e-7


def dw_floor(name, fam):
    """the weight-gradient floor of family fam in case name"""
    return DW_FLOOR_GIVEN.get(fam, DW_FLOOR[fam]) if CASES[name].get("hier") else DW_FLOOR[fam]


# spread between the two bias routes of the free-running CPU emulation (free_forward, route_spread), cases a - c; the inference
# kernel is held to 4 x this against the training forward
ROUTE_FLOOR = {"weight": 5.0e-4, "fg_feat": 8.0e-4, "bg_alpha": 6.0e-4}   # measured 4.6e-4, 7.1e-4, 5.7e-4 (case a)
W_FLOOR = 0.25           # per-sample weights, in units of weight_tolerance(): 4 x floor <= 1, so that tolerance is the bound


def al256(b):
    return (b + 255) & ~255


def bias_offset(stage):  # n3dt_layout.h: n3dt_bias_offset
    return 384 * stage if stage <= 8 else (384 * 8 + 32 if stage == 9 else 384 * 9 + 32)


def fold_region_floats(batch, n_rays, vd_dim):  # n3dt_layout.h: n3dt_fold_region_floats
    if vd_dim > 0:
        return ((batch * FOLD_STRIDE + 63) & ~63) + batch * n_rays * RAYFOLD_STRIDE
    return batch * FOLD_STRIDE


def n_blocks(B, n_rays, n_samples):
    return B * n_rays * ((n_samples + 31) // 32)


def saved_layout(B, n_rays, n_samples, vd_dim=0):
    """saved16_layout (train_x16.inc:50-64): byte offsets; the `+ 1` records are the dump record dead waves write."""
    nb, R = n_blocks(B, n_rays, n_samples), B * n_rays
    sizes = [("fold", 4 * fold_region_floats(B, n_rays, vd_dim)), ("xT", (nb + 1) * XT_TILES * 2 * PIECE), ("gS", (nb + 1) * 12 * PIECE),
             ("geo", nb * 64 * 4), ("weight", R * n_samples * 4), ("ray", R * PART_STRIDE * 4), ("gates", (nb + 1) * GATE_WORDS * 4),
             ("wm", 4 * 192 * 384)]
    return _offsets(sizes)


def ws_layout(B, n_rays, n_samples):
    """ws16_layout (train_x16.inc:65-87)."""
    nb, R = n_blocks(B, n_rays, n_samples), B * n_rays
    sizes = [("part", nb * PART_STRIDE * 4), ("wlocal", nb * 32 * 4), ("packT", BWD_PIECES_CAM * PIECE), ("dzT", (nb + 1) * DZ_TILES * 2 * PIECE),
             ("dsig", nb * 32 * 4), ("ddist", nb * 32 * 4), ("dpe5", nb * 32 * 64 * 4), ("dpe0", nb * 32 * 64 * 4), ("dfg", R * 256 * 4),
             ("dgray", R * 192 * 4), ("dwsum", R * 4), ("dfold", 4 * B * FOLD_STRIDE), ("rsrgb", 4 * B * 224), ("dwm", 4 * 224 * 384),
             ("dwpart", 4 * DW_MAX_LAUNCHES * DW_XCDS * 384 * 384), ("pace", 4 * DW_MAX_LAUNCHES * DW_PACE_SLOTS)]
    return _offsets(sizes)


def _offsets(sizes):
    out, o = {}, 0
    for name, n in sizes:
        out[name] = o
        o += al256(n)
    out["total"] = o
    return out


def library_totals(geom):
    """n3dt_train16_saved_bytes / n3dt_train16_ws_bytes of the built library (exported, not part of n3dt.h)."""
    from n3dt import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    out = []
    for name in ("n3dt_train16_saved_bytes", "n3dt_train16_ws_bytes"):
        fn = getattr(L, name)
        fn.restype = ctypes.c_size_t
        fn.argtypes = [ctypes.POINTER(_lib.Geom)]
        out.append(int(fn(ctypes.byref(geom))))
    return tuple(out)


def dw_slices(bpf, B, n_products=None, gy=1):
    """Slices per frame of a weight-gradient launch: dw_plan_slices (train_x16.inc:935-944) for a single product (n_products
    None), the `spf` loop of launch_dw_multi (:905-913) for the flat launch.  Returns (spf, blocks per slice)."""
    if n_products is None:
        spf = (256 + B * gy - 1) // (B * gy)
        spf = max(1, min(spf, bpf // 8))
    else:
        spf, best_t = 1, 1e30
        s = 1
        while s <= max(bpf // 8, 1) and n_products * B * s * gy <= 8 * 256:
            rounds = (n_products * B * s * gy + 255) // 256
            t = rounds * (((bpf + s - 1) // s) * 2450.0 + 45000.0)
            if t < best_t * 0.995:
                best_t, spf = t, s
            s += 1
    return spf, (bpf + spf - 1) // spf


# ---------------------------------------------------------------------------------------------
# bf16 <-> float64.  Round to nearest even straight from float64 (no double rounding through float32), which is what
# the kernels' (__bf16)v does to an fp32 value (v_cvt_pk_bf16_f32) and what torch.bfloat16 conversion does.
# ---------------------------------------------------------------------------------------------
FORMATS = {"bf16": (8, -126), "fp16": (11, -14)}   # significant bits (the hidden one included), exponent of the smallest normal number


def round16(z, fmt):
    """float64 -> the nearest value of the 16-bit format (ties to even, subnormals included, overflow to infinity), as float64"""
    p, emin = FORMATS[fmt]
    z = np.asarray(z, dtype=np.float64)
    a = np.abs(z)
    _, e = np.frexp(a)                      # a = m 2^e, m in [0.5, 1)
    e = np.maximum(e, emin + 1)             # below the smallest normal number the spacing stays 2^(emin + 1 - p) (subnormals)
    ulp = np.ldexp(1.0, e - p)
    with np.errstate(over="ignore", invalid="ignore"):
        r = np.rint(a / ulp) * ulp
        if fmt == "fp16":
            r = np.where(r > 65504.0, np.inf, r)
        return np.copysign(r, z)


def bits16(z, fmt):
    with np.errstate(over="ignore"):
        if fmt == "fp16":
            return np.ascontiguousarray(round16(z, fmt).astype(np.float16)).view(np.uint16)
        r = np.ascontiguousarray(round16(z, fmt).astype(np.float32))
    return (r.view(np.uint32) >> 16).astype(np.uint16)


def bits16_to_f64(bits, fmt):
    if fmt == "fp16":
        return np.ascontiguousarray(np.asarray(bits, dtype=np.uint16)).view(np.float16).astype(np.float64)
    b = np.ascontiguousarray(np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16)
    return b.view(np.float32).astype(np.float64)


def bf16_round(z):
    return round16(z, "bf16")


def bf16_bits(z):
    return bits16(z, "bf16")


def bf16_to_f64(bits):
    return bits16_to_f64(bits, "bf16")


def ordinal(bits):
    """16-bit patterns (bf16 or IEEE half: sign and magnitude both) on a line: neighbours differ by 1, -0 = +0 = 0."""
    m = (np.asarray(bits).astype(np.int32)) & 0x7FFF
    return np.where((np.asarray(bits).astype(np.int32) & 0x8000) != 0, -m, m)


def split_hi_lo(b32, fmt="bf16"):
    """X16::bias_frag (x16_core.h:67-69 bf16, :100-102 IEEE half): hi = rne16(b), lo = rne16(b - hi); returned as float64 (hi, lo)."""
    b = np.asarray(b32, dtype=np.float32).astype(np.float64)
    hi = round16(b, fmt)
    lo = round16((b - hi).astype(np.float32).astype(np.float64), fmt)
    return hi, lo


# ---------------------------------------------------------------------------------------------
# decoders / encoders of the saved formats
# ---------------------------------------------------------------------------------------------
_E = np.arange(32)
# tile image (x16_core.h:412-425, x16_image_lane_offset): lane (c, h) writes fragment f_s at byte 64 c + 32 s + 16 h, element j of
# f_s = channel 16 s + 8 (j >> 2) + 4 h + (j & 3): row c holds channels [0-3, 8-11, 4-7, 12-15 | 16-19, 24-27, 20-23, 28-31]
ROW_CH = 16 * (_E >> 4) + 8 * ((_E & 7) >> 2) + 4 * ((_E >> 3) & 1) + (_E & 3)
_HJ = np.arange(16)
FRAG16 = 8 * ((_HJ & 7) >> 2) + 4 * (_HJ >> 3) + (_HJ & 3)   # lane half h, element j (index 8 h + j) -> channel within the k-step
_HB = np.arange(64)
# gate word (nerf_fwd_x16.hip:200-217): bit b of a lane's word = accumulator register b & 15 of tile 2 w + (b >> 4); register r of lane
# half h = row (r & 3) + 8 (r >> 2) + 4 h of the tile (index 32 h + b -> channel within the word's 64)
GATE64 = 32 * ((_HB & 31) >> 4) + (_HB & 3) + 8 * ((_HB & 15) >> 2) + 4 * (_HB >> 5)


def decode_images(raw, n_tiles):
    """raw [..., n_tiles * 1024] 16-bit -> [..., 32 samples, n_tiles * 32 channels]"""
    raw = np.asarray(raw)
    img = raw.reshape(raw.shape[:-1] + (n_tiles, 32, 32))
    out = np.empty_like(img)
    out[..., ROW_CH] = img
    return np.ascontiguousarray(np.moveaxis(out, -3, -2)).reshape(raw.shape[:-1] + (32, n_tiles * 32))


def encode_images(x, n_tiles):
    x = np.asarray(x)
    t = np.moveaxis(x.reshape(x.shape[:-2] + (32, n_tiles, 32)), -2, -3)
    return np.ascontiguousarray(t[..., ROW_CH]).reshape(x.shape[:-2] + (n_tiles * 1024,))


def decode_frags(raw, n_ks):
    """lane-linear fragments: raw [..., n_ks * 512] 16-bit (piece ks, lane 32 h + c, element j) -> [..., 32 samples, n_ks * 16 channels],
    channel 16 ks + 8 (j >> 2) + 4 h + (j & 3) of sample c (train_x16.inc:144-145)"""
    raw = np.asarray(raw)
    f = raw.reshape(raw.shape[:-1] + (n_ks, 2, 32, 8))
    f = np.moveaxis(f, -3, -2).reshape(raw.shape[:-1] + (n_ks, 32, 16))   # [ks, c, 8 h + j]
    out = np.empty_like(f)
    out[..., FRAG16] = f
    return np.ascontiguousarray(np.moveaxis(out, -3, -2)).reshape(raw.shape[:-1] + (32, n_ks * 16))


def encode_frags(x, n_ks):
    x = np.asarray(x)
    t = np.moveaxis(x.reshape(x.shape[:-2] + (32, n_ks, 16)), -2, -3)[..., FRAG16]        # [ks, c, 8 h + j]
    t = np.moveaxis(t.reshape(x.shape[:-2] + (n_ks, 32, 2, 8)), -2, -3)                    # [ks, h, c, j]
    return np.ascontiguousarray(t).reshape(x.shape[:-2] + (n_ks * 512,))


def decode_gates(raw):
    """raw [..., 8 * 6 * 64] uint32 (layer, word, lane) -> bool [..., 8 layers, 32 samples, 384 channels]"""
    raw = np.asarray(raw, dtype=np.uint32)
    w = raw.reshape(raw.shape[:-1] + (8, 6, 2, 32))                                        # [layer, word, h, c]
    bits = ((w[..., None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool)             # [layer, word, h, c, b]
    bits = np.moveaxis(bits, -2, -4)                                                       # [layer, c, word, h, b]
    bits = bits.reshape(raw.shape[:-1] + (8, 32, 6, 64))
    out = np.empty_like(bits)
    out[..., GATE64] = bits
    return out.reshape(raw.shape[:-1] + (8, 32, 384))


def encode_gates(bits):
    bits = np.asarray(bits, dtype=bool)
    t = bits.reshape(bits.shape[:-3] + (8, 32, 6, 64))[..., GATE64]
    t = np.moveaxis(t.reshape(bits.shape[:-3] + (8, 32, 6, 2, 32)), -4, -2)                 # [layer, word, h, c, b]
    w = (t.astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=-1).astype(np.uint32)
    return w.reshape(bits.shape[:-3] + (GATE_WORDS,))


def decode_geo(raw):
    """raw [blocks, 64] fp32 -> (sigma pre-activation [blocks, 32], plane distance [blocks, 32])  (nerf_fwd_x16.hip:393-396)"""
    raw = np.asarray(raw, dtype=np.float32).reshape(-1, 64)
    return raw[:, :32], raw[:, 32:]


class Saved:
    """The live records of `saved` (the dump record is not decoded) as 16-bit patterns / fp32, points flattened block-major:
    point = block * 32 + lane, block = (frame * n_rays + ray) * bpr + sample block."""

    def __init__(self, buf, B, n_rays, n_samples, vd_dim=0):
        buf = np.asarray(buf, dtype=np.uint8)
        L = saved_layout(B, n_rays, n_samples, vd_dim)
        assert buf.size >= L["total"]
        nb = n_blocks(B, n_rays, n_samples)
        self.B, self.n_rays, self.n_samples, self.nb, self.bpr = B, n_rays, n_samples, nb, (n_samples + 31) // 32

        def region(name, nbytes, dtype):
            return buf[L[name]:L[name] + nbytes].view(dtype)
        self.fold = region("fold", 4 * B * FOLD_STRIDE, np.float32).reshape(B, FOLD_STRIDE).copy()
        x = decode_images(region("xT", nb * XT_TILES * 2 * PIECE, np.uint16).reshape(nb, XT_TILES * 1024), XT_TILES)
        self.x_bits = x.reshape(nb * 32, XT_TILES * 32)                 # [point, PE 64 | H0 384 | .. | H7 384]
        self.gs_bits = decode_frags(region("gS", nb * 12 * PIECE, np.uint16).reshape(nb, 12 * 512), 12).reshape(nb * 32, 192)
        sig, dist = decode_geo(region("geo", nb * 64 * 4, np.float32))
        self.sigma_pre, self.dist = sig.reshape(-1).copy(), dist.reshape(-1).copy()
        self.weight = region("weight", B * n_rays * n_samples * 4, np.float32).reshape(B * n_rays, n_samples).copy()
        g = decode_gates(region("gates", nb * GATE_WORDS * 4, np.uint32).reshape(nb, GATE_WORDS))   # [nb, 8, 32, 384]
        self.gates = np.moveaxis(g, 1, 0).reshape(8, nb * 32, 384)
        self.wm = region("wm", 4 * 192 * 384, np.float32).reshape(192, 384).copy()
        self.raw = {k: buf[L[k]:L[k] + n] for k, n in (("xT", nb * XT_TILES * 2 * PIECE), ("gS", nb * 12 * PIECE), ("geo", nb * 256),
                                                         ("gates", nb * GATE_WORDS * 4))}

    def pe_bits(self):
        return self.x_bits[:, :64]

    def h_bits(self, l):
        return self.x_bits[:, 64 + 384 * l:64 + 384 * (l + 1)]

    def frame_of_point(self):
        return np.repeat(np.arange(self.nb) // (self.n_rays * self.bpr), 32)

    def sample_of_point(self):
        return (np.tile(np.arange(32), self.nb) + 32 * np.repeat(np.arange(self.nb) % self.bpr, 32))

    def point_weight(self):
        """per point: the saved weight of its sample, 0 beyond n_samples (nerf_bwd_x16_kernel, train_x16.inc:329)"""
        s = self.sample_of_point()
        ray = np.repeat(np.arange(self.nb) // self.bpr, 32)
        return np.where(s < self.n_samples, self.weight[ray, np.minimum(s, self.n_samples - 1)], np.float32(0))


class Workspace:
    """What the backward leaves in the training workspace: dzT as bit patterns [point, 103 * 32] and the fp32 side tables."""

    def __init__(self, buf, B, n_rays, n_samples):
        buf = np.asarray(buf, dtype=np.uint8)
        L = ws_layout(B, n_rays, n_samples)
        assert buf.size >= L["dwpart"]  # (the per-XCD partial buffers behind it are not read)
        nb, R = n_blocks(B, n_rays, n_samples), B * n_rays

        def region(name, nbytes, dtype):
            return buf[L[name]:L[name] + nbytes].view(dtype)
        z = decode_images(region("dzT", nb * DZ_TILES * 2 * PIECE, np.uint16).reshape(nb, DZ_TILES * 1024), DZ_TILES)
        self.dz_all = z.reshape(nb * 32, DZ_TILES * 32)
        self.dsig = region("dsig", nb * 32 * 4, np.float32).copy()
        self.dgray = region("dgray", R * 192 * 4, np.float32).reshape(R, 192).copy()
        self.dfold = region("dfold", 4 * B * FOLD_STRIDE, np.float32).reshape(B, FOLD_STRIDE).copy()
        self.rsrgb = region("rsrgb", 4 * B * 224, np.float32).reshape(B, 224).copy()
        self.raw_dzT = buf[L["dzT"]:L["dzT"] + nb * DZ_TILES * 2 * PIECE]

    def dg_bits(self):       # [point, 192]
        return self.dz_all[:, :192]

    def dsig_row_bits(self):  # [point, 32]: channel 0 = d sigma, the rest zero
        return self.dz_all[:, 192:224]

    def dz_bits(self, l):
        o = 32 * (7 + 12 * l)
        return self.dz_all[:, o:o + 384]


# ---------------------------------------------------------------------------------------------
# the comparison rule
# ---------------------------------------------------------------------------------------------
def check16(stored_bits, z64, delta, fmt, relu=False, gate=None, act=None):
    """The comparison rule of the module docstring in the 16-bit format `fmt` ("bf16" or "fp16").  gate (bool, or None): entries
    whose gate is closed must be stored as zero.
    act: a monotone activation in place of the ReLU (the 2-D renderer's LeakyReLU, nr_restatement.py); the rule is unchanged.
    Returns dict(n, ambiguous, mismatches, max_ulp, worst): `worst` lists (flat index, stored, expected, z64, delta) of up to eight
    failing entries."""
    z64 = np.asarray(z64, dtype=np.float64)
    delta = np.broadcast_to(np.asarray(delta, dtype=np.float64), z64.shape)
    act = act or ((lambda v: np.maximum(v, 0.0)) if relu else (lambda v: v))
    e, a, b = bits16(act(z64), fmt), bits16(act(z64 - delta), fmt), bits16(act(z64 + delta), fmt)
    if gate is not None:
        closed = ~np.asarray(gate, dtype=bool)
        e, a, b = (np.where(closed, np.uint16(0), v) for v in (e, a, b))
    oe, oa, ob, os_ = ordinal(e), ordinal(a), ordinal(b), ordinal(stored_bits)
    ok = (oa <= os_) & (os_ <= ob)
    amb = oa != ob
    wide = (ob - oa) > 1          # delta is wider than the spacing of the result: more than two values are possible
    dist = np.abs(os_ - oe)       # the true distance, never clamped
    bad = np.flatnonzero(~ok)
    worst = [(int(i), float(bits16_to_f64(np.asarray(stored_bits).reshape(-1)[i:i + 1], fmt)[0]), float(bits16_to_f64(e.reshape(-1)[i:i + 1], fmt)[0]),
              float(z64.reshape(-1)[i]), float(delta.reshape(-1)[i])) for i in bad[:8]]
    narrow = dist[~wide]
    return {"n": int(z64.size), "ambiguous": int(amb.sum()), "mismatches": int(bad.size), "max_ulp": int(narrow.max()) if narrow.size else 0,
            "wide": int(wide.sum()), "max_ulp_wide": int(dist[wide].max()) if wide.any() else 0, "worst": worst}


def check_bf16(stored_bits, z64, delta, relu=False, gate=None, act=None):
    """check16 in bf16: see the module docstring."""
    return check16(stored_bits, z64, delta, "bf16", relu=relu, gate=gate, act=act)


def ambiguous_share16(z64, delta, fmt, relu=False, gate=None, act=None):
    """(share of ambiguous entries, share of wide-delta entries) of a stage"""
    z64 = np.asarray(z64, dtype=np.float64)
    act = act or ((lambda v: np.maximum(v, 0.0)) if relu else (lambda v: v))
    span = ordinal(bits16(act(z64 + delta), fmt)) - ordinal(bits16(act(z64 - delta), fmt))
    if gate is not None:
        span = np.where(np.asarray(gate, dtype=bool), span, 0)
    return float((span != 0).mean()), float((span > 1).mean())


def ambiguous_share(z64, delta, relu=False, gate=None, act=None):
    return ambiguous_share16(z64, delta, "bf16", relu=relu, gate=gate, act=act)


def report(tag, st):
    """The line every stage test prints: entries compared, ambiguous share, mismatches, largest ulp distance."""
    print("%-28s entries %9d  ambiguous %.4f %%  mismatches %d  max ulp %d  (wide-delta entries %d, their largest distance %d)" %
          (tag, st["n"], 100.0 * st["ambiguous"] / max(st["n"], 1), st["mismatches"], st["max_ulp"], st["wide"], st["max_ulp_wide"]))
    for w in st["worst"]:
        print("    entry %d: stored %.9g expected %.9g (z64 %.12g, delta %.3g)" % w)


# ---------------------------------------------------------------------------------------------
# weights as the kernels see them
# ---------------------------------------------------------------------------------------------
class Weights:
    """ws / bs: the 12 fp32 [out, in] matrices and biases in _lib.MLP_ORDER (numpy).  S, U: shape (+ gaze) and audio widths.
    wm: the forward's merged RGB matrix W_m [192, 384] fp32 (saved.wm); every matrix product of the fused path sees bf16(W)
    (nerf_aux.hip:90 for the forward stream, train_x16.inc:135 for the transposed one)."""

    def __init__(self, ws, bs, S, U, wm):
        self.S, self.U = S, U
        self.w32 = [np.asarray(w, dtype=np.float32).reshape(w.shape[0], -1).astype(np.float64) for w in ws]
        self.b32 = [np.asarray(b, dtype=np.float32).astype(np.float64) for b in bs]
        q = [bf16_round(w) for w in self.w32]
        z1 = np.zeros((384, 1))
        self.fwd = []                      # logical forward matrices [384, K], columns in the kernel's k order (n3dt_layout.h:7-16)
        for l in range(8):
            if l == 0:
                self.fwd.append(np.concatenate([q[0][:, :63], z1], axis=1))
            elif l == 5:
                self.fwd.append(np.concatenate([q[5][:, :63], z1, q[5][:, 63 + S:63 + S + 384]], axis=1))
            else:
                self.fwd.append(q[l])
        self.den = q[8].reshape(384)
        self.wm = bf16_round(np.asarray(wm, dtype=np.float32).astype(np.float64))
        # transposed stream of the dX chain (train16_pack_bwd_kernel, train_x16.inc:99-138): stage l consumes dZ_{l+1}
        self.bwd = {7: np.concatenate([self.wm, self.den[None, :]], axis=0)}                # [193, 384]: [W_m ; w_density]
        for l in range(6, -1, -1):
            self.bwd[l] = q[5][:, 63 + S:63 + S + 384] if l == 4 else q[l + 1]                # [k = rows of layer l + 1, 384]


def bias_rows(fold, frame_of_point, stage, n):
    """fp32 folded bias of every point's frame, [points, n]"""
    return fold[:, bias_offset(stage):bias_offset(stage) + n][frame_of_point]


def forward_input(x_bits, l):
    """X_l of hidden layer l in the kernel's k order: PE for layer 0, [PE, H4] for layer 5 (nerf_fwd_x16.hip:173-178, 375-385)"""
    if l == 0:
        return bf16_to_f64(x_bits[:, :64])
    h = bf16_to_f64(x_bits[:, 64 + 384 * (l - 1):64 + 384 * l])
    return np.concatenate([bf16_to_f64(x_bits[:, :64]), h], axis=1) if l == 5 else h


def linear64(X, Wq, b32=None):
    """z = X Wq^T (+ bias) in float64 and the magnitude |b| + sum |w x| the tolerance scales with.  The training forward feeds
    the bias as hi + lo bf16 halves through one MFMA (nerf_fwd_x16.hip:152-163; density: X16_BIAS_GLOBAL_MFMA, :348), so the
    exact bias of the product is hi + lo, not b."""
    z, mag = X @ Wq.T, np.abs(X) @ np.abs(Wq).T
    if b32 is not None:
        hi, lo = split_hi_lo(b32)
        z, mag = z + (hi + lo), mag + np.abs(np.asarray(b32, dtype=np.float64))
    return z, mag


def hidden_stage64(saved, W, l):
    """H_l = relu(bf16(b_l' + W_l X_l)) -- rounded at the pack, ReLU on the packed value, which commutes
    (nerf_fwd_x16.hip:134-140, x16_core.h:35-43)."""
    return linear64(forward_input(saved.x_bits, l), W.fwd[l], bias_rows(saved.fold, saved.frame_of_point(), l, 384))


def density_stage64(saved, W):
    """sigma pre-activation, kept in fp32 (nerf_fwd_x16.hip:220-221, 388-396): row 0 of the density tile on H7"""
    b = bias_rows(saved.fold, saved.frame_of_point(), 8, 1)
    z, mag = linear64(bf16_to_f64(saved.h_bits(7)), W.den[None, :], b)
    return z[:, 0], mag[:, 0]


def rgb_stage64(saved, W):
    """gS = bf16(relu(b_m' + W_m H7)): ReLU in fp32, rounded where it is stored (nerf_fwd_x16.hip:226-233)"""
    return linear64(bf16_to_f64(saved.h_bits(7)), W.wm, bias_rows(saved.fold, saved.frame_of_point(), 10, 192))


def dg_stage64(w32, dgray32_of_point):
    """dG[ch][s] = w_s dGray[ch] as the rank-1 MFMA forms it from hi / lo halves: d_hi w_hi + d_lo w_hi + d_hi w_lo
    (train_x16.inc:337-364); masked by gS != 0 at the pack (:371-372)."""
    w_hi, w_lo = split_hi_lo(w32)
    d_hi, d_lo = split_hi_lo(dgray32_of_point)
    t = [d_hi * w_hi[:, None], d_lo * w_hi[:, None], d_hi * w_lo[:, None]]
    return t[0] + t[1] + t[2], np.abs(t[0]) + np.abs(t[1]) + np.abs(t[2])


def dx_stage64(dz_next, W, l):
    """dZ_l = (W_{l+1}^T dZ_{l+1}) gated by H_l != 0 (x16_bwd_stage, train_x16.inc:247-264); l = 7 takes [dG | d sigma] through
    [W_m ; w_density]^T, l = 4 the H4 columns of FeaExt_module_5 (:391-399).  dz_next: float64 [points, 193 or 384]."""
    Wt = W.bwd[l]
    return dz_next @ Wt, np.abs(dz_next) @ np.abs(Wt)


def dx_input(ws, l):
    if l == 7:
        return np.concatenate([bf16_to_f64(ws.dg_bits()), bf16_to_f64(ws.dsig_row_bits()[:, :1])], axis=1)
    return bf16_to_f64(ws.dz_bits(l + 1))


def composite64(sigma_pre, dist, n_rays_total, bpr, n_samples):
    """per-sample weights of whole rays in float64 (reference NetWorks/utils.py:273-289): alpha = 1 - exp(-relu(sigma) dist),
    w = alpha prod_{t<s} (1 - alpha_t + 1e-10).  Inputs per point (block-major); returns (w, T) [rays, n_samples]."""
    s = np.asarray(sigma_pre, dtype=np.float64).reshape(n_rays_total, bpr * 32)[:, :n_samples]
    d = np.asarray(dist, dtype=np.float64).reshape(n_rays_total, bpr * 32)[:, :n_samples]
    alpha = 1.0 - np.exp(-np.maximum(s, 0.0) * d)
    x = 1.0 - alpha + 1e-10
    T = np.concatenate([np.ones((n_rays_total, 1)), np.cumprod(x, axis=1)[:, :-1]], axis=1)
    return alpha * T, T


def composite32(sigma_pre, dist, n_rays_total, bpr, n_samples):
    """the same in float32, sequential products (the CPU emulation the weight floor comes from)"""
    s = np.asarray(sigma_pre, dtype=np.float32).reshape(n_rays_total, bpr * 32)[:, :n_samples]
    d = np.asarray(dist, dtype=np.float32).reshape(n_rays_total, bpr * 32)[:, :n_samples]
    alpha = np.float32(1) - np.exp(-np.maximum(s, np.float32(0)) * d).astype(np.float32)
    x = np.float32(1) - alpha + np.float32(1e-10)
    T = np.ones((n_rays_total, n_samples), dtype=np.float32)
    for i in range(1, n_samples):
        T[:, i] = T[:, i - 1] * x[:, i - 1]
    return alpha * T


def weight_tolerance(w64, T64=None):
    """|w - w64| allowed at W_FLOOR = 1: relative 1e-5 of the weight (fp32 expf and the scan) plus absolute 2^-21 (the weights
    of a ray are fractions of 1).  The absolute term is what fp32 itself needs: alpha = 1 - e and x = e + 1e-10 are rounded at
    the scale of 1, so behind a nearly saturated sample (e ~ 1e-7) the transmittance -- and every later weight of the ray, all
    below 1e-7 -- carries a relative error of several per cent in the float32 CPU emulation too (case d_contrast)."""
    return 1e-5 * w64 + 2.0 ** -21


# ---------------------------------------------------------------------------------------------
# weight and bias gradients from decoded tiles, float64
# ---------------------------------------------------------------------------------------------
def grads64(saved, ws, W, codes, matmul=None, cast=np.float64, post=np.float64):
    """Every MLP gradient of the fused backward as float64 products of the decoded tiles, with the magnitude
    sum_points |dz| |x| each entry's bound scales with.  codes = (shape [B,S], appea [B,A], audio [B,U] or None), fp32.
    Returns {name: (value, magnitude, family)}; names: "w0".."w10", "b0".."b10" in _lib.MLP_ORDER numbering, "d_shape",
    "d_appea", "d_audio".  The un-merge follows train_x16.inc:15-16 and :1290-1298, the latent columns train_mlp.hip:532-575.
    `matmul` / `cast` / `post`: the fp32-ordered emulations of the CPU test substitute their own product over the points, its
    element type, and the element type of the small products behind it (un-merge, folding adjoint)."""
    mm = matmul or (lambda a, b: a.T @ b)
    pm = lambda a, b: (np.asarray(a).astype(post) @ np.asarray(b).astype(post)).astype(np.float64)  # noqa: E731
    f = lambda bits: bf16_to_f64(bits).astype(cast)  # noqa: E731
    S, U = W.S, W.U
    shape, appea, audio = (None if c is None else np.asarray(c, dtype=np.float32).astype(np.float64) for c in codes)
    B = saved.B
    frame = saved.frame_of_point()
    onehot = (frame[:, None] == np.arange(B)[None, :]).astype(cast)                          # [points, B]
    out = {}
    dz = {l: f(ws.dz_bits(l)) for l in range(8)}
    pe = f(saved.pe_bits())[:, :63]

    def prod(a, b):
        return np.asarray(mm(a, b), dtype=np.float64), np.abs(a.astype(np.float64)).T @ np.abs(b.astype(np.float64))
    # hidden products and PE columns (train_x16.inc:1270-1287)
    for l in range(1, 8):
        x = f(saved.h_bits(4 if l == 5 else l - 1))
        out["w%d_h" % l] = prod(dz[l], x) + ("hidden",)
    out["w0_pe"] = prod(dz[0], pe) + ("pe",)
    out["w5_pe"] = prod(dz[5], pe) + ("pe",)
    # per-frame row sums (bias gradients ride on the weight-gradient kernels: dw_x16_body's rowsum)
    rs = {l: prod(dz[l], onehot) for l in range(8)}                                           # [384, B]
    dgs = np.concatenate([f(ws.dg_bits()), f(ws.dsig_row_bits()[:, :1])], axis=1)            # [points, 193]
    rs_m = prod(dgs, onehot)                                                                  # [193, B]
    for l in range(8):     # per frame: what the weight-gradient kernels leave in dfold (bias_offset(l)), rs_rgb for the merged RGB rows
        out["rs%d" % l] = (rs[l][0].T, rs[l][1].T, "bias")                                    # [B, 384]
    out["rs_m"] = (rs_m[0].T, rs_m[1].T, "bias")                                              # [B, 193]: db_m | d b_density
    for l in (1, 2, 3, 4, 6, 7):
        out["b%d" % l] = (rs[l][0].sum(axis=1), rs[l][1].sum(axis=1), "bias")
    for l in (0, 5):
        out["b%d" % l] = (rs[l][0].sum(axis=1), rs[l][1].sum(axis=1), "bias")
    out["b8"] = (rs_m[0][192:193].sum(axis=1), rs_m[1][192:193].sum(axis=1), "bias")
    out["b10"] = (rs_m[0][:192].sum(axis=1), rs_m[1][:192].sum(axis=1), "bias")
    # merged RGB product and its un-merge
    h7 = f(saved.h_bits(7))
    dwm, dwm_mag = prod(dgs, h7)                                                              # [193, 384]
    out["w8"] = (dwm[192:193], dwm_mag[192:193], "rgb")
    out["dwm"] = (dwm[:192], dwm_mag[:192], "rgb")
    wr0, br0, wr1 = W.w32[9], W.b32[9], W.w32[10]
    wr1a = wr1[:, :384]
    dbm, dbm_mag = out["b10"][0], out["b10"][1]
    out["w10_a"] = (pm(dwm[:192], wr0.T) + pm(dbm[:, None], br0[None, :]), dwm_mag[:192] @ np.abs(wr0).T + np.outer(dbm_mag, np.abs(br0)), "unmerge")
    out["w9"] = (pm(wr1a.T, dwm[:192]), np.abs(wr1a).T @ dwm_mag[:192], "unmerge")
    out["b9"] = (pm(wr1a.T, dbm), np.abs(wr1a).T @ dbm_mag, "unmerge")
    # latent columns and code gradients (folding adjoint)
    su = shape if audio is None or U == 0 else np.concatenate([shape, audio], axis=1)          # [B, S + U]
    out["w0_lat"] = (pm(rs[0][0], su), rs[0][1] @ np.abs(su), "latent")
    out["w5_lat"] = (pm(rs[5][0], shape), rs[5][1] @ np.abs(shape), "latent")
    out["w10_lat"] = (pm(rs_m[0][:192], appea), rs_m[1][:192] @ np.abs(appea), "latent")
    w0l, w5l, w10l = W.w32[0][:, 63:], W.w32[5][:, 63:63 + S], wr1[:, 384:]
    d_su = (pm(rs[0][0].T, w0l), rs[0][1].T @ np.abs(w0l))                                       # [B, S + U]
    d5 = (pm(rs[5][0].T, w5l), rs[5][1].T @ np.abs(w5l))
    out["d_shape"] = (d_su[0][:, :S] + d5[0], d_su[1][:, :S] + d5[1], "latent")
    if U > 0:
        out["d_audio"] = (d_su[0][:, S:], d_su[1][:, S:], "latent")
    out["d_appea"] = (pm(rs_m[0][:192].T, w10l), rs_m[1][:192].T @ np.abs(w10l), "latent")
    return out


def assemble_grads(g, S):
    """{"w0".."w10", "b0".."b10"}: the library's `grads` tensors from the pieces of grads64 (value, magnitude, family per column block)"""
    cat = lambda parts, i: np.concatenate([p[i] for p in parts], axis=1)  # noqa: E731
    out = {}
    for l in range(8):
        if l == 0:
            parts = [g["w0_pe"], g["w0_lat"]]
        elif l == 5:
            parts = [g["w5_pe"], g["w5_lat"], g["w5_h"]]
        else:
            parts = [g["w%d_h" % l]]
        fam = np.concatenate([np.full(p[0].shape[1], i) for i, p in enumerate(parts)])
        out["w%d" % l] = (cat(parts, 0), cat(parts, 1), [p[2] for p in parts], fam)
    parts = [g["w10_a"], g["w10_lat"]]
    out["w10"] = (cat(parts, 0), cat(parts, 1), [p[2] for p in parts], np.concatenate([np.full(p[0].shape[1], i) for i, p in enumerate(parts)]))
    for k in ("w8", "w9"):
        out[k] = (g[k][0], g[k][1], [g[k][2]], np.zeros(g[k][0].shape[1], dtype=int))
    for k in ["b%d" % l for l in range(11)]:
        out[k] = (g[k][0][None, :], g[k][1][None, :], [g[k][2]], np.zeros(g[k][0].shape[0], dtype=int))
    return out


UNDERFLOW_TERMS = 385  # the longest small product behind a sum over the points: 384 columns of dW_m and the bias term (un-merge)


def grad_error(got, value, mag, n_points=0):
    """largest per-entry |got - value| / sum |dz| |x| (entries with a zero magnitude must be exactly zero).  n_points: the terms of
    a sum -- the points, times UNDERFLOW_TERMS for the products behind them; each may lose up to the smallest normal fp32
    number, 2^-126, to underflow (case d_contrast: weights of 1e-30 behind a saturated sample give products of 1e-40), which no
    relative bound covers and which is taken off the error first (1e-32 at most: nothing next to any gradient that matters)."""
    got, value, mag = (np.asarray(a, dtype=np.float64) for a in (got, value, mag))
    err = np.maximum(np.abs(got - value) - n_points * 2.0 ** -126, 0.0)
    zero = mag == 0
    assert not np.any(err[zero] != 0), "an entry no point contributes to is not zero"
    return float((err[~zero] / mag[~zero]).max()) if (~zero).any() else 0.0


# ---------------------------------------------------------------------------------------------
# float32-ordered emulations (the floors) and the free-running CPU emulation of a case
# ---------------------------------------------------------------------------------------------
def lin32_seq16(X, Wq, b32=None, exact_bias=False):
    """16-wide k-steps in sequence, as the MFMA stream walks them; the bias first: as hi + lo (the training forward's extra MFMA)
    or, exact_bias, as the fp32 value itself (the inference kernel's C operand, nerf_fwd_x16.hip:147-150)"""
    Xf, Wf = X.astype(np.float32), Wq.astype(np.float32)
    acc = np.zeros((X.shape[0], Wq.shape[0]), dtype=np.float32)
    if b32 is not None and exact_bias:
        acc = acc + np.asarray(b32, dtype=np.float32)
    elif b32 is not None:
        hi, lo = split_hi_lo(b32)
        acc = acc + (hi.astype(np.float32) + lo.astype(np.float32))
    for k0 in range(0, X.shape[1], 16):
        acc = acc + Xf[:, k0:k0 + 16] @ Wf[:, k0:k0 + 16].T
    return acc


def pairwise_rows(n, rows=128):
    """the points lin32_pairwise evaluates: `rows` of them spread evenly over all frames, blocks and lanes (an odd stride walks
    through every lane of the 32-sample blocks, the partial ones included)"""
    step = max(1, n // rows) | 1
    return np.arange(0, n, step)[:rows]


def lin32_pairwise(X, Wq, b32=None, rows=128):
    """numpy's pairwise sum over the products of each entry, on pairwise_rows() of the points (the product tensor is rows x N x K)"""
    sel = pairwise_rows(X.shape[0], rows)
    Xf, Wf = X[sel].astype(np.float32), Wq.astype(np.float32)
    acc = np.empty((Xf.shape[0], Wf.shape[0]), dtype=np.float32)
    for i in range(0, Xf.shape[0], 32):
        acc[i:i + 32] = (Xf[i:i + 32, None, :] * Wf[None, :, :]).sum(axis=-1, dtype=np.float32)
    if b32 is not None:
        hi, lo = split_hi_lo(np.asarray(b32)[sel])
        acc = acc + (hi + lo).astype(np.float32)   # (the bias every order sums is the stream's hi + lo, exact in fp32)
    return acc


def lin32_torch(X, Wq, b32=None):
    acc = torch.matmul(torch.from_numpy(X.astype(np.float32)), torch.from_numpy(np.ascontiguousarray(Wq.astype(np.float32).T))).numpy()
    if b32 is not None:
        hi, lo = split_hi_lo(b32)
        acc = acc + (hi + lo).astype(np.float32)
    return acc


LIN32 = (("seq16", lin32_seq16), ("pairwise", lin32_pairwise), ("torch", lin32_torch))


def dw32_seq(per):
    """a.T @ b in float32, 16 points at a time in sequence inside slices of `per` blocks (dw_x16_body: two k-steps per block,
    blocks of a slice in order), the slices then added in order"""
    def mm(a, b):
        a, b = a.astype(np.float32), b.astype(np.float32)
        total = np.zeros((a.shape[1], b.shape[1]), dtype=np.float32)
        for s0 in range(0, a.shape[0], per * 32):
            acc = np.zeros_like(total)
            for k0 in range(s0, min(s0 + per * 32, a.shape[0]), 16):
                acc = acc + a[k0:k0 + 16].T @ b[k0:k0 + 16]
            total = total + acc
        return total
    return mm


def dw32_numpy(a, b):
    return a.astype(np.float32).T @ b.astype(np.float32)


def dw32_torch(a, b):
    return torch.matmul(torch.from_numpy(np.ascontiguousarray(a.astype(np.float32).T)), torch.from_numpy(np.ascontiguousarray(b.astype(np.float32)))).numpy()


CASES = {
    # B, rays, samples                                 (test_gpu_x16_stagewise.py says what each exercises)
    "a": dict(B=2, n_rays=16, n_samples=24, weights="seed0", kw={}),
    "b": dict(B=1, n_rays=9, n_samples=40, weights="seed0", kw={}),
    "c": dict(B=2, n_rays=25, n_samples=40, weights="seed0", kw={}),
    "d_contrast": dict(B=2, n_rays=16, n_samples=24, weights="contrast", kw={}),
    "d_gaze": dict(B=2, n_rays=16, n_samples=24, weights="seed0", kw={"include_gaze": True, "eye_gaze_dim": 64, "audio_dim": 0}),
    # the hierarchical pass: z_planes_given = 1; case_inputs returns the 16 + 24 + 1 planes (hier_stagewise.given_planes) where t_rand goes
    "e_hier": dict(B=2, n_rays=16, n_samples=40, weights="seed0", kw={}, hier=(16, 24)),
}
FEATMAP_SIZE = 8  # the rays of a case are taken from an 8 x 8 grid


def case_options():
    from n3dt import BaseOptions
    return BaseOptions({"featmap_size": FEATMAP_SIZE, "featmap_nc": 256, "pred_img_size": 4 * FEATMAP_SIZE, "num_sample_coarse": 32})


def case_rays(n_rays):
    """n_rays of the 64 grid rays, spread over the image"""
    return np.unique(np.round(np.linspace(0, FEATMAP_SIZE * FEATMAP_SIZE - 1, n_rays)).astype(np.int64))


def case_inputs(name):
    """(opt, state dict, frame inputs restricted to the case's rays, t_rand, d_merge): everything seeded, CPU tensors"""
    from n3dt import synthetic as syn
    c = CASES[name]
    opt = case_options()
    sd = syn.contrast_state_dict(opt, seed=0) if c["weights"] == "contrast" else syn.make_state_dict(opt, seed=0, bg_noise=0.1, **c["kw"])
    inp = syn.frame_inputs(opt, c["B"], **c["kw"])
    rays = torch.from_numpy(case_rays(c["n_rays"]))
    assert len(rays) == c["n_rays"]
    inp = dict(inp)
    inp["batch_xy"] = inp["batch_xy"][:, :, rays].contiguous()
    t_rand = syn.stratified_noise(c["B"], c["n_rays"], c["n_samples"], 7)
    if c.get("hier"):   # given planes [B, rays, samples + 1]: the kernels take them through the t_rand argument
        import hier_stagewise as hh
        t_rand = torch.from_numpy(hh.given_planes(inp["batch_Tvecs"].numpy().reshape(c["B"], 3)[:, 2], c["n_rays"], c["hier"][0], c["hier"][1], 0,
                                                  opt.world_z1, opt.world_z2))
        assert tuple(t_rand.shape) == (c["B"], c["n_rays"], c["n_samples"] + 1)
    d_merge = torch.randn(c["B"], c["n_rays"], 256, generator=torch.Generator().manual_seed(9))
    return opt, sd, inp, rays, t_rand, d_merge


def mlp_arrays(sd, prefix="fg_CD_predictor."):
    from n3dt import _lib
    ws = [sd[prefix + n + ".weight"].reshape(sd[prefix + n + ".weight"].shape[0], -1).numpy() for n in _lib.MLP_ORDER]
    bs = [sd[prefix + n + ".bias"].numpy() for n in _lib.MLP_ORDER]
    return ws, bs


def sample_points64(xy, R, T, Kinv, n_samples, z1, z2, t_rand, given=False):
    """GenSamplePoints in float64 (n3dt_device.h:33-106): points [B, rays, samples, 3], plane distances [B, rays, samples].
    given (z_planes_given, n3dt_device.h:90-93): t_rand holds the samples + 1 planes of every ray themselves"""
    xy, R, T, Kinv, t_rand = (np.asarray(a, dtype=np.float64) for a in (xy, R, T, Kinv, t_rand))
    B, _, n_rays = xy.shape
    h = np.concatenate([xy, np.ones((B, 1, n_rays))], axis=1)
    w = np.einsum("bij,bjk,bkr->bir", R, Kinv, h)
    d = w / np.linalg.norm(w, axis=1, keepdims=True)                      # [B, 3, rays]
    l = -1.0 / d[:, 2]
    T = T.reshape(B, 3)
    t = np.linspace(0.0, 1.0, n_samples + 1)
    zv = (T[:, 2:3] - z1) * (1.0 - t)[None] + (T[:, 2:3] - z2) * t[None]   # [B, edges]
    mid = 0.5 * (zv[:, 1:] + zv[:, :-1])
    lower = np.concatenate([zv[:, :1], mid], axis=1)
    upper = np.concatenate([mid, zv[:, -1:]], axis=1)
    z = t_rand if given else lower[:, None, :] + (upper - lower)[:, None, :] * t_rand           # [B, rays, edges]
    dist = (z[..., 1:] - z[..., :-1]) * l[..., None]
    pts = T[:, None, None, :] + (np.moveaxis(d, 1, 2) * l[..., None])[:, :, None, :] * z[..., :-1, None]
    return pts, dist


def embed64(pts):
    """Embedder (n3dt_device.h:108-118): [..., 3] -> [..., 64], channel 63 zero"""
    feats = [pts]
    for k in range(10):
        feats += [np.sin(pts * 2.0 ** k), np.cos(pts * 2.0 ** k)]
    return np.concatenate(feats + [np.zeros(pts.shape[:-1] + (1,))], axis=-1)


class Emulation:
    """Free-running CPU emulation of a case in the saved formats: the forward stores bf16(seq16 fp32 sums), the backward
    likewise, so that `Saved` / `Workspace`-shaped data of realistic values exists without a GPU.  Built through the encoders
    and read back through the decoders."""

    def __init__(self, name):
        c = CASES[name]
        opt, sd, inp, rays, t_rand, d_merge = case_inputs(name)
        B, n_rays, Ns = c["B"], c["n_rays"], c["n_samples"]
        bpr = (Ns + 31) // 32
        nb = n_blocks(B, n_rays, Ns)
        ws_, bs_ = mlp_arrays(sd)
        shape, appea = inp["shape_code"].numpy(), inp["appea_code"].numpy()
        audio = inp["audiostyle"].numpy() if inp["audiostyle"].shape[1] > 0 else None
        S, U, A = shape.shape[1], 0 if audio is None else audio.shape[1], appea.shape[1]
        self.codes, self.ws_, self.bs_, self.S, self.U = (shape, appea, audio), ws_, bs_, S, U
        w64 = [w.astype(np.float64) for w in ws_]
        b64 = [b.astype(np.float64) for b in bs_]
        wm = (w64[10][:, :384] @ w64[9]).astype(np.float32)
        self.W = Weights(ws_, bs_, S, U, wm)
        # folded biases (fold_latents_kernel, nerf_aux.hip:196-259), fp32 table
        fold = np.zeros((B, FOLD_STRIDE), dtype=np.float32)
        su = shape if audio is None else np.concatenate([shape, audio], axis=1)
        for l in range(8):
            fold[:, bias_offset(l):bias_offset(l) + 384] = b64[l]
        fold[:, 0:384] += (su @ w64[0][:, 63:].T).astype(np.float32)
        fold[:, bias_offset(5):bias_offset(5) + 384] += (shape @ w64[5][:, 63:63 + S].T).astype(np.float32)
        fold[:, bias_offset(8)] = b64[8][0]
        fold[:, bias_offset(10):bias_offset(10) + 192] = (b64[10] + w64[10][:, :384] @ b64[9] + appea @ w64[10][:, 384:].T).astype(np.float32)
        # sample points of padded blocks: lanes beyond n_samples carry the point 0 and dist 0 (n3dt_device.h:101-105)
        pts, dist = sample_points64(inp["batch_xy"].numpy(), inp["batch_Rmats"].numpy(), inp["batch_Tvecs"].numpy(), inp["batch_inv_inmats"].numpy(),
                                    Ns, opt.world_z1, opt.world_z2, t_rand.numpy(), given=bool(c.get("hier")))
        P = np.zeros((B, n_rays, bpr * 32, 3))
        P[:, :, :Ns] = pts
        D = np.zeros((B, n_rays, bpr * 32), dtype=np.float32)
        D[:, :, :Ns] = dist
        x_bits = np.zeros((nb * 32, XT_TILES * 32), dtype=np.uint16)
        x_bits[:, :64] = bf16_bits(embed64(P.reshape(-1, 3)))
        frame = np.repeat(np.arange(nb) // (n_rays * bpr), 32)
        for l in range(8):
            z32 = lin32_seq16(forward_input(x_bits, l), self.W.fwd[l], fold[frame, bias_offset(l):bias_offset(l) + 384])
            x_bits[:, 64 + 384 * l:64 + 384 * (l + 1)] = bf16_bits(np.maximum(z32.astype(np.float64), 0.0))
        h7 = bf16_to_f64(x_bits[:, 64 + 384 * 7:])
        sig = lin32_seq16(h7, self.W.den[None, :], fold[frame, bias_offset(8):bias_offset(8) + 1])[:, 0]
        gs = bf16_bits(np.maximum(lin32_seq16(h7, self.W.wm, fold[frame, bias_offset(10):bias_offset(10) + 192]).astype(np.float64), 0.0))
        wgt, _ = composite64(sig, D.reshape(-1), B * n_rays, bpr, Ns)
        gates = np.stack([x_bits[:, 64 + 384 * l:64 + 384 * (l + 1)] != 0 for l in range(8)])            # [8, points, 384]
        # the saved buffer, through the encoders
        L = saved_layout(B, n_rays, Ns)
        buf = np.zeros(L["total"], dtype=np.uint8)

        def put(name_, arr):
            raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
            buf[L[name_]:L[name_] + raw.size] = raw
        put("fold", fold)
        put("xT", encode_images(x_bits.reshape(nb, 32, XT_TILES * 32), XT_TILES))
        put("gS", encode_frags(gs.reshape(nb, 32, 192), 12))
        put("geo", np.concatenate([sig.reshape(nb, 32).astype(np.float32), D.reshape(nb, 32)], axis=1))
        put("weight", wgt.astype(np.float32))
        put("gates", encode_gates(np.moveaxis(gates.reshape(8, nb, 32, 384), 0, 1)))
        put("wm", wm)
        self.saved = Saved(buf, B, n_rays, Ns)
        assert np.array_equal(self.saved.x_bits, x_bits) and np.array_equal(self.saved.gs_bits, gs) and np.array_equal(self.saved.gates, gates)
        # ---- backward: d Gray of the ray head on a seeded d_merge, d sigma by float64 autograd through the compositing
        dgray = (d_merge.numpy().reshape(B * n_rays, 256).astype(np.float64) @ w64[11]).astype(np.float32)   # [rays, 192]
        s_t = torch.tensor(sig.reshape(B * n_rays, bpr * 32)[:, :Ns].astype(np.float64), requires_grad=True)
        d_t = torch.tensor(D.reshape(B * n_rays, bpr * 32)[:, :Ns].astype(np.float64))
        al = 1.0 - torch.exp(-torch.relu(s_t) * d_t)
        xx = 1.0 - al + 1e-10
        Tt = torch.cat([torch.ones(B * n_rays, 1, dtype=torch.float64), torch.cumprod(xx, dim=1)[:, :-1]], dim=1)
        g_act = torch.from_numpy(bf16_to_f64(gs).reshape(B * n_rays, bpr * 32, 192)[:, :Ns])
        ((al * Tt).unsqueeze(-1) * g_act * torch.from_numpy(dgray.astype(np.float64)).unsqueeze(1)).sum().backward()
        dsig = np.zeros((B * n_rays, bpr * 32), dtype=np.float32)
        dsig[:, :Ns] = s_t.grad.numpy()
        pw = self.saved.point_weight()
        ray_of_point = np.repeat(np.arange(nb) // bpr, 32)
        zg, _ = dg_stage64(pw, dgray[ray_of_point])
        dz_all = np.zeros((nb * 32, DZ_TILES * 32), dtype=np.uint16)
        dz_all[:, :192] = np.where(gs != 0, bf16_bits(zg), np.uint16(0))
        dz_all[:, 192] = bf16_bits(dsig.reshape(-1).astype(np.float64))
        nxt = np.concatenate([bf16_to_f64(dz_all[:, :192]), bf16_to_f64(dz_all[:, 192:193])], axis=1)
        for l in range(7, -1, -1):
            z32 = lin32_seq16(nxt, self.W.bwd[l].T)
            bits = np.where(gates[l], bf16_bits(z32.astype(np.float64)), np.uint16(0))
            dz_all[:, 32 * (7 + 12 * l):32 * (7 + 12 * l) + 384] = bits
            nxt = bf16_to_f64(bits)
        Lw = ws_layout(B, n_rays, Ns)
        wbuf = np.zeros(Lw["total"], dtype=np.uint8)
        raw = encode_images(dz_all.reshape(nb, 32, DZ_TILES * 32), DZ_TILES).view(np.uint8).reshape(-1)
        wbuf[Lw["dzT"]:Lw["dzT"] + raw.size] = raw
        for name_, arr in (("dsig", dsig), ("dgray", dgray)):
            r = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
            wbuf[Lw[name_]:Lw[name_] + r.size] = r
        self.ws = Workspace(wbuf, B, n_rays, Ns)
        assert np.array_equal(self.ws.dz_all, dz_all)


def free_forward(saved, W, w2, b2, exact_bias):
    """Free-running fp32 emulation of the fused forward from the decoded PE tiles to what the ray head returns: per-sample weights
    [rays, n_samples], fg_feat [rays, 256] = W2 sum_s w_s g_s + b2 sum_s w_s, bg_alpha [rays] = 1 - sum_s w_s.  exact_bias picks the
    bias route (lin32_seq16): the only difference between nerf_fwd_x16_kernel<bf16> and the training forward."""
    frame = saved.frame_of_point()
    pe = bf16_to_f64(saved.pe_bits())
    h = None
    for l in range(8):
        X = pe if l == 0 else (np.concatenate([pe, h], axis=1) if l == 5 else h)
        z = lin32_seq16(X, W.fwd[l], bias_rows(saved.fold, frame, l, 384), exact_bias)
        h = bf16_to_f64(bf16_bits(np.maximum(z.astype(np.float64), 0.0)))
    sig = lin32_seq16(h, W.den[None, :], bias_rows(saved.fold, frame, 8, 1), exact_bias)[:, 0]
    g = np.maximum(lin32_seq16(h, W.wm, bias_rows(saved.fold, frame, 10, 192), exact_bias), np.float32(0))
    R, Ns = saved.nb // saved.bpr, saved.n_samples
    w = composite32(sig, saved.dist, R, saved.bpr, Ns)
    g = g.reshape(R, saved.bpr * 32, 192)[:, :Ns]
    gray = np.einsum("rs,rsc->rc", w, g).astype(np.float32)
    wsum = w.sum(axis=1, dtype=np.float32)
    fg = gray @ np.asarray(w2, dtype=np.float32).T + np.asarray(b2, dtype=np.float32)[None, :] * wsum[:, None]
    return {"weight": w, "fg_feat": fg.astype(np.float32), "bg_alpha": np.float32(1) - wsum}


def route_spread(a, b):
    """the measure of the bias-route comparison, per quantity: largest |a - b|, weights and bg_alpha absolute (fractions of 1),
    fg_feat relative to the largest |fg_feat|"""
    out = {}
    for k in ("weight", "fg_feat", "bg_alpha"):
        x, y = np.asarray(a[k], dtype=np.float64), np.asarray(b[k], dtype=np.float64)
        out[k] = float(np.abs(x - y).max() / (np.abs(y).max() if k == "fg_feat" else 1.0))
    return out


def forward_stages(saved, W):
    """(tag, z64, magnitude, relu, stored bits or None) of every teacher-forced forward stage with a bf16 result"""
    for l in range(8):
        z, mag = hidden_stage64(saved, W, l)
        yield "H%d" % l, z, mag, True, saved.h_bits(l)
    z, mag = rgb_stage64(saved, W)
    yield "gS", z, mag, True, saved.gs_bits


def dx_stages(saved, ws, W):
    """(tag, z64, magnitude, gate, stored bits) of the dX chain, l = 7 .. 0"""
    for l in range(7, -1, -1):
        z, mag = dx_stage64(dx_input(ws, l), W, l)
        yield "dZ%d" % l, z, mag, saved.gates[l], ws.dz_bits(l)
