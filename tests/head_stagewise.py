"""Stage-by-stage float64 restatement of the kernels around the fused MLP kernel in the inference forward, for the
tests that pin them (test_head_stagewise_cpu.py, test_gpu_head_stagewise.py).  A helper module, not a test file: CPU only.

The kernels (csrc/nerf_aux.hip): pack_mlp_kernel / pack_tail_kernel / small_gemm_kernel, fold_latents_kernel, rayfold_kernel,
ray_vd_bias_kernel, chw_to_hwc_kernel and the three per-ray heads ray_head_kernel, ray_head_mfma_kernel<false> and
ray_head_mfma_kernel<true, bf16 | f16>.  n3dt_render_fwd / n3dt_render_fwd16 work in a caller-owned workspace and n3dt_mlp_pack
leaves the whole packed buffer, so every output of these kernels is recomputed here from the kernel's own bit-exact inputs.

Layouts restated (each function names the one it restates): the render workspace carve `fold (+ rayfold) | part | wlocal | bghwc`
(n3dt_api.hip: render_carve), the packed buffer `matrices | W2^T | b2 | W_m | W2 hi/lo fragments` (n3dt_layout.h), the
element -> (row, col) maps of pack_mlp_kernel, the bf16x3 piece doubling and logical_weight's column selection (nerf_aux.hip).

The comparison rule, per entry:   |got - ref64| <= U_family * magnitude,   magnitude = the sum of the absolute terms of that entry
    fold            |b| + sum |w c|                          (merged entry: the 384 terms Wr1[:, :384] . br0 as well)
    W_m             sum_k |a_k b_k|
    vd              sum_j |w_vd pe_j|
    block           sum_s |wlocal_s|                         (part[G + 0] against the sum of its block's wlocal)
    chain           sum_k |pref_k s_k|                       (depth; bg_alpha = 1 - wsum adds ONE_ULP, see bound_bg_alpha)
    G               sum_k |pref_k part_kj|                   (lives in LDS only: CPU tests and the magnitude of fg)
    fg              sum_j |G_j W2_jc| + |b2_c wsum|          (|G_j| taken as G's own magnitude)
    merge           the same + |(1 - wsum) bg|
    rgb0            sum_c |w3_c mg_c| + |b|
U_family = 4 x the largest error of that family's float32-ordered CPU emulation against float64 over all CASES (the "bound 4 x
the floor" of DESIGN 3.12: the margin covers the MFMA's unspecified internal order and FMA contraction).  The floors are the
constants FLOOR below, each beside its measured value; test_head_stagewise_cpu.py re-measures every one and fails if one moved
up.  No number here comes from a GPU run.  Bitwise stages (the packed weights, copied biases, rayfold, bghwc, weight, merge16)
have no unit.
"""
import functools

import numpy as np
import torch

import f32_stagewise as fs
import hier_stagewise as hh
import x16_stagewise as xs

F32, BF16, F16, BF16X3 = 0, 1, 2, 3                    # n3dt.h: N3DT_F32 ..
PRECS = {"fp32": F32, "bf16": BF16, "fp16": F16, "bf16x3": BF16X3}
FMT16 = {BF16: "bf16", F16: "fp16", BF16X3: "bf16"}    # the matrices' 16-bit format
MAP16 = {BF16: "bf16", F16: "fp16", BF16X3: "fp16"}    # the head's 16-bit map type (n3dt_api.hip:205-207: bf16x3 renders on the f16 path)
G, C, HID, PE_DIM = 192, 256, 384, 63                  # n3dt_device.h: N3DT_G, N3DT_C, N3DT_HID, N3DT_PE_DIM
PART_STRIDE = G + 4                                    # n3dt_device.h: N3DT_PART_STRIDE
FOLD_STRIDE = 384 * 10 + 32 + 192                      # n3dt_layout.h: N3DT_FOLD_STRIDE
FOLD_USED = 384 * 9 + 32 + 192                         # the last entry (stage 10) ends here; the rest of a row is never written
RAYFOLD_STRIDE = 192
NSTAGE = 11
HEAD_RAYS, RH_RAYS, HEAD_MAX_BPR = 8, 32, 64           # nerf_aux.hip:342-343, :434
ONE_ULP = 2.0 ** -24                                   # spacing of float32 in [0.5, 1), where bg_alpha = 1 - wsum is rounded
# float32 has no relative accuracy below its smallest normal number 2^-126 (gradual underflow, or flush to zero): each term of an entry
# may lose that much absolutely.  No entry here has more than 1024 terms, so 2^-116 is allowed on top of U x magnitude everywhere; it
# matters only where pref has underflowed (cases deep and contrast: products of 1e-10 transmittances).
ABS_SLACK = 2.0 ** -116

# ---- the measured floors: largest |emulation32 - ref64| / magnitude over all CASES (and both block sizes, 16 and 32, for the head)
FLOOR = {
    "fold": 5.0e-8,        # measured 4.93e-8 (ragged, unmerged)   64-lane stride with fmaf + butterfly, then bias + sum
    "wm": 3.0e-7,          # measured 2.93e-7 (vd)                 small_gemm: one fmaf chain over k = 0 .. 383
    "vd": 1.8e-7,          # measured 1.78e-7 (span)               float32 sin / cos of the float32 direction, 27 fmaf in ascending j
    "block": 1.2e-7,       # measured 1.16e-7 (span, 16)           halving butterfly over the 16 / 32 lanes of a block
    "chain": 1.4e-7,       # measured 1.39e-7 (deep, 16)           the sequential pref / ws / ds chain, 64 blocks
    "G": 3.9e-7,           # measured 3.80e-7 (deep, 16)           sum over the blocks in ascending k on the float32 pref
    "fg_fma": 2.3e-7,      # measured 2.24e-7 (contrast, 16)       ray_head_kernel: 192 fmaf in ascending j on the float32 G, + b2 wsum
    "merge_fma": 2.3e-7,   # measured 2.24e-7 (contrast, 16)
    "fg_mfma": 3.0e-6,     # measured 2.96e-6 (span, 16)           hi hi + hi lo + lo hi per k-step of 16, float32 sums: the lo lo term
    "merge_mfma": 2.5e-6,  # measured 2.41e-6 (contrast, 16)       that is never formed dominates (2^-18 of a term)
    "rgb0": 2.3e-8,        # measured 2.30e-8 (hier_span, 16)      two channels per lane, five-step tree over 32 lanes, four waves, + bias
    # the given-plane cases (hier, hier_span) where their floor is above the table's: their own entries, the entries above stay
    "fg_fma_hier": 2.6e-7,    # measured 2.51e-7 (hier, 32)
    "fg_mfma_hier": 3.2e-6,   # measured 3.17e-6 (hier_span, 16)
}
FACTOR = 4.0


def unit(family):
    return FACTOR * FLOOR[family]


def family_of(name, family):
    """the entry of FLOOR that judges `family` in case `name`: a given-plane case's own entry where it has one"""
    own = family + "_hier"
    return own if CASES[name].get("hier") and own in FLOOR else family


def bound_bg_alpha(mag_chain):
    """bg_alpha = 1.0f - wsum: the chain's bound on wsum plus the rounding of the subtraction.  The result lies in [0, 1 + 1e-10], so
    that rounding is at most half of ONE_ULP; ONE_ULP itself is allowed ("one float32 ulp of 1", read at its smaller meaning)."""
    return unit("chain") * mag_chain + ONE_ULP


# ---------------------------------------------------------------------------------------------------------------------
# layouts
# ---------------------------------------------------------------------------------------------------------------------
def al256(b):
    return (b + 255) & ~255


def stage_dims(s):
    """n3dt_layout.h: n3dt_stage -> (N, K, layer)"""
    return {0: (384, 64, 0), 5: (384, 448, 5), 8: (32, 384, 8), 9: (384, 384, 9), 10: (192, 384, 10)}.get(s, (384, 384, s))


def stage_offset(s):
    """n3dt_layout.h: n3dt_stage_offset (elements)"""
    return sum(stage_dims(i)[0] * stage_dims(i)[1] for i in range(s))


MATRIX_ELEMS = stage_offset(NSTAGE)                    # n3dt_packed_matrix_elems
TAIL_W2T, TAIL_B2, TAIL_WM = 0, G * C, G * C + C       # floats inside the tail (nerf_aux.hip:147-148, :173)
TAIL_FRAGS = G * C + C + G * HID                       # n3dt_tail_w2_frags_offset
TAIL_FLOATS = TAIL_FRAGS + 12 * 8 * 2 * 256            # n3dt_packed_tail_floats


def bias_offset(stage):
    """n3dt_layout.h: n3dt_bias_offset"""
    return 384 * stage if stage <= 8 else (384 * 8 + 32 if stage == 9 else 384 * 9 + 32)


def packed_region_bytes(p):
    """n3dt_layout.h: n3dt_packed_region_bytes = n3dt_packed_tail_offset"""
    return al256(MATRIX_ELEMS * (4 if p == F32 else 2) * (2 if p == BF16X3 else 1))


def packed_bytes(p):
    """n3dt_api.hip: n3dt_mlp_packed_bytes"""
    return packed_region_bytes(p) + 4 * TAIL_FLOATS


def block_samples(p):
    """n3dt_api.hip: block_samples"""
    return 16 if p == F32 else 32


def rayfold_offset(B):
    """n3dt_layout.h: n3dt_rayfold_offset (floats)"""
    return (B * FOLD_STRIDE + 63) & ~63


def fold_region_floats(B, n_rays, vd):
    """n3dt_layout.h: n3dt_fold_region_floats"""
    return rayfold_offset(B) + B * n_rays * RAYFOLD_STRIDE if vd > 0 else B * FOLD_STRIDE


def render_carve(B, n_rays, Ns, p, vd=0):
    """n3dt_api.hip: render_carve -> byte offsets, the bytes each region really holds (`*_used`), bpr, bs and the total"""
    bs = block_samples(p)
    bpr = (Ns + bs - 1) // bs
    blocks = B * n_rays * bpr
    c = {"bs": bs, "bpr": bpr, "blocks": blocks, "fold": 0, "fold_used": 4 * fold_region_floats(B, n_rays, vd)}
    c["part"] = al256(c["fold_used"])
    c["part_used"] = blocks * PART_STRIDE * 4
    c["wlocal"] = c["part"] + al256(c["part_used"])
    c["wlocal_used"] = blocks * bs * 4
    c["bghwc"] = c["wlocal"] + al256(c["wlocal_used"])
    c["bghwc_used"] = n_rays * C * 4
    c["total"] = c["bghwc"] + al256(c["bghwc_used"])
    return c


def pack_index_map(N, K, p):
    """pack_mlp_kernel (nerf_aux.hip:109-122): element e of a stage -> (row, col) of its logical matrix.
    fp32 (16x16x4 A operand):    e = ((ot (K/16) + k4) 64 + lane) 4 + j -> row 16 ot + (lane & 15), col 16 k4 + 4 j + (lane >> 4)
    16-bit (32x32x16 A operand): e = ((ot (K/16) + ks) 64 + lane) 8 + j -> row 32 ot + (lane & 31),
                                                                  col 32 (ks >> 1) + 16 (ks & 1) + 8 (j >> 2) + 4 (lane >> 5) + (j & 3)"""
    e = np.arange(N * K)
    if p == F32:
        j, lane, t = e & 3, (e >> 2) & 63, e >> 8
        k4, ot = t % (K // 16), t // (K // 16)
        return ot * 16 + (lane & 15), 16 * k4 + 4 * j + (lane >> 4)
    j, lane, t = e & 7, (e >> 3) & 63, e >> 9
    ks, ot = t % (K // 16), t // (K // 16)
    return ot * 32 + (lane & 31), 32 * (ks >> 1) + 16 * (ks & 1) + 8 * (j >> 2) + 4 * (lane >> 5) + (j & 3)


def logical_weight(ws, stage, S, fault=None):
    """logical_weight (nerf_aux.hip:15-27) as whole float32 matrices [N, K]: the PE columns, the zero column 63, the latent columns
    removed (they are folded into the bias), module 5's skip columns behind 63 + S, the density row in a 32-row tile.
    fault "zero63": column 63 holds the first latent column;  "skip": the skip columns are read one column early."""
    w = [np.asarray(x, dtype=np.float32) for x in ws]
    z = np.zeros((384, 1), dtype=np.float32)
    if stage == 0:
        return np.concatenate([w[0][:, :63], w[0][:, 63:64] if fault == "zero63" else z], axis=1)
    if stage == 5:
        o = 63 + S - (1 if fault == "skip" else 0)
        return np.concatenate([w[5][:, :63], w[5][:, 63:64] if fault == "zero63" else z, w[5][:, o:o + 384]], axis=1)
    if stage == 8:
        out = np.zeros((32, 384), dtype=np.float32)
        out[0] = w[8][0]
        return out
    if stage == 10:
        return np.ascontiguousarray(w[10][:, :384])
    return w[stage]


def split_bf16(v32):
    """(__bf16)v and (__bf16)(v - (float)hi) as bit patterns (nerf_aux.hip:136-137, :163-164, :539-541)"""
    v = np.asarray(v32, dtype=np.float32)
    hi = xs.bits16(v.astype(np.float64), "bf16")
    rest = (v - xs.bits16_to_f64(hi, "bf16").astype(np.float32)).astype(np.float32)
    return hi, xs.bits16(rest.astype(np.float64), "bf16")


def round_bits(v32, fmt):
    """RNE bf16 / IEEE half of float32 values, as uint16"""
    v = np.asarray(v32, dtype=np.float32)
    return xs.bits16(v.astype(np.float64), fmt)


def pack_expected(ws, bs, S, p, wm32, prefill, fault=None):
    """The whole n3dt_mlp_pack buffer, byte for byte (uint8), over a `prefill` byte pattern, and the number of bytes the kernels write.
    wm32: the tail's float32 W_m [192, 384] (the 16-bit matrices are packed from it; fp32 never forms it: its slot keeps the prefill).
    fault: logical_weight's, or "swap": the hi and lo pieces of the first bf16x3 piece of stage 1 change places."""
    region = packed_region_bytes(p)
    buf = np.full(region + 4 * TAIL_FLOATS, prefill, dtype=np.uint8)
    written = 0
    mat = buf[:region].view(np.float32 if p == F32 else np.uint16)
    for s in range(NSTAGE):
        if p != F32 and s == 10:
            continue                                   # its slot stays unused (nerf_aux.hip:103)
        merged = p != F32 and s == 9
        N, K, _ = stage_dims(10 if merged else s)
        W = np.asarray(wm32, dtype=np.float32) if merged else logical_weight(ws, s, S, fault)
        row, col = pack_index_map(N, K, p)
        v = W[row, col]
        at = stage_offset(s) + np.arange(N * K)
        if p == F32:
            mat[at] = v
        elif p == BF16X3:                              # piece P -> pieces 2P (hi) and 2P + 1 (lo), 512 elements each
            P, inn = at >> 9, at & 511
            hi, lo = split_bf16(v)
            if fault == "swap":
                first = P == (stage_offset(1) >> 9)
                hi, lo = np.where(first, lo, hi), np.where(first, hi, lo)
            mat[2 * P * 512 + inn] = hi
            mat[(2 * P + 1) * 512 + inn] = lo
        else:
            mat[at] = round_bits(v, FMT16[p])
        written += N * K * (4 if p == F32 else 4 if p == BF16X3 else 2)
    tail = buf[region:].view(np.float32)
    w2 = np.asarray(ws[11], dtype=np.float32)
    tail[TAIL_W2T:TAIL_B2] = w2.T.reshape(-1)
    tail[TAIL_B2:TAIL_WM] = np.asarray(bs[11], dtype=np.float32)
    written += 4 * (G * C + C)
    if p != F32:
        tail[TAIL_WM:TAIL_FRAGS] = np.asarray(wm32, dtype=np.float32).reshape(-1)
        written += 4 * G * HID
    # pack_tail_kernel: piece ((ks 8 + tile) 2 + part), lane-linear: lane (column 32 tile + (lane & 31)) holds k = 16 ks + 8 (lane >> 5) + j
    piece, lane, j = np.meshgrid(np.arange(12 * 8 * 2), np.arange(64), np.arange(8), indexing="ij")
    part, tile, ks = piece & 1, (piece >> 1) & 7, piece >> 4
    hi, lo = split_bf16(w2[32 * tile + (lane & 31), 16 * ks + 8 * (lane >> 5) + j])
    buf[region + 4 * TAIL_FRAGS:].view(np.uint16)[:] = np.where(part == 0, hi, lo).reshape(-1)
    written += 12 * 8 * 2 * 64 * 8 * 2
    return buf, written


# ---------------------------------------------------------------------------------------------------------------------
# float32-ordered helpers
# ---------------------------------------------------------------------------------------------------------------------
def f32(a):
    return np.asarray(a).astype(np.float32)


def f64(a):
    return np.asarray(a).astype(np.float64)


def fma32(a, b, c):
    """fmaf: the product of two float32 values is exact in float64; one rounding of the sum"""
    return (f64(a) * f64(b) + f64(c)).astype(np.float32)


def halving_sum(v):
    """the __shfl_xor butterflies over the last axis (a power of two): pairs (l, l ^ off), off = n/2 .. 1, in float32"""
    v = f32(v)
    while v.shape[-1] > 1:
        h = v.shape[-1] // 2
        v = v[..., :h] + v[..., h:]
    return v[..., 0]


# ---------------------------------------------------------------------------------------------------------------------
# merged matrix, fold table, view-direction bias
# ---------------------------------------------------------------------------------------------------------------------
def merged_matrix64(ws):
    """W_m = Wr1[:, 0:384] Wr0 (nerf_aux.hip:172-175) in float64 and sum_k |a_k b_k|"""
    a, b = f64(ws[10])[:, :HID], f64(ws[9])
    return a @ b, np.abs(a) @ np.abs(b)


def merged_matrix32(ws):
    """small_gemm_kernel's sum: acc = fmaf(a, b, acc) over k = 0 .. 383 in order (the 32-wide slabs follow each other), C = 0 + acc"""
    a, b = f32(ws[10])[:, :HID], f32(ws[9])
    acc = np.zeros((G, HID), dtype=np.float32)
    for k in range(HID):
        acc = fma32(a[:, k:k + 1], b[k][None, :], acc)
    return acc


def fold_terms(ws, bs, codes, S, A, U, merged, fault=None):
    """fold_latents_kernel per stage: (stage, rows W [N, n_code], code [B, n_code], bias [N]) of the three folded entries.
    fault "no_br0": the merged entry without Wr1[:, :384] . br0."""
    shape, appea, audio = codes
    su = shape if U == 0 else np.concatenate([shape, audio], axis=1)
    out = [(0, ws[0][:, 63:63 + S + U], su, bs[0]), (5, ws[5][:, 63:63 + S], shape, bs[5])]
    if merged and fault != "no_br0":
        out.append((10, ws[10], np.concatenate([np.broadcast_to(bs[9], (shape.shape[0], HID)), appea], axis=1), bs[10]))
    else:
        out.append((10, ws[10][:, HID:], appea, bs[10]))
    return out


def fold_ref(ws, bs, codes, S, A, U, merged, fault=None):
    """The per-frame bias table (n3dt_layout.h:72-79) in float64: (ref [B, FOLD_USED], magnitude, exact) -- `exact` marks the plain
    copies b1..b4, b6, b7, brgb0 and the density tile (row 0 = its bias, rows 1..31 zero), which are held bitwise."""
    B = codes[0].shape[0]
    ref = np.zeros((B, FOLD_USED))
    mag = np.zeros((B, FOLD_USED))
    exact = np.ones(FOLD_USED, dtype=bool)
    for s in (1, 2, 3, 4, 6, 7, 9):
        ref[:, bias_offset(s):bias_offset(s) + 384] = f64(bs[s])
    ref[:, bias_offset(8)] = f64(bs[8])[0]
    for s, W, code, b in fold_terms(ws, bs, codes, S, A, U, merged, fault):
        o, n = bias_offset(s), W.shape[0]
        ref[:, o:o + n] = f64(b) + f64(code) @ f64(W).T
        mag[:, o:o + n] = np.abs(f64(b)) + np.abs(f64(code)) @ np.abs(f64(W)).T
        exact[o:o + n] = False
    return ref, mag, exact


def fold_emul(ws, bs, codes, S, A, U, merged):
    """float32 in the kernel's order: lane l sums columns l, l + 64, .. with fmaf, the 64 lanes meet in a butterfly, then bias + sum"""
    B = codes[0].shape[0]
    out = np.zeros((B, FOLD_USED), dtype=np.float32)
    for s, W, code, b in fold_terms(ws, bs, codes, S, A, U, merged):
        n_code = W.shape[1]
        pad = (-n_code) % 64
        Wp = np.concatenate([f32(W), np.zeros((W.shape[0], pad), dtype=np.float32)], axis=1)
        for f in range(B):
            cp = np.concatenate([f32(code[f]), np.zeros(pad, dtype=np.float32)])
            acc = np.zeros((W.shape[0], 64), dtype=np.float32)
            for i in range(0, n_code + pad, 64):
                acc = fma32(Wp[:, i:i + 64], cp[None, i:i + 64], acc)
            out[f, bias_offset(s):bias_offset(s) + W.shape[0]] = f32(b) + fs.butterfly_sum(acc)[:, 0]
    return out


def vd_encode(d, dt):
    """Embedder_4 of the float32 direction d [..., 3] (nerf_aux.hip:305-314): [d, sin(2^k d), cos(2^k d)], k = 0 .. 3"""
    d = f32(d)
    feats = [d.astype(dt)]
    for k in range(4):
        a = (d * np.float32(2 ** k)).astype(dt)   # exact scaling
        feats += [np.sin(a), np.cos(a)]
    return np.concatenate(feats, axis=-1)


def vd_ref(w_vd, d):
    """ray_bias[ray][o] = sum_j w_vd[o][j] pe_j in float64 on the float32 direction, and sum_j |w pe|"""
    pe = vd_encode(d, np.float64)
    return pe @ f64(w_vd).T, np.abs(pe) @ np.abs(f64(w_vd)).T


def vd_emul(w_vd, d):
    pe = vd_encode(d, np.float32)
    acc = np.zeros(pe.shape[:-1] + (G,), dtype=np.float32)
    for j in range(27):
        acc = fma32(f32(w_vd)[:, j], pe[..., j:j + 1], acc)
    return acc


# ---------------------------------------------------------------------------------------------------------------------
# the head
# ---------------------------------------------------------------------------------------------------------------------
def pref32(part):
    """the head's sequential float32 product (nerf_aux.hip:358-366, :460-468): pref[k] = prod_{i<k} part[i][G + 2]"""
    t = f32(part)[:, :, G + 2]
    out = np.ones(t.shape, dtype=np.float32)
    for k in range(1, t.shape[1]):
        out[:, k] = out[:, k - 1] * t[:, k - 1]
    return out


def weight_expected(part, wlocal, Ns, bs):
    """weight[ray][s] = pref[s / bs] * wlocal[ray][s / bs][s % bs]: two float32 values, one multiply -- bitwise"""
    R, bpr = part.shape[0], part.shape[1]
    w = pref32(part)[:, :, None] * f32(wlocal).reshape(R, bpr, bs)
    return w.reshape(R, bpr * bs)[:, :Ns]


def bg_rows(bg_hwc, R, n_rays, fault=None):
    """the background row of every ray: row rg % n_rays of the ray-major map (nerf_aux.hip:408-410, :566-568, :598-600).
    fault "prev_frame": the same ray index one frame earlier -- the map does not depend on the frame, so this is the SAME row;
    fault "no_wrap": the row index runs on across a frame boundary inside a 32-ray workgroup, min(first % n_rays + r, n_rays - 1)."""
    rg = np.arange(R)
    if fault == "prev_frame":
        rg = np.maximum(rg - n_rays, rg % n_rays)
    row = rg % n_rays
    if fault == "no_wrap":
        first = (rg // RH_RAYS) * RH_RAYS
        row = np.minimum(first % n_rays + (rg - first), n_rays - 1)
    return f64(bg_hwc)[row]


def head_ref(part, W2, b2, bg=None, fault=None):
    """The head in float64 from the read-back part [R, bpr, PART_STRIDE] (float32), W2 [256, 192], b2 [256] and the rays' background
    rows bg [R, 256] (or None).  Returns every stage with its magnitude: pref, wsum, dsum, G, fg, merge, bg_alpha.
    faults: "pref_prev" pref of block k taken as block k - 1's; "lost_block" the second block (the only one at bpr = 1) lost from G;
    "no_b2" the b2 wsum term dropped; "lane_half" rays 4..7 of every eight swapped with 0..3 (the h of (r & 3) + 8 (r >> 2) + 4 h)."""
    p = f64(part)
    R, bpr = p.shape[:2]
    t = p[:, :, G + 2]
    pref = np.concatenate([np.ones((R, 1)), np.cumprod(t, axis=1)[:, :-1]], axis=1)
    if fault == "pref_prev":
        pref = np.concatenate([pref[:, :1], pref[:, :-1]], axis=1)
    o = {"pref": pref}
    o["wsum"], o["mag_chain_w"] = (pref * p[:, :, G]).sum(1), np.abs(pref * p[:, :, G]).sum(1)
    o["dsum"], o["mag_chain_d"] = (pref * p[:, :, G + 1]).sum(1), np.abs(pref * p[:, :, G + 1]).sum(1)
    pg = pref.copy()
    if fault == "lost_block":
        pg[:, min(1, bpr - 1)] = 0.0
    o["G"] = np.einsum("rk,rkj->rj", pg, p[:, :, :G])
    o["mag_G"] = np.einsum("rk,rkj->rj", np.abs(pref), np.abs(p[:, :, :G]))
    w2, bb = f64(W2), f64(b2)
    bterm = np.zeros((R, C)) if fault == "no_b2" else bb[None, :] * o["wsum"][:, None]
    o["fg"] = o["G"] @ w2.T + bterm
    o["mag_fg"] = o["mag_G"] @ np.abs(w2).T + np.abs(bb[None, :] * o["wsum"][:, None])
    if fault == "lane_half":
        r = np.arange(R)
        src = np.minimum(r ^ 4, R - 1)
        o["fg"] = o["fg"][src]
    o["bg_alpha"] = 1.0 - o["wsum"]
    if bg is not None:
        o["merge"] = o["fg"] + o["bg_alpha"][:, None] * f64(bg)
        o["mag_merge"] = o["mag_fg"] + np.abs(o["bg_alpha"][:, None] * f64(bg))
    return o


def rgb0_ref(mg32, w3, b3, fault=None):
    """rgb0[ray][k] = sum_c w3[k][c] mg[ray][c] + b[k] on the kernel's own float32 merged values mg [R, 256]; and its magnitude.
    fault "label": the ray register named one butterfly step off -- rsel's bits rotated by one (nerf_aux.hip:639-640)."""
    m = f64(mg32)
    ref, mag = m @ f64(w3).T + f64(b3), np.abs(m) @ np.abs(f64(w3)).T + np.abs(f64(b3))
    if fault == "label":
        R = m.shape[0]
        r = np.arange(R)
        rr, h = r % RH_RAYS, ((r % RH_RAYS) >> 2) & 1
        rsel = (rr & 3) | ((rr >> 3) << 2)                     # rr = (rsel & 3) + 8 (rsel >> 2) + 4 h
        rs2 = ((rsel << 1) & 15) | (rsel >> 3)
        src = np.minimum((r // RH_RAYS) * RH_RAYS + (rs2 & 3) + 8 * (rs2 >> 2) + 4 * h, R - 1)
        ref = ref[src]
    return ref, mag


def head_chain32(part):
    """the sequential float32 chain: pref[k] = Trun; ws += Trun po[0]; ds += Trun po[1]; Trun *= po[2]"""
    p = f32(part)
    pref = pref32(p)
    ws = np.zeros(p.shape[0], dtype=np.float32)
    ds = np.zeros(p.shape[0], dtype=np.float32)
    for k in range(p.shape[1]):
        ws = ws + pref[:, k] * p[:, k, G]
        ds = ds + pref[:, k] * p[:, k, G + 1]
    return pref, ws, ds


def head_G32(part, pref):
    """G[ray][j] = sum_k pref[k] part[k][j] in ascending k, float32 products and sums (both the quad path at bpr <= 2, whose
    pf0 v0 + pf1 v1 is the same two roundings, and the general loop)"""
    p = f32(part)
    acc = np.zeros((p.shape[0], G), dtype=np.float32)
    for k in range(p.shape[1]):
        acc = acc + pref[:, k:k + 1] * p[:, k, :G]
    return acc


def head_fma32(G32, ws, W2, b2):
    """ray_head_kernel: acc = fmaf(W2T[j][c], G[j], acc) in ascending j, fg = acc + b2 wsum"""
    return fs.mm_fma_chain(G32, W2) + f32(b2)[None, :] * ws[:, None]


def split_f64(v32):
    hi, lo = split_bf16(v32)
    return xs.bits16_to_f64(hi, "bf16"), xs.bits16_to_f64(lo, "bf16")


def head_mfma32(G32, ws, W2, b2, drop=None):
    """ray_head_mfma_kernel: both factors split into bf16 hi + lo, per k-step of 16 the three products hi hi, hi lo (a_hi b_lo),
    lo hi (a_lo b_hi), every product exact in float32, summed one by one in float32; then + b2 wsum.  drop: "a_lo_b_hi" | "a_hi_b_lo"."""
    a_hi, a_lo = split_f64(G32)            # [R, 192]
    b_hi, b_lo = split_f64(W2)             # [256, 192]
    acc = np.zeros((G32.shape[0], C), dtype=np.float32)
    for ks in range(G // 16):
        for name, a, b in (("hh", a_hi, b_hi), ("a_hi_b_lo", a_hi, b_lo), ("a_lo_b_hi", a_lo, b_hi)):
            if name == drop:
                continue
            for k in range(16 * ks, 16 * ks + 16):
                acc = (acc.astype(np.float64) + a[:, k:k + 1] * b[None, :, k]).astype(np.float32)
    return acc + f32(b2)[None, :] * ws[:, None]


def mfma_terms64(G32, W2):
    """the float64 value of each of the four hi / lo products of G W2^T (for the deliberate faults)"""
    a_hi, a_lo = split_f64(G32)
    b_hi, b_lo = split_f64(W2)
    return {"hh": a_hi @ b_hi.T, "a_hi_b_lo": a_hi @ b_lo.T, "a_lo_b_hi": a_lo @ b_hi.T}


def merge32(fg32, ws, bg):
    return fg32 + (np.float32(1) - ws)[:, None] * f32(bg)


def rgb0_emul(mg32, w3, b3):
    """lane (wave, r31) holds channels 64 wave + r31 and + 32: pr = w3 mg, then fmaf; the 32 lanes of a half-wave meet in a halving
    tree (16, 8, 4, 2, 1); the four waves as (s0 + s1) + (s2 + s3) + b (nerf_aux.hip:608, :625-649)"""
    m, w = f32(mg32), f32(w3)
    R = m.shape[0]
    out = np.zeros((R, 3), dtype=np.float32)
    for k in range(3):
        s = []
        for wave in range(4):
            c0 = 64 * wave + np.arange(32)
            pr = fma32(w[k, c0 + 32][None, :], m[:, c0 + 32], w[k, c0][None, :] * m[:, c0])
            s.append(halving_sum(pr))
        out[:, k] = ((s[0] + s[1]) + (s[2] + s[3])) + f32(b3)[k]
    return out


def block_sum32(wlocal, bs):
    """part[G + 0]: the block's weights met in a halving butterfly over its 16 / 32 lanes"""
    return halving_sum(f32(wlocal).reshape(-1, bs))


# ---------------------------------------------------------------------------------------------------------------------
# the cases and their seeded inputs
# ---------------------------------------------------------------------------------------------------------------------
CASES = {
    # B x rays x samples                                        (test_gpu_head_stagewise.py says what each exercises)
    "one": dict(B=1, n_rays=1, n_samples=32, weights="seed0", kw={}),
    "ragged": dict(B=3, n_rays=7, n_samples=40, weights="seed0", kw={}),
    "span": dict(B=3, n_rays=45, n_samples=65, weights="seed0", kw={}),
    "full": dict(B=2, n_rays=32, n_samples=32, weights="seed0", kw={}),
    "deep": dict(B=1, n_rays=2, n_samples=1024, weights="seed0", kw={}),
    "contrast": dict(B=3, n_rays=7, n_samples=40, weights="contrast", kw={}),
    "gaze": dict(B=3, n_rays=7, n_samples=40, weights="seed0", kw={"include_gaze": True, "eye_gaze_dim": 64, "audio_dim": 0}),
    "vd": dict(B=3, n_rays=7, n_samples=40, weights="seed0", kw={}, vd=True),
    # the hierarchical pass: z_planes_given = 1, the case carries its N_c + N_f + 1 planes (hier_stagewise.given_planes), one ray's by hand
    "hier": dict(B=3, n_rays=7, n_samples=40, weights="seed0", kw={}, hier=(16, 24)),
    "hier_span": dict(B=3, n_rays=45, n_samples=65, weights="seed0", kw={}, hier=(24, 41)),
}
FEATMAP_SIZE = 8


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """Everything a case's call takes, seeded, as CPU tensors / numpy: the options, the state dict, the frame inputs restricted to the
    case's free ray set (`batch_xy[:, :, rays]`), the 12 float32 matrices as the library gets them (include_vd: RGB_layer_1 without
    its 27 view-direction columns, which are `w_vd`), the codes, the background rows of the rays and feat_2_rgb[0]."""
    from n3dt import BaseOptions, synthetic as syn
    c = CASES[name]
    vd = bool(c.get("vd"))
    opt = BaseOptions({"featmap_size": FEATMAP_SIZE, "featmap_nc": 256, "pred_img_size": 4 * FEATMAP_SIZE, "num_sample_coarse": c["n_samples"]})
    if c["weights"] == "contrast":
        sd = syn.contrast_state_dict(opt, seed=0)
    else:
        sd = syn.make_state_dict(opt, seed=0, bg_noise=0.1, include_vd=vd, **c["kw"])
    inp = dict(syn.frame_inputs(opt, c["B"], **c["kw"]))
    rays = torch.from_numpy(xs.case_rays(c["n_rays"]))
    assert len(rays) == c["n_rays"]
    inp["batch_xy"] = inp["batch_xy"][:, :, rays].contiguous()
    del inp["batch_uv"]
    ws, bs = xs.mlp_arrays(sd)
    ws, bs = [np.ascontiguousarray(w, dtype=np.float32) for w in ws], [np.ascontiguousarray(b, dtype=np.float32) for b in bs]
    w10_full, w_vd = ws[10], None
    if vd:
        w_vd = np.ascontiguousarray(ws[10][:, HID:HID + 27])
        ws[10] = np.ascontiguousarray(np.concatenate([ws[10][:, :HID], ws[10][:, HID + 27:]], axis=1))
    d = syn.mlp_dims(opt, **c["kw"])
    S, A, U = d["shape_dim"], d["appea_dim"], d["audio_dim"]
    assert ws[0].shape[1] == 63 + S + U and ws[5].shape[1] == 63 + S + HID and ws[10].shape[1] == HID + A
    audio = inp["audiostyle"].numpy().astype(np.float32) if U > 0 else None
    codes = (inp["shape_code"].numpy().astype(np.float32), inp["appea_code"].numpy().astype(np.float32), audio)
    planes = None
    if c.get("hier"):
        planes = hh.given_planes(inp["batch_Tvecs"].numpy().reshape(c["B"], 3)[:, 2], c["n_rays"], c["hier"][0], c["hier"][1], 0, opt.world_z1, opt.world_z2)
        assert planes.shape == (c["B"], c["n_rays"], c["n_samples"] + 1)
    bg_chw = np.ascontiguousarray(sd["neural_render.bg_featmap"].reshape(C, -1)[:, rays].numpy())     # [C, n_rays]
    return {"name": name, "c": c, "opt": opt, "sd": sd, "inp": inp, "rays": rays, "ws": ws, "bs": bs, "w10_full": w10_full, "w_vd": w_vd, "vd": 27 if vd else 0,
            "S": S, "A": A, "U": U, "codes": codes, "bg_chw": bg_chw, "bg_hwc": np.ascontiguousarray(bg_chw.T),
            "w3": sd["neural_render.feat_2_rgb_list.0.weight"].reshape(3, C).numpy().copy(),
            "b3": sd["neural_render.feat_2_rgb_list.0.bias"].numpy().copy(),
            "B": c["B"], "n_rays": c["n_rays"], "Ns": c["n_samples"], "planes": planes}


def directions32(ci):
    """the float32 ray directions [B, rays, 3] as n3dt_ray_setup forms them (f32_stagewise.ray_setup)"""
    inp = ci["inp"]
    return fs.ray_setup(np.float32, inp["batch_xy"].numpy(), inp["batch_Rmats"].numpy(), inp["batch_inv_inmats"].numpy())[4]


# ---------------------------------------------------------------------------------------------------------------------
# the whole chain in float64 (CPU stand-in of the fused kernel: the source of `part` on a machine without a GPU)
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cpu_points(name):
    """Per-sample g = relu(RGB_layer_1) [R, Ns, 192] and the density pre-activation sigma64 [R, Ns] in float64, from the ORACLE's float32
    sample points and encodings through the restated logical matrices and the restated fold table (merged and unmerged forms, which
    must agree); plane distances, z values and the density that is composited (`sigma`) are the oracle's per-sample values."""
    from oracle import oracle as orc
    ci = case_inputs(name)
    inp, opt, B, n_rays, Ns = ci["inp"], ci["opt"], ci["B"], ci["n_rays"], ci["Ns"]
    s = orc.sample(inp["batch_xy"].numpy(), inp["batch_Rmats"].numpy(), inp["batch_Tvecs"].numpy(), inp["batch_inv_inmats"].numpy(), Ns,
                   opt.world_z1, opt.world_z2)
    if ci["planes"] is not None:   # z_planes_given: the oracle's FineSample._calc_sample_points_by_zvals on the case's planes
        s.update(orc.sample_planes(inp["batch_xy"].numpy(), inp["batch_Rmats"].numpy(), inp["batch_Tvecs"].numpy(), inp["batch_inv_inmats"].numpy(),
                                   ci["planes"]))
    pe = orc.embed(s["pts"])                                                     # [B, 63, rays, Ns] float32
    x = np.concatenate([f64(pe), np.zeros((B, 1, n_rays, Ns))], axis=1)          # channel 63 = the zero padding
    x = np.moveaxis(x, 1, -1).reshape(B, n_rays * Ns, 64)
    ws, bs, S, A, U = ci["ws"], ci["bs"], ci["S"], ci["A"], ci["U"]
    L = [f64(logical_weight(ws, l, S)) for l in range(NSTAGE)]
    fu = fold_ref(ws, bs, ci["codes"], S, A, U, merged=False)[0]
    fm = fold_ref(ws, bs, ci["codes"], S, A, U, merged=True)[0]
    wm = merged_matrix64(ws)[0]
    rb = np.zeros((B, n_rays, 1, G))
    if ci["vd"]:
        rb = vd_ref(ci["w_vd"], directions32(ci))[0][:, :, None, :]

    def b(table, stage, n):
        return table[:, None, bias_offset(stage):bias_offset(stage) + n]

    h = np.maximum(x @ L[0].T + b(fu, 0, 384), 0.0)
    for l in range(1, 8):
        h = np.maximum((np.concatenate([x, h], axis=-1) if l == 5 else h) @ L[l].T + b(fu, l, 384), 0.0)
    sigma = (h @ L[8].T)[..., 0] + fu[:, None, bias_offset(8)]
    sigma_mag = (h @ np.abs(L[8]).T)[..., 0] + np.abs(fu[:, None, bias_offset(8)])
    # the oracle's own per-sample density (float32, after its ReLU): the compositing below takes IT, so that a sharp density head
    # (case contrast: gain 400) does not turn the oracle's float32 rounding of sigma into a difference of the composited maps;
    # the restated sigma is compared with it directly (test_head_stagewise_cpu.py)
    vd_pe = orc.embed_dirs(s["ray_d"], Ns) if ci["vd"] else None
    dens_o = orc.mlp(ci["sd"], pe, ci["codes"][0], ci["codes"][1], ci["codes"][2], vd=vd_pe)[1]
    per_ray = lambda v: (v.reshape(B, n_rays, Ns, G) + rb).reshape(B * n_rays, Ns, G)
    g_m = np.maximum(per_ray(h @ wm.T + b(fm, 10, G)), 0.0)
    g_u = np.maximum(per_ray((h @ L[9].T + b(fu, 9, 384)) @ L[10].T + b(fu, 10, G)), 0.0)
    assert np.abs(g_m - g_u).max() <= 1e-11 * max(1.0, np.abs(g_u).max()), "merged and unmerged RGB stage disagree"
    R = B * n_rays
    return {"g": g_m, "sigma": f64(dens_o).reshape(R, Ns), "sigma64": sigma.reshape(R, Ns), "sigma_mag": sigma_mag.reshape(R, Ns),
            "dist": f64(s["z_dists"]).reshape(R, Ns), "zval": f64(s["zvals"]).reshape(R, Ns)}


@functools.lru_cache(maxsize=None)
def cpu_part(name, bs):
    """part [R, bpr, PART_STRIDE] and wlocal [R, bpr, bs] as the fused kernels leave them (nerf_fwd_f32.hip:108-140, nerf_fwd_x16.hip:
    399-418), from cpu_points, rounded to float32: per block alpha = 1 - exp(-relu(sigma) dist), x = 1 - alpha + 1e-10, the in-block
    exclusive product Tl, w = alpha Tl; part = [sum w g | sum w | sum w zval | prod x | 0].  Lanes beyond n_samples: dist = 0, w = 0."""
    pt = cpu_points(name)
    R, Ns = pt["sigma"].shape
    bpr = (Ns + bs - 1) // bs
    pad = bpr * bs - Ns

    def blocks(v):
        return np.concatenate([v, np.zeros((R, pad) + v.shape[2:])], axis=1).reshape((R, bpr, bs) + v.shape[2:])

    alpha = 1.0 - np.exp(-np.maximum(blocks(pt["sigma"]), 0.0) * blocks(pt["dist"]))
    live = blocks(np.ones((R, Ns))) > 0
    x = np.where(live, 1.0 - alpha + 1e-10, 1.0)
    Tl = np.concatenate([np.ones((R, bpr, 1)), np.cumprod(x, axis=2)[:, :, :-1]], axis=2)
    w = alpha * Tl
    part = np.zeros((R, bpr, PART_STRIDE))
    part[:, :, :G] = np.einsum("rks,rksj->rkj", w, blocks(pt["g"]))
    part[:, :, G] = w.sum(2)
    part[:, :, G + 1] = (w * blocks(pt["zval"])).sum(2)
    part[:, :, G + 2] = np.prod(x, axis=2)
    return f32(part), f32(w)


# ---------------------------------------------------------------------------------------------------------------------
# reporting
# ---------------------------------------------------------------------------------------------------------------------
def ratio(got, ref, mag, extra=0.0):
    """largest (|got - ref| - extra - ABS_SLACK) / magnitude over the entries (0 where that error is 0, whatever the magnitude)"""
    err = np.maximum(np.abs(f64(got) - ref) - extra - ABS_SLACK, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0.0, 0.0, err / mag)
    return float(q.max()) if q.size else 0.0


def report(tag, family, r):
    """prints a figure before it is judged: the largest error in units of the family's bound"""
    print("%-44s %-10s worst / bound = %.3f   (|err| / magnitude %.3e, unit %.3e)" % (tag, family, r / unit(family), r, unit(family)))
    return r / unit(family)
