"""csrc/lpips.hip BY STAGE, through the two buffers n3dt_lpips_pack and n3dt_lpips leave behind: the packed weights and the caller-owned
workspace (test_lpips_stagewise_cpu.py, test_gpu_lpips_stagewise.py; DESIGN 3.14 and the LPIPS bullet of section 4).  CPU only.

test_gpu_lpips.py judges a score and five layer values per pair: means over every pixel and channel of a difference between two
images that went through the same code.  An error common to both images cancels, a local one is divided by the pixel count, and
the distance kernel's pixel -> partial assignment is seen through the sum only.  Here every stored value is judged alone.

  layout      ws_layout / pack_layout restate lp_workspace() and lp_layout() of lpips.hip (maps of lpips_core.h, each rounded up to 64
              floats, then [5][B][128] doubles; per layer hi | lo fragment matrices, then biases, then lin vectors, each rounded up
              to 256 bytes); pack_decode restates conv_frag.h's cf_pack_decode
  reference   every stage in float64 FROM THE STORED INPUT of that stage (teacher-forced): in0 in float32 numpy (bitwise), conv from
              the stored padded input with the state dict's fp32 weights, pool from the stored relu (bitwise), partials from the
              stored relu maps, layers and the score from the stored partials (bitwise, sequential sums)
  emulation   the kernels' arithmetic in float32, written into a synthetic workspace and pack buffer: operands split hi + lo, the
              products lo hi, hi lo, hi hi per K step of 16 into an fp32 accumulator, K tap-major and channel fastest.  It is the
              source of the floors, it must pass every rule, and with one deliberate fault each the named rule must report it.

Rules (judge / judge_pack; every stored value falls under exactly one):
  pack        byte for byte over the prefill
  in0         bitwise; halo +0
  conv1..5    per entry |got - ref| <= 4 floor_l S, S = |b| + sum |w||x|; equal where S == 0; halo of relu3 / relu4 +0 bits
  pool1, 2    bitwise; halo +0
  partials    per part |got - ref| <= 1e-13 S_p, S_p = sum_pixels sum_c |w_c| (|n0_c| + |n1_c|)^2 -- a bound from the arithmetic, not a
              measurement: fewer than 100 float64 roundings per term; a part without a pixel is +0
  layers out  bitwise from the stored partials
  untouched   every byte outside the regions keeps the prefill
  identical   a pair of identical images has every partial +0
A conv bound is MARGIN = 4 x FLOOR[l]; test_lpips_stagewise_cpu.py re-measures the floors.  No bound comes from a GPU run."""
import collections
import functools

import numpy as np
import torch
import torch.nn.functional as F

import lpips_restatement as lr
import vgg_stagewise as vs
from eval_restatement import quantise

LAYERS = 5
CIN = (3, 64, 192, 384, 256)
COUT = (64, 192, 384, 256, 256)
KSIZE = (11, 5, 3, 3, 3)
STRIDE = (4, 1, 1, 1, 1)
K = tuple(k * k * c for k, c in zip(KSIZE, CIN))          # 363, 1600, 1728, 3456, 2304
KP = tuple((k + 15) // 16 * 16 for k in K)                 # 368 for conv1
PARTS = 128
MAX_BATCH = 64
NAMES = ("in0", "relu1", "pool1", "relu2", "pool2", "relu3", "relu4", "relu5")
PAD = {"in0": 2, "relu1": 0, "pool1": 2, "relu2": 0, "pool2": 1, "relu3": 1, "relu4": 1, "relu5": 0}
RELU = ("relu1", "relu2", "relu3", "relu4", "relu5")
CONV_IN = ("in0", "pool1", "pool2", "relu3", "relu4")
SHIFT = np.array(lr.SHIFT, np.float32)
SCALE = np.array(lr.SCALE, np.float32)
EPS = 1e-10
MARGIN = 4.0
PARTIAL_BOUND = 1e-13
OLD_SCORE_TOL, OLD_LAYER_TOL = 1.142e-5, 1.270e-4          # test_gpu_lpips.py's bounds, for the fault table's second column
PREFILL = 0xA5

# B, H, W: the smallest shapes at which each loop can go wrong
CASES = collections.OrderedDict((("min", (1, 31, 31)), ("odd", (3, 67, 61)), ("wide", (2, 127, 95)), ("cap", (64, 31, 31))))
RUNS = (("min", "reference"), ("min", "standard"), ("odd", "reference"), ("odd", "standard"), ("wide", "reference"), ("wide", "standard"),
        ("cap", "reference"))
FAULT_RUNS = (("min", "standard"), ("odd", "reference"), ("odd", "standard"), ("wide", "standard"))
SEED = {("min", "reference"): 11, ("min", "standard"): 11, ("odd", "reference"): 3, ("odd", "standard"): 12,
        ("wide", "reference"): 13, ("wide", "standard"): 13, ("cap", "reference"): 17}
# odd: the quiet level and the stripe's colour as FED bytes, chosen per mode so that the rows and columns the pools drop hold the
# largest values of relu1 and relu2 (_texture, dropped_hold_the_largest)
ODD_BASE = {"reference": 8, "standard": 120}
ODD_STRIPE = {"reference": (102, 204, 51), "standard": (255, 0, 102)}

# The emulation's largest |emulated - ref| / S per conv layer over RUNS, the three accumulation forms (test_lpips_stagewise_cpu.py
# ::test_floors_have_not_moved prints and re-checks them)
FLOOR = (3.5e-6, 1.7e-6, 2.5e-6, 2.5e-6, 3.35e-6)


def bound(l):
    return MARGIN * FLOOR[l]


# ---------------------------------------------------------------------------------------------
# layout
# ---------------------------------------------------------------------------------------------
def rup(n, a):
    return (n + a - 1) // a * a


def feat_extent(l, n):
    r1 = (n + 4 - 11) // 4 + 1
    if l == 0:
        return r1
    r2 = (r1 - 3) // 2 + 1
    return r2 if l == 1 else (r2 - 3) // 2 + 1


def shapes(B, H, W):
    """name -> the stored shape [2B, rows, columns, C], halo included (lpips_core.h: lp_maps)"""
    n = 2 * B
    fh, fw = [feat_extent(l, H) for l in range(LAYERS)], [feat_extent(l, W) for l in range(LAYERS)]
    out = collections.OrderedDict()
    out["in0"] = (n, H + 4, W + 4, 3)
    out["relu1"] = (n, fh[0], fw[0], 64)
    out["pool1"] = (n, fh[1] + 4, fw[1] + 4, 64)
    out["relu2"] = (n, fh[1], fw[1], 192)
    out["pool2"] = (n, fh[2] + 2, fw[2] + 2, 192)
    out["relu3"] = (n, fh[2] + 2, fw[2] + 2, 384)
    out["relu4"] = (n, fh[2] + 2, fw[2] + 2, 256)
    out["relu5"] = (n, fh[2], fw[2], 256)
    return out


def ws_layout(B, H, W):
    """(name -> (byte offset, shape), byte offset of the [5][B][128] double partials, total bytes): lp_workspace()"""
    off, reg = 0, collections.OrderedDict()
    for name, shp in shapes(B, H, W).items():
        reg[name] = (off, shp)
        off += rup(int(np.prod(shp)), 64) * 4
    return reg, off, off + LAYERS * B * PARTS * 8


def ws_views(ws, B, H, W):
    """name -> float32 view of the map, and "partial" -> float64 [5, B, 128], of the workspace bytes (uint8 numpy)"""
    ws = np.asarray(ws)
    reg, poff, total = ws_layout(B, H, W)
    assert ws.dtype == np.uint8 and ws.size >= total, (ws.dtype, ws.size, total)
    v = {name: ws[o:o + 4 * int(np.prod(shp))].view(np.float32).reshape(shp) for name, (o, shp) in reg.items()}
    v["partial"] = ws[poff:total].view(np.float64).reshape(LAYERS, B, PARTS)
    return v


def ws_written(B, H, W):
    """bool per workspace byte: inside a region a call writes"""
    reg, poff, total = ws_layout(B, H, W)
    m = np.zeros(total, bool)
    for o, shp in reg.values():
        m[o:o + 4 * int(np.prod(shp))] = True
    m[poff:total] = True
    return m


def pack_layout():
    """(w [5] byte offsets of the hi matrices, elems [5], bias [5], lin [5], total): lp_layout(); lo lies right behind hi"""
    off, w, elems, bias, lin = 0, [], [], [], []
    for l in range(LAYERS):
        elems.append(KP[l] * COUT[l])
        w.append(off)
        off = rup(off + elems[l] * 2 * 2, 256)
    for dst in (bias, lin):
        for l in range(LAYERS):
            dst.append(off)
            off = rup(off + COUT[l] * 4, 256)
    return w, elems, bias, lin, off


def pack_decode(e, ntiles):
    """flat element e of a fragment matrix [kp/16][ntiles][64][8] -> (k, n): cf_pack_decode"""
    e = np.asarray(e, np.int64)
    frag, within = e // 512, e % 512
    lane, j = within >> 3, within & 7
    s, t = frag // ntiles, frag % ntiles
    return 16 * s + 8 * (lane >> 5) + j, 32 * t + (lane & 31)


def bf16_bits(a, truncate=False):
    """float32 -> the uint16 bits of its bf16 (round to nearest even, or truncated)"""
    a = np.ascontiguousarray(a, np.float32)
    if truncate:
        return (a.view(np.uint32) >> 16).astype(np.uint16)
    return torch.from_numpy(a).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def bits_to_f32(b):
    return (np.asarray(b, np.uint16).astype(np.uint32) << 16).view(np.float32)


@functools.lru_cache(maxsize=None)
def weights():
    """([(w [C_out, C_in, k, k], b, lin)] float32 numpy, the state dict) of synthetic.lpips_alex_state_dict(lr.WEIGHTS_SEED)"""
    from n3dt import synthetic as syn
    from n3dt.eval_utils import load_lpips_alex
    sd = syn.lpips_alex_state_dict(lr.WEIGHTS_SEED)
    return tuple(tuple(t.numpy() for t in layer) for layer in load_lpips_alex(sd)), sd


def weight_matrix(w):
    """B [kp, C_out] float32 with B[tap C_in + ci, co] = w[co, ci, ky, kx], rows k >= K zero"""
    co, ci, k, _ = w.shape
    m = np.ascontiguousarray(np.asarray(w, np.float32).transpose(2, 3, 1, 0)).reshape(k * k * ci, co)
    return np.concatenate([m, np.zeros((rup(m.shape[0], 16) - m.shape[0], co), np.float32)])


def expected_pack(W, nbytes=None, prefill=PREFILL, fault=None):
    """the packed buffer as bytes: hi = bf16_rne(w), lo = bf16_rne(w - hi) in fragment order, biases and lin copied, the rest prefill"""
    pw, elems, pb, pl, total = pack_layout()
    buf = np.full(total if nbytes is None else nbytes, prefill, np.uint8)
    for l, (w, b, lin) in enumerate(W):
        m = weight_matrix(w)
        k, n = pack_decode(np.arange(elems[l]), COUT[l] // 32)
        v = m[k, n]
        trunc = fault == "pack_trunc"
        hi = bf16_bits(v, trunc)
        lo = bf16_bits(v - bits_to_f32(hi), trunc)
        if fault == "pack_swap":
            hi, lo = lo, hi
        buf[pw[l]:pw[l] + 4 * elems[l]] = np.concatenate([hi, lo]).view(np.uint8)
        buf[pb[l]:pb[l] + 4 * COUT[l]] = np.ascontiguousarray(b, np.float32).view(np.uint8)
        buf[pl[l]:pl[l] + 4 * COUT[l]] = np.ascontiguousarray(lin, np.float32).view(np.uint8)
    return buf


def decode_pack(buf):
    """[(bhi [kp, C_out], blo, bias, lin)] float32 from the packed bytes, as the kernels read them"""
    pw, elems, pb, pl, _ = pack_layout()
    out = []
    for l in range(LAYERS):
        bits = buf[pw[l]:pw[l] + 4 * elems[l]].view(np.uint16)
        k, n = pack_decode(np.arange(elems[l]), COUT[l] // 32)
        hi, lo = np.zeros((KP[l], COUT[l]), np.float32), np.zeros((KP[l], COUT[l]), np.float32)
        hi[k, n], lo[k, n] = bits_to_f32(bits[:elems[l]]), bits_to_f32(bits[elems[l]:])
        out.append((hi, lo, buf[pb[l]:pb[l] + 4 * COUT[l]].view(np.float32).copy(), buf[pl[l]:pl[l] + 4 * COUT[l]].view(np.float32).copy()))
    return out


def judge_pack(buf, W):
    """None, or what is wrong with the packed bytes (pack buffer plus whatever the caller allocated behind it)"""
    pw, elems, _, _, total = pack_layout()
    want = expected_pack(W, len(buf))
    if np.array_equal(buf, want):
        return None
    j = int(np.flatnonzero(buf != want)[0])
    where = "behind the buffer" if j >= total else "bias / lin"
    for l in range(LAYERS):
        if pw[l] <= j < pw[l] + 4 * elems[l]:
            e = (j - pw[l]) // 2
            k, n = pack_decode(e % elems[l], COUT[l] // 32)
            where = "conv%d %s element %d = (k %d, n %d)" % (l + 1, "hi" if e < elems[l] else "lo", e % elems[l], k, n)
    return "pack: %d bytes differ, the first at %d (%s): got 0x%02x expected 0x%02x" % (int((buf != want).sum()), j, where, buf[j], want[j])


# ---------------------------------------------------------------------------------------------
# the inputs of the cases
# ---------------------------------------------------------------------------------------------
def _texture(case, mode, H, W):
    """(level [3, H, W], amplitude [H, W]) of the texture level +- amplitude.  odd: a quiet image (a level the scaling sends near 0,
    amplitude 6) except for full contrast in input rows 65, 66 and columns 57..60, which only relu1's row 15 and column 13 read --
    what pool1 drops -- and a flat stripe of colour ODD_STRIPE in columns 49..56, which reaches relu2 through pool1's column 5 alone:
    relu2's columns 3, 4, 5 then each see that one column through another tap column, and the stripe's colour is the one of
    the 6^3 grid at which column 5 -- what pool2 drops -- answers most."""
    level = np.full((3, H, W), 128, np.int64)
    if case != "odd":
        return level, np.full((H, W), 100, np.int64)
    level[:] = ODD_BASE[mode]
    level[:, :, 49:57] = np.asarray(ODD_STRIPE[mode]).reshape(3, 1, 1)
    amp = np.full((H, W), 6, np.int64)
    amp[65:, :] = 127
    amp[:, 57:] = 127
    level[:, amp == 127] = 128
    return level, amp


def fed_bytes(case, mode):
    """(a, b) uint8 [B, 3, H, W]: the byte images the NETWORK is to see (before the scaling), integer arithmetic only.  Pair 0 always
    differs; in `wide` pair 1 and in `cap` every pair b % 8 == 7 are identical images."""
    B, H, W = CASES[case]
    rng = np.random.default_rng(1000 + SEED[(case, mode)])
    level, amp = _texture(case, mode, H, W)
    sa = rng.integers(0, 2, (B, 3, H, W)) * 2 - 1
    flip = rng.integers(0, 4, (B, 3, H, W)) == 0            # a quarter of the signs differ between the two images
    jit = rng.integers(-5, 6, (B, 3, H, W))
    a = np.clip(level[None] + sa * amp[None, None], 0, 255)
    b = np.clip(level[None] + np.where(flip, -sa, sa) * amp[None, None] + jit, 0, 255)
    same = [i for i in range(B) if (case == "wide" and i == 1) or (case == "cap" and i % 8 == 7)]
    b[same] = a[same]
    return a.astype(np.uint8), b.astype(np.uint8)


SPECIALS = (np.nan, -0.0, -0.25, 1.5, 0.0, 1.0, np.inf, -np.inf, 100.75 / 255.0, 0.999)


def images(case, mode):
    """(pred, gt) float32 [B, 3, H, W], planar, as n3dt_lpips takes them.  standard: the fed bytes / 255; reference: the image whose
    quantised HWC bytes, reshaped (not transposed) to [3, H, W], are the fed bytes.  Pair 0 then gets NaN, -0.0, values below 0 and
    above 1, exactly 0 and 1, infinities and values between two bytes at fixed places of its upper left part."""
    B, H, W = CASES[case]
    out = []
    for fed in fed_bytes(case, mode):
        x = fed.astype(np.float32) / np.float32(255.0)
        if mode == "reference":
            f = np.arange(3 * H * W)
            src = np.empty((B, 3 * H * W), np.float32)
            src[:, (f % 3) * (H * W) + f // 3] = x.reshape(B, -1)
            x = src.reshape(B, 3, H, W)
        out.append(x)
    for i, img in enumerate(out):
        for j, v in enumerate(SPECIALS):
            img[0, (i + j) % 3, 3 + 2 * (j // 4) + i, 2 + 3 * (j % 4)] = v
    return out[0], out[1]


def identical_pairs(pred, gt):
    return [b for b in range(len(pred)) if np.array_equal(pred[b].view(np.uint32), gt[b].view(np.uint32))]


# ---------------------------------------------------------------------------------------------
# the stages
# ---------------------------------------------------------------------------------------------
def in0_expected(pred, gt, mode):
    """the prologue in float32 numpy: padded NHWC [2B, H + 4, W + 4, 3], halo +0"""
    x = np.concatenate([pred, gt]).astype(np.float32)
    n, _, H, W = x.shape
    if mode == "standard":
        u = np.where(x > 0, x, np.float32(0))               # negative, -0 and NaN
        u = np.where(u > 1, np.float32(1), u)
        u = np.float32(2) * u - np.float32(1)
    else:
        hwc = np.ascontiguousarray(quantise(x.transpose(0, 2, 3, 1)))
        u = hwc.reshape(n, 3, H, W).astype(np.float32)      # the reshape, not a transpose
    v = (u - SHIFT.reshape(1, 3, 1, 1)) / SCALE.reshape(1, 3, 1, 1)
    assert v.dtype == np.float32
    return np.pad(np.ascontiguousarray(v.transpose(0, 2, 3, 1)), ((0, 0), (2, 2), (2, 2), (0, 0)))


def conv_reference(xpad, l):
    """relu(b + sum w x) of the STORED padded input in float64 with the state dict's weights: (ref, S), NHWC interior"""
    w, b, _ = weights()[0][l]
    xt, wt, bt = vs._t(xpad, torch.float64), torch.from_numpy(w).double(), torch.from_numpy(b).double()
    ref = F.relu(F.conv2d(xt, wt, bt, stride=STRIDE[l]))
    S = F.conv2d(xt.abs(), wt.abs(), bt.abs(), stride=STRIDE[l])
    return vs._n(ref), vs._n(S)


def out_extent(l, xpad):
    return (xpad.shape[1] - KSIZE[l]) // STRIDE[l] + 1, (xpad.shape[2] - KSIZE[l]) // STRIDE[l] + 1


def im2col(xpad, l, fault=None):
    """[n Ho Wo, kp] float32, column k = tap C_in + ci (conv1: tap 3 + ci), columns k >= K zero"""
    k, s = KSIZE[l], STRIDE[l]
    n = xpad.shape[0]
    Ho, Wo = out_extent(l, xpad)
    taps = []
    for ky in range(k):
        for kx in range(k):
            yy = ky - 1 if fault == "tap_row" and ky == kx == k - 1 else ky     # the last tap's row offset one row off
            taps.append(xpad[:, yy:yy + s * (Ho - 1) + 1:s, kx:kx + s * (Wo - 1) + 1:s, :])
    cols = np.concatenate(taps, axis=-1).reshape(n * Ho * Wo, K[l])
    extra = np.zeros((cols.shape[0], KP[l] - K[l]), np.float32)
    if fault == "gather_363" and l == 0:                    # k = 363..367 taken as live: "tap" 121.. = row 11 of the field
        flat = np.concatenate([xpad.reshape(-1), np.zeros(16 * xpad.shape[2] * 3, np.float32)])
        img, y, x = np.unravel_index(np.arange(cols.shape[0]), (n, Ho, Wo))
        base = ((img * xpad.shape[1] + y * s) * xpad.shape[2] + x * s) * 3
        for j in range(KP[0] - K[0]):
            kk = K[0] + j
            tap, ci = kk // 3, kk % 3
            extra[:, j] = flat[base + ((tap // k) * xpad.shape[2] + tap % k) * 3 + ci]
    return np.concatenate([cols, extra], axis=1)


def conv_seq16(cols, bhi, blo, descending=False, fault=None, drop=None):
    """the conv kernels' loop in float32: per K step of 16 the products alo bhi, ahi blo, ahi bhi, each step's 16-term dot product
    added to a float32 accumulator.  drop = (rows, columns): the wave tile whose last K step is left out."""
    ahi, alo = (a.astype(np.float64) for a in vs.hi_lo(cols))
    bhi, blo = bhi.astype(np.float64), blo.astype(np.float64)
    acc = np.zeros((cols.shape[0], bhi.shape[1]), np.float32)
    steps = list(range(cols.shape[1] // 16))
    for s in (reversed(steps) if descending else steps):
        k = slice(16 * s, 16 * s + 16)
        prods = []
        if fault != "no_lo_hi":
            prods.append(alo[:, k] @ bhi[k])
        if fault != "no_hi_lo":
            prods.append(ahi[:, k] @ blo[k])
        prods.append(ahi[:, k] @ bhi[k])
        for p in prods:
            p = p.astype(np.float32)
            if drop is not None and s == steps[-1]:
                p[drop[0], drop[1]] = 0
            acc = acc + p
    return acc


def conv_torch32(xpad, l):
    """the same three split products through torch's float32 convolution (another accumulation order), weights split from fp32"""
    w = weights()[0][l][0]
    (ahi, alo), (whi, wlo) = vs.hi_lo(xpad), vs.hi_lo(w)
    f = lambda a, b: F.conv2d(vs._t(a, torch.float32), torch.from_numpy(b), stride=STRIDE[l])
    out = vs._n((f(alo, whi) + f(ahi, wlo)) + f(ahi, whi))
    return out.reshape(-1, COUT[l])


def epilogue(acc, bias, fault=None):
    if fault == "bias_odd_tile":                           # the bias of column co - 32 in the odd column tile
        co = np.arange(len(bias))
        bias = bias[np.where((co // 32) % 2 == 1, co - 32, co)]
    return np.maximum(acc + bias[None, :].astype(np.float32), np.float32(0))


def pool_expected(relu, fault=None):
    """the 3 x 3 / 2 maximum of a stored relu map [n, Hi, Wi, C] (interior, float32)"""
    n, Hi, Wi, C = relu.shape
    Ho, Wo = (Hi - 3) // 2 + 1, (Wi - 3) // 2 + 1
    o = 1 if fault == "pool_shift" else 0                  # the window one to the right and down where the map has room
    oy, ox = (o if 2 * (Ho - 1) + 2 + o < Hi else 0), (o if 2 * (Wo - 1) + 2 + o < Wi else 0)
    out = None
    for dy in range(3):
        for dx in range(3):
            q = relu[:, oy + dy:oy + dy + 2 * (Ho - 1) + 1:2, ox + dx:ox + dx + 2 * (Wo - 1) + 1:2, :]
            out = q.copy() if out is None else np.maximum(out, q)
    return out


def part_of_pixel(npix, fault=None):
    """the partial a pixel's term is added to, -1 for none: workgroup p, wave w takes i = 4 p + w + 512 t"""
    i = np.arange(npix) % (4 * PARTS)
    if fault == "part_wave":                               # wave w takes 4 p + w + 1
        return (i - 1) // 4
    return i // 4


def pixel_terms(f0, f1, lin, eps=EPS):
    """(d, S) per pixel of interior maps [h, w, C] in float64: d = sum_c w_c (n0_c - n1_c)^2, S = sum_c |w_c| (|n0_c| + |n1_c|)^2"""
    f0, f1, w = (np.asarray(a, np.float64) for a in (f0, f1, lin))
    with np.errstate(invalid="ignore", divide="ignore"):
        n0 = f0 / (np.sqrt((f0 * f0).sum(-1, keepdims=True)) + eps)
        n1 = f1 / (np.sqrt((f1 * f1).sum(-1, keepdims=True)) + eps)
    d = (w * (n0 - n1) ** 2).sum(-1).reshape(-1)
    S = (np.abs(w) * (np.abs(n0) + np.abs(n1)) ** 2).sum(-1).reshape(-1)
    return d, S


def interior(name, m):
    p = PAD[name]
    return m[:, p:m.shape[1] - p, p:m.shape[2] - p, :] if p else m


def partials_reference(feat, B, lin, fault=None):
    """(ref [B, 128], S [B, 128], owns [128]) of an interior relu map [2B, h, w, C]"""
    npix = feat.shape[1] * feat.shape[2]
    part = part_of_pixel(npix, fault)
    ref, S = np.zeros((B, PARTS)), np.zeros((B, PARTS))
    for b in range(B):
        second = B + b - 1 if fault == "pair_prev" else B + b
        d, s = pixel_terms(feat[b], feat[second], lin, 0.0 if fault == "no_eps" else EPS)
        ok = part >= 0
        ref[b] = np.bincount(part[ok], weights=d[ok], minlength=PARTS)
        S[b] = np.bincount(part[ok], weights=s[ok], minlength=PARTS)
    return ref, S, np.bincount(part[part >= 0], minlength=PARTS) > 0


def seq_sum(v):
    s = 0.0
    for x in v:
        s = s + float(x)
    return s


def finish(partial, npix, fault=None):
    """(out [B], layers [5, B]) float64 from the stored partials [5, B, 128]: sequential sums in index order"""
    B = partial.shape[1]
    layers = np.array([[seq_sum(partial[l, b]) / float(npix[l]) for b in range(B)] for l in range(LAYERS)])
    if fault == "layer_order":
        out = np.array([(((layers[4, b] + layers[3, b]) + layers[2, b]) + layers[1, b]) + layers[0, b] for b in range(B)])
    else:
        out = np.array([(((layers[0, b] + layers[1, b]) + layers[2, b]) + layers[3, b]) + layers[4, b] for b in range(B)])
    return out, layers


# ---------------------------------------------------------------------------------------------
# the emulated chain: a synthetic workspace and pack buffer
# ---------------------------------------------------------------------------------------------
FAULTS = collections.OrderedDict((
    ("kdrop_conv5", "conv5"), ("kdrop_conv2", "conv2"), ("bias_odd_tile", "conv"), ("no_lo_hi", "conv"), ("no_hi_lo", "conv"),
    ("tap_row", "conv"), ("row_past_M", "relu4 halo"), ("gather_363", None), ("pool_shift", "pool"), ("pool_halo", "pool"),
    ("relu3_halo_cell", "relu3 halo"), ("part_wave", "partials"), ("pair_prev", "partials"), ("no_eps", "partials"),
    ("layer_order", "out"), ("pack_swap", "pack"), ("pack_trunc", "pack")))
# faults no rule can see, with the reason; test_lpips_stagewise_cpu.py asserts that they stay invisible
INDISTINGUISHABLE = {
    "gather_363": "the packed rows 363..367 are +0 (held byte for byte) and in0 is finite, so the extra products are exactly 0",
}


def emulate(case, mode, prefill=PREFILL, fault=None, measure=None):
    """(workspace bytes, pack bytes, out [B], layers [5, B]) of the float32 emulation of the whole chain.  measure: a list that
    receives (layer, largest |emulated - ref| / S over the three accumulation forms), teacher-forced on this chain's own maps."""
    B, H, W = CASES[case]
    Wt = weights()[0]
    pred, gt = images(case, mode)
    reg, poff, total = ws_layout(B, H, W)
    ws = np.full(total, prefill, np.uint8)
    v = ws_views(ws, B, H, W)
    pack = expected_pack(Wt, fault=fault)
    dec = decode_pack(pack)
    v["in0"][...] = in0_expected(pred, gt, mode)
    for l in range(LAYERS):
        if l in (1, 2):
            name = "pool%d" % l
            if fault != "pool_halo":
                v[name][...] = 0
            interior(name, v[name])[...] = pool_expected(v["relu%d" % l], fault)
        if l == 2:
            for name in ("relu3", "relu4"):
                keep = v[name][-1, -1, -1, :].copy()
                v[name][...] = 0
                if fault == "relu3_halo_cell" and name == "relu3":
                    v[name][-1, -1, -1, :] = keep
        xpad = v[CONV_IN[l]]
        bhi, blo, bias, _ = dec[l]
        cols = im2col(xpad, l, fault)
        drop = (slice(0, 64), slice(0, 64)) if fault == "kdrop_conv%d" % (l + 1) else None
        got = epilogue(conv_seq16(cols, bhi, blo, fault=fault, drop=drop), bias, fault)
        dst = interior(RELU[l], v[RELU[l]])
        if fault == "row_past_M":                           # row M (the clamped pixel M - 1 again) stored at its unclamped address:
            _, Hp, Wp, C = reg[RELU[l]][1]                  # pixel (0, 0) of an image behind the last one (lp_out_pixel)
            p = PAD[RELU[l]]
            o = reg[RELU[l]][0] + 4 * (((xpad.shape[0] * Hp + p) * Wp + p) * C)
            ws[o:o + 4 * C] = np.ascontiguousarray(got[-1]).view(np.uint8)
        dst[...] = got.reshape(dst.shape)
        if measure is not None:
            ref, S = conv_reference(xpad, l)
            forms = (got, epilogue(conv_seq16(cols, bhi, blo, descending=True), bias), epilogue(conv_torch32(xpad, l), bias))
            measure.append((l, max(float(vs.ratio(g.reshape(ref.shape), ref, S).max()) for g in forms)))
    npix = []
    for l in range(LAYERS):
        feat = interior(RELU[l], v[RELU[l]])
        v["partial"][l] = partials_reference(feat, B, dec[l][3], fault)[0]
        npix.append(feat.shape[1] * feat.shape[2])
    out, layers = finish(v["partial"], npix, fault)
    return ws, pack, out, layers


# ---------------------------------------------------------------------------------------------
# the rules
# ---------------------------------------------------------------------------------------------
def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(u), b.view(u))


def halo_is_plus_zero(name, m):
    q = np.array(m, copy=True)
    interior(name, q)[...] = 0
    return not q.view(np.uint32).any()


def dropped_hold_the_largest(v):
    """odd: None, or what is wrong -- relu1's last row and column and relu2's last column, which no pool window reaches, must each
    hold values above everything the pools do read"""
    r1, r2 = v["relu1"], v["relu2"]
    kept1, kept2 = float(r1[:, :15, :13].max()), float(r2[:, :, :5].max())
    got = (("relu1 row 15", float(r1[:, 15].max()), kept1), ("relu1 column 13", float(r1[:, :, 13].max()), kept1),
           ("relu2 column 5", float(r2[:, :, 5].max()), kept2))
    bad = ["%s holds at most %.6g, the pooled part %.6g" % g for g in got if not g[1] > g[2]]
    return "; ".join(bad) if bad else None


def judge(case, mode, ws, out, layers, prefill=PREFILL):
    """Every rule on one call's workspace (uint8), out [B] and layers [5, B].  Returns (worst, fails): worst maps a family to its
    largest error / bound (exact rules: 0 or inf), fails is a list of (rule, message)."""
    B, H, W = CASES[case]
    Wt = weights()[0]
    pred, gt = images(case, mode)
    reg, poff, total = ws_layout(B, H, W)
    ws = np.asarray(ws)
    v = ws_views(ws, B, H, W)
    worst, fails = collections.OrderedDict(), []

    def exact(rule, ok, msg):
        worst[rule] = max(worst.get(rule, 0.0), 0.0 if ok else np.inf)
        if not ok:
            fails.append((rule, "%s %s %s: %s" % (case, mode, rule, msg)))

    want = in0_expected(pred, gt, mode)
    exact("in0", same_bits(interior("in0", v["in0"]), interior("in0", want)),
          "%d interior floats differ from float32 (u - shift) / scale" % int((interior("in0", v["in0"]).view(np.uint32) != interior("in0", want).view(np.uint32)).sum()))
    exact("in0 halo", halo_is_plus_zero("in0", v["in0"]), "the halo is not +0")
    for l in range(LAYERS):
        if l in (1, 2):
            name, src = "pool%d" % l, v["relu%d" % l]
            exact(name, same_bits(interior(name, v[name]), pool_expected(src)), "not the 3 x 3 / 2 maximum of the stored relu%d" % l)
            exact(name + " halo", halo_is_plus_zero(name, v[name]), "the halo is not +0")
        ref, S = conv_reference(v[CONV_IN[l]], l)
        rule = "conv%d" % (l + 1)
        w, msg = vs.compare(interior(RELU[l], v[RELU[l]]), ref, S, bound(l), "%s %s %s from the stored %s" % (case, mode, rule, CONV_IN[l]))
        worst[rule] = w / bound(l)
        if msg:
            fails.append((rule, msg))
        if PAD[RELU[l]]:
            exact(RELU[l] + " halo", halo_is_plus_zero(RELU[l], v[RELU[l]]), "the halo is not +0")
    same = identical_pairs(pred, gt)
    npix, wp = [], 0.0
    for l in range(LAYERS):
        feat = interior(RELU[l], v[RELU[l]])
        npix.append(feat.shape[1] * feat.shape[2])
        ref, S, owns = partials_reference(feat, B, Wt[l][2])
        got = v["partial"][l]
        w, msg = vs.compare(got, ref, S, PARTIAL_BOUND, "%s %s partials of layer %d [pair, part]" % (case, mode, l))
        wp = max(wp, w / PARTIAL_BOUND)
        if msg:
            fails.append(("partials", msg))
        exact("partials empty", not got[:, ~owns].view(np.uint64).any(), "layer %d: a part that owns no pixel is not +0" % l)
        exact("identical", not got[same].view(np.uint64).any(), "layer %d: an identical pair has a partial that is not +0" % l)
    worst["partials"] = wp
    want_out, want_layers = finish(v["partial"], npix)
    exact("layers", same_bits(np.asarray(layers, np.float64), want_layers), "not the sequential sum of the stored partials / pixels")
    exact("out", same_bits(np.asarray(out, np.float64), want_out), "not (((l0 + l1) + l2) + l3) + l4 of the stored partials")
    free = ~ws_written(B, H, W)
    exact("untouched", bool(np.all(ws[:total][free] == prefill)) and bool(np.all(ws[total:] == prefill)),
          "a byte outside the regions lost the prefill")
    if case == "odd":
        msg = dropped_hold_the_largest(v)
        exact("dropped rows", msg is None, msg)
    return worst, fails


def same_results(ws_a, ws_b, B, H, W):
    """None, or the first map / partial that differs in bits between two workspaces of one call (read-before-write)"""
    a, b = ws_views(ws_a, B, H, W), ws_views(ws_b, B, H, W)
    for name in a:
        if not same_bits(a[name], b[name]):
            return name
    return None


@functools.lru_cache(maxsize=None)
def restated(case, mode):
    """(score [B], layers [5, B]) of the free-running float64 restatement (lpips_restatement), what test_gpu_lpips.py compares with"""
    pred, gt = images(case, mode)
    return lr.lpips_batch(pred, gt, weights()[1], mode)


def old_bounds_report(case, mode, out, layers):
    """would test_gpu_lpips.py's relative bounds on the score and the layer values have reported this result?"""
    s, l = restated(case, mode)
    with np.errstate(invalid="ignore", divide="ignore"):
        es = np.abs(np.asarray(out) - s) / s
        el = np.abs(np.asarray(layers) - l) / l
    es, el = es[s > 0], el[l > 0]
    bad = not np.all(np.isfinite(out)) or not np.all(np.isfinite(layers))
    return bool(bad or (es.size and es.max() > OLD_SCORE_TOL) or (el.size and el.max() > OLD_LAYER_TOL))
