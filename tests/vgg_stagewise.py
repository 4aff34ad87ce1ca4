"""Float64 restatement of csrc/vgg_loss.hip BY STAGE, for the stage-wise pins of the VGG perceptual term (test_vgg_stagewise_cpu.py,
test_gpu_vgg_stagewise.py).  CPU only, numpy / torch.

Every discontinuity of the term's gradient -- the L1 sign at a block end, a ReLU gate, a pool arg-max -- is a function of `saved`,
the activations the forward hands to the caller and the backward takes back.  Read from that buffer, the backward is LINEAR in g,
and the float64 restatement below with the same gates is an exact reference: no gate band, every entry compared.

  layout      saved_maps / build_saved / workspace_views mirror act_ptr / act_floats / fwd_ws_floats of vgg_loss.hip: ten padded NHWC
              maps [2B, H+2, W+2, C] (predictions first), each segment rounded up to 64 floats; in0 [2B, 226, 226, 3] and the 4 x 256
              L1 partials at the front of the forward workspace
  forward     prologue, conv_stage (conv + bias + ReLU, optional 2x2 max-pool on its input), l1_terms -- each a function of its input
  backward    junction, dgrad, resize_adjoint, composed by backward(), which returns every intermediate
  emulation   the kernels' arithmetic in float32, only to MEASURE floors: operands split hi = bf16_rne(x), lo = bf16_rne(x - hi),
              products hi hi + hi lo + lo hi (fp32 mode) or hi hi alone (bf16 mode), float32 accumulation.  conv_seq16 accumulates K in
              steps of 16 as the MFMA loop does (small geometries); conv_emulated is the same products through torch's float32
              convolution (the 224^2 maps).  Bitwise agreement with the MFMA is not the aim.

Comparison rule (nr_restatement.compare's): per entry |got - ref| <= bound x S; where S == 0 the two must be equal.
  conv stage   S = sum |a| |w| + |bias|, a float64 convolution of absolute values
  prologue     S = the same bilinear taps over (|u| + |mean|) / std
  terms        S = the term (a sum of non-negative entries)
  d_merge      no single dot product: per entry relative to max |ref|, and relative L2
bf16 mode: the reference rounds BOTH operands to bf16 (RNE) first -- forward: activation and weight; backward: incoming gradient and
weight -- so what is left is accumulation error only.

A GPU bound is MARGIN = 4 x the floor of its stage family and precision (the MFMA's accumulation order is not the emulation's).  The
floors are the constants FLOOR below; test_vgg_stagewise_cpu.py re-measures them on the CPU and fails if one has moved up.  No bound
comes from a GPU run."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

CIN = (3, 64, 64, 128, 128, 256, 256, 256, 512, 512)        # vgg_loss.hip: kCin
COUT = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512)     # kCout
SIDE = (224, 224, 112, 112, 56, 56, 56, 28, 28, 28)         # kH
POOL_IN = (False, False, True, False, True, False, False, True, False, False)   # kPoolIn
BLOCK_END = (1, 3, 6, 9)                                    # kBlockEnd
S224 = 224
L1_BLOCKS = 256
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
FLT_MAX = float(np.finfo(np.float32).max)
MARGIN = 4.0
PRECISIONS = ("fp32", "bf16")
WEIGHTS_SEED = 5

# (n_img, H, W) of the single-stage cases: M = 70 (the ragged second 32-row tile of one wave, H != W), M = 360 (crosses a workgroup,
# idle waves), M = 256 exactly, and a map whose every pixel is border.  Layers 2, 4, 7 read the un-pooled (2H, 2W) input.
STAGE_GEOMETRIES = ((2, 5, 7), (3, 12, 10), (1, 16, 16), (2, 1, 3))
RESIZE_SIZES = (16, 100, 224, 225, 512, 1000)
PRODUCTION = {"B": 1, "P": 64, "seed": 31, "g_total": 0.37, "bg": 1.0}
CRAFTED = ("block0", "block1", "block2", "block3", "ties", "scattered")

# Floors: the emulation's largest error under the comparison rule, per stage family and precision, over every case the GPU tests
# use (test_vgg_stagewise_cpu.py::test_floors_have_not_moved_up prints and re-checks them).  d_merge: (per entry / max |ref|, L2).
FLOOR = {
    "fp32": {"prologue": 7.5e-6, "conv_fwd": 8.4e-6, "conv_dgrad": 1.9e-6, "terms": 6.7e-8, "d_merge_max": 6.8e-5, "d_merge_l2": 5.7e-5},
    "bf16": {"prologue": 7.5e-6, "conv_fwd": 2.6e-7, "conv_dgrad": 8.4e-8, "terms": 6.7e-8, "d_merge_max": 4.4e-3, "d_merge_l2": 4.0e-3},
}


def bound(prec, family):
    return MARGIN * FLOOR[prec][family]


# ---------------------------------------------------------------------------------------------
# layout
# ---------------------------------------------------------------------------------------------
def rup64(n):
    return (n + 63) // 64 * 64


def act_floats(n_img, l):
    return n_img * (SIDE[l] + 2) * (SIDE[l] + 2) * COUT[l]


def saved_offsets(B):
    """(offset of map l in floats for l = 0..9, total floats): act_ptr / n3dt_vgg_saved_floats"""
    off, t = [], 0
    for l in range(10):
        off.append(t)
        t += rup64(act_floats(2 * B, l))
    return off, t


def saved_maps(saved, B):
    """the ten PADDED maps [2B, H+2, W+2, C] as views of the flat float32 `saved`"""
    saved = np.asarray(saved).reshape(-1)
    off, total = saved_offsets(B)
    assert saved.dtype == np.float32 and saved.size >= total, (saved.dtype, saved.size, total)
    return [saved[off[l]:off[l] + act_floats(2 * B, l)].reshape(2 * B, SIDE[l] + 2, SIDE[l] + 2, COUT[l]) for l in range(10)]


def interior(p):
    return p[:, 1:-1, 1:-1, :]


def padded(a):
    return np.pad(a, ((0, 0), (1, 1), (1, 1), (0, 0)))


def halo_is_zero(p):
    q = np.array(p, copy=True)
    q[:, 1:-1, 1:-1, :] = 0
    return not q.any()


def build_saved(maps, B):
    """a flat float32 `saved` from ten interior maps [2B, H, W, C]: halo zero, segments rounded up to 64 floats"""
    off, total = saved_offsets(B)
    out = np.zeros(total, np.float32)
    for l, m in enumerate(maps):
        assert m.shape == (2 * B, SIDE[l], SIDE[l], COUT[l]), (l, m.shape)
        out[off[l]:off[l] + act_floats(2 * B, l)] = padded(np.asarray(m, np.float32)).reshape(-1)
    return out


def workspace_views(ws, B):
    """(in0 [2B, 226, 226, 3] padded, partials [4, 256]) from the front of the forward workspace (float32)"""
    ws = np.asarray(ws).reshape(-1)
    n = 2 * B * (S224 + 2) * (S224 + 2) * 3
    return ws[:n].reshape(2 * B, S224 + 2, S224 + 2, 3), ws[rup64(n):rup64(n) + 4 * L1_BLOCKS].reshape(4, L1_BLOCKS)


# ---------------------------------------------------------------------------------------------
# small helpers
# ---------------------------------------------------------------------------------------------
def bf16_rne(a):
    """round to bf16 (nearest even), returned in a's dtype"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype).numpy()


def ident(a):
    return a


def _t(a, dtype):
    """NHWC numpy -> NCHW torch"""
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).permute(0, 3, 1, 2)


def _n(t):
    """NCHW torch -> NHWC numpy"""
    return t.permute(0, 2, 3, 1).contiguous().numpy()


@functools.lru_cache(maxsize=None)
def weights(seed=WEIGHTS_SEED):
    """the ten (w [C_out, C_in, 3, 3], b [C_out]) float32 numpy pairs of synthetic.vgg16_features_state_dict(seed), and the state dict"""
    from n3dt import synthetic as syn
    from n3dt.perceptual import load_vgg16_features
    sd = syn.vgg16_features_state_dict(seed)
    return tuple((w.numpy(), b.numpy()) for w, b in load_vgg16_features(sd)), sd


def pool2(x):
    n, h, w, c = x.shape
    return x.reshape(n, h // 2, 2, w // 2, 2, c).max(axis=(2, 4))


# ---------------------------------------------------------------------------------------------
# forward stages
# ---------------------------------------------------------------------------------------------
def src_index(n_out, n_in, dt=np.float64):
    """PyTorch's upsample_bilinear2d source index, align_corners=False (vgg_src_index): i0, i1, l0, l1 per output index"""
    scale = dt(n_in) / dt(n_out)
    src = scale * (np.arange(n_out).astype(dt) + dt(0.5)) - dt(0.5)
    src = np.maximum(src, dt(0))
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = np.clip(src - i0.astype(dt), dt(0), dt(1))
    return i0, i1, dt(1) - l1, l1


def resize_matrix(P, dt=np.float64):
    """A [224, P]: resized = A @ image @ A.T along each axis"""
    i0, i1, l0, l1 = src_index(S224, P, dt)
    A = np.zeros((S224, P), dt)
    np.add.at(A, (np.arange(S224), i0), l0)
    np.add.at(A, (np.arange(S224), i1), l1)
    return A


def _bilinear(v, dt):
    """v [n, 3, P, P] -> [n, 224, 224, 3] in the kernel's association hy0 (wx0 a + wx1 b) + hy1 (wx0 c + wx1 d)"""
    P = v.shape[-1]
    i0, i1, l0, l1 = src_index(S224, P, dt)
    hy0, hy1 = l0[None, None, :, None], l1[None, None, :, None]
    wx0, wx1 = l0[None, None, None, :], l1[None, None, None, :]
    r0, r1 = v[:, :, i0, :], v[:, :, i1, :]
    out = hy0 * (wx0 * r0[:, :, :, i0] + wx1 * r0[:, :, :, i1]) + hy1 * (wx0 * r1[:, :, :, i0] + wx1 * r1[:, :, :, i1])
    return np.ascontiguousarray(out.transpose(0, 2, 3, 1))


def prologue(merge, gt, mask, bg, dt=np.float64, mag=False):
    """in0 interior [2B, 224, 224, 3]: nan_to_num(merge) and gt with bg where mask < 0.5, normalised, bilinear to 224^2.  dt=float32
    is the kernel's arithmetic.  mag: S of the comparison rule instead (the taps over (|u| + |mean|) / std)."""
    x = np.nan_to_num(np.asarray(merge, np.float32), nan=0.0, posinf=FLT_MAX, neginf=-FLT_MAX).astype(dt)
    y = np.asarray(gt, np.float32).astype(dt)
    if mask is not None:
        y = np.where(np.asarray(mask, np.float32) >= 0.5, y, dt(bg))
    u = np.concatenate([x, y], axis=0)
    mean, std = (np.asarray(c, np.float32).astype(dt).reshape(1, 3, 1, 1) for c in (MEAN, STD))   # float32 constants, as the reference's
    v = (np.abs(u) + np.abs(mean)) / std if mag else (u - mean) / std
    return _bilinear(v.astype(dt), dt)


def conv_stage(x, w, b, pool_in=False, q=ident):
    """ReLU(conv3x3(pad 1) + bias) of an interior NHWC map in float64; pool_in: a 2x2 max-pool on x first.  q rounds both operands
    (bf16 mode).  Returns (out, S) with S = sum |a| |w| + |bias|."""
    x = np.asarray(x, np.float64)
    if pool_in:
        x = pool2(x)
    xt, wt = _t(q(x), torch.float64), torch.from_numpy(q(np.asarray(w, np.float64)))
    bt = torch.from_numpy(np.asarray(b, np.float64))
    out = F.relu(F.conv2d(xt, wt, bt, padding=1))
    S = F.conv2d(xt.abs(), wt.abs(), bt.abs(), padding=1)
    return _n(out), _n(S)


def l1_terms(ends, B):
    """[t0, t1, t2, t3, ((t0 + t1) + t2) + t3] of the four block-end maps [2B, H, W, C] in float64"""
    t = [float(np.abs(np.asarray(m[:B], np.float64) - np.asarray(m[B:], np.float64)).mean()) for m in ends]
    return np.array(t + [((t[0] + t[1]) + t[2]) + t[3]])


def forward(merge, gt, mask, bg, W, q=ident):
    """the stages composed: (in0, the ten maps, terms[5]), all float64"""
    x = prologue(merge, gt, mask, bg)
    B = x.shape[0] // 2
    in0, maps = x, []
    for l in range(10):
        x, _ = conv_stage(x, W[l][0], W[l][1], POOL_IN[l], q)
        maps.append(x)
    return in0, maps, l1_terms([maps[l] for l in BLOCK_END], B)


# ---------------------------------------------------------------------------------------------
# gate-forced backward
# ---------------------------------------------------------------------------------------------
def route_pool(dpool, x):
    """the adjoint of max_pool2d(x, 2, 2) with PyTorch's arg-max: the FIRST maximum of each window in row-major order (the kernel's
    strict `>` scan).  dpool [B, h, w, C], x [B, 2h, 2w, C] -> [B, 2h, 2w, C]"""
    B, H, Wd, C = x.shape
    h, w = H // 2, Wd // 2
    v = x.reshape(B, h, 2, w, 2, C).transpose(0, 1, 3, 5, 2, 4).reshape(B, h, w, C, 4)
    am = np.argmax(v, axis=-1)     # numpy: the first occurrence
    out = np.zeros((B, h, w, C, 4), dpool.dtype)
    np.put_along_axis(out, am[..., None], dpool[..., None], axis=-1)
    return np.ascontiguousarray(out.reshape(B, h, w, C, 2, 2).transpose(0, 1, 4, 2, 5, 3)).reshape(B, H, Wd, C)


def junction(act, dpool, g, B, dt=np.float64):
    """dZ of a block-end conv from its stored map [2B, H, W, C]: (x > 0) (g sign(x - y) / N_b + the routed pooled gradient)"""
    x, y = act[:B], act[B:]
    N = float(x.size)
    gs = dt(g) * dt(1.0 / N) if dt == np.float32 else g / N
    d = (gs * np.sign(x.astype(np.float64) - y.astype(np.float64))).astype(dt)
    if dpool is not None:
        d = d + route_pool(dpool.astype(dt), x)
    return np.where(x > 0, d, dt(0))


def dgrad(dz, w, gate=None, q=ident):
    """the input gradient of conv3x3(pad 1) in float64 (conv_transpose2d), kept where gate > 0.  q rounds the incoming gradient and
    the weights (bf16 mode).  Returns (d_in, S)."""
    dt_, wt = _t(q(np.asarray(dz, np.float64)), torch.float64), torch.from_numpy(q(np.asarray(w, np.float64)))
    d = _n(F.conv_transpose2d(dt_, wt, padding=1))
    S = _n(F.conv_transpose2d(dt_.abs(), wt.abs(), padding=1))
    if gate is not None:
        d = np.where(np.asarray(gate) > 0, d, 0.0)
    return d, S


def resize_adjoint(d_in0, merge, dt=np.float64):
    """d_merge [B, 3, P, P] from d_in0 [B, 224, 224, 3]: the adjoint of the bilinear resize, 1 / std, 0 where merge is not finite"""
    merge = np.asarray(merge)
    A = resize_matrix(merge.shape[-1], dt)
    std = np.asarray(STD, np.float32).astype(dt)
    d = np.einsum("oy,bopc,px->bcyx", A, np.asarray(d_in0, dt), A, optimize=True).astype(dt) / std.reshape(1, 3, 1, 1)
    return np.where(np.isfinite(merge), d, dt(0))


def backward(maps, W, g, merge, q=ident, conv_adj=None, dt=np.float64):
    """The backward with every gate, sign and arg-max read from `maps` (ten interior maps [2B, H, W, C], as stored).  Returns
    {"dz<l>": gradient of conv l's output, "dpool<b>": the pooled gradient entering block b's end from block b + 1, "d_in0",
    "d_merge"}.  conv_adj(dz, w) replaces the float64 dgrad (the emulations); dt is the junction's and the resize's arithmetic."""
    B = maps[0].shape[0] // 2
    out, dpool = {}, None
    for b in (3, 2, 1, 0):
        le = BLOCK_END[b]
        lfirst = 0 if b == 0 else BLOCK_END[b - 1] + 1
        dz = junction(maps[le], dpool, g, B, dt)
        if dpool is not None:
            out["dpool%d" % b] = dpool
        for l in range(le, lfirst - 1, -1):
            out["dz%d" % l] = dz
            d = dgrad(dz, W[l][0], None, q)[0] if conv_adj is None else conv_adj(dz, W[l][0])
            if l > lfirst:
                dz = np.where(maps[l - 1][:B] > 0, d, dt(0)).astype(dt)
            else:
                dpool = d.astype(dt)
    out["d_in0"] = dpool
    out["d_merge"] = resize_adjoint(dpool, merge, dt)
    return out


# ---------------------------------------------------------------------------------------------
# the kernels' arithmetic, in float32 (floors only)
# ---------------------------------------------------------------------------------------------
def hi_lo(a):
    a = np.asarray(a, np.float32)
    hi = bf16_rne(a)
    return hi, bf16_rne(a - hi)


def conv_emulated(x, w, prec, transpose=False):
    """x interior NHWC float32, w [C_out, C_in, 3, 3] -> the three (fp32) or one (bf16) products through torch's float32 convolution"""
    f = F.conv_transpose2d if transpose else F.conv2d
    ahi, alo = hi_lo(x)
    whi, wlo = hi_lo(w)
    A, Wh = _t(ahi, torch.float32), torch.from_numpy(whi)
    out = f(A, Wh, padding=1)
    if prec == "fp32":
        out = (f(_t(alo, torch.float32), Wh, padding=1) + f(A, torch.from_numpy(wlo), padding=1)) + out
    return _n(out)


def weight_matrix(w, transpose=False):
    """the B matrix of the implicit GEMM: forward [tap C_in + ci, co] = w[co, ci, ky, kx]; dgrad [tap C_out + co, ci] =
    w[co, ci, 2 - ky, 2 - kx] (the pack's layout, unpadded)"""
    w = np.asarray(w)
    co, ci = w.shape[:2]
    if not transpose:
        return np.ascontiguousarray(w.transpose(2, 3, 1, 0)).reshape(9 * ci, co)
    return np.ascontiguousarray(w[:, :, ::-1, ::-1].transpose(2, 3, 0, 1)).reshape(9 * co, ci)


def conv_seq16(x, w, prec, transpose=False):
    """the conv kernel's loop: K = 9 C in steps of 16 (k = tap C + c), per step alo bhi, ahi blo, ahi bhi (fp32) or ahi bhi (bf16),
    each step's 16-term dot product added to a float32 accumulator.  x interior NHWC; small geometries only (im2col)."""
    xp = padded(np.asarray(x, np.float32))
    n, H, Wd, C = x.shape
    cols = np.concatenate([xp[:, ky:ky + H, kx:kx + Wd, :] for ky in range(3) for kx in range(3)], axis=-1).reshape(n * H * Wd, 9 * C)
    Bm = weight_matrix(np.asarray(w, np.float32), transpose)
    ahi, alo = (a.astype(np.float64) for a in hi_lo(cols))
    bhi, blo = (a.astype(np.float64) for a in hi_lo(Bm))
    acc = np.zeros((cols.shape[0], Bm.shape[1]), np.float32)
    for k in range(0, 9 * C, 16):
        s = slice(k, k + 16)
        if prec == "fp32":
            acc = acc + (alo[:, s] @ bhi[s]).astype(np.float32)
            acc = acc + (ahi[:, s] @ blo[s]).astype(np.float32)
        acc = acc + (ahi[:, s] @ bhi[s]).astype(np.float32)
    return acc.reshape(n, H, Wd, -1)


def conv_stage_emulated(x, w, b, pool_in, prec, conv=conv_seq16):
    x = np.asarray(x, np.float32)
    if pool_in:
        x = pool2(x)
    return np.maximum(conv(x, w, prec) + np.asarray(b, np.float32), np.float32(0))


def l1_terms_emulated(ends, B):
    """vgg_l1_partial_kernel / vgg_l1_finish_kernel in float32: float4 groups, 65536 strided threads, tree reductions"""
    def tree(v):   # v [..., 256]
        v = v.copy()
        w = 128
        while w:
            v[..., :w] = v[..., :w] + v[..., w:2 * w]
            w //= 2
        return v[..., 0]
    t = []
    for m in ends:
        m = np.asarray(m, np.float32)
        d = np.abs(m[:B] - m[B:]).reshape(-1, 4)
        v = (d[:, 0] + d[:, 1]) + (d[:, 2] + d[:, 3])
        T = L1_BLOCKS * 256
        v = np.concatenate([v, np.zeros(-v.size % T, np.float32)]).reshape(-1, T)
        s = np.zeros(T, np.float32)
        for row in v:
            s = s + row
        part = tree(s.reshape(L1_BLOCKS, 256))
        t.append(np.float32(tree(part)) / np.float32(float(m[:B].size)))
    return np.array(t + [((t[0] + t[1]) + t[2]) + t[3]], np.float32)


def backward_emulated(maps, W, g, merge, prec):
    """backward() in the kernels' arithmetic: float32 junction and resize, split-operand dgrads through torch's float32 convolution"""
    return backward([np.asarray(m, np.float32) for m in maps], W, np.float32(g), merge,
                    conv_adj=lambda dz, w: conv_emulated(dz, w, prec, transpose=True), dt=np.float32)


def reference_q(prec):
    return bf16_rne if prec == "bf16" else ident


# ---------------------------------------------------------------------------------------------
# the comparison rule
# ---------------------------------------------------------------------------------------------
def ratio(got, ref, S):
    """per entry |got - ref| / S; where S == 0: 0 if equal, inf otherwise"""
    g, r, s = (np.asarray(a, np.float64) for a in (got, ref, S))
    assert g.shape == r.shape == s.shape, (g.shape, r.shape, s.shape)
    err = np.abs(g - r)
    return np.where(s > 0, err / np.where(s > 0, s, 1.0), np.where(err > 0, np.inf, 0.0))


def compare(got, ref, S, bnd, tag):
    """(largest |got - ref| / S, None or the failure message naming the worst entry)"""
    rel = ratio(got, ref, S)
    j = int(np.argmax(rel))
    worst = float(rel.reshape(-1)[j])
    if worst <= bnd:
        return worst, None
    idx = tuple(int(v) for v in np.unravel_index(j, rel.shape))
    return worst, "%s: entry %s got %.9g expected %.9g S %.3g: %.3g of S, bound %.3g (%d of %d entries over)" % (
        tag, list(idx), np.asarray(got).reshape(-1)[j], np.asarray(ref).reshape(-1)[j], np.asarray(S).reshape(-1)[j], worst, bnd,
        int((rel > bnd).sum()), rel.size)


def compare_gradient(got, ref, bnd_max, bnd_l2, tag):
    """the end-to-end rule: (per entry / max |ref|, relative L2, None or the failure message)"""
    g, r = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert g.shape == r.shape, (g.shape, r.shape)
    top, nrm = float(np.abs(r).max()), float(np.linalg.norm(r))
    err = np.abs(g - r)
    j = int(np.argmax(err))
    mx = float(err.reshape(-1)[j]) / top if top > 0 else (np.inf if err.any() else 0.0)
    l2 = float(np.linalg.norm(g - r)) / nrm if nrm > 0 else (np.inf if err.any() else 0.0)
    if mx <= bnd_max and l2 <= bnd_l2:
        return mx, l2, None
    idx = tuple(int(v) for v in np.unravel_index(j, err.shape))
    return mx, l2, "%s: worst entry %s got %.9g expected %.9g, %.3g of max|ref| (bound %.3g); relative L2 %.3g (bound %.3g)" % (
        tag, list(idx), g.reshape(-1)[j], r.reshape(-1)[j], mx, bnd_max, l2, bnd_l2)


# ---------------------------------------------------------------------------------------------
# the cases, shared by the CPU floors and the GPU tests
# ---------------------------------------------------------------------------------------------
def stage_case(layer, transpose, geom, gate_pad=False):
    """inputs of one single-stage call: x interior NHWC (0.5 randn; the un-pooled size for the forward of layers 2, 4, 7) and, for a
    dgrad, a gate in {-1, 0, 1} of the output's shape"""
    n, H, Wd = geom
    rng = np.random.RandomState(1000 * layer + 100 * int(transpose) + 7 * n + 3 * H + Wd)
    if transpose:
        x = (0.5 * rng.standard_normal((n, H, Wd, COUT[layer]))).astype(np.float32)
        gate = rng.randint(-1, 2, size=(n, H, Wd, CIN[layer])).astype(np.float32)
        return x, gate
    k = 2 if POOL_IN[layer] else 1
    return (0.5 * rng.standard_normal((n, k * H, k * Wd, CIN[layer]))).astype(np.float32), None


def stage_reference(layer, transpose, geom, prec):
    """(ref, S) of a single-stage case in float64, with the operand rounding of `prec`"""
    W, _ = weights()
    x, gate = stage_case(layer, transpose, geom)
    q = reference_q(prec)
    if transpose:
        return dgrad(x, W[layer][0], gate, q)
    return conv_stage(x, W[layer][0], W[layer][1], POOL_IN[layer], q)


def stage_emulated(layer, transpose, geom, prec):
    W, _ = weights()
    x, gate = stage_case(layer, transpose, geom)
    if transpose:
        return np.where(gate > 0, conv_seq16(x, W[layer][0], prec, transpose=True), np.float32(0))
    return conv_stage_emulated(x, W[layer][0], W[layer][1], POOL_IN[layer], prec)


def production_case(B=PRODUCTION["B"], P=PRODUCTION["P"], seed=PRODUCTION["seed"], nan=5):
    """(merge with NaN pixels, gt, mask) float32 [B, 3 | 1, P, P]: a soft disk mask, as the training masks are"""
    g = torch.Generator().manual_seed(seed)
    merge = torch.rand(B, 3, P, P, generator=g)
    merge.view(-1)[torch.randperm(merge.numel(), generator=g)[:nan]] = float("nan")
    gt = torch.rand(B, 3, P, P, generator=g)
    yy, xx = torch.meshgrid(torch.arange(P), torch.arange(P), indexing="ij")
    r = ((yy - P / 2.0) ** 2 + (xx - P / 2.0) ** 2).sqrt() / P
    mask = ((0.35 - r) * 8 + 0.5).clamp(0, 1).view(1, 1, P, P).repeat(B, 1, 1, 1)
    return merge.numpy(), gt.numpy(), mask.numpy()


def resize_merge(P, B=1):
    """a merge image of side P for the resize sweep: only its size and its NaN pixels matter to the backward"""
    rng = np.random.RandomState(P)
    m = rng.rand(B, 3, P, P).astype(np.float32)
    m.reshape(-1)[rng.choice(m.size, 4, replace=False)] = np.nan
    return m


TIE_PATTERNS = np.array([[1, 1, 1, 1],            # all four equal
                         [1, 1, 0.5, 0.25], [1, 0.5, 1, 0.25], [1, 0.5, 0.25, 1],      # two equal maxima, one of them first
                         [0.5, 1, 1, 0.25], [0.5, 1, 0.25, 1], [0.25, 0.5, 1, 1],      # two equal maxima, neither first
                         [0, 0, 0, 0]], np.float32)                                   # a tie at zero: the ReLU gate kills it


def crafted_maps(maps, kind, B=1):
    """Hand-made `saved` maps (interior, float32) from stored ones.
      block<b>   the target half of every block-end map set equal to its prediction half except at block b: the gradient enters
                 at one junction only
      equal      ... at every block end: d_merge is exactly 0
      ties       block-end map 1 (pooled into block 2): window k of the raster takes TIE_PATTERNS[k % 8] times a per-channel positive
                 scale, in every channel; its target equals the prediction at every other entry (sign 0) and differs elsewhere
      scattered  maps 0 (a ReLU gate) and 3 (a block end under a pool): 0 everywhere except single positive entries, about 1 in 97"""
    out = [np.array(m, np.float32, copy=True) for m in maps]
    if kind == "equal" or kind.startswith("block"):
        keep = -1 if kind == "equal" else int(kind[5:])
        for b, l in enumerate(BLOCK_END):
            if b != keep:
                out[l][B:] = out[l][:B]
    elif kind == "ties":
        m = out[1]
        _, H, Wd, C = m.shape
        k = (np.arange(H // 2)[:, None] * (Wd // 2) + np.arange(Wd // 2)[None, :]) % 8
        pat = TIE_PATTERNS[k].reshape(H // 2, Wd // 2, 2, 2).transpose(0, 2, 1, 3).reshape(H, Wd)
        scale = (0.25 + 0.125 * (np.arange(C) % 7)).astype(np.float32)
        m[:B] = pat[None, :, :, None] * scale[None, None, None, :]
        e = np.arange(m[:B].size).reshape(m[:B].shape)
        m[B:] = np.where(e % 2 == 0, m[:B], m[:B] + np.where(e % 4 == 1, np.float32(0.5), np.float32(-0.5)))
    elif kind == "scattered":
        for l in (0, 3):
            m = out[l]
            e = np.arange(m[:B].size).reshape(m[:B].shape)
            m[:B] = np.where(e % 97 == 5, np.float32(0.75) + (e % 5).astype(np.float32) * np.float32(0.125), np.float32(0))
    else:
        raise ValueError(kind)
    return out
