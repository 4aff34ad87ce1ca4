"""A float64 restatement of the 3-D face reconstruction net and its aligner the way the reference computes them
(s_face3d/models/networks.py's ReconNetWrapper over resnet50; s_face3d/util/preprocess.py's align_img under
CropAndExtract.generate, with PIL's BICUBIC resize), written from n3dt.face_recon's table, and an emulation of the arithmetic
csrc/face_recon.hip uses.  tests/golden/face_recon*.{npz,json} (tools/gen_golden_face_recon.py, from the reference's own class and
functions in float64, and PIL) pins the restatement; the GPU tests are judged against the fixture within bounds the tool measured
with the emulation.

  restatement   Conv2d, eval-mode BatchNorm2d by its formula, ReLU, max_pool2d(3, 2, 1), the residual sum in the reference's order,
                the mean, the seven final_layers concatenated; extract_5p, the y flip, the fallback, POS as two 5 x 4 least-squares
                problems through one pseudo-inverse, the truncations, and PIL's two-pass bicubic resample restricted to the crop.
                float64 throughout.
  emulation     per convolution: BatchNorm folded into weight and bias in float64 and rounded to fp32, input and weights split into
                two bf16 values each, the three products lo*hi + hi*lo + hi*hi as fp32 convolutions (fp32 accumulation), bias,
                residual and ReLU in fp32; the pool in fp32; the average and the head in float64 from fp32 operands, rounded once.
                Its distance from the reference's float64 values is the floor the GPU tests' bounds are 4 x of (the order of the
                fp32 sums differs between this and the MFMA).
"""
import numpy as np
import torch
import torch.nn.functional as F

from n3dt.face_recon import AVG_BLOCK, BN_EPS, BN_PARTS, CONVS, CROP, HEAD_BLOCK, HEAD_COLS, N_CONVS, POOL_BLOCK, block_names, pos_pinv

WEIGHTS_SEED = 11
INPUT_SEED = 57
SAMPLE_STRIDE = 331
N_BLOCKS = len(block_names())
CASES = {"a": (2, 64, 64), "b": (3, 72, 56), "c": (1, 32, 32), "real": (1, 224, 224)}
SMALL_CASES = ("a", "b", "c")
ALIGN_CASES = {"p": (3, 64, 64), "q": (3, 96, 80)}  # (frames, H, W)
RESCALE = 102.0


def fixture_images(case):
    """the network's input [n,3,H,W] float64 in [0,1], exactly representable in fp32: gradients plus noise, quantised to 1/256"""
    n, H, W = CASES[case]
    g = torch.Generator().manual_seed(INPUT_SEED + sum(ord(c) for c in case))
    yy, xx = torch.meshgrid(torch.arange(float(H)), torch.arange(float(W)), indexing="ij")
    out = torch.empty(n, 3, H, W)
    for i in range(n):
        for c in range(3):
            a, b, p = (torch.rand(3, generator=g) * 0.4).tolist()
            out[i, c] = 0.5 + 0.25 * torch.sin(a * yy + b * xx + 20 * p) + 0.15 * torch.randn(H, W, generator=g)
    return (out.clamp(0, 1) * 256).round().clamp(0, 255).double() / 256.0


def fixture_frames(case):
    """frames [n,H,W,3] uint8 RGB with a noise component.  The aligner sees u8 / 255 as float32 [n,3,H,W]; PIL sees the bytes."""
    n, H, W = ALIGN_CASES[case]
    g = torch.Generator().manual_seed(INPUT_SEED + 1000 + sum(ord(c) for c in case))
    yy, xx = torch.meshgrid(torch.arange(float(H)), torch.arange(float(W)), indexing="ij")
    out = torch.empty(n, H, W, 3)
    for i in range(n):
        for c in range(3):
            a, b, p = (torch.rand(3, generator=g) * 0.3).tolist()
            out[i, :, :, c] = 118 + 70 * torch.sin(a * yy + b * xx + 20 * p) + 30 * torch.randn(H, W, generator=g)
    return out.clamp(0, 255).to(torch.uint8).numpy()


def frames_f32(u8):
    return (torch.as_tensor(u8).permute(0, 3, 1, 2).float() / 255.0).contiguous()


def landmarks_68(lm5_flipped, H, rng):
    """68 image landmarks (y down) whose extract_5p and y flip give lm5_flipped [5,2]: the eyes as two corners around their mean"""
    lm = rng.uniform(5.0, 60.0, size=(68, 2))
    le, re, nose, lmouth, rmouth = lm5_flipped
    d = rng.uniform(1.0, 3.0, size=(2, 2))
    lm[36], lm[39] = le - d[0], le + d[0]
    lm[42], lm[45] = re - d[1], re + d[1]
    lm[30], lm[48], lm[54] = nose, lmouth, rmouth
    lm[[36, 39, 42, 45, 30, 48, 54], 1] = (H - 1) - lm[[36, 39, 42, 45, 30, 48, 54], 1]
    return lm


def fixture_landmarks(case, lm3d_std):
    """per frame None (the fallback), or image landmarks [68,2] / [5,2] float64, y down.  Built from a wanted scale s and crop
    corner, so that the fixture holds: upscale and downscale, a crop over the left and top border (p0), over the right and bottom
    border (q0), resized images smaller than the crop (p1, q1), a NaN frame (p2: the status) and a frame of -1 (q2: the fallback).
    The fallback is ill-conditioned in the reference itself: its t is exactly (w0 / 2, h0 / 2), so the argument of `left` is
    w / 2 - 112 and that of `up` h / 2 - 112, and since w0 s + h0 s = 408 one of w, h is even (or both products are integers): one
    truncation always sits on an integer and falls to whichever side the solver's last bit pushes it.  At 96 x 80 that is `up`."""
    n, H, W = ALIGN_CASES[case]
    rng = np.random.default_rng(INPUT_SEED + sum(ord(c) for c in case))
    std = np.asarray(lm3d_std, dtype=np.float64)
    # (points, s, left, up) wanted, approximately: POS sees s_pos = 102 / s and t from the landmarks below
    wanted = {"p": [(68, 2.53, -17.4, -9.6), (5, 0.63, -90.3, -85.7), "nan"], "q": [(5, 2.41, 21.3, 33.6), (68, 0.83, -70.2, -66.4), None]}[case]
    out = []
    for spec in wanted:
        if spec is None:
            out.append(np.full((68, 2), -1.0))
            continue
        if spec == "nan":
            lm = rng.uniform(5.0, 60.0, size=(5, 2))
            lm[3, 0] = np.nan
            out.append(lm)
            continue
        points, s, left, up = spec
        w, h = int(W * s), int(H * s)
        t0 = (left - w / 2 + CROP / 2) / s + W / 2
        t1 = H / 2 - (up - h / 2 + CROP / 2) / s
        lm5 = (RESCALE / s) * std[:, :2] + np.array([t0, t1]) + rng.normal(0.0, 0.4, size=(5, 2))  # flipped coordinates (y up)
        if points == 5:
            lm = lm5.copy()
            lm[:, 1] = (H - 1) - lm[:, 1]
        else:
            lm = landmarks_68(lm5, H, rng)
        out.append(lm)
    return out


# ---- the network: b indexes block_names(); float64 or the kernel's arithmetic --------------------------------------------------------
def split(x):
    hi = x.bfloat16().float()
    return hi, (x - hi).bfloat16().float()


def bn_params(sd, bn):
    return [sd["%s.%s" % (bn, part)].double() for part in BN_PARTS]


def folded(sd, b):
    """(weight, bias) float64 of convolution b with its eval-mode BatchNorm folded in: the pack kernel's arithmetic"""
    conv, bn = CONVS[b][:2]
    gamma, beta, mean, var = bn_params(sd, bn)
    scale = gamma / torch.sqrt(var + BN_EPS)
    return sd[conv + ".weight"].double() * scale.view(-1, 1, 1, 1), beta - mean * scale


def head_matrix(sd):
    w = torch.cat([sd["final_layers.%d.weight" % i].double().reshape(c, -1) for i, c in enumerate(HEAD_COLS)])
    return w, torch.cat([sd["final_layers.%d.bias" % i].double() for i in range(len(HEAD_COLS))])


def block(sd, b, x, skip=None, emulated=False):
    """block b on x (and the identity `skip` for a bottleneck's third convolution) -> its output: float64 as the reference
    computes it, or fp32 by the kernel's arithmetic"""
    if b < N_CONVS:
        conv, bn, _, _, _, s, p, role, relu = CONVS[b]
        if emulated:
            w, bias = folded(sd, b)
            (xh, xl), (wh, wl) = split(x.float()), split(w.float())
            y = F.conv2d(xl, wh, None, stride=s, padding=p)
            y = y + F.conv2d(xh, wl, None, stride=s, padding=p)
            y = y + F.conv2d(xh, wh, None, stride=s, padding=p)
            y = y + bias.float()[None, :, None, None]
            if skip is not None:
                y = y + skip.float()
        else:
            gamma, beta, mean, var = bn_params(sd, bn)
            y = F.conv2d(x.double(), sd[conv + ".weight"].double(), None, stride=s, padding=p)
            y = (y - mean.view(1, -1, 1, 1)) / torch.sqrt(var.view(1, -1, 1, 1) + BN_EPS) * gamma.view(1, -1, 1, 1) + beta.view(1, -1, 1, 1)
            if skip is not None:
                y = y + skip.double()
        return torch.relu(y) if relu else y
    dtype = torch.float32 if emulated else torch.float64
    if b == POOL_BLOCK:
        return F.max_pool2d(x.to(dtype), 3, 2, 1)
    if b == AVG_BLOCK:
        return x.to(dtype).double().mean(dim=(2, 3), keepdim=True).to(dtype)
    w, bias = head_matrix(sd)
    if emulated:
        w, bias = w.float().double(), bias.float().double()
    return (x.to(dtype).double().flatten(1) @ w.t() + bias).to(dtype)


def chain(sd, x, emulated=False):
    """x [n,3,H,W] -> (inputs, skips, outputs) of the 56 blocks in block order, as the network feeds them (skips: None but for a
    bottleneck's third convolution)"""
    ins, skips, outs = [None] * N_BLOCKS, [None] * N_BLOCKS, [None] * N_BLOCKS

    def run(b, v, skip=None):
        ins[b], skips[b] = v, skip
        outs[b] = block(sd, b, v, skip, emulated)
        return outs[b]

    with torch.no_grad():
        x = run(POOL_BLOCK, run(0, x))
        b = 1
        while b < N_CONVS:
            down = b + 3 < N_CONVS and CONVS[b + 3][7] == 4
            y = run(b + 1, run(b, x))
            identity = run(b + 3, x) if down else x
            x = run(b + 2, y, identity)
            b += 4 if down else 3
        run(HEAD_BLOCK, run(AVG_BLOCK, x))
    return ins, skips, outs


def summary(act):
    """what the fixture keeps of an activation: its sum, its abs-sum and every SAMPLE_STRIDE-th element"""
    flat = act.double().reshape(-1)
    return float(flat.sum()), float(flat.abs().sum()), flat[::SAMPLE_STRIDE].numpy().copy()


# ---- the aligner, float64 numpy --------------------------------------------------------------------------------------------------
def five_points(lm, H, W, lm3d_std):
    """one frame's landmarks (None, [68,2] or [5,2]; image pixels, y down) -> the five points POS sees"""
    std = np.asarray(lm3d_std, dtype=np.float64)
    if lm is None or np.mean(lm) == -1:
        return (std[:, :2] + 1) / 2.0 * np.array([W, H], dtype=np.float64)
    lm = np.array(lm, dtype=np.float64)
    if lm.shape[0] != 5:
        lm = np.stack([(lm[36] + lm[39]) / 2, (lm[42] + lm[45]) / 2, lm[30], lm[48], lm[54]])
    lm[:, 1] = H - 1 - lm[:, 1]
    return lm


def similarity(lm5, H, W, pinv):
    """(trans_params (w0, h0, s, t0, t1), (w, h, left, up), status, the four truncations' arguments)"""
    k0, k1 = pinv @ lm5[:, 0], pinv @ lm5[:, 1]
    with np.errstate(all="ignore"):
        s = RESCALE / ((np.linalg.norm(k0[:3]) + np.linalg.norm(k1[:3])) / 2)
    t0, t1 = k0[3], k1[3]
    trans = np.array([W, H, s, t0, t1], dtype=np.float64)
    if not np.isfinite(trans).all() or not (1.0 / 16.0 <= s <= 16.0) or int(W * s) < 1 or int(H * s) < 1:
        return trans, (0, 0, 0, 0), 1, None
    w, h = int(W * s), int(H * s)
    args = (W * s, H * s, w / 2 - CROP / 2 + (t0 - W / 2) * s, h / 2 - CROP / 2 + (H / 2 - t1) * s)
    return trans, (w, h, int(args[2]), int(args[3])), 0, args


def cubic(x):
    x = np.abs(x)
    a = -0.5
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0, np.where(x < 2.0, (((x - 5.0) * x + 8.0) * x - 4.0) * a, 0.0))


def resample_matrix(first, count, size_in, size_out):
    """[count, size_in]: row i holds PIL's normalised bicubic weights of output index first + i of a resize size_in -> size_out, or
    zeros where that index lies outside [0, size_out)"""
    scale = size_in / size_out
    fs = max(scale, 1.0)
    support = 2.0 * fs
    M = np.zeros((count, size_in))
    for i in range(count):
        o = first + i
        if o < 0 or o >= size_out:
            continue
        center = (o + 0.5) * scale
        lo, hi = max(int(center - support + 0.5), 0), min(int(center + support + 0.5), size_in)
        wts = cubic((np.arange(lo, hi) - center + 0.5) / fs)
        M[i, lo:hi] = wts / wts.sum()
    return M


def crop(frame, geom, quantize=True):
    """frame [3,H,W] float in [0,1] -> the crop [3,224,224] float64 in [0,1]: pixel (left + X, up + Y) of the frame resized to (w, h)
    by PIL's BICUBIC, the horizontal pass first, clamped (and rounded to bytes where quantize) between and after the passes; 0
    outside the resized image"""
    w, h, left, up = geom
    _, H, W = frame.shape
    v = 255.0 * np.clip(np.nan_to_num(np.asarray(frame, dtype=np.float64), nan=0.0), 0.0, 1.0)
    rnd = (lambda t: np.floor(t + 0.5)) if quantize else (lambda t: t)
    v = rnd(v)
    Mx, My = resample_matrix(left, CROP, W, w), resample_matrix(up, CROP, H, h)
    tmp = np.clip(rnd(v @ Mx.T), 0.0, 255.0)                       # [3, H, 224]
    out = np.clip(rnd(np.einsum("yh,chx->cyx", My, tmp)), 0.0, 255.0)
    inside = ((My.sum(axis=1) != 0)[:, None] & (Mx.sum(axis=1) != 0)[None, :])
    return np.where(inside[None], out, 0.0) / 255.0


def align(frames, landmarks, lm3d_std, quantize=True):
    """frames [n,3,H,W] float in [0,1], landmarks a list per frame -> (crops [n,3,224,224] float64, trans [n,5], geom [n,4],
    status [n], the truncations' arguments per frame)"""
    pinv = pos_pinv(lm3d_std)
    n, _, H, W = frames.shape
    crops, trans, geoms, status, args = np.zeros((n, 3, CROP, CROP)), [], [], [], []
    for i in range(n):
        t, g, st, a = similarity(five_points(None if landmarks is None else landmarks[i], H, W, lm3d_std), H, W, pinv)
        if st == 0:
            crops[i] = crop(np.asarray(frames[i]), g, quantize)
        trans.append(t)
        geoms.append(g)
        status.append(st)
        args.append(a)
    return crops, np.array(trans), np.array(geoms, dtype=np.int64), np.array(status, dtype=np.int64), args


def measured_bounds(sd, x, ref_ins, ref_skips, ref_outs):
    """The emulation's error against the reference's float64 values, on the CPU alone: per block max |emulated block(fp32(x_b)) -
    y_b| with x (and the skip) the REFERENCE's activations, each block alone, then the emulated chain end to end: the 257
    coefficients"""
    with torch.no_grad():
        blocks = [float((block(sd, b, ref_ins[b].float(), None if ref_skips[b] is None else ref_skips[b].float(), True).double()
                         - ref_outs[b]).abs().max()) for b in range(N_BLOCKS)]
        coeffs = chain(sd, x.float(), True)[2][HEAD_BLOCK]
    return {"block": blocks, "coeffs": float((coeffs.double() - ref_outs[HEAD_BLOCK]).abs().max())}
