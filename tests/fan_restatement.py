"""A float64 restatement of the AWing FAN landmark chain (n3dt.FAN, csrc/fan.hip), written from the network's
description and held to the reference's own classes by tests/golden/fan* (tools/gen_golden_fan.py): the network block by block,
calculate_points per frame, and -- restated by hand, NOT recorded -- the glue of get_landmarks and extract_keypoint (the scale by the
crop, the 98 -> 68 table, the origin, the carry-forward) and the bilinear crop.  `emulate=True` runs every convolution in the
kernel's arithmetic instead: float64 folds rounded once to fp32, both operands split into two bf16s, three products accumulated
in fp32, fp32 epilogues.  The seeded inputs of every case live here so that no input is stored."""
import math

import numpy as np
import torch
import torch.nn.functional as F

WEIGHTS_SEED = 22
EPS = 1e-5
HEAT, CELLS, IMG = 64, 4096, 256
HG_BLOCKS = ("b1_4", "b2_4", "b1_3", "b2_3", "b1_2", "b2_2", "b1_1", "b2_1", "b2_plus_1", "b3_1", "b3_2", "b3_3", "b3_4")
CASES = {"m1": (1, 98, 2), "m2": (2, 98, 3), "m4": (4, 98, 1)}  # num_modules, num_landmarks, images
BLOCK_SHAPES = ((3, 12, 10), (1, 4, 4))  # ConvBlocks alone: 120 rows = one 64-row tile and a tail; 16 rows
POOL_SHAPE = (2, 8, 6)
SAMPLE_EVERY = 331
GPU_FACTOR = 4.0


def fixture_images(case):
    """[n,3,256,256] float32 BGR in [0,1]: smooth blobs under pixel noise, seeded"""
    M, N, n = CASES[case]
    gen = torch.Generator().manual_seed(1000 + M)
    low = F.interpolate(torch.rand(n, 3, 16, 16, generator=gen), size=(IMG, IMG), mode="bilinear", align_corners=False)
    return (0.5 * low + 0.5 * torch.rand(n, 3, IMG, IMG, generator=gen)).float().contiguous()


def block_input(name, shape, C, seed=0):
    gen = torch.Generator().manual_seed(hash_name(name) + 7919 * seed)
    n, H, W = shape
    return torch.randn(n, C, H, W, generator=gen).float()


def hash_name(name):
    return sum((i + 1) * ord(c) for i, c in enumerate(name)) % 100003


def coords(dim):
    r = torch.arange(dim, dtype=torch.int32).float() / (dim - 1)
    r = r * 2 - 1
    xx, yy = r[:, None].expand(dim, dim), r[None, :].expand(dim, dim)
    rr = torch.sqrt(torch.pow(xx, 2) + torch.pow(yy, 2))
    return torch.stack((xx, yy, rr / torch.max(rr))).double()


# ---- arithmetic ------------------------------------------------------------------------------------------------------------------
def _split(t):
    hi = t.float().bfloat16().float()
    return hi, (t.float() - hi).bfloat16().float()


def conv(x, w, emulate, stride=1):
    """x, w float64 -> float64; emulate: x and w rounded to fp32 and split, lo*hi + hi*lo + hi*hi accumulated in fp32"""
    pad = w.shape[-1] // 2
    if not emulate:
        return F.conv2d(x, w, None, stride, pad)
    xh, xl = _split(x)
    wh, wl = _split(w)
    y = F.conv2d(xl, wh, None, stride, pad) + F.conv2d(xh, wl, None, stride, pad) + F.conv2d(xh, wh, None, stride, pad)
    return y.double()


def bn_fold(sd, name):
    g = sd[name + ".weight"].double() / torch.sqrt(sd[name + ".running_var"].double() + EPS)
    return g, sd[name + ".bias"].double() - sd[name + ".running_mean"].double() * g


def pre(sd, name, x, emulate):
    g, b = bn_fold(sd, name)
    if emulate:
        t = (g.float()[None, :, None, None] * x.float()) + b.float()[None, :, None, None]
        return torch.relu(t).double()
    return torch.relu(g[None, :, None, None] * x + b[None, :, None, None])


def r32(t, emulate):
    return t.float().double() if emulate else t


def conv_block(sd, name, x, emulate=False):
    w1 = sd[name + ".conv1.weight"].double()
    cin, cout = w1.shape[1], w1.shape[0] * 2
    res = x
    if cin != cout:
        res = r32(conv(pre(sd, name + ".downsample.0", x, emulate), sd[name + ".downsample.2.weight"].double(), emulate), emulate)
    o1 = r32(conv(pre(sd, name + ".bn1", x, emulate), w1, emulate), emulate)
    o2 = r32(conv(pre(sd, name + ".bn2", o1, emulate), sd[name + ".conv2.weight"].double(), emulate), emulate)
    o3 = r32(conv(pre(sd, name + ".bn3", o2, emulate), sd[name + ".conv3.weight"].double(), emulate), emulate)
    return r32(torch.cat((o1, o2, o3), 1) + res, emulate)


def stem(sd, x, emulate=False):
    """the CoordConv stem + bn1 + ReLU: image channels through the convolution, coordinate channels as a constant map"""
    w, b = sd["conv1.conv.weight"].double(), sd["conv1.conv.bias"].double()
    g, sh = bn_fold(sd, "bn1")
    cmap = F.conv2d(coords(IMG)[None], w[:, 3:], None, 2, 3)[0]
    cmap = (cmap + (b - sd["bn1.running_mean"].double())[:, None, None]) * g[:, None, None] + sd["bn1.bias"].double()[:, None, None]
    wf = w[:, :3] * g[:, None, None, None]
    if emulate:
        cmap, wf = cmap.float().double(), wf.float().double()
    return r32(torch.relu(r32(conv(x, wf, emulate, 2), emulate) + cmap[None]), emulate)


def coordconv(sd, s, x, gate, emulate=False):
    """the hourglass CoordConv of stack s; gate: bool/uint8 [n,64,64] or None"""
    w, b = sd["m%d.coordconv.conv.weight" % s].double()[:, :, 0, 0], sd["m%d.coordconv.conv.bias" % s].double()
    c = coords(HEAT)
    m1 = torch.einsum("oc,chw->ohw", w[:, 256:259], c) + b[:, None, None]
    y = conv(x, w[:, :256, None, None], emulate)
    if emulate:
        m1 = m1.float().double()
    y = r32(r32(y, emulate) + m1[None], emulate)
    if s > 0:
        m2 = torch.einsum("oc,chw->ohw", w[:, 259:261], c[:2])
        if emulate:
            m2 = m2.float().double()
        y = r32(y + gate[:, None].double() * m2[None], emulate)
    return y


def plain(sd, name, x, emulate=False, skip=None, relu=False, post=None):
    w, b = sd[name + ".weight"].double(), sd[name + ".bias"].double()
    if post is not None:
        g, _ = bn_fold(sd, post)
        b = (b - sd[post + ".running_mean"].double()) * g + sd[post + ".bias"].double()
        w = w * g[:, None, None, None]
    if emulate:
        w, b = w.float().double(), b.float().double()
    y = r32(r32(conv(x, w, emulate), emulate) + b[None, :, None, None], emulate)
    if skip is not None:
        y = r32(y + skip, emulate)
    return torch.relu(y) if relu else y


def pool(x):
    return F.avg_pool2d(x, 2, 2)


def upadd(low, up):
    return up + F.interpolate(low, scale_factor=2, mode="nearest")


def gate_of(heat):
    """the reference's fp32 comparison on the fp32 heat map's last channel"""
    return torch.clamp(heat[:, -1].float(), 0.0, 1.0) > 0.05


def forward(sd, x, M, N, end_relu=False, gates=None, emulate=False, record=None):
    """x [n,3,256,256] -> (heat maps [M][n,N+1,64,64] float64, gates used [M-1][n,64,64] bool).  gates: forced.  record: a dict
    that takes {block name: (input, skip, gate, output)}"""
    rec = (lambda k, *v: record.__setitem__(k, v)) if record is not None else (lambda k, *v: None)
    x = x.double()

    def cb(name, t):
        y = conv_block(sd, name, t, emulate)
        rec(name.replace("top_m_", "top_m_"), t, None, None, y)
        return y

    def hourglass(s, level, t):
        up1 = cb("m%d.b1_%d" % (s, level), t)
        low = cb("m%d.b2_%d" % (s, level), r32(pool(t), emulate))
        low = hourglass(s, level - 1, low) if level > 1 else cb("m%d.b2_plus_1" % s, low)
        low = cb("m%d.b3_%d" % (s, level), low)
        return r32(upadd(low, up1), emulate)

    y = stem(sd, x, emulate)
    rec("conv1", x, None, None, y)
    y = r32(pool(cb("conv2", y)), emulate)
    previous = cb("conv4", cb("conv3", y))
    heats, used, tmp = [], [], None
    for s in range(M):
        g = None
        if s > 0:
            g = gates[s - 1].bool() if gates is not None else gate_of(tmp)
            used.append(g)
        cc = coordconv(sd, s, previous, g, emulate)
        rec("m%d.coordconv" % s, previous, None, g, cc)
        ll = cb("top_m_%d" % s, hourglass(s, 4, cc))
        l2 = plain(sd, "conv_last%d" % s, ll, emulate, relu=True, post="bn_end%d" % s)
        rec("conv_last%d" % s, ll, None, None, l2)
        tmp = plain(sd, "l%d" % s, l2, emulate, relu=end_relu)
        rec("l%d" % s, l2, None, None, tmp)
        heats.append(tmp)
        if s < M - 1:
            a = plain(sd, "bl%d" % s, l2, emulate, skip=previous)
            rec("bl%d" % s, l2, previous, None, a)
            nxt = plain(sd, "al%d" % s, tmp, emulate, skip=a)
            rec("al%d" % s, tmp, a, None, nxt)
            previous = nxt
    return heats, used


def run_block(sd, name, x, skip=None, gate=None, emulate=False, end_relu=False):
    """one block of FAN.block_names alone"""
    x = x.double()
    skip = None if skip is None else skip.double()
    if name == "conv1":
        return stem(sd, x, emulate)
    if name == "avg_pool":
        return r32(pool(x), emulate)
    if name == "upsample_add":
        return r32(upadd(x, skip), emulate)
    if name.endswith(".coordconv"):
        return coordconv(sd, int(name[1:name.index(".")]), x, gate, emulate)
    if name.startswith("conv_last"):
        return plain(sd, name, x, emulate, relu=True, post="bn_end" + name[9:])
    if name[0] == "l" and name[1:].isdigit():
        return plain(sd, name, x, emulate, relu=end_relu)
    if name[:2] in ("bl", "al") and name[2:].isdigit():
        return plain(sd, name, x, emulate, skip=skip)
    return conv_block(sd, name, x, emulate)


def summary(t):
    """(sum, abs-sum, every 331st element) of a float64 tensor"""
    flat = t.reshape(-1).double()
    return float(flat.sum()), float(flat.abs().sum()), flat[::SAMPLE_EVERY].numpy().copy()


# ---- the decode --------------------------------------------------------------------------------------------------------------------
def decode(heat):
    """calculate_points on one frame's heat maps [N,64,64] (B = 1) -> [N,2] float64, or None where the reference raises IndexError"""
    flat = np.asarray(heat).reshape(heat.shape[0], CELLS)
    idx = flat.argmax(axis=1)
    if (idx == CELLS - 1).any():
        return None
    rows = np.arange(flat.shape[0])
    xu, xd = flat[rows, idx + 1], flat[rows, np.where(idx == 0, CELLS - 1, idx - 1)]
    yu = flat[rows, CELLS - 1] if (idx + HEAT >= CELLS).any() else flat[rows, idx + HEAT]
    yd = flat[rows, 0] if (idx - HEAT <= 0).any() else flat[rows, idx - HEAT]
    pts = np.stack((idx % HEAT, idx // HEAT), axis=1).astype(np.float64)
    pts += 0.25 * np.sign(np.stack((xu.astype(np.float64) - xd, yu.astype(np.float64) - yd), axis=1))
    return pts + 0.5


def decode_heatmaps(case, N=5):
    """[N,64,64] float32: seeded noise in [0, 0.5) with the case's peaks planted"""
    rng = np.random.default_rng(hash_name(case))
    h = (rng.random((N, CELLS)) * 0.5).astype(np.float32)

    def peak(l, cell, v=1.0):
        h[l, cell] = v

    if case == "interior":
        for l, c in enumerate((64 * 5 + 7, 64 * 30 + 31, 64 * 40 + 2, 64 * 62 + 60, 64 * 17 + 17)):
            peak(l, c)
    elif case == "last_row":
        for l, c in enumerate((64 * 63 + 5, 64 * 30 + 31, 64 * 40 + 2, 64 * 20 + 60, 64 * 17 + 17)):
            peak(l, c)
    elif case == "row0":
        for l, c in enumerate((9, 64 * 30 + 31, 64 * 40 + 2, 64 * 20 + 60, 64 * 17 + 17)):
            peak(l, c)
    elif case == "cell64":
        for l, c in enumerate((64, 64 * 30 + 31, 64 * 40 + 2, 64 * 20 + 60, 64 * 17 + 17)):
            peak(l, c)
    elif case == "cell0":
        for l, c in enumerate((0, 64 * 30 + 31, 64 * 40 + 2, 64 * 20 + 60, 64 * 17 + 17)):
            peak(l, c)
    elif case == "row_end":
        for l, c in enumerate((64 * 10 + 63, 64 * 30 + 0, 64 * 40 + 2, 64 * 20 + 60, 64 * 17 + 17)):
            peak(l, c)
    elif case == "tie":
        for l, c in enumerate((64 * 10 + 9, 64 * 30 + 31, 64 * 40 + 2, 64 * 20 + 60, 64 * 17 + 17)):
            peak(l, c)
        peak(0, 64 * 50 + 3)  # the same value later: the first index wins
        peak(1, 64 * 12 + 1)
    elif case == "equal_neighbours":
        for l, c in enumerate((64 * 10 + 9, 64 * 30 + 31, 64 * 40 + 2, 64 * 20 + 60, 64 * 17 + 17)):
            peak(l, c)
        h[0, 64 * 10 + 8] = h[0, 64 * 10 + 10] = 0.25
        h[1, 64 * 29 + 31] = h[1, 64 * 31 + 31] = 0.125
    elif case == "cell4095":
        for l, c in enumerate((64 * 10 + 9, 4095, 64 * 40 + 2, 64 * 20 + 60, 64 * 17 + 17)):
            peak(l, c)
    else:
        raise KeyError(case)
    return h.reshape(N, HEAT, HEAT)


DECODE_CASES = ("interior", "last_row", "row0", "cell64", "cell0", "row_end", "tie", "equal_neighbours", "cell4095")


# ---- the glue, restated by hand ------------------------------------------------------------------------------------------------------
def box_ok(box, H, W):
    y1, y2, x1, x2 = (int(v) for v in box)
    return y1 >= 0 and x1 >= 0 and y2 > y1 and x2 > x1 and y2 <= H and x2 <= W


def glue(pts, boxes, H, W, table=None, carry=True, N=98):
    """pts: per frame [N,2] float64 in heat-map cells or None (the decode failed) -> ([F,P,2] float64, status [F]): get_landmarks'
    scale by (w / 64, h / 64), landmark_98_to_68 as a table of two source indices into a float32 array, extract_keypoint's integer
    origin added in float32, -1 for a frame without a face, and the list branch's carry-forward"""
    out, status = [], []
    P = len(table) if table is not None else N
    for p, box in zip(pts, boxes):
        st = (2 if p is None else 0) | (0 if box_ok(box, H, W) else 4)
        status.append(st)
        if st:
            kp = out[-1].copy() if (carry and out) else -np.ones((P, 2))
        else:
            y1, y2, x1, x2 = (int(v) for v in box)
            scaled = p * np.array([(x2 - x1) / 64, (y2 - y1) / 64])
            if table is not None:
                kp = np.zeros((P, 2), dtype=np.float32)
                for q, (a, b) in enumerate(table):
                    kp[q] = (scaled[a] + scaled[b]) / 2
                kp[:, 0] += x1
                kp[:, 1] += y1
                kp = kp.astype(np.float64)
            else:
                kp = scaled + np.array([float(x1), float(y1)])
        out.append(kp)
    return np.stack(out), np.array(status, dtype=np.int32)


def crop(frames, boxes):
    """frames [F,3,H,W] float32 RGB, boxes [F,4] -> [F,3,256,256] float32 BGR: bilinear with half-pixel centres, float64, rounded once"""
    F_, _, H, W = frames.shape
    out = np.zeros((F_, 3, IMG, IMG), dtype=np.float32)
    d = np.arange(IMG, dtype=np.float64)
    for f in range(F_):
        if not box_ok(boxes[f], H, W):
            continue
        y1, y2, x1, x2 = (int(v) for v in boxes[f])

        def taps(n):
            src = np.maximum((n / IMG) * (d + 0.5) - 0.5, 0.0)
            a = np.minimum(src.astype(np.int64), n - 1)
            return a, np.minimum(a + 1, n - 1), src - a

        ya, yb, wy = taps(y2 - y1)
        xa, xb, wx = taps(x2 - x1)
        src = frames[f].astype(np.float64)[:, y1:y2, x1:x2]
        top = (1.0 - wx) * src[:, ya][:, :, xa] + wx * src[:, ya][:, :, xb]
        bot = (1.0 - wx) * src[:, yb][:, :, xa] + wx * src[:, yb][:, :, xb]
        out[f] = (((1.0 - wy)[:, None] * top + wy[:, None] * bot)[::-1]).astype(np.float32)
    return out


# ---- stability -----------------------------------------------------------------------------------------------------------------------
def unstable_gate_cells(heat, delta):
    """bool [n,64,64]: |clamp(v) - 0.05| < delta on the last channel"""
    v = torch.clamp(heat[:, -1].double(), 0.0, 1.0)
    return (v - 0.05).abs() < delta


def unstable_landmarks(heat, delta):
    """bool [n,N]: the top-1 - top-2 gap or a neighbour difference calculate_points takes the sign of is below delta (frame-wide
    flags as the decode has them); a frame the reference raises on is unstable throughout"""
    h = np.asarray(heat.double())[:, :-1]
    n, N = h.shape[:2]
    out = np.zeros((n, N), dtype=bool)
    for f in range(n):
        flat = h[f].reshape(N, CELLS)
        top2 = np.sort(flat, axis=1)[:, -2:]
        idx = flat.argmax(axis=1)
        if (idx == CELLS - 1).any():
            out[f] = True
            continue
        rows = np.arange(N)
        xu, xd = flat[rows, idx + 1], flat[rows, np.where(idx == 0, CELLS - 1, idx - 1)]
        yu = flat[rows, CELLS - 1] if (idx + HEAT >= CELLS).any() else flat[rows, idx + HEAT]
        yd = flat[rows, 0] if (idx - HEAT <= 0).any() else flat[rows, idx - HEAT]
        out[f] = (top2[:, 1] - top2[:, 0] < delta) | (np.abs(xu - xd) < delta) | (np.abs(yu - yd) < delta)
    return out
