"""A float64 restatement of the S3FD face detector the way the reference's face_detection/detection/sfd computes it, written from
n3dt.s3fd's table, and an emulation of the arithmetic csrc/s3fd.hip uses for it.  tests/golden/s3fd*.{npz,json}
(tools/gen_golden_s3fd.py, from the reference's own class and functions in float64) pins the restatement; the GPU tests are judged
against the fixture within bounds the tool measured with the emulation.

  restatement   Conv2d + ReLU, max_pool2d(2, 2), L2Norm by its formula, the twelve head maps with cls1's max-out, the two-way
                softmax, bbox.py's decode, greedy NMS with the +1 areas, api.py's clip and truncation, the loader's pads and
                get_smoothened_boxes.  float64 throughout.
  emulation     per convolution: fp32 weights, input and weights split into two bf16 values each, the three products lo*hi + hi*lo
                + hi*hi as fp32 convolutions (fp32 accumulation), bias and ReLU in fp32; pools in fp32; L2Norm in float64 from fp32
                operands, rounded once; scores, decode and NMS in float64 from the fp32 head maps.  Its distance from the
                reference's float64 values is the floor the GPU tests' bounds are 4 x of (the order of the fp32 sums differs
                between this and the MFMA).
"""
import numpy as np
import torch
import torch.nn.functional as F

from n3dt.s3fd import CONVS, FIRST_HEAD, FIRST_NORM, FIRST_POOL, LEVEL_CONF, LEVEL_SOURCES, MEANS, N_LEVELS, NORMS, block_names

WEIGHTS_SEED = 2047
INPUT_SEED = 91
SAMPLE_STRIDE = 211
NORM_EPS = 1e-10
N_BLOCKS = len(block_names())
CASES = {"a": (3, 64, 96), "b": (2, 37, 70), "c": (1, 33, 161), "clip": (9, 64, 96)}
SMOOTH_CASES = (2, 3, 4, 5, 9)  # clip lengths the smoothing is recorded for: the first F frames of "clip"
PADS = (0, 10, 0, 0)
SMOOTH_T = 5
MAX_FACES = 16


def fixture_frames(case):
    """frames [n,H,W,3] uint8 RGB: smooth gradients plus blobs and noise, different in every channel and frame.  The detector sees
    u8 / 255 as float32 [n,3,H,W]; the reference sees the bytes, BGR."""
    n, H, W = CASES[case]
    g = torch.Generator().manual_seed(INPUT_SEED + sum(ord(c) for c in case))
    yy, xx = torch.meshgrid(torch.arange(float(H)), torch.arange(float(W)), indexing="ij")
    out = torch.empty(n, H, W, 3)
    for i in range(n):
        cy, cx = (torch.rand(2, generator=g) * torch.tensor([H, W])).tolist()
        blob = torch.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2.0 * (0.2 * min(H, W)) ** 2))
        for c in range(3):
            a, b, p = (torch.rand(3, generator=g) * 0.3).tolist()
            out[i, :, :, c] = 118 + 60 * torch.sin(a * yy + b * xx + 20 * p) + 50 * blob * (c - 1) + 25 * torch.randn(H, W, generator=g)
    return out.clamp(0, 255).to(torch.uint8).numpy()


def frames_f32(u8):
    """[n,H,W,3] uint8 RGB -> the detector's input frames float32 [n,3,H,W] in [0,1]"""
    return (torch.as_tensor(u8).permute(0, 3, 1, 2).float() / 255.0).contiguous()


def prologue(frames, dtype=torch.float64):
    """frames float32 [n,3,H,W] -> 255 u - mean in float64 (rounded once to `dtype`): the kernel's prologue"""
    u = torch.nan_to_num(frames.double(), nan=0.0, posinf=1.0, neginf=0.0).clamp(0.0, 1.0)
    return (255.0 * u - torch.tensor(MEANS, dtype=torch.float64)[None, :, None, None]).to(dtype)


def conv_params(sd, name, dtype):
    return sd[name + ".weight"].to(dtype), sd[name + ".bias"].to(dtype)


def head_names(l):
    return LEVEL_SOURCES[l] + "_mbox_conf", LEVEL_SOURCES[l] + "_mbox_loc"


# ---- one block: b indexes block_names(); float64 or the kernel's arithmetic ------------------------------------------------------
def split(x):
    hi = x.bfloat16().float()
    return hi, (x - hi).bfloat16().float()


def conv64(x, w, bias, stride, pad):
    return F.conv2d(x.double(), w.double(), bias.double(), stride=stride, padding=pad)


def conv_emulated(x, w, bias, stride, pad):
    (xh, xl), (wh, wl) = split(x.float()), split(w.float())
    y = F.conv2d(xl, wh, None, stride=stride, padding=pad)
    y = y + F.conv2d(xh, wl, None, stride=stride, padding=pad)
    y = y + F.conv2d(xh, wh, None, stride=stride, padding=pad)
    return y + bias.float()[None, :, None, None]


def l2norm(x, weight):
    """x / (sqrt(sum_c x^2) + eps) * weight in float64 (net_s3fd.py:16-19)"""
    x = x.double()
    norm = x.pow(2).sum(dim=1, keepdim=True).sqrt() + NORM_EPS
    return x / norm * weight.double().view(1, -1, 1, 1)


def block(sd, b, x, emulated=False):
    """block b on x -> its output: float64, or fp32 by the kernel's arithmetic.  A head pair gives conf then loc columns, without
    the max-out."""
    conv = conv_emulated if emulated else conv64
    dtype = torch.float32 if emulated else torch.float64
    x = x.to(dtype)
    if b < FIRST_POOL:
        name, _, _, _, s, p, _, _ = CONVS[b]
        return torch.relu(conv(x, *conv_params(sd, name, dtype), s, p))
    if b < FIRST_NORM:
        return F.max_pool2d(x, 2, 2)
    if b < FIRST_HEAD:
        return l2norm(x, sd[NORMS[b - FIRST_NORM] + ".weight"]).to(dtype)
    cn, ln = head_names(b - FIRST_HEAD)
    (wc, bc), (wl, bl) = conv_params(sd, cn, dtype), conv_params(sd, ln, dtype)
    return conv(x, torch.cat((wc, wl)), torch.cat((bc, bl)), 1, 1)


def maxout(head, l):
    """a head pair's raw columns -> (cls [n,2,h,w], reg [n,4,h,w]); level 0: net_s3fd.py:124-127"""
    conf = LEVEL_CONF[l]
    cls, reg = head[:, :conf], head[:, conf:]
    if l == 0:
        cls = torch.cat((torch.max(torch.max(cls[:, 0:1], cls[:, 1:2]), cls[:, 2:3]), cls[:, 3:4]), dim=1)
    return cls, reg


def chain(sd, x, emulated=False):
    """x: the mean-subtracted input [n,3,H,W] -> (inputs, outputs) of the 33 blocks in block order, as the network feeds them"""
    ins, outs = [None] * N_BLOCKS, [None] * N_BLOCKS
    with torch.no_grad():
        pool = 0
        for c, (_, _, _, _, _, _, has_pool, level) in enumerate(CONVS):
            ins[c] = x
            x = outs[c] = block(sd, c, x, emulated)
            if level:
                l = level - 1
                src = x
                if l < len(NORMS):
                    ins[FIRST_NORM + l] = x
                    src = outs[FIRST_NORM + l] = block(sd, FIRST_NORM + l, x, emulated)
                ins[FIRST_HEAD + l] = src
                outs[FIRST_HEAD + l] = block(sd, FIRST_HEAD + l, src, emulated)
            if has_pool:
                ins[FIRST_POOL + pool] = x
                x = outs[FIRST_POOL + pool] = block(sd, FIRST_POOL + pool, x, emulated)
                pool += 1
    return ins, outs


def head_maps(outs):
    """[cls1, reg1, .., cls6, reg6] of a chain's outputs: the reference's forward"""
    maps = []
    for l in range(N_LEVELS):
        maps += list(maxout(outs[FIRST_HEAD + l], l))
    return maps


def forward64(sd, x):
    return head_maps(chain(sd, x.double())[1])


# ---- the tail, float64 numpy -----------------------------------------------------------------------------------------------------
def scores_and_boxes(maps):
    """the twelve head maps -> (score [n,P], box [n,P,4]) in float64, positions level-major, then y, then x"""
    scores, boxes = [], []
    for l in range(N_LEVELS):
        cls, reg = maps[2 * l].double(), maps[2 * l + 1].double()
        n, _, h, w = cls.shape
        stride = 4 << l
        m = torch.max(cls[:, 0], cls[:, 1])
        e0, e1 = torch.exp(cls[:, 0] - m), torch.exp(cls[:, 1] - m)
        scores.append((e1 / (e0 + e1)).reshape(n, h * w))
        yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
        ps = float(stride * 4)
        cx = (stride / 2 + xx * stride)[None] + reg[:, 0] * 0.1 * ps
        cy = (stride / 2 + yy * stride)[None] + reg[:, 1] * 0.1 * ps
        bw, bh = ps * torch.exp(reg[:, 2] * 0.2), ps * torch.exp(reg[:, 3] * 0.2)
        cx = cx - bw / 2
        cy = cy - bh / 2
        boxes.append(torch.stack((cx, cy, bw + cx, bh + cy), dim=-1).reshape(n, h * w, 4))
    return torch.cat(scores, dim=1).numpy(), torch.cat(boxes, dim=1).numpy()


def overlap(a, b):
    """bbox.py:44-64's overlap of box a with boxes b [m,4], +1 areas"""
    aa = (a[2] - a[0] + 1) * (a[3] - a[1] + 1)
    ab = (b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1)
    w = np.maximum(0.0, np.minimum(a[2], b[:, 2]) - np.maximum(a[0], b[:, 0]) + 1)
    h = np.maximum(0.0, np.minimum(a[3], b[:, 3]) - np.maximum(a[1], b[:, 1]) + 1)
    return w * h / (aa + ab - w * h)


def greedy_nms(score, box, max_faces=MAX_FACES, visited=None):
    """one image: (dets [k,5] in descending score, left).  The highest remaining score > 0.5 (ties: the lowest position) is kept,
    every remaining position overlapping it by more than 0.3 goes.  `visited`, a list, receives every overlap computed."""
    alive = np.nonzero(score > 0.5)[0]
    dets = []
    while alive.size and len(dets) < max_faces:
        best = alive[np.argmax(score[alive])]  # argmax returns the first of equals: the lowest position
        dets.append(np.concatenate((box[best], score[best:best + 1])))
        rest = alive[alive != best]
        ovr = overlap(box[best], box[rest])
        if visited is not None:
            visited.extend(ovr.tolist())
        alive = rest[ovr <= 0.3]
    return (np.array(dets) if dets else np.zeros((0, 5))), int(alive.size)


def top_rect(dets):
    """api.py:69-77: None, or the top detection clipped at 0 and truncated -> (x1, y1, x2, y2)"""
    if len(dets) == 0:
        return None
    d = np.clip(dets[0], 0, None)
    return tuple(int(v) for v in d[:-1])


def pad_rect(rect, H, W, pads=PADS):
    """data_loader_xgaze_new.py:156-159 -> [x1, y1, x2, y2]"""
    pady1, pady2, padx1, padx2 = pads
    return [max(0, rect[0] - padx1), max(0, rect[1] - pady1), min(W, rect[2] + padx2), min(H, rect[3] + pady2)]


def smooth_boxes(boxes, T):
    """get_smoothened_boxes restated with integers: the window's sum over its length, truncated toward zero, in place"""
    boxes = [list(b) for b in boxes]
    F_ = len(boxes)
    for i in range(F_):
        if i + T > F_:
            start = F_ - T
            if start < 0:
                start = max(0, F_ + start)
            window = boxes[start:]
        else:
            window = boxes[i:i + T]
        boxes[i] = [int(sum(b[c] for b in window) / len(window)) for c in range(4)]  # int() truncates toward zero, as the assignment does
    return boxes


def crop_boxes(rects, H, W, pads=PADS, T=SMOOTH_T):
    """per-frame rects (None: no face -> the whole frame, as strict=False does) -> ([[y1, y2, x1, x2]], found)"""
    found = [r is not None for r in rects]
    padded = [pad_rect(r, H, W, pads) if r is not None else [0, 0, W, H] for r in rects]
    if T:
        padded = smooth_boxes(padded, T)
    return [[b[1], b[3], b[0], b[2]] for b in padded], found


def summary(act):
    """what the fixture keeps of an activation: its sum, its abs-sum and every 211th element"""
    flat = act.double().reshape(-1)
    return float(flat.sum()), float(flat.abs().sum()), flat[::SAMPLE_STRIDE].numpy().copy()


def measured_bounds(sd, frames, ref_ins, ref_outs, ref_maps, ref_score, ref_box):
    """The emulation's error against the reference's float64 values, on the CPU alone: per block max |emulated block(fp32(x_b)) -
    y_b| with x the REFERENCE's activations (each block alone, fed the fp32-rounded reference input), then the emulated chain end
    to end from the float frames: head maps, scores, box coordinates."""
    with torch.no_grad():
        blocks = [float((block(sd, b, ref_ins[b].float(), True).double() - ref_outs[b]).abs().max()) for b in range(N_BLOCKS)]
        maps = head_maps(chain(sd, prologue(frames, torch.float32), True)[1])
    score, box = scores_and_boxes(maps)
    return {"block": blocks, "heads": [float((m.double() - r).abs().max()) for m, r in zip(maps, ref_maps)],
            "score": float(np.abs(score - ref_score).max()), "box": float(np.abs(box - ref_box).max())}
