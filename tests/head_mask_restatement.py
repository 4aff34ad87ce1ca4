"""A float64 restatement of the head-mask generator the way the reference computes it (DataProcess/BiSeNet.py on
DataProcess/resnet.py; DataProcess/Gen_HeadMask.py's process_single_image over correct_head_mask.py), written from
n3dt.head_mask's table, and an emulation of the arithmetic csrc/head_mask.hip uses.  tests/golden/head_mask*.{npz,json}
(tools/gen_golden_head_mask.py, from the reference's own classes in float64) pins the network; the GPU tests are judged against the
fixture within bounds the tool measured with the emulation.  OpenCV is not installed: the post-process is pinned to scipy.ndimage
piece by piece (tests/test_head_mask_cpu.py), not to OpenCV itself.

  restatement   Conv2d, eval-mode BatchNorm2d by its formula, ReLU, max_pool2d(3, 2, 1), relu(shortcut + residual), the attention
                modules' global averages, 1 x 1 convolutions and sigmoids, F.interpolate(nearest), the concatenation, feat * atten +
                feat, the heads; F.interpolate(bilinear, align_corners=True) and argmax for the reference's labels.  float64.
  emulation     per spatial convolution: BatchNorm folded into weight and bias in float64 and rounded to fp32, input and weights
                split into two bf16 values each, the three products lo*hi + hi*lo + hi*hi as fp32 convolutions, bias, shortcut and
                ReLU in fp32; the fetch transform v * scale + term in fp32 in front of the nearest upsample; the pool in fp32; the
                small stage (mean, 1 x 1 convolution, activation) in float64 from fp32 operands, rounded once.
  label rule    per output pixel the four cells' logits interpolated in float64 by the align_corners weights, first maximum.
  post-process  numpy integers: dilation ignoring out-of-range taps, LUT, largest 8-connected component (root = smallest raster
                index, ties to the smaller root), the hair erosion as N + S + E + W < 4 centre, OpenCV's 8-bit hue.
"""
import numpy as np
import torch
import torch.nn.functional as F

from n3dt.head_mask import (ARM16, ARM16_ATT, ARM32, ARM32_ATT, AVG, BN_EPS, BN_PARTS, CONVS, FFM_1, FFM_2, FFM_BLK, HEAD16, HEAD32, MEAN, N_CONVS, OUT,
                            OUT16, OUT32, POOL_BLOCK, RELU, SIGMOID, SKIP_BLOCKS, SMALL, block_names, default_lut, ellipse)

WEIGHTS_SEED = 3
INPUT_SEED = 83
SAMPLE_STRIDE = 257
N_CLASSES = 19
N_BLOCKS = len(block_names())
CASES = {"a": (2, 64, 64), "b": (1, 88, 72), "c": (3, 42, 104), "d": (65, 32, 32), "real": (1, 512, 512)}
BLOCK_CASES = ("a", "b", "c")
STD = (0.229, 0.224, 0.225)


def fixture_frames(case):
    """frames [n,H,W,3] uint8 RGB: per channel a few smooth blobs over a gradient, plus noise, seeded"""
    n, H, W = CASES[case]
    g = torch.Generator().manual_seed(INPUT_SEED + sum(ord(c) for c in case))
    yy, xx = torch.meshgrid(torch.arange(float(H)) / H, torch.arange(float(W)) / W, indexing="ij")
    out = torch.empty(n, H, W, 3)
    for i in range(n):
        for c in range(3):
            a, b, p = (torch.rand(3, generator=g) * 9.0).tolist()
            out[i, :, :, c] = 118 + 70 * torch.sin(a * yy + b * xx + p) * torch.cos(b * yy - a * xx) + 30 * torch.randn(H, W, generator=g)
    return out.clamp(0, 255).to(torch.uint8).numpy()


def normalise(u8):
    """ToTensor + Normalize in fp32, as the reference's transform computes them: [n,H,W,3] bytes -> [n,3,H,W] float32"""
    x = torch.as_tensor(u8).permute(0, 3, 1, 2).float() / 255.0
    return ((x - torch.tensor(MEAN)[None, :, None, None]) / torch.tensor(STD)[None, :, None, None]).contiguous()


# ---- the network: b indexes block_names() ---------------------------------------------------------------------------------------
def split(x):
    hi = x.bfloat16().float()
    return hi, (x - hi).bfloat16().float()


def bn_params(sd, bn):
    return [sd["%s.%s" % (bn, part)].double() for part in BN_PARTS]


def folded(sd, b):
    """(weight, bias) float64 of convolution b with its eval-mode BatchNorm (if any) folded in: the pack kernel's arithmetic"""
    conv, bn = CONVS[b][:2]
    w = sd[conv + ".weight"].double()
    if bn is None:
        return w, torch.zeros(w.shape[0], dtype=torch.float64)
    gamma, beta, mean, var = bn_params(sd, bn)
    scale = gamma / torch.sqrt(var + BN_EPS)
    return w * scale.view(-1, 1, 1, 1), beta - mean * scale


def activate(y, act):
    return torch.relu(y) if act == RELU else torch.sigmoid(y) if act == SIGMOID else y


def block(sd, b, x, aux=None, scale=None, addvec=None, size=None, emulated=False):
    """block b on x -> its output: float64 as the reference computes it, or fp32 by the kernel's arithmetic.  aux: the shortcut of
    a BasicBlock's conv2, the second half of ffm.convblk's channels, or conv_head16's added map; scale, addvec [n,C]; size: the
    extent x is read at through the nearest rule"""
    dtype = torch.float32 if emulated else torch.float64
    x = x.to(dtype)
    if b == POOL_BLOCK:
        return F.max_pool2d(x, 3, 2, 1)
    conv, bn, _, _, _, s, p, kind, act = CONVS[b]
    if kind == SMALL:
        mean = x.double().mean(dim=(2, 3))
        w, bias = folded(sd, b)
        if emulated:
            return activate(mean @ w.float().double().flatten(1).t() + bias.float().double(), act).float()
        y = F.conv2d(mean[:, :, None, None], sd[conv + ".weight"].double())
        if bn is not None:
            gamma, beta, mu, var = bn_params(sd, bn)
            y = (y - mu.view(1, -1, 1, 1)) / torch.sqrt(var.view(1, -1, 1, 1) + BN_EPS) * gamma.view(1, -1, 1, 1) + beta.view(1, -1, 1, 1)
        return activate(y, act).flatten(1)
    if scale is not None:
        term = addvec.to(dtype)[:, :, None, None] if addvec is not None else aux.to(dtype) if aux is not None else x if b == OUT else 0.0
        x = x * scale.to(dtype)[:, :, None, None] + term
    elif b == FFM_BLK:
        x = torch.cat([x, aux.to(dtype)], dim=1)
    if size is not None and tuple(size) != tuple(x.shape[2:]):
        x = F.interpolate(x, tuple(size), mode="nearest")
    skip = aux if b in SKIP_BLOCKS else None
    if emulated:
        w, bias = folded(sd, b)
        (xh, xl), (wh, wl) = split(x), split(w.float())
        y = F.conv2d(xl, wh, None, stride=s, padding=p)
        y = y + F.conv2d(xh, wl, None, stride=s, padding=p)
        y = y + F.conv2d(xh, wh, None, stride=s, padding=p)
        y = y + bias.float()[None, :, None, None]
        if skip is not None:
            y = y + skip.float()
    else:
        y = F.conv2d(x, sd[conv + ".weight"].double(), None, stride=s, padding=p)
        if bn is not None:
            gamma, beta, mu, var = bn_params(sd, bn)
            y = (y - mu.view(1, -1, 1, 1)) / torch.sqrt(var.view(1, -1, 1, 1) + BN_EPS) * gamma.view(1, -1, 1, 1) + beta.view(1, -1, 1, 1)
        if skip is not None:
            y = skip.double() + y
    return activate(y, act)


def chain(sd, x, emulated=False, outputs=7):
    """x [n,3,H,W] normalised -> (ins, outs): per block its arguments (a dict for block()) and its output, as the network feeds
    them; blocks the selected outputs do not need stay None"""
    ins, outs = [None] * N_BLOCKS, [None] * N_BLOCKS

    def run(b, v, **kw):
        ins[b] = dict(x=v, **kw)
        outs[b] = block(sd, b, v, emulated=emulated, **kw)
        return outs[b]

    with torch.no_grad():
        t = run(POOL_BLOCK, run(0, x))
        b, feats = 1, []
        for layer in range(4):
            for i in range(2):
                down = layer > 0 and i == 0
                y = run(b, t)
                t = run(b + 1, y, aux=run(b + 2, t) if down else t)
                b += 3 if down else 2
            feats.append(t)
        _, f8, f16, f32 = feats
        avg = run(AVG, f32)
        a32 = run(ARM32, f32)
        cp16 = run(HEAD32, a32, scale=run(ARM32_ATT, a32), addvec=avg, size=tuple(f16.shape[2:]))
        if outputs & 3:
            a16 = run(ARM16, f16)
            cp8 = run(HEAD16, a16, scale=run(ARM16_ATT, a16), aux=cp16, size=tuple(f8.shape[2:]))
        if outputs & 1:
            f = run(FFM_BLK, f8, aux=cp8)
            att = run(FFM_2, run(FFM_1, f)[:, :, None, None])
            run(OUT + 1, run(OUT, f, scale=att))
        if outputs & 2:
            run(OUT16 + 1, run(OUT16, cp8))
        if outputs & 4:
            run(OUT32 + 1, run(OUT32, cp16))
    return ins, outs


LOGIT_BLOCKS = (OUT + 1, OUT16 + 1, OUT32 + 1)


def upsample(logits, H, W):
    """the reference's F.interpolate(.., (H, W), mode='bilinear', align_corners=True), float64"""
    return F.interpolate(logits.double(), (H, W), mode="bilinear", align_corners=True)


def lerp_axis(n_in, n_out):
    """(i0, i1, w1) per output index: src = d (in - 1) / (out - 1), float64"""
    scale = (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
    src = scale * np.arange(n_out, dtype=np.float64)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    return i0, np.where(i0 < n_in - 1, i0 + 1, i0), src - i0


def labels_from_logits(logits, H, W):
    """the kernel's label rule: logits [n,C,h,w] (fp32 values) -> uint8 [n,H,W]"""
    lg = np.asarray(logits, dtype=np.float64)
    y0, y1, wy = lerp_axis(lg.shape[2], H)
    x0, x1, wx = lerp_axis(lg.shape[3], W)
    wy, wx = wy[None, None, :, None], wx[None, None, None, :]
    top = lg[:, :, y0][:, :, :, x0] * (1.0 - wx) + lg[:, :, y0][:, :, :, x1] * wx
    bot = lg[:, :, y1][:, :, :, x0] * (1.0 - wx) + lg[:, :, y1][:, :, :, x1] * wx
    return np.argmax((1.0 - wy) * top + wy * bot, axis=1).astype(np.uint8)  # numpy's argmax: the first maximum


def unpack_labels(packed, count):
    """the fixture's five packed bit planes -> uint8 labels [count]"""
    bits = np.unpackbits(packed, axis=1)[:, :count]
    return sum(bits[k].astype(np.uint8) << k for k in range(5))


def margins(up):
    """up [n,C,H,W] float64 -> the top-two margin per pixel"""
    top2 = torch.topk(up, 2, dim=1).values
    return (top2[:, 0] - top2[:, 1]).numpy()


def summary(act):
    """what the fixture keeps of an activation: its sum, its abs-sum and every SAMPLE_STRIDE-th element"""
    flat = act.double().reshape(-1)
    return float(flat.sum()), float(flat.abs().sum()), flat[::SAMPLE_STRIDE].numpy().copy()


def measured_bounds(sd, x, ref_ins, ref_outs):
    """The emulation's error against the reference's float64 values, on the CPU alone: per block max |emulated block(fp32 of the
    REFERENCE's inputs) - reference output|, each block alone, then the emulated chain end to end: the three logit maps"""
    with torch.no_grad():
        blocks = []
        for b in range(N_BLOCKS):
            kw = {k: (v.float() if torch.is_tensor(v) else v) for k, v in ref_ins[b].items()}
            blocks.append(float((block(sd, b, emulated=True, **kw).double() - ref_outs[b]).abs().max()))
        emu = chain(sd, x.float(), True)[1]
    return {"block": blocks, "logits": [float((emu[b].double() - ref_outs[b]).abs().max()) for b in LOGIT_BLOCKS]}


# ---- the post-process, numpy integers -----------------------------------------------------------------------------------------------
def dilate(img, element, anchor, iterations):
    """img uint8 [H,W]: `iterations` dilations by element [eh,ew] anchored at (ay, ax); taps outside the map are ignored"""
    el = np.asarray(element) != 0
    (eh, ew), (ay, ax) = el.shape, anchor
    H, W = img.shape
    cur = img.copy()
    for _ in range(iterations):
        pad = np.zeros((H + eh, W + ew), dtype=np.uint8)
        pad[ay:ay + H, ax:ax + W] = cur
        out = np.zeros_like(cur)
        for i, j in zip(*np.nonzero(el)):
            out = np.maximum(out, pad[i:i + H, j:j + W])  # pixel (y + i - ay, x + j - ax)
        cur = out
    return cur


def component_roots(mask):
    """mask bool [H,W] -> int64 [H,W]: every set pixel's component root, the component's smallest raster index (8-connectivity);
    -1 elsewhere.  Minimum propagation over the 3 x 3 neighbourhood with pointer jumping, until nothing changes."""
    H, W = mask.shape
    big = H * W
    lab = np.where(mask, np.arange(big).reshape(H, W), big)
    while True:
        pad = np.full((H + 2, W + 2), big, dtype=np.int64)
        pad[1:-1, 1:-1] = lab
        m = lab
        for dy in range(3):
            for dx in range(3):
                m = np.minimum(m, pad[dy:dy + H, dx:dx + W])
        m = np.where(mask, m, big)
        flat = np.append(m.reshape(-1), big)
        for _ in range(4):
            flat = flat[flat]
        m = flat[:-1].reshape(H, W)
        if np.array_equal(m, lab):
            break
        lab = m
    return np.where(mask, lab, -1)


def largest_component(img):
    """remover_free_block: img uint8 [H,W] with every non-zero pixel outside the largest 8-connected component of the non-zero
    pixels zeroed; an area tie goes to the smaller root (the reference's `>` keeps the first label)"""
    roots = component_roots(img != 0)
    if not (roots >= 0).any():
        return img.copy()
    counts = np.bincount(roots[roots >= 0])
    return np.where(roots == int(np.argmax(counts)), img, 0).astype(np.uint8)


def erode_hair(img, iterations):
    """erosion_hair_region in integers: with face = 2 and hair = 1 in the working image, a pixel whose ORIGINAL label is hair (2)
    is zeroed when N + S + E + W < 4 centre (zero border); every pass reads the previous pass's image"""
    t = np.where(img == 1, 2, np.where(img == 2, 1, img)).astype(np.int64)
    for _ in range(iterations):
        pad = np.pad(t, 1)
        s = pad[:-2, 1:-1] + pad[2:, 1:-1] + pad[1:-1, :-2] + pad[1:-1, 2:]
        t = np.where((img == 2) & (s < 4 * t), 0, t)
    return np.where(t == 1, 2, np.where(t == 2, 1, t)).astype(np.uint8)


def hue(b, g, r):
    """OpenCV's 8-bit hue (range 180) of cvtColor(.., COLOR_BGR2HSV) for integer arrays b, g, r"""
    b, g, r = (np.asarray(v, dtype=np.int64) for v in (b, g, r))
    v = np.maximum(np.maximum(b, g), r)
    diff = v - np.minimum(np.minimum(b, g), r)
    hdiv = np.zeros(256, dtype=np.int64)
    hdiv[1:] = np.rint((180 << 12) / (6.0 * np.arange(1, 256))).astype(np.int64)
    h = np.where(v == r, g - b, np.where(v == g, b - r + 2 * diff, r - g + 4 * diff))
    h = (h * hdiv[diff] + (1 << 11)) >> 12
    return np.where(h < 0, h + 180, h)


def green(rgb, hue_range=(36, 70)):
    """rgb uint8 [...,3] -> bool: the pixels the reference's green-screen filter clears.  It hands its RGB image to COLOR_BGR2HSV, so
    OpenCV takes the true R as B and the true B as R"""
    h = hue(rgb[..., 0], rgb[..., 1], rgb[..., 2])
    return (h >= hue_range[0]) & (h <= hue_range[1])


def resize_bytes(img, H, W):
    """img uint8 [h,w] or [h,w,C] -> H x W: bilinear with half-pixel centres (src = (d + 0.5) in / out - 0.5, clamped at 0), float64,
    rounded to the nearest byte"""
    def axis(n_in, n_out):
        src = np.maximum((n_in / n_out) * (np.arange(n_out) + 0.5) - 0.5, 0.0)
        i0 = np.minimum(src.astype(np.int64), n_in - 1)
        return i0, np.minimum(i0 + 1, n_in - 1), src - i0
    y0, y1, wy = axis(img.shape[0], H)
    x0, x1, wx = axis(img.shape[1], W)
    v = np.asarray(img, dtype=np.float64)
    shape = (-1, 1) + (1,) * (v.ndim - 2)
    wy, wx = wy.reshape(shape), wx.reshape((1, -1) + (1,) * (v.ndim - 2))
    top = (1.0 - wx) * v[y0][:, x0] + wx * v[y0][:, x1]
    bot = (1.0 - wx) * v[y1][:, x0] + wx * v[y1][:, x1]
    return np.floor((1.0 - wy) * top + wy * bot + 0.5).astype(np.uint8)


def postprocess(labels, rgb, lut=None, element=None, anchor=None, dilations=3, erosions=7, hue_range=(36, 70)):
    """labels uint8 [H,W], rgb uint8 [H,W,3] -> (head, eye) uint8 in {0, 255}: process_single_image behind its argmax"""
    lut = default_lut() if lut is None else lut
    element = ellipse() if element is None else np.asarray(element)
    anchor = (element.shape[0] // 2, element.shape[1] // 2) if anchor is None else anchor
    eye = dilate(np.where((labels == 4) | (labels == 5), 255, 0).astype(np.uint8), element, anchor, dilations)
    res = largest_component(erode_hair(largest_component(lut[labels]), erosions))
    head = np.where((res != 0) & ~green(rgb, hue_range), 255, 0).astype(np.uint8)
    return head, eye & head
