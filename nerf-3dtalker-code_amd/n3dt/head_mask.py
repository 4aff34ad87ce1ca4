"""The head-mask generator on libn3dt: frames to head and eye masks (the reference's DataProcess/Gen_HeadMask.py -- BiSeNet over
ResNet-18, argmax, LUT, largest component, hair erosion, green-screen filter, dilated eye mask -- which writes the `*_mask.png` and
`*_mask_eye.png` its loader reads for every item), frozen and inference-only (n3dt_head_mask_*, csrc/head_mask.hip; DESIGN section
3.21).

36 convolutions in state-dict order with their BatchNorms folded in; the label of a pixel is decided from the low-resolution logits
without the full-resolution volume; the post-process runs on byte maps with integer arithmetic.  `HeadMask` takes the CALLER'S
weights under the keys of `BiSeNet`; the pretrained faceparsing_model.pth has never been run through this code, and OpenCV's
connected-component numbering, ellipse, hue tables and resize are restated from knowledge of them -- all parity unpinned.  There is
no CPU path, no training mode and no gradient.
"""
import ctypes

import numpy as np
import torch

from . import ops
from ._host import PackedCache, chunks, count_or_raise, gpu_images, gpu_tensor, only_keys, open_state_dict, pack, take, workspace
from ._lib import HEAD_MASK_BLOCKS, HEAD_MASK_CONVS, HEAD_MASK_MAX_CLASSES, HeadMaskParams, check, lib

BN_EPS = 1e-5
MIN_HW = 32
BN_PARTS = ("weight", "bias", "running_mean", "running_var")
STEM, SPATIAL, SMALL = 0, 1, 2
NONE, RELU, SIGMOID = 0, 1, 2
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


def _convs():
    """(conv key, bn key or None, C_in, C_out (0: n_classes), kernel, stride, padding, kind, activation) in state-dict order --
    csrc/head_mask_core.h's HM_TABLE holds the same table"""
    out = [("cp.resnet.conv1", "cp.resnet.bn1", 3, 64, 7, 2, 3, STEM, RELU)]
    cin = 64
    for layer, cout in enumerate((64, 128, 256, 512)):
        for b in range(2):
            stride = 2 if (b == 0 and layer > 0) else 1
            p = "cp.resnet.layer%d.%d." % (layer + 1, b)
            out.append((p + "conv1", p + "bn1", cin, cout, 3, stride, 1, SPATIAL, RELU))
            out.append((p + "conv2", p + "bn2", cout, cout, 3, 1, 1, SPATIAL, RELU))
            if cin != cout or stride != 1:
                out.append((p + "downsample.0", p + "downsample.1", cin, cout, 1, stride, 0, SPATIAL, NONE))
            cin = cout
    for arm, c in (("cp.arm16", 256), ("cp.arm32", 512)):
        out.append((arm + ".conv.conv", arm + ".conv.bn", c, 128, 3, 1, 1, SPATIAL, RELU))
        out.append((arm + ".conv_atten", arm + ".bn_atten", 128, 128, 1, 1, 0, SMALL, SIGMOID))
    out.append(("cp.conv_head32.conv", "cp.conv_head32.bn", 128, 128, 3, 1, 1, SPATIAL, RELU))
    out.append(("cp.conv_head16.conv", "cp.conv_head16.bn", 128, 128, 3, 1, 1, SPATIAL, RELU))
    out.append(("cp.conv_avg.conv", "cp.conv_avg.bn", 512, 128, 1, 1, 0, SMALL, RELU))
    out.append(("ffm.convblk.conv", "ffm.convblk.bn", 256, 256, 1, 1, 0, SPATIAL, RELU))
    out.append(("ffm.conv1", None, 256, 64, 1, 1, 0, SMALL, RELU))
    out.append(("ffm.conv2", None, 64, 256, 1, 1, 0, SMALL, SIGMOID))
    for head, c, mid in (("conv_out", 256, 256), ("conv_out16", 128, 64), ("conv_out32", 128, 64)):
        out.append((head + ".conv.conv", head + ".conv.bn", c, mid, 3, 1, 1, SPATIAL, RELU))
        out.append((head + ".conv_out", None, mid, 0, 1, 1, 0, SPATIAL, NONE))
    return tuple(out)


CONVS = _convs()
N_CONVS = len(CONVS)
POOL_BLOCK = N_CONVS
ARM16, ARM16_ATT, ARM32, ARM32_ATT, HEAD32, HEAD16, AVG, FFM_BLK, FFM_1, FFM_2, OUT, OUT16, OUT32 = 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 32, 34
SKIP_BLOCKS = (2, 4, 6, 9, 11, 14, 16, 19)  # a BasicBlock's conv2: relu(shortcut + residual)
assert N_CONVS == HEAD_MASK_CONVS and [c[0] for c in CONVS].index("cp.arm16.conv.conv") == ARM16
assert tuple(b for b, c in enumerate(CONVS) if c[0].endswith(".conv2") and "resnet" in c[0]) == SKIP_BLOCKS


def conv_out(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def block_names():
    """the 37 blocks of the single-block entry in its order"""
    return [c[0] for c in CONVS] + ["cp.resnet.maxpool"]


def block_shape(b, Hi, Wi, n_classes=19):
    """(C_in, C_out, Ho, Wo) of block b on an Hi x Wi input (a small block: Ho = Wo = 1)"""
    if b == POOL_BLOCK:
        return 64, 64, conv_out(Hi, 3, 2, 1), conv_out(Wi, 3, 2, 1)
    _, _, cin, cout, k, s, p, kind, _ = CONVS[b]
    cout = cout or n_classes
    if kind == SMALL:
        return cin, cout, 1, 1
    return cin, cout, conv_out(Hi, k, s, p), conv_out(Wi, k, s, p)


def feature_sizes(H, W):
    """((H2, W2), (H4, W4), (H8, W8), (H16, W16), (H32, W32)): the stem's and the pool's outputs and the three feature maps"""
    out = [(conv_out(H, 7, 2, 3), conv_out(W, 7, 2, 3))]
    for _ in range(4):
        out.append((conv_out(out[-1][0], 3, 2, 1), conv_out(out[-1][1], 3, 2, 1)))
    return tuple(out)


def logit_size(H, W, output):
    """the low-resolution size of output 0 (out), 1 (out16) -- both 1/8 -- or 2 (out32, 1/16)"""
    z = feature_sizes(H, W)
    return z[3] if output == 2 else z[2]


def state_dict_keys(n_classes=19):
    """{key: shape} of every tensor of BiSeNet(n_classes), in its state-dict order"""
    keys = {}
    for conv, bn, cin, cout, k, _, _, _, _ in CONVS:
        cout = cout or n_classes
        keys[conv + ".weight"] = (cout, cin, k, k)
        if bn is not None:
            for part in BN_PARTS:
                keys["%s.%s" % (bn, part)] = (cout,)
            keys[bn + ".num_batches_tracked"] = ()
    return keys


def load_head_mask(obj, n_classes=19):
    """[(conv weight, bn weight, bn bias, running mean, running var) or (conv weight,)] x 36, fp32 wherever they are, from a state
    dict with the reference's keys or the path of such a file (faceparsing_model.pth, loaded onto the CPU).  Strict: a missing
    key, a key the network does not have and a wrongly shaped tensor are refused with the key; num_batches_tracked is accepted
    (also absent) and ignored."""
    obj = open_state_dict("load_head_mask", obj)
    want = state_dict_keys(n_classes)
    only_keys("load_head_mask", obj, want)

    def get(key):
        return take("load_head_mask", obj, key, want[key]).float()  # a float32 tensor stays the caller's: its version counter is watched

    return [(get(c[0] + ".weight"),) + (tuple(get("%s.%s" % (c[1], part)) for part in BN_PARTS) if c[1] else ()) for c in CONVS]


def ellipse(rows=20, cols=20):
    """OpenCV's getStructuringElement(MORPH_ELLIPSE, (cols, rows)) from knowledge of it: row i spans c - dx .. c + dx with
    dx = round(c sqrt((r^2 - dy^2) / r^2)), r = rows // 2, c = cols // 2, dy = i - r; uint8 [rows, cols]; its default anchor is (c, r)"""
    r, c = rows // 2, cols // 2
    inv_r2 = 1.0 / (r * r) if r else 0.0
    out = np.zeros((rows, cols), dtype=np.uint8)
    for i in range(rows):
        dy = i - r
        if abs(dy) <= r:
            dx = int(np.rint(c * np.sqrt((r * r - dy * dy) * inv_r2)))
            out[i, max(c - dx, 0):min(c + dx + 1, cols)] = 1
    return out


def default_lut():
    """labels 1..13 -> 1 (face, neck), 17 -> 2 (hair), everything else 0"""
    lut = np.zeros(256, dtype=np.uint8)
    lut[1:14] = 1
    lut[17] = 2
    return lut


def _bytes(who, name, x, dims):
    return gpu_tensor(who, name, x, torch.uint8, (None,) * dims, "a uint8 tensor of %d dimensions" % dims)


class HeadMask(object):
    """The reference's GenHeadMask on libn3dt, with caller-supplied weights (see load_head_mask).

    `net.forward(x)` is `BiSeNet.forward` on a normalised [n,3,H,W]: (out, out16, out32), each [n,n_classes,H,W];
    `net.logits(x, output)` the low-resolution map in front of the upsample; `net.parse(frames)` the uint8 label map the reference
    takes from output `output` (2: pred_res[2]); `net.postprocess(labels, rgb)` and `net.masks(frames)` give (head, eye), uint8
    [F,H,W] in {0, 255} on the device.  Frames are uint8 [F,H,W,3] RGB, or float [F,3,H,W] in [0,1], rounded to bytes once.
    `size`: the side the reference resizes every image to (512) in front of the network: frames of another size are resized to
    size x size through bytes (half-pixel bilinear, not OpenCV's fixed-point INTER_LINEAR), parsed and post-processed there, and the
    masks resized back to the frame's own (H, W) -- the reference's `width, height, _ = img.shape` swap, which transposes the output
    size of non-square frames, is not copied.  At size x size frames both resizes are identities, the pinned case.  size=None parses
    frames at their own size.  Runs without gradients, stream-ordered, without a host synchronisation, bitwise reproducible; a frame's result
    depends neither on its position in the batch nor on how a clip is split into calls."""

    def __init__(self, weights, n_classes=19, output=2, size=512, eye_element=None, hue_range=(36, 70), erosion_iters=7, lut=None, dilations=3):
        if not isinstance(n_classes, int) or not 1 <= n_classes <= HEAD_MASK_MAX_CLASSES:
            raise ValueError("HeadMask: n_classes must be an integer in 1..32, got %r" % (n_classes,))
        if output not in (0, 1, 2):
            raise ValueError("HeadMask: output must be 0 (out), 1 (out16) or 2 (out32), got %r" % (output,))
        if size is not None and (not isinstance(size, int) or not MIN_HW <= size <= 4096):
            raise ValueError("HeadMask: size must be None or an integer in 32..4096, got %r" % (size,))
        self.n_classes, self.output, self.size = n_classes, output, size
        self.convs = load_head_mask(weights, n_classes)
        el = ellipse() if eye_element is None else np.ascontiguousarray(np.asarray(eye_element) != 0, dtype=np.uint8)
        if el.ndim != 2 or not (1 <= el.shape[0] <= 64 and 1 <= el.shape[1] <= 64):
            raise ValueError("HeadMask: eye_element must be a 2-D array at most 64 x 64, got shape %s" % (el.shape,))
        self.element, self.anchor = el, (el.shape[0] // 2, el.shape[1] // 2)
        lo, hi = (int(v) for v in hue_range)
        if not 0 <= lo <= hi <= 255:
            raise ValueError("HeadMask: hue_range must be 0 <= lo <= hi <= 255, got %r" % (hue_range,))
        self.hue_range = (lo, hi)
        if not isinstance(erosion_iters, int) or not 0 <= erosion_iters <= 1024 or not isinstance(dilations, int) or not 0 <= dilations <= 64:
            raise ValueError("HeadMask: erosion_iters must be in 0..1024 and dilations in 0..64")
        self.erosion_iters, self.dilations = erosion_iters, dilations
        lut = default_lut() if lut is None else np.ascontiguousarray(np.asarray(lut))
        if lut.shape != (256,) or lut.dtype != np.uint8:
            raise ValueError("HeadMask: lut must be a uint8 array of 256 entries")
        self.lut = lut
        self._packed, self._consts = PackedCache(lambda: [t for group in self.convs for t in group], self._pack), {}

    def repack(self):
        self._packed.clear()

    def _pack(self, device, dev):
        p, at = HeadMaskParams(), 0
        p.n_classes, p.bn_eps = self.n_classes, BN_EPS
        for j, group in enumerate(self.convs):
            p.weight[j] = dev[at].data_ptr()
            if len(group) > 1:
                p.bn_weight[j], p.bn_bias[j], p.bn_mean[j], p.bn_var[j] = (t.data_ptr() for t in dev[at + 1:at + 5])
            at += len(group)
        return pack("n3dt_head_mask_pack", lib().n3dt_head_mask_packed_bytes(), device, ctypes.byref(p)), dev

    def _packed_for(self, device):
        return self._packed.get(device)

    def _consts_for(self, device):
        key = (device.type, device.index)
        if key not in self._consts:
            self._consts[key] = (torch.as_tensor(self.lut).to(device), torch.as_tensor(self.element).to(device).contiguous())
        return self._consts[key]

    @staticmethod
    def max_images(H, W):
        """images of H x W one call takes: the library's workspace budget"""
        return count_or_raise(lib().n3dt_head_mask_max_images(H, W))

    def _run(self, x, outputs, upsample, chunk):
        n, _, H, W = x.shape
        dev = x.device
        packed = self._packed_for(dev)
        outs = [None, None, None]
        for o in range(3):
            if outputs & (1 << o):
                h, w = (H, W) if upsample else logit_size(H, W, o)
                outs[o] = torch.empty(n, self.n_classes, h, w, dtype=torch.float32, device=dev)
        for i, m in chunks(n, self.max_images(H, W), chunk):
            ws = workspace("head_mask", lib().n3dt_head_mask_workspace_bytes(m, H, W), dev)
            ptrs = [ops._ptr(None if t is None else t[i:]) for t in outs]
            check(lib().n3dt_head_mask_fwd(m, H, W, self.n_classes, ops._ptr(packed), ops._ptr(x[i:]), outputs, int(upsample), ptrs[0], ptrs[1], ptrs[2],
                                           ops._ptr(ws), ctypes.c_size_t(ws.numel()), ops._stream()), "n3dt_head_mask_fwd")
        return outs

    @torch.no_grad()
    def forward(self, x, chunk=None):
        """x [n,3,H,W] float32, normalised, 32 <= H, W <= 4096 -> (out, out16, out32), each [n,n_classes,H,W]: the class's own
        outputs.  `chunk` caps the images per call; results do not depend on it."""
        return tuple(self._run(gpu_images("HeadMask.forward", "x", x, MIN_HW), 7, True, chunk))

    __call__ = forward

    @torch.no_grad()
    def logits(self, x, output=None, chunk=None):
        """the low-resolution logits [n,n_classes,h,w] of output 0, 1 or 2 (default: the constructor's); only what that output
        needs is run"""
        output = self.output if output is None else output
        if output not in (0, 1, 2):
            raise ValueError("HeadMask.logits: output must be 0, 1 or 2, got %r" % (output,))
        return self._run(gpu_images("HeadMask.logits", "x", x, MIN_HW), 1 << output, False, chunk)[output]

    @torch.no_grad()
    def frames(self, frames):
        """uint8 [F,H,W,3] RGB or float [F,3,H,W] in [0,1] -> (rgb uint8 [F,H,W,3], x float32 [F,3,H,W] normalised as ToTensor +
        Normalize do)"""
        frames = gpu_tensor("HeadMask.frames", "frames", frames)
        if frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[3] == 3:
            F, H, W, is_float = frames.shape[0], frames.shape[1], frames.shape[2], 0
        elif frames.is_floating_point() and frames.dim() == 4 and frames.shape[1] == 3:
            frames = frames.float().contiguous()
            F, H, W, is_float = frames.shape[0], frames.shape[2], frames.shape[3], 1
        else:
            raise ValueError("HeadMask.frames: frames must be uint8 [F,H,W,3] or float [F,3,H,W], got %s %s" % (frames.dtype, tuple(frames.shape)))
        if F < 1 or H < 1 or W < 1:
            raise ValueError("HeadMask.frames: empty frames")
        rgb = torch.empty(F, H, W, 3, dtype=torch.uint8, device=frames.device)
        x = torch.empty(F, 3, H, W, dtype=torch.float32, device=frames.device)
        check(lib().n3dt_head_mask_frames(F, H, W, ops._ptr(frames), is_float, ops._ptr(rgb), ops._ptr(x), ops._stream()), "n3dt_head_mask_frames")
        return rgb, x

    @torch.no_grad()
    def labels(self, logits, H, W):
        """low-resolution logits [n,C,h,w] float32 -> uint8 [n,H,W]: the argmax of their bilinear (align_corners) interpolation"""
        logits = gpu_tensor("HeadMask.labels", "logits", logits)
        if logits.dtype != torch.float32 or logits.dim() != 4 or not 1 <= logits.shape[1] <= 256:
            raise ValueError("HeadMask.labels: logits must be float32 [n,C,h,w] with C <= 256, got %s %s" % (logits.dtype, tuple(logits.shape)))
        n, C, h, w = logits.shape
        out = torch.empty(n, H, W, dtype=torch.uint8, device=logits.device)
        check(lib().n3dt_head_mask_labels(n, C, h, w, H, W, ops._ptr(logits), ops._ptr(out), ops._stream()), "n3dt_head_mask_labels")
        return out

    @torch.no_grad()
    def resize(self, img, H, W):
        """uint8 [F,h,w] or [F,h,w,C] -> the same at H x W: half-pixel bilinear in float64, rounded to the nearest byte"""
        img = gpu_tensor("HeadMask.resize", "img", img)
        if img.dtype != torch.uint8 or img.dim() not in (3, 4) or img.shape[0] < 1 or (img.dim() == 4 and not 1 <= img.shape[3] <= 4):
            raise ValueError("HeadMask.resize: img must be uint8 [F,h,w] or [F,h,w,C] with C <= 4, got %s %s" % (img.dtype, tuple(img.shape)))
        C = img.shape[3] if img.dim() == 4 else 1
        out = torch.empty((img.shape[0], H, W) + tuple(img.shape[3:]), dtype=torch.uint8, device=img.device)
        check(lib().n3dt_head_mask_resize(img.shape[0], img.shape[1], img.shape[2], C, ops._ptr(img), H, W, ops._ptr(out), ops._stream()),
              "n3dt_head_mask_resize")
        return out

    def _network_frames(self, frames):
        """(rgb, x) at the size the network runs at"""
        rgb, x = self.frames(frames)
        if self.size is not None and tuple(rgb.shape[1:3]) != (self.size, self.size):
            rgb, x = self.frames(self.resize(rgb, self.size, self.size))
        return rgb, x

    @torch.no_grad()
    def parse(self, frames, chunk=None):
        """frames -> uint8 labels at the size the network runs at ([F,size,size], or the frames' own with size=None): argmax of
        output `output`, as the reference takes it from pred_res[2]"""
        rgb, x = self._network_frames(frames)
        return self.labels(self.logits(x, chunk=chunk), x.shape[2], x.shape[3])

    @torch.no_grad()
    def green(self, rgb):
        """rgb uint8 [F,H,W,3] -> uint8 [F,H,W]: 255 on the pixels the green-screen filter clears"""
        rgb = _bytes("HeadMask.green", "rgb", rgb, 4)
        if rgb.shape[3] != 3:
            raise ValueError("HeadMask.green: rgb must be [F,H,W,3]")
        F, H, W, _ = rgb.shape
        out = torch.empty(F, H, W, dtype=torch.uint8, device=rgb.device)
        check(lib().n3dt_head_mask_green(F, H, W, ops._ptr(rgb), self.hue_range[0], self.hue_range[1], ops._ptr(out), ops._stream()), "n3dt_head_mask_green")
        return out

    @torch.no_grad()
    def postprocess(self, labels, rgb):
        """labels uint8 [F,H,W], rgb uint8 [F,H,W,3] -> (head, eye) uint8 [F,H,W] in {0, 255}"""
        labels = _bytes("HeadMask.postprocess", "labels", labels, 3)
        rgb = _bytes("HeadMask.postprocess", "rgb", rgb, 4)
        F, H, W = labels.shape
        if tuple(rgb.shape) != (F, H, W, 3) or rgb.device != labels.device:
            raise ValueError("HeadMask.postprocess: rgb must be %s on the labels' device, got %s" % ((F, H, W, 3), tuple(rgb.shape)))
        dev = labels.device
        lut, element = self._consts_for(dev)
        head = torch.empty(F, H, W, dtype=torch.uint8, device=dev)
        eye = torch.empty(F, H, W, dtype=torch.uint8, device=dev)
        ws = workspace("head_mask_post", lib().n3dt_head_mask_postprocess_workspace_bytes(F, H, W), dev)
        check(lib().n3dt_head_mask_postprocess(F, H, W, ops._ptr(labels), ops._ptr(rgb), ops._ptr(lut), ops._ptr(element), self.element.shape[0],
                                               self.element.shape[1], self.anchor[0], self.anchor[1], self.dilations, self.erosion_iters,
                                               self.hue_range[0], self.hue_range[1], ops._ptr(head), ops._ptr(eye), ops._ptr(ws),
                                               ctypes.c_size_t(ws.numel()), ops._stream()), "n3dt_head_mask_postprocess")
        return head, eye

    @torch.no_grad()
    def masks(self, frames, chunk=None):
        """frames -> (head, eye), uint8 [F,H,W] with values 0 / 255, left on the device: what the reference writes to `*_mask.png`
        and `*_mask_eye.png`.  Chunked by max_images (or `chunk`); chunking does not change a bit."""
        frames = gpu_tensor("HeadMask.masks", "frames", frames)
        own = tuple(frames.shape[1:3]) if frames.dtype == torch.uint8 else tuple(frames.shape[2:4])
        rgb, x = self._network_frames(frames)
        F, _, H, W = x.shape
        if H < MIN_HW or W < MIN_HW:
            raise ValueError("HeadMask.masks: frames must be at least 32 x 32")
        head = torch.empty(F, H, W, dtype=torch.uint8, device=x.device)
        eye = torch.empty(F, H, W, dtype=torch.uint8, device=x.device)
        for i, m in chunks(F, self.max_images(H, W), chunk):
            lab = self.labels(self.logits(x[i:i + m]), H, W)
            head[i:i + m], eye[i:i + m] = self.postprocess(lab, rgb[i:i + m])
        if own != (H, W):
            head, eye = self.resize(head, own[0], own[1]), self.resize(eye, own[0], own[1])
        return head, eye

    @torch.no_grad()
    def block(self, b, x, aux=None, scale=None, addvec=None, size=None):
        """block b (0..36, block_names()) alone on x [n,C_in,Hs,Ws].  `size` (Hi, Wi): blocks 24 and 25 read x through torch's
        nearest rule as an Hi x Wi map.  aux: the shortcut of a BasicBlock's conv2, the second 128 channels of block 27's input,
        or with `scale` block 25's added map; scale, addvec [n,C_in]: the fetched value v becomes v * scale + (addvec | aux | v on
        block 30 | 0).  A small block gives [n,C_out]."""
        if not isinstance(b, int) or not 0 <= b < HEAD_MASK_BLOCKS:
            raise ValueError("HeadMask.block: block must be an integer in 0..36, got %r" % (b,))
        x = gpu_tensor("HeadMask.block", "x", x)
        if x.dtype != torch.float32 or x.dim() != 4:
            raise ValueError("HeadMask.block: x must be a float32 GPU tensor [n,C,H,W]")
        n, C, Hs, Ws = x.shape
        Hi, Wi = (Hs, Ws) if size is None else (int(size[0]), int(size[1]))
        cin, cout, Ho, Wo = block_shape(b, Hi, Wi, self.n_classes)
        if C != (128 if b == FFM_BLK else cin) or n < 1 or Ho < 1 or Wo < 1:
            raise ValueError("HeadMask.block: block %d takes [n,%d,H,W] with a non-empty output, got %s" % (b, cin, tuple(x.shape)))
        small = b < N_CONVS and CONVS[b][7] == SMALL
        extra = []
        for name, t, shape in (("aux", aux, None), ("scale", scale, (n, cin)), ("addvec", addvec, (n, cin))):
            if t is not None:
                t = gpu_tensor("HeadMask.block", name, t)
                if t.dtype != torch.float32 or (shape is not None and tuple(t.shape) != shape):
                    raise ValueError("HeadMask.block: %s must be float32 %s" % (name, shape or "[n,C,H,W]"))
            extra.append(t)
        aux, scale, addvec = extra
        if aux is not None:
            want = (n, cout, Ho, Wo) if b in SKIP_BLOCKS else (n, 128, Hs, Ws)
            if tuple(aux.shape) != want:
                raise ValueError("HeadMask.block: aux must be %s, got %s" % (want, tuple(aux.shape)))
        packed = self._packed_for(x.device)
        ws = workspace("head_mask_block", lib().n3dt_head_mask_block_workspace_bytes(b, n, Hi, Wi, Hs, Ws), x.device)
        out = torch.empty((n, cout) if small else (n, cout, Ho, Wo), dtype=torch.float32, device=x.device)
        check(lib().n3dt_head_mask_block(b, n, Hi, Wi, Hs, Ws, self.n_classes, ops._ptr(packed), ops._ptr(x), ops._ptr(aux), ops._ptr(scale),
                                         ops._ptr(addvec), ops._ptr(out), ops._ptr(ws), ctypes.c_size_t(ws.numel()), ops._stream()),
              "n3dt_head_mask_block")
        return out
