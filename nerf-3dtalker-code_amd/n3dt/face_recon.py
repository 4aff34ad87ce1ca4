"""The 3-D face reconstruction net on libn3dt: frames to expression codes (the reference's net_recon -- s_face3d/models/networks.py,
ReconNetWrapper over resnet50 with use_last_fc=False -- behind s_face3d/util/preprocess.py's align_img, which its data loader's
CropAndExtract.generate runs on the CPU for every item), frozen and inference-only (n3dt_face_recon_*, csrc/face_recon.hip; DESIGN
section 3.19).

53 convolutions in state-dict order with their BatchNorms folded in, the max pool, the global average and the seven final_layers
as one 2048 -> 257 matrix; in front of them the aligner: five landmarks, the similarity of POS, and the 224 x 224 crop of PIL's
BICUBIC resize computed per output pixel.  `FaceRecon` takes the CALLER'S weights under the keys of `ReconNetWrapper` and the
caller's `lm3d_std`; the pretrained checkpoint has never been run through this code, and the landmarks stay the caller's -- both are
parity unpinned.  There is no CPU path, no training mode and no gradient.
"""
import ctypes

import numpy as np
import torch

from . import ops
from ._host import PackedCache, chunks, count_or_raise, gpu_images, gpu_tensor, only_keys, open_state_dict, pack, take, workspace
from ._lib import FACE_RECON_BLOCKS, FACE_RECON_COEFFS, FaceReconParams, check, lib

LAYERS = (3, 4, 6, 3)
HEAD_COLS = (80, 64, 80, 3, 27, 2, 1)  # id, exp, tex, angle, gamma, (tx, ty), tz: the reference's concatenation order
SPLIT = (("id", 0, 80), ("exp", 80, 144), ("tex", 144, 224), ("angle", 224, 227), ("gamma", 227, 254), ("trans", 254, 257))
FEAT = 2048
COEFFS = sum(HEAD_COLS)
CROP = 224
MIN_HW = 32
BN_EPS = 1e-5  # nn.BatchNorm2d's default, which every module of the reference's ResNet keeps


def _convs():
    """(conv name, bn name, C_in, C_out, kernel, stride, padding, role, ReLU) in state-dict order -- csrc/face_recon_core.h's
    fr_conv holds the same table.  role: 0 stem, 1..3 a bottleneck's conv1..conv3, 4 its downsample branch"""
    out = [("backbone.conv1", "backbone.bn1", 3, 64, 7, 2, 3, 0, True)]
    inplanes = 64
    for layer, blocks in enumerate(LAYERS):
        planes = 64 << layer
        for b in range(blocks):
            stride = 2 if (b == 0 and layer > 0) else 1
            p = "backbone.layer%d.%d." % (layer + 1, b)
            out.append((p + "conv1", p + "bn1", inplanes, planes, 1, 1, 0, 1, True))
            out.append((p + "conv2", p + "bn2", planes, planes, 3, stride, 1, 2, True))
            out.append((p + "conv3", p + "bn3", planes, planes * 4, 1, 1, 0, 3, True))
            if b == 0:
                out.append((p + "downsample.0", p + "downsample.1", inplanes, planes * 4, 1, stride, 0, 4, False))
            inplanes = planes * 4
    return tuple(out)


CONVS = _convs()
N_CONVS = len(CONVS)
POOL_BLOCK, AVG_BLOCK, HEAD_BLOCK = N_CONVS, N_CONVS + 1, N_CONVS + 2
BN_PARTS = ("weight", "bias", "running_mean", "running_var")


def conv_out(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def block_names():
    """the 56 blocks of the single-block entry in its order"""
    return [c[0] for c in CONVS] + ["backbone.maxpool", "backbone.avgpool", "final_layers"]


def block_shape(b, Hi, Wi):
    """(C_in, C_out, Ho, Wo) of block b on an Hi x Wi input"""
    if b < N_CONVS:
        _, _, cin, cout, k, s, p, _, _ = CONVS[b]
        return cin, cout, conv_out(Hi, k, s, p), conv_out(Wi, k, s, p)
    if b == POOL_BLOCK:
        return 64, 64, conv_out(Hi, 3, 2, 1), conv_out(Wi, 3, 2, 1)
    if b == AVG_BLOCK:
        return FEAT, FEAT, 1, 1
    return FEAT, COEFFS, 1, 1


def state_dict_keys():
    """{key: shape} of every tensor of ReconNetWrapper('resnet50', use_last_fc=False), in its state-dict order"""
    keys = {}

    def conv_bn(c):
        conv, bn, cin, cout, k = c[:5]
        keys[conv + ".weight"] = (cout, cin, k, k)
        for part in BN_PARTS:
            keys["%s.%s" % (bn, part)] = (cout,)
        keys[bn + ".num_batches_tracked"] = ()

    for c in CONVS:
        conv_bn(c)
    for i, cols in enumerate(HEAD_COLS):
        keys["final_layers.%d.weight" % i] = (cols, FEAT, 1, 1)
        keys["final_layers.%d.bias" % i] = (cols,)
    return keys


def load_face_recon(obj):
    """([(conv weight, bn weight, bn bias, running mean, running var)] x 53, [(weight, bias)] x 7), fp32 wherever they are, from a
    state dict with the reference's keys, a dict holding one under 'net_recon', or the path of such a file (loaded onto the CPU).
    Strict: a missing key, a key the network does not have and a wrongly shaped tensor are refused with the key;
    num_batches_tracked is accepted (also absent) and ignored."""
    obj = open_state_dict("load_face_recon", obj, unwrap=("net_recon",))
    want = state_dict_keys()
    only_keys("load_face_recon", obj, want)

    def get(key):
        return take("load_face_recon", obj, key, want[key]).float()  # a float32 tensor stays the caller's: its version counter is watched

    convs = [(get(c[0] + ".weight"),) + tuple(get("%s.%s" % (c[1], part)) for part in BN_PARTS) for c in CONVS]
    heads = [(get("final_layers.%d.weight" % i), get("final_layers.%d.bias" % i)) for i in range(len(HEAD_COLS))]
    return convs, heads


def pos_pinv(lm3d_std):
    """POS solves two decoupled 5 x 4 least-squares problems whose matrix [lm3d_std, 1] depends on lm3d_std alone: its
    pseudo-inverse [4,5], float64, on the host"""
    A = np.concatenate((np.asarray(lm3d_std, dtype=np.float64), np.ones((5, 1))), axis=1)
    return np.linalg.pinv(A)


class FaceRecon(object):
    """The reference's `net_recon` behind `align_img`, on libn3dt, with caller-supplied weights (see load_face_recon) and the
    caller's `lm3d_std`, the float64 [5,3] array the reference's load_lm3d returns.

    `net.forward(x)` is `ReconNetWrapper.forward`: [n,3,H,W] -> the 257 coefficients; `net.coeffs(x)` the reference's split_coeff
    dict of views.  `net.align(frames, landmarks)` is align_img as CropAndExtract.generate calls it: float32 RGB frames in [0,1]
    and landmarks [n,68,2] or [n,5,2] in image pixels -> (crops [n,3,224,224], trans_params [n,5] float64, status [n] int32).
    `net.expressions(frames, landmarks)` is the loader's data_info['wav_gen']: [n,64] on the device.  Runs without gradients,
    stream-ordered, without a host synchronisation, bitwise reproducible; a frame's result depends neither on its position in
    the batch nor on how a clip is split into calls.  The weights are packed once per device and again when a weight tensor's
    version has changed -- for float32 tensors, which are held as the caller's.  A tensor of another dtype is converted to a
    float32 copy at construction: an in-place update of such a state dict is NOT seen; build a new FaceRecon (or call it with
    float32 weights)."""

    def __init__(self, weights, lm3d_std):
        self.convs, self.heads = load_face_recon(weights)
        lm = np.array(lm3d_std, dtype=np.float64)
        if lm.shape != (5, 3) or not np.isfinite(lm).all():
            raise ValueError("FaceRecon: lm3d_std must be a finite [5,3] array, got %s" % (lm.shape,))
        self.lm3d_std = lm
        self.pinv = pos_pinv(lm)
        self._packed = PackedCache(lambda: [t for group in self.convs for t in group] + [t for pair in self.heads for t in pair], self._pack)
        self._std = {}
        self.last_geometry = None  # align's integer (w, h, left, up) per frame, int32 [n,4] on the device

    def repack(self):
        self._packed.clear()

    def _pack(self, device, dev):
        p = FaceReconParams()
        for j in range(N_CONVS):
            p.weight[j], p.bn_weight[j], p.bn_bias[j], p.bn_mean[j], p.bn_var[j] = (t.data_ptr() for t in dev[5 * j:5 * j + 5])
            p.bn_eps[j] = BN_EPS
        for i in range(len(HEAD_COLS)):
            p.head_weight[i], p.head_bias[i] = dev[5 * N_CONVS + 2 * i].data_ptr(), dev[5 * N_CONVS + 2 * i + 1].data_ptr()
        return pack("n3dt_face_recon_pack", lib().n3dt_face_recon_packed_bytes(), device, ctypes.byref(p)), dev

    def _packed_for(self, device):
        return self._packed.get(device)

    def _std_for(self, device):
        key = (device.type, device.index)
        if key not in self._std:
            self._std[key] = (torch.as_tensor(self.lm3d_std).to(device).contiguous(), torch.as_tensor(self.pinv).to(device).contiguous())
        return self._std[key]

    @staticmethod
    def max_images(H, W):
        """images of H x W one call takes: the library's workspace budget"""
        return count_or_raise(lib().n3dt_face_recon_max_images(H, W))

    @torch.no_grad()
    def forward(self, x, chunk=None):
        """x [n,3,H,W] float32, 32 <= H, W <= 4096 -> [n,257].  `chunk` caps the images per call (default: the workspace
        budget); results do not depend on it."""
        x = gpu_images("FaceRecon.forward", "x", x, MIN_HW)
        n, _, H, W = x.shape
        dev = x.device
        packed = self._packed_for(dev)
        out = torch.empty(n, COEFFS, dtype=torch.float32, device=dev)
        for i, m in chunks(n, self.max_images(H, W), chunk):
            ws = workspace("face_recon", lib().n3dt_face_recon_workspace_bytes(m, H, W), dev)
            check(lib().n3dt_face_recon_fwd(m, H, W, ops._ptr(packed), ops._ptr(x[i:]), ops._ptr(out[i:]), ops._ptr(ws), ctypes.c_size_t(ws.numel()),
                                            ops._stream()), "n3dt_face_recon_fwd")
        return out

    __call__ = forward

    def coeffs(self, x):
        """the reference's split_coeff of forward(x): views 'id' [n,80], 'exp' [n,64], 'tex' [n,80], 'angle' [n,3], 'gamma' [n,27],
        'trans' [n,3]"""
        full = self.forward(x)
        return {name: full[:, a:b] for name, a, b in SPLIT}

    @torch.no_grad()
    def align(self, frames, landmarks=None, quantize=True):
        """frames [n,3,H,W] float32 RGB in [0,1]; landmarks [n,68,2] or [n,5,2] image pixels (x, y), y down, or None: every frame
        gets the fallback (lm3d_std[:, :2] + 1) / 2 * (W, H) that a frame whose landmarks average exactly -1 gets ->
        (crops [n,3,224,224] float32 in [0,1], trans_params [n,5] float64 = (w0, h0, s, t0, t1), status [n] int32: 1 for non-finite
        landmarks, a resized side < 1 or s outside [1/16, 16]; such a frame's crop is zeros).  quantize=True goes through bytes as
        PIL does (the frame is read as floor(255 u + 0.5), both passes round); False rounds nothing."""
        frames = gpu_images("FaceRecon.align", "frames", frames, 2)
        n, _, H, W = frames.shape
        dev = frames.device
        points = 0
        if landmarks is not None:
            gpu_tensor("FaceRecon.align", "landmarks", landmarks, copy=False)
            if landmarks.dim() != 3 or landmarks.shape[0] != n or landmarks.shape[1] not in (68, 5) or landmarks.shape[2] != 2:
                raise ValueError("FaceRecon.align: landmarks must be [n,68,2] or [n,5,2], got %s" % (tuple(landmarks.shape),))
            landmarks = landmarks.detach().double().contiguous()
            points = landmarks.shape[1]
        lm3d, pinv = self._std_for(dev)
        crops = torch.empty(n, 3, CROP, CROP, dtype=torch.float32, device=dev)
        trans = torch.empty(n, 5, dtype=torch.float64, device=dev)
        geom = torch.empty(n, 4, dtype=torch.int32, device=dev)
        status = torch.empty(n, dtype=torch.int32, device=dev)
        check(lib().n3dt_face_recon_align(n, H, W, ops._ptr(frames), ops._ptr(landmarks), points, ops._ptr(lm3d), ops._ptr(pinv), int(bool(quantize)),
                                          ops._ptr(crops), ops._ptr(trans), ops._ptr(geom), ops._ptr(status), ops._stream()), "n3dt_face_recon_align")
        self.last_geometry = geom
        return crops, trans, status

    def expressions(self, frames, landmarks=None):
        """frames [F,3,H,W] float32 RGB in [0,1] on the GPU (Wav2LipClip.generate's output as it is) -> the 64 expression
        coefficients [F,64] on the device: the loader's data_info['wav_gen'].  `align`'s status is NOT returned: a frame with
        non-finite or degenerate landmarks silently gives the network's answer to an all-zero crop, which nothing tells from a real
        code.  Where the landmarks are not trusted, call `align` and look at its status, then `forward(crops)[:, 80:144]`."""
        crops, _, _ = self.align(frames, landmarks)
        return self.forward(crops)[:, 80:144]

    @torch.no_grad()
    def block(self, b, x, skip=None):
        """block b (0..55, block_names()) alone on x [n, C_in, Hi, Wi] -> [n, C_out, Ho, Wo]; a bottleneck's third convolution
        takes the identity as skip [n, C_out, Ho, Wo]; the average gives [n,2048,1,1], the head takes that and gives [n,257]"""
        if not isinstance(b, int) or not 0 <= b < FACE_RECON_BLOCKS:
            raise ValueError("FaceRecon.block: block must be an integer in 0..55, got %r" % (b,))
        if not torch.is_tensor(x) or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 4:
            raise ValueError("FaceRecon.block: x must be a float32 GPU tensor [n,C,H,W]")
        n, C, Hi, Wi = x.shape
        cin, cout, Ho, Wo = block_shape(b, Hi, Wi)
        if C != cin or n < 1 or Ho < 1 or Wo < 1:
            raise ValueError("FaceRecon.block: block %d takes [n,%d,H,W] with a non-empty output, got %s" % (b, cin, tuple(x.shape)))
        third = b < N_CONVS and CONVS[b][7] == 3
        if third != (skip is not None):
            raise ValueError("FaceRecon.block: a bottleneck's third convolution, and no other block, takes a skip")
        if skip is not None:
            if not torch.is_tensor(skip) or not skip.is_cuda or skip.dtype != torch.float32 or tuple(skip.shape) != (n, cout, Ho, Wo):
                raise ValueError("FaceRecon.block: skip must be a float32 GPU tensor %s" % ((n, cout, Ho, Wo),))
            skip = skip.detach().contiguous()
        x = x.detach().contiguous()
        packed = self._packed_for(x.device)
        ws = workspace("face_recon_block", lib().n3dt_face_recon_block_workspace_bytes(b, n, Hi, Wi), x.device)
        out = torch.empty((n, FACE_RECON_COEFFS) if b == HEAD_BLOCK else (n, cout, Ho, Wo), dtype=torch.float32, device=x.device)
        check(lib().n3dt_face_recon_block(b, n, Hi, Wi, ops._ptr(packed), ops._ptr(x), ops._ptr(skip), ops._ptr(out), ops._ptr(ws),
                                          ctypes.c_size_t(ws.numel()), ops._stream()), "n3dt_face_recon_block")
        return out
