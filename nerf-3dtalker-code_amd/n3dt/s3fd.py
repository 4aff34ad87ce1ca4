"""The S3FD face detector on libn3dt: frames to Wav2Lip crop boxes (the reference's face_detection/detection/sfd under
face_detection/api.py, which its data loader's face_detect runs on the CPU for every frame), frozen and inference-only
(n3dt_s3fd_*, csrc/s3fd.hip).

19 backbone convolutions in state-dict order, five max pools, three L2Norms and six levels' conf / loc heads; then scores, decode
and greedy NMS in float64 on the device, and the loader's pads and box smoothing.  `S3FD` takes the CALLER'S weights under the keys
of `net_s3fd.s3fd`; the pretrained `s3fd-619a316812.pth` has never been run through this code, and the reference feeds byte
frames where this takes float frames -- both are parity unpinned.  There is no CPU path, no training mode and no gradient.
"""
import ctypes

import torch

from . import ops
from ._host import PackedCache, chunks, count_or_raise, gpu_images, only_keys, open_state_dict, pack, take, workspace
from ._lib import S3FD_BLOCKS, S3fdParams, check, lib

# (name, C_in, C_out, kernel, stride, padding, pool behind it, detection level fed) -- csrc/s3fd_core.h holds the same table
CONVS = (
    ("conv1_1", 3, 64, 3, 1, 1, False, 0), ("conv1_2", 64, 64, 3, 1, 1, True, 0),
    ("conv2_1", 64, 128, 3, 1, 1, False, 0), ("conv2_2", 128, 128, 3, 1, 1, True, 0),
    ("conv3_1", 128, 256, 3, 1, 1, False, 0), ("conv3_2", 256, 256, 3, 1, 1, False, 0), ("conv3_3", 256, 256, 3, 1, 1, True, 1),
    ("conv4_1", 256, 512, 3, 1, 1, False, 0), ("conv4_2", 512, 512, 3, 1, 1, False, 0), ("conv4_3", 512, 512, 3, 1, 1, True, 2),
    ("conv5_1", 512, 512, 3, 1, 1, False, 0), ("conv5_2", 512, 512, 3, 1, 1, False, 0), ("conv5_3", 512, 512, 3, 1, 1, True, 3),
    ("fc6", 512, 1024, 3, 1, 3, False, 0), ("fc7", 1024, 1024, 1, 1, 0, False, 4),
    ("conv6_1", 1024, 256, 1, 1, 0, False, 0), ("conv6_2", 256, 512, 3, 2, 1, False, 5),
    ("conv7_1", 512, 128, 1, 1, 0, False, 0), ("conv7_2", 128, 256, 3, 2, 1, False, 6),
)
LEVEL_SOURCES = ("conv3_3_norm", "conv4_3_norm", "conv5_3_norm", "fc7", "conv6_2", "conv7_2")
LEVEL_C = (256, 512, 512, 1024, 512, 256)
LEVEL_CONF = (4, 2, 2, 2, 2, 2)
NORMS = ("conv3_3_norm", "conv4_3_norm", "conv5_3_norm")
N_CONVS, N_POOLS, N_NORMS, N_LEVELS = len(CONVS), 5, 3, 6
FIRST_POOL, FIRST_NORM, FIRST_HEAD = N_CONVS, N_CONVS + N_POOLS, N_CONVS + N_POOLS + N_NORMS
MIN_HW = 32
MEANS = (104.0, 117.0, 123.0)  # on R, G, B in that order: the reference's own quirk (api.py:65, detect.py:59)


def conv_out(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def level_sizes(H, W):
    """[(h, w)] of the six detection levels (strides 4 .. 128) for an H x W frame"""
    out = []
    for _, _, _, k, s, p, pool, level in CONVS:
        H, W = conv_out(H, k, s, p), conv_out(W, k, s, p)
        if level:
            out.append((H, W))
        if pool:
            H, W = H // 2, W // 2
    return out


def positions(H, W):
    return sum(h * w for h, w in level_sizes(H, W))


def block_names():
    """the 33 blocks of the single-block entry in its order"""
    pools = ["pool%d" % (i + 1) for i in range(N_POOLS)]
    return [c[0] for c in CONVS] + pools + list(NORMS) + [s + "_mbox" for s in LEVEL_SOURCES]


def block_shape(b, Hi, Wi):
    """(C_in, C_out, Ho, Wo) of block b on an Hi x Wi input"""
    if b < FIRST_POOL:
        _, cin, cout, k, s, p, _, _ = CONVS[b]
        return cin, cout, conv_out(Hi, k, s, p), conv_out(Wi, k, s, p)
    if b < FIRST_NORM:
        c = [t[2] for t in CONVS if t[6]][b - FIRST_POOL]
        return c, c, Hi // 2, Wi // 2
    if b < FIRST_HEAD:
        return LEVEL_C[b - FIRST_NORM], LEVEL_C[b - FIRST_NORM], Hi, Wi
    return LEVEL_C[b - FIRST_HEAD], LEVEL_CONF[b - FIRST_HEAD] + 4, Hi, Wi


def state_dict_keys():
    """{key: shape} of every tensor of net_s3fd.s3fd, in its state-dict order"""
    keys = {}
    for name, cin, cout, k, _, _, _, _ in CONVS:
        keys[name + ".weight"] = (cout, cin, k, k)
        keys[name + ".bias"] = (cout,)
    for name, c in zip(NORMS, LEVEL_C):
        keys[name + ".weight"] = (c,)
    for src, c, conf in zip(LEVEL_SOURCES, LEVEL_C, LEVEL_CONF):
        for part, n in (("conf", conf), ("loc", 4)):
            keys["%s_mbox_%s.weight" % (src, part)] = (n, c, 3, 3)
            keys["%s_mbox_%s.bias" % (src, part)] = (n,)
    return keys


def load_s3fd(obj):
    """([(weight, bias)] x 31, [norm weight] x 3), fp32 wherever they are, from a state dict with the reference's keys or the
    path of such a file (loaded onto the CPU).  Strict: a missing key, a key the detector does not have and a wrongly shaped
    tensor are refused with the key."""
    obj = open_state_dict("load_s3fd", obj)
    want = state_dict_keys()
    only_keys("load_s3fd", obj, want)

    def get(key):
        return take("load_s3fd", obj, key, want[key]).float()  # a float32 tensor stays the caller's: its version counter is watched

    names = [c[0] for c in CONVS] + ["%s_mbox_%s" % (s, part) for s in LEVEL_SOURCES for part in ("conf", "loc")]
    return [(get(n + ".weight"), get(n + ".bias")) for n in names], [get(n + ".weight") for n in NORMS]


class S3FD(object):
    """The reference's `s3fd` under `SFDDetector` and `FaceAlignment.get_detections_for_batch`, on libn3dt, with caller-supplied
    weights (see load_s3fd).

    `det.forward(x)` is `s3fd.forward`: the mean-subtracted [n,3,H,W] -> [cls1, reg1, .., cls6, reg6].  `det.detect(frames)` takes
    float32 RGB frames in [0,1] and leaves `dets [n,max_faces,5]` (x1, y1, x2, y2, score; float64) and `count [n]` on the device;
    `det.boxes(frames)` gives a whole clip's crop boxes int32 [F,4] = (y1, y2, x1, x2), padded and smoothed as the reference's
    face_detect does, which face_inputs, paste and Wav2LipClip.generate take as they are.  Runs without gradients,
    stream-ordered, bitwise reproducible; a frame's detections depend neither on its position in the batch nor on how a clip is
    split into calls.  The weights are packed once per device and again when a weight tensor's version has changed."""

    def __init__(self, weights):
        self.weights, self.norms = load_s3fd(weights)
        self._packed = PackedCache(lambda: [t for pair in self.weights for t in pair] + self.norms, self._pack)

    def repack(self):
        self._packed.clear()

    def _pack(self, device, dev):
        p, pairs = S3fdParams(), len(self.weights)
        for i in range(pairs):
            p.weight[i], p.bias[i] = dev[2 * i].data_ptr(), dev[2 * i + 1].data_ptr()
        for i, t in enumerate(dev[2 * pairs:]):
            p.norm_weight[i] = t.data_ptr()
        return pack("n3dt_s3fd_pack", lib().n3dt_s3fd_packed_bytes(), device, ctypes.byref(p)), dev

    def _packed_for(self, device):
        return self._packed.get(device)

    @staticmethod
    def max_images(H, W):
        """frames of H x W one call takes: the library's workspace budget"""
        return count_or_raise(lib().n3dt_s3fd_max_images(H, W))

    @staticmethod
    def _workspace(n, H, W, device):
        return workspace("s3fd", lib().n3dt_s3fd_workspace_bytes(n, H, W), device)

    @torch.no_grad()
    def forward(self, x):
        x = gpu_images("S3FD.forward", "x", x, MIN_HW)
        n, _, H, W = x.shape
        dev = x.device
        packed = self._packed_for(dev)
        out = []
        for h, w in level_sizes(H, W):
            out += [torch.empty(n, 2, h, w, dtype=torch.float32, device=dev), torch.empty(n, 4, h, w, dtype=torch.float32, device=dev)]
        for i, m in chunks(n, self.max_images(H, W)):
            ws = self._workspace(m, H, W, dev)
            ptrs = (ctypes.c_void_p * 12)(*[t[i:].data_ptr() for t in out])
            check(lib().n3dt_s3fd_heads(m, H, W, ops._ptr(packed), ops._ptr(x[i:]), ptrs, ops._ptr(ws), ctypes.c_size_t(ws.numel()), ops._stream()),
                  "n3dt_s3fd_heads")
        return out

    __call__ = forward

    @torch.no_grad()
    def detect(self, frames, max_faces=16, scores=False, chunk=None):
        """frames [n,3,H,W] float32 RGB in [0,1] -> (dets [n,max_faces,5] float64, count [n] int32) on the device, without a
        synchronisation; with scores=True also the face score of every head position [n,P] float64 and `left [n]`, the positions
        still standing where max_faces cut the NMS short.  `chunk` caps the frames per call (default: the workspace budget);
        results do not depend on it."""
        frames = gpu_images("S3FD.detect", "frames", frames, MIN_HW)
        n, _, H, W = frames.shape
        dev = frames.device
        packed = self._packed_for(dev)
        dets = torch.empty(n, max_faces, 5, dtype=torch.float64, device=dev)
        count = torch.empty(n, dtype=torch.int32, device=dev)
        left = torch.empty(n, dtype=torch.int32, device=dev)
        sc = torch.empty(n, positions(H, W), dtype=torch.float64, device=dev) if scores else None
        for i, m in chunks(n, self.max_images(H, W), chunk):
            ws = self._workspace(m, H, W, dev)
            check(lib().n3dt_s3fd_detect(m, H, W, ops._ptr(packed), ops._ptr(frames[i:]), int(max_faces), None if sc is None else ops._ptr(sc[i:]),
                                         ops._ptr(dets[i:]), ops._ptr(count[i:]), ops._ptr(left[i:]), ops._ptr(ws), ctypes.c_size_t(ws.numel()),
                                         ops._stream()), "n3dt_s3fd_detect")
        return (dets, count, sc, left) if scores else (dets, count)

    def detect_from_batch(self, frames, max_faces=16):
        """the reference's SFDDetector.detect_from_batch: per frame the list of kept [x1, y1, x2, y2, score] in descending score.
        Synchronises."""
        dets, count = self.detect(frames, max_faces)
        dets, count = dets.cpu().numpy(), count.cpu().numpy()
        return [[dets[i, j] for j in range(int(count[i]))] for i in range(dets.shape[0])]

    def boxes(self, frames, pads=(0, 10, 0, 0), smooth=5, strict=True, chunk=None):
        """A whole clip's crop boxes: frames [F,3,H,W] -> int32 [F,4] = (y1, y2, x1, x2) on the device, from each frame's
        top-scoring detection, clipped at 0 and truncated (api.py:74-76), padded by pads = (pady1, pady2, padx1, padx2) and clamped
        to the frame (data_loader_xgaze_new.py:156-159), then smoothed over `smooth` frames by get_smoothened_boxes literally
        (0 or None: wav_nosmooth).  The clip is detected in chunks of the workspace budget and smoothed as a whole.
        strict=True synchronises once and raises the reference's ValueError naming the first frame without a face.
        strict=False returns (boxes, found) without a synchronisation; a frame without a face enters the smoothing as the whole
        frame -- NOT the reference's behaviour, which raises."""
        frames = gpu_images("S3FD.boxes", "frames", frames, MIN_HW)
        F, _, H, W = frames.shape
        T = int(smooth or 0)
        pads = [int(p) for p in pads]
        if len(pads) != 4:
            raise ValueError("S3FD.boxes: pads must be (pady1, pady2, padx1, padx2)")
        dets, count = self.detect(frames, 1, chunk=chunk)
        dev = frames.device
        out = torch.empty(F, 4, dtype=torch.int32, device=dev)
        found = torch.empty(F, dtype=torch.int32, device=dev)
        scratch = torch.empty(F, 8, dtype=torch.int32, device=dev)
        check(lib().n3dt_s3fd_boxes(F, H, W, 1, ops._ptr(dets), ops._ptr(count), pads[0], pads[1], pads[2], pads[3], T, ops._ptr(out), ops._ptr(found),
                                    ops._ptr(scratch), ops._stream()), "n3dt_s3fd_boxes")
        if not strict:
            return out, found
        missing = (found == 0).nonzero()
        if missing.numel():
            raise ValueError("Face not detected! Ensure the video contains a face in all the frames. (frame %d)" % int(missing[0, 0]))
        return out

    @torch.no_grad()
    def block(self, b, x):
        """block b (0..32, block_names()) alone on x [n, C_in, Hi, Wi] -> [n, C_out, Ho, Wo]; a head pair gives its conf columns,
        then its loc columns, without the max-out"""
        if not isinstance(b, int) or not 0 <= b < S3FD_BLOCKS:
            raise ValueError("S3FD.block: block must be an integer in 0..32, got %r" % (b,))
        if not torch.is_tensor(x) or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 4:
            raise ValueError("S3FD.block: x must be a float32 GPU tensor [n,C,H,W]")
        n, C, Hi, Wi = x.shape
        cin, cout, Ho, Wo = block_shape(b, Hi, Wi)
        if C != cin or n < 1 or Ho < 1 or Wo < 1:
            raise ValueError("S3FD.block: block %d takes [n,%d,H,W] with a non-empty output, got %s" % (b, cin, tuple(x.shape)))
        x = x.detach().contiguous()
        packed = self._packed_for(x.device)
        ws = workspace("s3fd_block", lib().n3dt_s3fd_block_workspace_bytes(b, n, Hi, Wi), x.device)
        out = torch.empty(n, cout, Ho, Wo, dtype=torch.float32, device=x.device)
        check(lib().n3dt_s3fd_block(b, n, Hi, Wi, ops._ptr(packed), ops._ptr(x), ops._ptr(out), ops._ptr(ws), ctypes.c_size_t(ws.numel()),
                                    ops._stream()), "n3dt_s3fd_block")
        return out
