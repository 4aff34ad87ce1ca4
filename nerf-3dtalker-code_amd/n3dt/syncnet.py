"""A lip-sync metric on libn3dt: Wav2Lip's expert `SyncNet_color` (the reference's wav_models/syncnet.py), frozen and
inference-only, and a streaming meter over it (n3dt_syncnet_*, csrc/syncnet.hip).

The network is a 17-block face encoder over windows of five consecutive lower-half face crops ([15,48,96], BGR, channel 3 t + c)
and a 14-block audio encoder over 16-column mel windows ([1,80,16]); each ends in a unit-norm 512-vector and their cosine is the
sync probability.  `SyncNet` takes the CALLER'S weights under the reference's state-dict keys.  The pretrained expert
(`lipsync_expert.pth`) has never been run through this code, and the reference holds no code that feeds the class: the window
convention below (lower half of a 96 x 96 crop, BGR, / 255, five frames along the channels) is written from knowledge of Wav2Lip
and OpenCV's fixed-point byte `resize` is not reproduced -- both are parity unpinned.  What is pinned to the reference's class,
per block and end to end in float64, is every block, the normalisation and the cosine (tests/golden/syncnet.*).
There is no CPU path, no training mode and no gradient.
"""
import ctypes

import torch

from . import ops
from ._host import PackedCache, chunks, gpu_tensor, open_state_dict, pack, take, workspace
from ._lib import SYNCNET_BLOCKS, SyncnetParams, check, lib

# (C_in, C_out, (kh, kw), (sh, sw), padding, residual) of the 31 blocks: 0..16 the face encoder on [15,48,96], 17..30 the audio
# encoder on [1,80,16] (csrc/syncnet_core.h holds the same table for the kernels)
FACE_BLOCKS = (
    (15, 32, (7, 7), (1, 1), 3, False),
    (32, 64, (5, 5), (1, 2), 1, False), (64, 64, (3, 3), (1, 1), 1, True), (64, 64, (3, 3), (1, 1), 1, True),
    (64, 128, (3, 3), (2, 2), 1, False), (128, 128, (3, 3), (1, 1), 1, True), (128, 128, (3, 3), (1, 1), 1, True),
    (128, 128, (3, 3), (1, 1), 1, True),
    (128, 256, (3, 3), (2, 2), 1, False), (256, 256, (3, 3), (1, 1), 1, True), (256, 256, (3, 3), (1, 1), 1, True),
    (256, 512, (3, 3), (2, 2), 1, False), (512, 512, (3, 3), (1, 1), 1, True), (512, 512, (3, 3), (1, 1), 1, True),
    (512, 512, (3, 3), (2, 2), 1, False), (512, 512, (3, 3), (1, 1), 0, False), (512, 512, (1, 1), (1, 1), 0, False),
)
AUDIO_BLOCKS = (
    (1, 32, (3, 3), (1, 1), 1, False), (32, 32, (3, 3), (1, 1), 1, True), (32, 32, (3, 3), (1, 1), 1, True),
    (32, 64, (3, 3), (3, 1), 1, False), (64, 64, (3, 3), (1, 1), 1, True), (64, 64, (3, 3), (1, 1), 1, True),
    (64, 128, (3, 3), (3, 3), 1, False), (128, 128, (3, 3), (1, 1), 1, True), (128, 128, (3, 3), (1, 1), 1, True),
    (128, 256, (3, 3), (3, 2), 1, False), (256, 256, (3, 3), (1, 1), 1, True), (256, 256, (3, 3), (1, 1), 1, True),
    (256, 512, (3, 3), (1, 1), 0, False), (512, 512, (1, 1), (1, 1), 0, False),
)
BLOCKS = FACE_BLOCKS + AUDIO_BLOCKS
FACE_SHAPE, MEL_SHAPE = (15, 48, 96), (1, 80, 16)
EMB = 512
WINDOW_FRAMES = 5
MEL_COLS = 16
MAX_CALL = 128  # windows per launch sequence: bounds the workspace (about 1.5 MB a window); results do not depend on it


def block_names():
    """the state-dict prefix of each of the 31 blocks, in table order"""
    return ["face_encoder.%d" % i for i in range(len(FACE_BLOCKS))] + ["audio_encoder.%d" % i for i in range(len(AUDIO_BLOCKS))]


def block_shapes():
    """[(input [C,H,W], output [C,H,W])] of the 31 blocks"""
    out = []
    for blocks, shape in ((FACE_BLOCKS, FACE_SHAPE), (AUDIO_BLOCKS, MEL_SHAPE)):
        _, h, w = shape
        for cin, cout, (kh, kw), (sh, sw), pad, _ in blocks:
            ho, wo = (h + 2 * pad - kh) // sh + 1, (w + 2 * pad - kw) // sw + 1
            out.append(((cin, h, w), (cout, ho, wo)))
            h, w = ho, wo
    return out


_PARTS = (("conv_block.0.weight", None), ("conv_block.0.bias", 1), ("conv_block.1.weight", 1), ("conv_block.1.bias", 1),
          ("conv_block.1.running_mean", 1), ("conv_block.1.running_var", 1))


def load_syncnet(state_dict):
    """[(weight, bias, bn_weight, bn_bias, running_mean, running_var)] x 31 (fp32, CPU or wherever they are) from a state dict
    with the reference's keys `face_encoder.{i}.conv_block.0.weight|bias`, `face_encoder.{i}.conv_block.1.weight|bias|running_mean|
    running_var` and the same under `audio_encoder`.  A leading `module.` is dropped, `num_batches_tracked` and any other key is
    ignored.  A missing or wrongly shaped tensor is refused with its key."""
    who = "load_syncnet"
    sd = open_state_dict(who, state_dict, strip_module=True, paths=False)
    # a float32 tensor stays the caller's: its version counter is watched
    return [tuple(take(who, sd, "%s.%s" % (name, part), (cout, cin, kh, kw) if dims is None else (cout,)).float() for part, dims in _PARTS)
            for name, (cin, cout, (kh, kw), _, _, _) in zip(block_names(), BLOCKS)]


def _gpu_f32(who, name, t, shape):
    """`t` as a contiguous fp32 GPU tensor [n, *shape]; shape[0] == 1 may be left out"""
    if torch.is_tensor(t) and t.dtype == torch.float32 and shape[0] == 1 and t.dim() == len(shape) and tuple(t.shape[1:]) == tuple(shape[1:]):
        t = t.unsqueeze(1)
    return gpu_tensor(who, name, t, torch.float32, (None,) + tuple(shape), "float32 [n,%s]" % ",".join(str(s) for s in shape), empty="holds no window")


def check_boxes(who, boxes, n_frames, height, width):
    """boxes as a list of n_frames x 4 or 1 x 4 ints, each (y1, y2, x1, x2) with 0 <= y1 < y2 <= height, 0 <= x1 < x2 <= width"""
    if torch.is_tensor(boxes):
        boxes = boxes.tolist()
    boxes = [list(boxes)] if boxes and not isinstance(boxes[0], (list, tuple)) else [list(b) for b in boxes]
    if len(boxes) not in (1, n_frames):
        raise ValueError("%s: boxes must hold one box or one per frame (%d), got %d" % (who, n_frames, len(boxes)))
    for b in boxes:
        if len(b) != 4 or any(int(v) != v for v in b):
            raise ValueError("%s: a box is four integers (y1, y2, x1, x2), got %r" % (who, b))
        y1, y2, x1, x2 = (int(v) for v in b)
        if not (0 <= y1 < y2 <= height and 0 <= x1 < x2 <= width):
            raise ValueError("%s: box %r does not lie inside the %d x %d frame (need 0 <= y1 < y2 <= H, 0 <= x1 < x2 <= W)" % (who, b, height, width))
    return [[int(v) for v in b] for b in boxes]


class SyncNet(object):
    """The reference's `SyncNet_color` in eval mode on libn3dt, with caller-supplied weights (see load_syncnet).

    `net(mel_windows, face_windows) -> (audio_emb, face_emb)`, both [n,512] fp32 and unit-norm: the reference's `forward`.
    mel_windows [n,1,80,16] (or [n,80,16]), face_windows [n,15,48,96], float32 GPU tensors of any strides.
    `net.cos(mel_windows, face_windows)` -> [n] float64, the cosine of the two (computed in float64 before the embeddings are
    rounded to fp32).  `net.cos(mel_windows, frames=..., boxes=...)` builds the face windows from frames [n+4,3,H,W] itself.
    `net.face_windows(frames, boxes)` is that prologue alone; `net.block(b, x)` runs one block, `net.layers(...)` all 31 in turn.
    Stream-ordered, no synchronisation, capturable after a first call, bitwise reproducible; a window's result depends neither on
    its position in the batch nor on the batch size.  Batch norm is folded into the weights when they are packed, once per
    device, and again when a weight tensor's version has changed since (an in-place update); `repack()` forces it."""

    def __init__(self, state_dict):
        self.weights = load_syncnet(state_dict)
        self._packed = PackedCache(lambda: [t for block in self.weights for t in block], self._pack)

    def repack(self):
        self._packed.clear()

    def _pack(self, device, dev):
        p, at = SyncnetParams(), 0
        for i, block in enumerate(self.weights):  # dev holds the blocks' tensors one behind the other
            for (field, _), t in zip(SyncnetParams._fields_, dev[at:at + len(block)]):
                getattr(p, field)[i] = t.data_ptr()
            at += len(block)
        return pack("n3dt_syncnet_pack", lib().n3dt_syncnet_packed_bytes(), device, ctypes.byref(p)), dev

    def _packed_for(self, device):
        return self._packed.get(device)

    @staticmethod
    def _workspace(n, device):
        return workspace("syncnet", lib().n3dt_syncnet_workspace_bytes(n), device)

    @staticmethod
    def _frames(who, frames, boxes, n=None):
        """(frames contiguous, boxes int32 [k,4] on the device, n windows)"""
        gpu_tensor(who, "frames", frames, copy=False)
        if frames.dtype != torch.float32 or frames.dim() != 4 or frames.shape[1] != 3:
            raise ValueError("%s: frames must be float32 [F,3,H,W], got %s %s" % (who, frames.dtype, tuple(frames.shape)))
        F, _, H, W = frames.shape
        if F < WINDOW_FRAMES:
            raise ValueError("%s: a window needs %d consecutive frames, got %d" % (who, WINDOW_FRAMES, F))
        if n is not None and F != n + WINDOW_FRAMES - 1:
            raise ValueError("%s: %d windows need %d frames, got %d" % (who, n, n + WINDOW_FRAMES - 1, F))
        if torch.is_tensor(boxes) and boxes.is_cuda:  # already on the device: the kernel clamps a box into the frame
            if boxes.dtype != torch.int32 or boxes.dim() != 2 or boxes.shape[1] != 4 or boxes.shape[0] not in (1, F):
                raise ValueError("%s: device boxes must be int32 [1,4] or [%d,4], got %s %s" % (who, F, boxes.dtype, tuple(boxes.shape)))
            dev_boxes = boxes.contiguous()
        else:
            dev_boxes = torch.tensor(check_boxes(who, boxes, F, H, W), dtype=torch.int32).to(frames.device)
        return frames.detach().contiguous(), dev_boxes, F - WINDOW_FRAMES + 1

    def face_windows(self, frames, boxes):
        """frames [F,3,H,W] float32 RGB in [0,1] (GPU, any strides) and one crop box (y1, y2, x1, x2) per frame or one for all ->
        the F - 4 face windows [F-4,15,48,96]: each frame cropped, resampled to 96 x 96 bilinearly with half-pixel centres
        (F.interpolate(mode="bilinear", align_corners=False, antialias=False), in float64, rounded once), rows 48..95 kept,
        RGB reversed to BGR, window i = frames i..i+4 along the channels.  Values outside [0,1] are clamped and NaN counts as 0."""
        frames, dev_boxes, n = self._frames("face_windows", frames, boxes)
        out = torch.empty((n,) + FACE_SHAPE, dtype=torch.float32, device=frames.device)
        H, W = frames.shape[2:]
        for i, m in chunks(n, 1024):
            bx = dev_boxes if dev_boxes.shape[0] == 1 else dev_boxes[i:i + m + WINDOW_FRAMES - 1]
            check(lib().n3dt_syncnet_face_windows(m, H, W, ops._ptr(frames[i:]), ops._ptr(bx), bx.shape[0], ops._ptr(out[i:]), ops._stream()),
                  "n3dt_syncnet_face_windows")
        return out

    def _run(self, mel_windows, face_windows=None, frames=None, boxes=None):
        """(audio_emb [n,512] fp32, face_emb [n,512] fp32, cos [n] float64)"""
        who = "SyncNet"
        mel = _gpu_f32(who, "mel_windows", mel_windows, MEL_SHAPE)
        n = mel.shape[0]
        if (face_windows is None) == (frames is None):
            raise ValueError("SyncNet: give face_windows or frames (with boxes), not both and not neither")
        dev_boxes = None
        if frames is None:
            faces = _gpu_f32(who, "face_windows", face_windows, FACE_SHAPE)
            if faces.shape[0] != n or faces.device != mel.device:
                raise ValueError("SyncNet: mel_windows %s and face_windows %s differ in windows or device" % (tuple(mel.shape), tuple(faces.shape)))
        else:
            frames, dev_boxes, _ = self._frames(who, frames, boxes, n)
            if frames.device != mel.device:
                raise ValueError("SyncNet: mel_windows and frames are on different devices")
        dev = mel.device
        packed = self._packed_for(dev)
        a_emb = torch.empty(n, EMB, dtype=torch.float32, device=dev)
        f_emb = torch.empty(n, EMB, dtype=torch.float32, device=dev)
        cos = torch.empty(n, dtype=torch.float64, device=dev)
        L = lib()
        for i, m in chunks(n, MAX_CALL):
            ws = self._workspace(m, dev)
            if frames is None:
                fw, fr, bx, nb, H, W = ops._ptr(faces[i:]), None, None, 0, 0, 0
            else:
                b = dev_boxes if dev_boxes.shape[0] == 1 else dev_boxes[i:i + m + WINDOW_FRAMES - 1]
                fw, fr, bx, nb, H, W = None, ops._ptr(frames[i:]), ops._ptr(b), b.shape[0], frames.shape[2], frames.shape[3]
            check(L.n3dt_syncnet_fwd(m, ops._ptr(packed), ops._ptr(mel[i:]), fw, fr, bx, nb, H, W, ops._ptr(a_emb[i:]), ops._ptr(f_emb[i:]),
                                     ops._ptr(cos[i:]), ops._ptr(ws), ctypes.c_size_t(ws.numel()), ops._stream()), "n3dt_syncnet_fwd")
        return a_emb, f_emb, cos

    def __call__(self, mel_windows, face_windows):
        return self._run(mel_windows, face_windows)[:2]

    def cos(self, mel_windows, face_windows=None, frames=None, boxes=None):
        return self._run(mel_windows, face_windows, frames, boxes)[2]

    def block(self, b, x):
        """block b (0..30) of the table alone on x [n, C_in, H, W] -> [n, C_out, Ho, Wo]; n <= 1024"""
        if not isinstance(b, int) or not 0 <= b < SYNCNET_BLOCKS:
            raise ValueError("SyncNet.block: block must be an integer in 0..30, got %r" % (b,))
        shape_in, shape_out = block_shapes()[b]
        x = _gpu_f32("SyncNet.block", "x", x, shape_in)
        n = x.shape[0]
        packed = self._packed_for(x.device)
        ws = self._workspace(n, x.device)
        out = torch.empty((n,) + shape_out, dtype=torch.float32, device=x.device)
        check(lib().n3dt_syncnet_block(b, n, ops._ptr(packed), ops._ptr(x), ops._ptr(out), ops._ptr(ws), ctypes.c_size_t(ws.numel()), ops._stream()),
              "n3dt_syncnet_block")
        return out

    def layers(self, mel_windows, face_windows):
        """the 31 blocks' activations [n, C, H, W] in table order (face encoder first), each block fed the previous one's output:
        the values the chained network holds, through the single-block entry"""
        x = _gpu_f32("SyncNet.layers", "face_windows", face_windows, FACE_SHAPE)
        m = _gpu_f32("SyncNet.layers", "mel_windows", mel_windows, MEL_SHAPE)
        out = []
        for b in range(SYNCNET_BLOCKS):
            if b == len(FACE_BLOCKS):
                x = m
            x = self.block(b, x)
            out.append(x)
        return out


def window_start(i, fps):
    """the mel column face window i starts at: the reference's crop_audio_window (XGaze_utils/data_loader_xgaze_new.py:324)"""
    return int(80. * (i / float(fps)))


def window_starts(first, count, n_mel_frames, fps):
    """(the mel starts of the kept windows among first .. first + count - 1, how many were dropped): a window whose 16 columns
    would pass the end of the n_mel_frames columns is dropped.  The starts grow with i, so the kept windows come first."""
    kept = []
    for i in range(first, first + count):
        s = window_start(i, fps)
        if s + MEL_COLS <= n_mel_frames:
            kept.append(s)
    return kept, count - len(kept)


def device_starts(first, n, fps, device):
    """window_start(i, fps) for i = first .. first + n - 1 as int32 on `device`, in the same float64 arithmetic (IEEE division and
    product, truncation), without an upload"""
    idx = torch.arange(first, first + n, dtype=torch.float64, device=device)
    return ((idx / float(fps)) * 80.0).to(torch.int32)


class SyncMeter(object):
    """A streaming lip-sync score of a rendered sequence against its audio.

        meter = SyncMeter(syncnet, mel, fps=25.0, box=(y1, y2, x1, x2), max_shift=0)
        for frames in batches:        # consecutive frames [N,3,H,W] float32 RGB in [0,1], GPU, N >= 0, in order
            meter.push(frames)
        meter.result()                # synchronises once

    `mel` is [80,T] on the device (MelFrontend.melspectrogram).  The meter keeps the last four frames, forms every complete
    5-frame window i = 0 .. N - 5 and pairs it with mel columns s .. s + 15, s = int(80. * (i / float(fps))) in Python doubles.
    A window whose mel slice would pass the end of `mel` is dropped and counted, as the reference's get_segmented_mels gives up
    there.  `box` is the mouth-side face crop of every frame (default: the whole frame); choosing it is the caller's.
    result(): {"sync_conf": the mean cosine, "sync_loss": the mean of min(-log cos, 100) (Wav2Lip's BCE against 1 with torch's
    log clamp), "n_windows", "n_dropped"}; with max_shift = S > 0 also "curve": for k = -S..S the mean over i of the cosine of
    face window i with audio window i + k (both among the kept windows; from the fp32 embeddings, in float64), and "offset":
    the k of the curve's maximum.  Without a window the two means are NaN.
    The result does not depend on how the frames were partitioned into pushes, bit for bit: a window's numbers do not depend on
    its batch, and the means are taken once, over all windows, in result()."""

    def __init__(self, syncnet, mel, fps=25.0, box=None, max_shift=0):
        if not isinstance(syncnet, SyncNet):
            raise TypeError("SyncMeter: syncnet must be a SyncNet, got %s" % type(syncnet).__name__)
        gpu_tensor("SyncMeter", "mel", mel, copy=False)
        if mel.dtype not in (torch.float32, torch.float64) or mel.dim() != 2 or mel.shape[0] != 80 or mel.shape[1] < 1:
            raise ValueError("SyncMeter: mel must be float32 or float64 [80, T], got %s %s" % (mel.dtype, tuple(mel.shape)))
        if not float(fps) > 0.0:
            raise ValueError("SyncMeter: fps must be positive, got %r" % (fps,))
        if not isinstance(max_shift, int) or max_shift < 0:
            raise ValueError("SyncMeter: max_shift must be a non-negative integer, got %r" % (max_shift,))
        self.net, self.mel, self.fps, self.max_shift = syncnet, mel.detach().contiguous(), float(fps), max_shift
        self.box = None if box is None else check_boxes("SyncMeter", box, 1, 1 << 30, 1 << 30)[0]
        self._dev_box = None
        self.reset()

    def reset(self):
        self._tail = None            # the last (up to four) frames
        self._seen = 0               # frames pushed so far
        self._next = 0               # the next window index
        self.n_windows = self.n_dropped = 0
        self._cos, self._audio, self._face = [], [], []

    def _box_for(self, frames):
        H, W = frames.shape[2:]
        if self._dev_box is None or self._dev_box[0] != (H, W):
            box = check_boxes("SyncMeter", self.box if self.box is not None else (0, H, 0, W), 1, H, W)
            # filled on the device value by value: an upload would make the host wait
            self._dev_box = ((H, W), torch.cat([torch.full((1,), v, dtype=torch.int32, device=frames.device) for v in box[0]]).reshape(1, 4))
        return self._dev_box[1]

    def push(self, frames):
        if not torch.is_tensor(frames) or not frames.is_cuda:
            raise ValueError("SyncMeter.push: frames must be a GPU tensor (there is no CPU path)")
        if frames.dtype != torch.float32 or frames.dim() != 4 or frames.shape[1] != 3:
            raise ValueError("SyncMeter.push: frames must be float32 [N,3,H,W], got %s %s" % (frames.dtype, tuple(frames.shape)))
        if frames.device != self.mel.device:
            raise ValueError("SyncMeter.push: frames and mel are on different devices")
        if self._tail is not None and self._tail.shape[2:] != frames.shape[2:]:
            raise ValueError("SyncMeter.push: the frame size changed from %s to %s" % (tuple(self._tail.shape[2:]), tuple(frames.shape[2:])))
        if frames.shape[0] == 0:
            return
        frames = frames.detach()
        buf = frames if self._tail is None else torch.cat([self._tail, frames])
        self._seen += frames.shape[0]
        count = self._seen - (WINDOW_FRAMES - 1) - self._next  # complete windows not yet scored; they start at buf[0]
        self._tail = buf[-(WINDOW_FRAMES - 1):].clone() if buf.shape[0] > WINDOW_FRAMES - 1 else buf
        if count <= 0:
            return
        first = self._next
        self._next += count
        kept, dropped = window_starts(first, count, self.mel.shape[1], self.fps)
        self.n_dropped += dropped
        if not kept:
            return
        n = len(kept)  # the starts grow with i: the kept windows are the first n
        self.n_windows += n
        dev = self.mel.device
        start = device_starts(first, n, self.fps, dev)
        T = self.mel.shape[1]
        mel_windows = torch.empty(n, 1, 80, MEL_COLS, dtype=torch.float32, device=dev)
        check(lib().n3dt_mel_windows(T, ops._ptr(self.mel), T, int(self.mel.dtype == torch.float64), n, ops._ptr(start), ops._ptr(mel_windows),
                                     ops._stream()), "n3dt_mel_windows")
        a, f, c = self.net._run(mel_windows, frames=buf[:n + WINDOW_FRAMES - 1], boxes=self._box_for(buf))
        self._cos.append(c)
        if self.max_shift:
            self._audio.append(a)
            self._face.append(f)

    def _device_result(self):
        """float64 [2 + (2 S + 1)] on the device: sync_conf, sync_loss, then the curve"""
        dev = self.mel.device
        if not self._cos:
            return torch.full((2 + (2 * self.max_shift + 1 if self.max_shift else 0),), float("nan"), dtype=torch.float64, device=dev)
        cos = torch.cat(self._cos)
        parts = [cos.mean().reshape(1), torch.clamp(-torch.log(cos), max=100.0).mean().reshape(1)]
        if self.max_shift:
            a, f = torch.cat(self._audio).double(), torch.cat(self._face).double()
            n = cos.shape[0]
            for k in range(-self.max_shift, self.max_shift + 1):
                lo, hi = max(0, -k), min(n, n - k)
                if hi <= lo:
                    parts.append(torch.full((1,), float("nan"), dtype=torch.float64, device=dev))
                else:
                    parts.append((f[lo:hi] * a[lo + k:hi + k]).sum(dim=1).mean().reshape(1))
        return torch.cat(parts)

    def _finish(self, values):
        res = {"sync_conf": values[0], "sync_loss": values[1], "n_windows": self.n_windows, "n_dropped": self.n_dropped}
        if self.max_shift:
            curve = list(values[2:])
            res["curve"] = curve
            finite = [v for v in curve if v == v]
            res["offset"] = (curve.index(max(finite)) - self.max_shift) if finite else 0  # the first maximum, as argmax gives it
        return res

    def result(self):
        return self._finish(self._device_result().tolist())
