"""Wav2Lip's generator on libn3dt: audio-driven lip-synced 96 x 96 faces (the reference's wav_models/wav2lip.py, which its data
loader runs on the CPU for every item), frozen and inference-only (n3dt_wav2lip_*, csrc/wav2lip.hip).

51 blocks in state-dict order: an 18-block face encoder over [6,96,96] (the masked target crop and a reference crop, BGR) whose
seven groups' outputs are kept as skip features, a 13-block audio encoder over mel windows [1,80,16], an 18-block decoder (six
ConvTranspose2d blocks; behind each of its seven groups the skip feature is concatenated), Conv2d(80,32,3) and the plain
nn.Conv2d(32,3,1) with its sigmoid.  `Wav2Lip` takes the CALLER'S weights under the reference's state-dict keys; the pretrained
`wav2lip.pth` has never been run through this code and OpenCV's byte `resize` is not reproduced -- both are parity unpinned.
What is pinned to the reference's class, per block and end to end in float64, is every block, the concatenations and the sigmoid
(tests/golden/wav2lip.*).  There is no CPU path, no training mode and no gradient.
"""
import ctypes

import numpy as np
import torch

from . import ops
from ._host import PackedCache, chunks, gpu_tensor, only_keys, open_state_dict, pack, take, workspace
from ._lib import WAV2LIP_BLOCKS, Wav2lipParams, check, lib
from .syncnet import check_boxes

FACE_GROUPS = (1, 3, 4, 3, 3, 2, 2)
DECODER_GROUPS = (1, 2, 3, 3, 3, 3, 3)


def _c(cin, cout, k, s, p, res=False):
    s = s if isinstance(s, tuple) else (s, s)
    return (False, cin, cout, (k, k), s, p, 0, res)


def _t(cin, cout, k, s, p, op=0):
    return (True, cin, cout, (k, k), (s, s), p, op, False)


# (transposed, C_in, C_out, (kh, kw), (sh, sw), padding, output_padding, residual) of the 51 blocks (csrc/wav2lip_core.h holds the
# same table for the kernels): 0..17 the face encoder, 18..30 the audio encoder, 31..48 the decoder, 49..50 the output block
FACE_BLOCKS = (
    _c(6, 16, 7, 1, 3),
    _c(16, 32, 3, 2, 1), _c(32, 32, 3, 1, 1, True), _c(32, 32, 3, 1, 1, True),
    _c(32, 64, 3, 2, 1), _c(64, 64, 3, 1, 1, True), _c(64, 64, 3, 1, 1, True), _c(64, 64, 3, 1, 1, True),
    _c(64, 128, 3, 2, 1), _c(128, 128, 3, 1, 1, True), _c(128, 128, 3, 1, 1, True),
    _c(128, 256, 3, 2, 1), _c(256, 256, 3, 1, 1, True), _c(256, 256, 3, 1, 1, True),
    _c(256, 512, 3, 2, 1), _c(512, 512, 3, 1, 1, True),
    _c(512, 512, 3, 1, 0), _c(512, 512, 1, 1, 0),
)
AUDIO_BLOCKS = (
    _c(1, 32, 3, 1, 1), _c(32, 32, 3, 1, 1, True), _c(32, 32, 3, 1, 1, True),
    _c(32, 64, 3, (3, 1), 1), _c(64, 64, 3, 1, 1, True), _c(64, 64, 3, 1, 1, True),
    _c(64, 128, 3, 3, 1), _c(128, 128, 3, 1, 1, True), _c(128, 128, 3, 1, 1, True),
    _c(128, 256, 3, (3, 2), 1), _c(256, 256, 3, 1, 1, True),
    _c(256, 512, 3, 1, 0), _c(512, 512, 1, 1, 0),
)
DECODER_BLOCKS = (
    _c(512, 512, 1, 1, 0),
    _t(1024, 512, 3, 1, 0), _c(512, 512, 3, 1, 1, True),
    _t(1024, 512, 3, 2, 1, 1), _c(512, 512, 3, 1, 1, True), _c(512, 512, 3, 1, 1, True),
    _t(768, 384, 3, 2, 1, 1), _c(384, 384, 3, 1, 1, True), _c(384, 384, 3, 1, 1, True),
    _t(512, 256, 3, 2, 1, 1), _c(256, 256, 3, 1, 1, True), _c(256, 256, 3, 1, 1, True),
    _t(320, 128, 3, 2, 1, 1), _c(128, 128, 3, 1, 1, True), _c(128, 128, 3, 1, 1, True),
    _t(160, 64, 3, 2, 1, 1), _c(64, 64, 3, 1, 1, True), _c(64, 64, 3, 1, 1, True),
)
OUTPUT_BLOCKS = (_c(80, 32, 3, 1, 1), _c(32, 3, 1, 1, 0))
BLOCKS = FACE_BLOCKS + AUDIO_BLOCKS + DECODER_BLOCKS + OUTPUT_BLOCKS
FIRST_AUDIO, FIRST_DECODER, HEAD = len(FACE_BLOCKS), len(FACE_BLOCKS) + len(AUDIO_BLOCKS), len(BLOCKS) - 1
FACE_SHAPE, MEL_SHAPE, OUT_SHAPE = (6, 96, 96), (1, 80, 16), (3, 96, 96)
MEL_COLS = 16
MAX_CALL = 128  # windows per launch sequence, the library's cap: bounds the workspace (11.2 MB a window); results do not depend on it


def _group_ends(groups, first):
    ends, at = [], first
    for g in groups:
        at += g
        ends.append(at - 1)
    return ends


# the blocks whose output is a skip feature, and the decoder blocks behind which it is concatenated: SKIP_OF[decoder block] = face block
FACE_ENDS = _group_ends(FACE_GROUPS, 0)
DECODER_ENDS = _group_ends(DECODER_GROUPS, FIRST_DECODER)
SKIP_OF = dict(zip(DECODER_ENDS, reversed(FACE_ENDS)))


def block_names():
    """the state-dict prefix of each of the 51 blocks, in table order"""
    names = ["face_encoder_blocks.%d.%d" % (i, j) for i, g in enumerate(FACE_GROUPS) for j in range(g)]
    names += ["audio_encoder.%d" % j for j in range(len(AUDIO_BLOCKS))]
    names += ["face_decoder_blocks.%d.%d" % (i, j) for i, g in enumerate(DECODER_GROUPS) for j in range(g)]
    return names + ["output_block.0", "output_block.1"]


def block_shapes():
    """[(input [C,H,W], output [C,H,W])] of the 51 blocks; a decoder group's first block takes the concatenation"""
    out = []
    for blocks, shape in ((FACE_BLOCKS, FACE_SHAPE), (AUDIO_BLOCKS, MEL_SHAPE), (DECODER_BLOCKS + OUTPUT_BLOCKS, (512, 1, 1))):
        _, h, w = shape
        for tr, cin, cout, (kh, kw), (sh, sw), pad, op, _ in blocks:
            if tr:
                ho, wo = (h - 1) * sh - 2 * pad + kh + op, (w - 1) * sw - 2 * pad + kw + op
            else:
                ho, wo = (h + 2 * pad - kh) // sh + 1, (w + 2 * pad - kw) // sw + 1
            out.append(((cin, h, w), (cout, ho, wo)))
            h, w = ho, wo
    return out


_PARTS = (("conv_block.0.weight", None), ("conv_block.0.bias", 1), ("conv_block.1.weight", 1), ("conv_block.1.bias", 1),
          ("conv_block.1.running_mean", 1), ("conv_block.1.running_var", 1))
_HEAD_PARTS = (("weight", None), ("bias", 1))


def state_dict_keys():
    """{key: shape} of every tensor the generator needs"""
    keys = {}
    for b, (name, (tr, cin, cout, (kh, kw), _, _, _, _)) in enumerate(zip(block_names(), BLOCKS)):
        for part, dims in (_HEAD_PARTS if b == HEAD else _PARTS):
            keys["%s.%s" % (name, part)] = ((cin, cout, kh, kw) if tr else (cout, cin, kh, kw)) if dims is None else (cout,)
    return keys


def load_wav2lip(obj):
    """[(weight, bias, bn_weight, bn_bias, running_mean, running_var)] x 50 + [(weight, bias)] (fp32, wherever they are) from a
    state dict with the reference's keys, a checkpoint dict holding one under "state_dict", or the path of such a file (loaded onto
    the CPU).  `module.` is dropped from the keys as the reference's load_model does; `num_batches_tracked` is ignored.  Strict: a
    missing key, a key the generator does not have and a wrongly shaped tensor are refused with the key."""
    who = "load_wav2lip"
    obj = open_state_dict(who, obj, unwrap=("state_dict",), expected="a state dict, a checkpoint dict or a path")
    sd = {(k.replace("module.", "") if isinstance(k, str) else k): v for k, v in obj.items()}  # anywhere in the key, as load_model does
    want = state_dict_keys()
    only_keys(who, [k for k in sd if not (isinstance(k, str) and k.endswith("num_batches_tracked"))], want)
    # a float32 tensor stays the caller's: its version counter is watched
    keys = [["%s.%s" % (name, part) for part, _ in (_HEAD_PARTS if b == HEAD else _PARTS)] for b, name in enumerate(block_names())]
    return [tuple(take(who, sd, key, want[key]).float() for key in block) for block in keys]


def _gpu_f32(who, name, t, shape):
    return gpu_tensor(who, name, t, torch.float32, (None,) + tuple(shape), "float32 [n,%s]" % ",".join(str(s) for s in shape), empty="holds no window")


def flatten_sequences(audio_sequences, face_sequences):
    """the reference's 5-D form, audio [B,T,1,80,16] and faces [B,6,T,96,96], flattened time-major as wav2lip.py:93-94 does --
    torch.cat([a[:, i] for i in range(T)]), torch.cat([f[:, :, i] for i in range(T)]) -- as views where the strides allow"""
    if not torch.is_tensor(audio_sequences) or not torch.is_tensor(face_sequences) or audio_sequences.dim() != 5 or face_sequences.dim() != 5:
        raise ValueError("Wav2Lip: the 5-D form takes audio [B,T,1,80,16] and faces [B,6,T,96,96]")
    B, T = audio_sequences.shape[:2]
    if face_sequences.shape[0] != B or face_sequences.shape[2] != T:
        raise ValueError("Wav2Lip: audio %s and faces %s differ in B or T" % (tuple(audio_sequences.shape), tuple(face_sequences.shape)))
    audio = audio_sequences.transpose(0, 1).reshape((T * B,) + tuple(audio_sequences.shape[2:]))
    faces = face_sequences.permute(2, 0, 1, 3, 4).reshape((T * B, face_sequences.shape[1]) + tuple(face_sequences.shape[3:]))
    return audio, faces


def unflatten_sequences(x, B, T):
    """[T B, C, H, W] -> [B, C, T, H, W]: torch.stack(torch.split(x, B, dim=0), dim=2) (wav2lip.py:119-120)"""
    return x.reshape((T, B) + tuple(x.shape[1:])).permute(1, 2, 0, 3, 4)


class Wav2Lip(object):
    """The reference's `Wav2Lip` in eval mode on libn3dt, with caller-supplied weights (see load_wav2lip).

    `net(audio_sequences, face_sequences)` is the reference's `forward`: [n,1,80,16] and [n,6,96,96] -> [n,3,96,96], or
    [B,T,1,80,16] and [B,6,T,96,96] -> [B,3,T,96,96] (flattened time-major as the reference does); float32 GPU tensors of any
    strides; faces BGR in [0,1].  `net.block(b, x, skip=None)` runs one block, `net.layers(...)` all 51 in turn.
    Runs without gradients, stream-ordered, no synchronisation, bitwise reproducible; a window's result depends neither on its
    position in the batch nor on the batch size.  Batch norm is folded into the weights when they are packed, once per device,
    and again when a weight tensor's version has changed since (an in-place update); `repack()` forces it."""

    def __init__(self, weights):
        self.weights = load_wav2lip(weights)
        self._packed = PackedCache(lambda: [t for block in self.weights for t in block], self._pack)

    def repack(self):
        self._packed.clear()

    def _pack(self, device, dev):
        p, at = Wav2lipParams(), 0
        for i, block in enumerate(self.weights):  # dev holds the blocks' tensors one behind the other; the head has two
            for (field, _), t in zip(Wav2lipParams._fields_, dev[at:at + len(block)]):
                getattr(p, field)[i] = t.data_ptr()
            at += len(block)
        return pack("n3dt_wav2lip_pack", lib().n3dt_wav2lip_packed_bytes(), device, ctypes.byref(p)), dev

    def _packed_for(self, device):
        return self._packed.get(device)

    @staticmethod
    def _workspace(n, device):
        return workspace("wav2lip", lib().n3dt_wav2lip_workspace_bytes(n), device)

    @torch.no_grad()
    def __call__(self, audio_sequences, face_sequences):
        who = "Wav2Lip"
        five = torch.is_tensor(face_sequences) and face_sequences.dim() > 4
        if five:
            B, T = audio_sequences.shape[:2] if torch.is_tensor(audio_sequences) and audio_sequences.dim() == 5 else (0, 0)
            audio_sequences, face_sequences = flatten_sequences(audio_sequences, face_sequences)
        mel = _gpu_f32(who, "audio_sequences", audio_sequences, MEL_SHAPE)
        faces = _gpu_f32(who, "face_sequences", face_sequences, FACE_SHAPE)
        n = mel.shape[0]
        if faces.shape[0] != n or faces.device != mel.device:
            raise ValueError("Wav2Lip: audio_sequences %s and face_sequences %s differ in windows or device" % (tuple(mel.shape), tuple(faces.shape)))
        dev = mel.device
        packed = self._packed_for(dev)
        out = torch.empty((n,) + OUT_SHAPE, dtype=torch.float32, device=dev)
        for i, m in chunks(n, MAX_CALL):
            ws = self._workspace(m, dev)
            check(lib().n3dt_wav2lip_fwd(m, ops._ptr(packed), ops._ptr(mel[i:]), ops._ptr(faces[i:]), ops._ptr(out[i:]), ops._ptr(ws),
                                         ctypes.c_size_t(ws.numel()), ops._stream()), "n3dt_wav2lip_fwd")
        if five:
            out = unflatten_sequences(out, B, T)
        return out

    @torch.no_grad()
    def block(self, b, x, skip=None):
        """block b (0..50) of the table alone on x [n, C_in, H, W] -> [n, C_out, Ho, Wo]; n <= 128.  For the last block of a decoder
        group, with `skip` [n, C_skip, Ho, Wo] the result is the concatenation [n, C_out + C_skip, Ho, Wo].  Block 50 gives the
        logits (no sigmoid)."""
        if not isinstance(b, int) or not 0 <= b < WAV2LIP_BLOCKS:
            raise ValueError("Wav2Lip.block: block must be an integer in 0..50, got %r" % (b,))
        shapes = block_shapes()
        shape_in, shape_out = shapes[b]
        x = _gpu_f32("Wav2Lip.block", "x", x, shape_in)
        n = x.shape[0]
        if skip is not None:
            if b not in SKIP_OF:
                raise ValueError("Wav2Lip.block: block %d does not end in a concatenation" % b)
            skip_shape = shapes[SKIP_OF[b]][1]
            skip = _gpu_f32("Wav2Lip.block", "skip", skip, skip_shape)
            if skip.shape[0] != n or skip.device != x.device:
                raise ValueError("Wav2Lip.block: x and skip differ in windows or device")
            shape_out = (shape_out[0] + skip_shape[0],) + tuple(shape_out[1:])
        packed = self._packed_for(x.device)
        ws = self._workspace(n, x.device)
        out = torch.empty((n,) + tuple(shape_out), dtype=torch.float32, device=x.device)
        check(lib().n3dt_wav2lip_block(b, n, ops._ptr(packed), ops._ptr(x), None if skip is None else ops._ptr(skip), ops._ptr(out), ops._ptr(ws),
                                       ctypes.c_size_t(ws.numel()), ops._stream()), "n3dt_wav2lip_block")
        return out

    def layers(self, audio_sequences, face_sequences):
        """the 51 blocks' own outputs [n, C_out, H, W] in table order (the last: the logits), each block fed what the chained
        network feeds it, concatenations included, through the single-block entry"""
        x = _gpu_f32("Wav2Lip.layers", "face_sequences", face_sequences, FACE_SHAPE)
        m = _gpu_f32("Wav2Lip.layers", "audio_sequences", audio_sequences, MEL_SHAPE)
        out = []
        for b in range(WAV2LIP_BLOCKS):
            if b == FIRST_AUDIO:
                x = m
            if b in SKIP_OF:
                x = self.block(b, x, out[SKIP_OF[b]])
                out.append(x[:, :BLOCKS[b][2]])
            else:
                x = self.block(b, x)
                out.append(x)
        return out


def _frames(who, name, frames):
    return gpu_tensor(who, name, frames, torch.float32, (None, 3, None, None), "float32 [F,3,H,W]")


def _boxes(who, boxes, frames):
    F, _, H, W = frames.shape
    if torch.is_tensor(boxes) and boxes.is_cuda:  # already on the device: the kernels clamp a box into the frame
        if boxes.dtype != torch.int32 or boxes.dim() != 2 or boxes.shape[1] != 4 or boxes.shape[0] not in (1, F):
            raise ValueError("%s: device boxes must be int32 [1,4] or [%d,4], got %s %s" % (who, F, boxes.dtype, tuple(boxes.shape)))
        return boxes.contiguous()
    return torch.tensor(check_boxes(who, boxes, F, H, W), dtype=torch.int32).to(frames.device)


def face_inputs(frames, boxes, ref_frames=None):
    """frames [F,3,H,W] float32 RGB in [0,1] (GPU) and one crop box (y1, y2, x1, x2) per frame or one for all -> the generator's
    input [F,6,96,96]: channels 0..2 the frame's crop resampled to 96 x 96 (bilinear, half-pixel centres, float64), BGR, rows 48..95
    zero; channels 3..5 the crop of ref_frames (default: the frame itself, as the reference's datagen does), unmasked.  This is the
    reference's wav_getitem.  Values outside [0,1] are clamped and NaN counts as 0."""
    who = "face_inputs"
    frames = _frames(who, "frames", frames)
    if ref_frames is not None:
        ref_frames = _frames(who, "ref_frames", ref_frames)
        if ref_frames.shape != frames.shape or ref_frames.device != frames.device:
            raise ValueError("face_inputs: frames %s and ref_frames %s differ" % (tuple(frames.shape), tuple(ref_frames.shape)))
    dev_boxes = _boxes(who, boxes, frames)
    F, _, H, W = frames.shape
    out = torch.empty((F,) + FACE_SHAPE, dtype=torch.float32, device=frames.device)
    for i, m in chunks(F, 4096):
        bx = dev_boxes if dev_boxes.shape[0] == 1 else dev_boxes[i:i + m]
        check(lib().n3dt_wav2lip_face_inputs(m, H, W, ops._ptr(frames[i:]), None if ref_frames is None else ops._ptr(ref_frames[i:]), ops._ptr(bx),
                                             bx.shape[0], ops._ptr(out[i:]), ops._stream()), "n3dt_wav2lip_face_inputs")
    return out


def paste(faces, frames, boxes):
    """faces [F,3,96,96] (BGR, the generator's output) resampled to each box's size and written over [y1:y2, x1:x2] of a copy of
    frames [F,3,H,W] (RGB) -> [F,3,H,W]; outside the boxes the result is the frames, bit for bit (talker_trainer.py:991-995 with a
    float bilinear resample in place of OpenCV's byte resize)."""
    who = "paste"
    frames = _frames(who, "frames", frames)
    F, _, H, W = frames.shape
    faces = _gpu_f32(who, "faces", faces, OUT_SHAPE)
    if faces.shape[0] != F or faces.device != frames.device:
        raise ValueError("paste: faces %s and frames %s differ in frames or device" % (tuple(faces.shape), tuple(frames.shape)))
    dev_boxes = _boxes(who, boxes, frames)
    out = torch.empty_like(frames)
    for i, m in chunks(F, 4096):
        bx = dev_boxes if dev_boxes.shape[0] == 1 else dev_boxes[i:i + m]
        check(lib().n3dt_wav2lip_paste(m, H, W, ops._ptr(faces[i:]), ops._ptr(frames[i:]), ops._ptr(bx), bx.shape[0], ops._ptr(out[i:]),
                                       ops._stream()), "n3dt_wav2lip_paste")
    return out


def segmented_mels(mel, frame_id, fps):
    """The reference's get_segmented_mels over crop_audio_window (XGaze_utils/data_loader_xgaze_new.py:319-343) on mel [80,T]: the
    five windows [5,80,16] of frames frame_id - 1 .. frame_id + 3 -- or, where frame_id - 1 < 0, of frames 1 .. 5 -- and None where
    one of them passes the end."""
    mels = []
    start_frame_num = frame_id + 1
    if start_frame_num - 2 < 0:
        start_frame_num = 3
    for i in range(start_frame_num, start_frame_num + 5):
        start_idx = int(80. * ((i - 2) / float(fps)))
        m = mel[:, start_idx:start_idx + MEL_COLS]
        if m.shape[1] != MEL_COLS:
            return None
        mels.append(m)
    return torch.stack(mels) if torch.is_tensor(mel) else np.asarray(mels)


def chunk_start(T, i, fps):
    """the first mel column of frame i's chunk in `main` (data_loader_xgaze_new.py:261-269): the last 16 where it would pass the end"""
    mel_idx_multiplier = 80. / fps
    start_idx = int(i * mel_idx_multiplier)
    return T - MEL_COLS if start_idx + MEL_COLS > T else start_idx


def chunk(mel, i, fps):
    """frame i's mel chunk [80,16] of mel [80,T] by main's rule"""
    s = chunk_start(mel.shape[1], i, fps)
    return mel[:, s:s + MEL_COLS]


class Wav2LipClip(object):
    """Frames and a mel spectrogram in, lip-synced frames out:

        clip = Wav2LipClip(Wav2Lip(weights))
        out = clip.generate(frames, boxes, mel, fps=25.0)      # [F,3,H,W]

    frames [F,3,H,W] float32 RGB in [0,1]; boxes one (y1, y2, x1, x2) per frame or one for all; mel [80,T] on the device
    (MelFrontend.melspectrogram).  Frame i is driven by chunk(mel, i, fps); its crop is masked, generated against ref_frames' crop
    (default: itself) and pasted back.  Batches of at most MAX_CALL frames; nothing synchronises with the host."""

    def __init__(self, net):
        if not isinstance(net, Wav2Lip):
            raise TypeError("Wav2LipClip: net must be a Wav2Lip, got %s" % type(net).__name__)
        self.net = net

    @staticmethod
    def mel_windows(mel, first, n, fps):
        """chunk(mel, i, fps) for i = first .. first + n - 1 as [n,1,80,16] float32: the starts are formed on the device in the
        same float64 arithmetic (IEEE product, truncation), without an upload"""
        gpu_tensor("Wav2LipClip", "mel", mel, copy=False)
        if mel.dtype not in (torch.float32, torch.float64) or mel.dim() != 2 or mel.shape[0] != 80 or mel.shape[1] < MEL_COLS:
            raise ValueError("Wav2LipClip: mel must be float32 or float64 [80, T >= 16], got %s %s" % (mel.dtype, tuple(mel.shape)))
        mel = mel.detach().contiguous()
        T = mel.shape[1]
        idx = torch.arange(first, first + n, dtype=torch.float64, device=mel.device)
        start = (idx * (80. / fps)).to(torch.int64)
        start = torch.where(start + MEL_COLS > T, torch.full_like(start, T - MEL_COLS), start).to(torch.int32)
        out = torch.empty(n, 1, 80, MEL_COLS, dtype=torch.float32, device=mel.device)
        check(lib().n3dt_mel_windows(T, ops._ptr(mel), T, int(mel.dtype == torch.float64), n, ops._ptr(start), ops._ptr(out), ops._stream()),
              "n3dt_mel_windows")
        return out

    def generate(self, frames, boxes, mel, fps, ref_frames=None):
        frames = _frames("Wav2LipClip.generate", "frames", frames)
        if not float(fps) > 0.0:
            raise ValueError("Wav2LipClip.generate: fps must be positive, got %r" % (fps,))
        dev_boxes = _boxes("Wav2LipClip.generate", boxes, frames)
        F = frames.shape[0]
        out = []
        for i, m in chunks(F, MAX_CALL):
            bx = dev_boxes if dev_boxes.shape[0] == 1 else dev_boxes[i:i + m]
            fr = frames[i:i + m]
            x = face_inputs(fr, bx, None if ref_frames is None else ref_frames[i:i + m])
            g = self.net(self.mel_windows(mel, i, m, float(fps)), x)
            out.append(paste(g, fr, bx))
        return torch.cat(out) if len(out) > 1 else out[0]
