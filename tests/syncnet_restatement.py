"""A float64 restatement of the lip-sync expert the way the reference's wav_models/syncnet.py + wav_models/conv.py compute it, and an
emulation of the arithmetic csrc/syncnet.hip uses for it.  tests/golden/syncnet.* (tools/gen_golden_syncnet.py, from the
reference's own class in float64) pins the restatement; the GPU tests are judged against the restatement.

  restatement   per block: convolution with the UNFOLDED weights, then batch norm by its formula
                (y - mean) / sqrt(var + eps) * gamma + beta, then the block's own input for residual blocks, then ReLU; then
                x / max(||x||_2, 1e-12) and the dot product.  float64 throughout.
  emulation     per block: the weights with batch norm folded in float64 and rounded to fp32, input and weights split into two
                bf16 values each, the three products hi*hi + hi*lo + lo*hi as fp32 convolutions (fp32 accumulation), the folded
                bias, the residual, ReLU, all in fp32.  Its distance from the reference's float64 values is the floor the GPU
                tests' bounds are 4 x of (the order of the fp32 sums differs between this and the MFMA).
  prologue      crop, bilinear resample with half-pixel centres, lower half, BGR, five frames along the channels
  meter         window starts, the drop rule and the means of n3dt.SyncMeter as literal loops
"""
import numpy as np
import torch
import torch.nn.functional as F

from n3dt.syncnet import BLOCKS, FACE_BLOCKS, block_names

WEIGHTS_SEED = 2025
INPUT_SEED = 77
N_WINDOWS = 3
SAMPLE_STRIDE = 97
BN_EPS = 1e-5
N_FACE = len(FACE_BLOCKS)


def fixture_inputs():
    """(face windows [3,15,48,96] uint8, mel windows [3,1,80,16] uint8): the network sees faces / 255 and mel / 32 - 4.
    The faces are smooth gradients plus noise (an image, not white noise), different in every frame and window."""
    g = torch.Generator().manual_seed(INPUT_SEED)
    yy, xx = torch.meshgrid(torch.arange(48.0), torch.arange(96.0), indexing="ij")
    faces = torch.empty(N_WINDOWS, 15, 48, 96)
    for w in range(N_WINDOWS):
        for c in range(15):
            a, b, p = (torch.rand(3, generator=g) * 0.15).tolist()
            faces[w, c] = 128 + 80 * torch.sin(a * yy + b * xx + 40 * p) + 30 * torch.randn(48, 96, generator=g)
    faces_u8 = faces.clamp(0, 255).to(torch.uint8)
    mel_u8 = torch.randint(0, 256, (N_WINDOWS, 1, 80, 16), generator=g, dtype=torch.uint8)
    return faces_u8.numpy(), mel_u8.numpy()


def faces_from_u8(u8):
    return torch.as_tensor(u8).double() / 255.0


def mel_from_u8(u8):
    return torch.as_tensor(u8).double() / 32.0 - 4.0


def block_params(sd, b, dtype=torch.float64):
    name = block_names()[b]
    keys = ("conv_block.0.weight", "conv_block.0.bias", "conv_block.1.weight", "conv_block.1.bias", "conv_block.1.running_mean",
            "conv_block.1.running_var")
    return [sd["%s.%s" % (name, k)].to(dtype) for k in keys]


def block64(sd, b, x):
    """one block in float64: conv -> batch norm (eval) -> + x if residual -> ReLU"""
    _, _, _, stride, pad, residual = BLOCKS[b]
    w, bias, gamma, beta, mean, var = block_params(sd, b)
    y = F.conv2d(x.double(), w, bias, stride=stride, padding=pad)
    y = (y - mean[None, :, None, None]) / torch.sqrt(var[None, :, None, None] + BN_EPS) * gamma[None, :, None, None] + beta[None, :, None, None]
    if residual:
        y = y + x
    return torch.relu(y)


def normalize(x):
    """F.normalize(p=2, dim=1): x / max(||x||_2, 1e-12)"""
    x = x.double().reshape(x.shape[0], -1)
    return x / torch.sqrt((x * x).sum(dim=1, keepdim=True)).clamp_min(1e-12)


def chain(block_fn, sd, faces, mel, dtype):
    """(the 31 activations, audio_emb, face_emb, cos) with `block_fn(sd, b, x)` for every block"""
    acts, x = [], faces.to(dtype)
    for b in range(len(BLOCKS)):
        if b == N_FACE:
            x = mel.to(dtype)
        x = block_fn(sd, b, x)
        acts.append(x)
    f, a = normalize(acts[N_FACE - 1]), normalize(acts[-1])
    return acts, a, f, (a * f).sum(dim=1)


def chain64(sd, faces, mel):
    with torch.no_grad():
        return chain(block64, sd, faces, mel, torch.float64)


# ---- the kernel's arithmetic ---------------------------------------------------------------------------------------------------
def fold(sd, b):
    """(w', b') fp32: s = gamma / sqrt(var + eps) in float64, w' = fp32(w s), b' = fp32((b - mean) s + beta)"""
    w, bias, gamma, beta, mean, var = block_params(sd, b)
    s = gamma / torch.sqrt(var + BN_EPS)
    return (w * s[:, None, None, None]).float(), ((bias - mean) * s + beta).float()


def split(x):
    """x (fp32) = hi + lo + (what two bf16 values cannot hold): both as fp32 tensors holding bf16 values"""
    hi = x.bfloat16().float()
    return hi, (x - hi).bfloat16().float()


def block_emulated(sd, b, x):
    """one block as the kernel forms it, on x fp32: three fp32 convolutions of split operands, + b', + x if residual, ReLU"""
    _, _, _, stride, pad, residual = BLOCKS[b]
    w, bias = fold(sd, b)
    x = x.float()
    (xh, xl), (wh, wl) = split(x), split(w)
    y = F.conv2d(xl, wh, None, stride=stride, padding=pad)
    y = y + F.conv2d(xh, wl, None, stride=stride, padding=pad)
    y = y + F.conv2d(xh, wh, None, stride=stride, padding=pad)
    y = y + bias[None, :, None, None]
    if residual:
        y = y + x
    return torch.relu(y)


def chain_emulated(sd, faces, mel):
    with torch.no_grad():
        return chain(block_emulated, sd, faces, mel, torch.float32)


def block_inputs(acts, faces, mel):
    """the input of each of the 31 blocks, given the chain's activations"""
    return [faces if b == 0 else mel if b == N_FACE else acts[b - 1] for b in range(len(BLOCKS))]


def measured_bounds(sd, faces, mel, ref_acts, ref_a, ref_f, ref_cos):
    """The emulation's error against float64 reference values, on the CPU alone: per block max |emulated block(fp32(x_b)) -
    x_{b+1}| with x the REFERENCE's activations (each block alone, fed the fp32-rounded reference input), then the emulated
    chain's embeddings and cosine end to end."""
    inputs = block_inputs(ref_acts, faces, mel)
    with torch.no_grad():
        blocks = [float((block_emulated(sd, b, inputs[b].float()).double() - ref_acts[b]).abs().max()) for b in range(len(BLOCKS))]
    _, a, f, cos = chain_emulated(sd, faces, mel)
    return {"block": blocks, "embedding": max(float((a - ref_a).abs().max()), float((f - ref_f).abs().max())),
            "cos": float((cos - ref_cos).abs().max())}


def summary(act):
    """what the fixture keeps of an activation: its sum, its abs-sum and every 97th element"""
    flat = act.double().reshape(-1)
    return float(flat.sum()), float(flat.abs().sum()), flat[::SAMPLE_STRIDE].numpy().copy()


# ---- the face-window prologue ---------------------------------------------------------------------------------------------------
def axis_weights(n_in, n_out=96):
    """F.interpolate(mode='bilinear', align_corners=False) along one axis: (i0, i1, weight of i1) for every output index"""
    src = np.maximum((n_in / n_out) * (np.arange(n_out, dtype=np.float64) + 0.5) - 0.5, 0.0)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    return i0, np.minimum(i0 + 1, n_in - 1), src - i0


def resample96(img):
    """img [C, h, w] float64 -> [C, 96, 96]"""
    y0, y1, wy = axis_weights(img.shape[1])
    x0, x1, wx = axis_weights(img.shape[2])
    top = img[:, y0][:, :, x0] * (1.0 - wx) + img[:, y0][:, :, x1] * wx
    bot = img[:, y1][:, :, x0] * (1.0 - wx) + img[:, y1][:, :, x1] * wx
    return top * (1.0 - wy)[None, :, None] + bot * wy[None, :, None]


def face_windows(frames, boxes):
    """frames [F,3,H,W] (numpy, RGB) and one box (y1, y2, x1, x2) per frame or one for all -> [F-4,15,48,96] float64: values clamped to
    [0,1] with NaN -> 0, crop, resample to 96 x 96, rows 48.., BGR, window i = frames i..i+4 along the channels"""
    frames = np.asarray(frames, dtype=np.float64)
    frames = np.clip(np.nan_to_num(frames, nan=0.0, posinf=1.0, neginf=0.0), 0.0, 1.0)
    boxes = [boxes] * len(frames) if not isinstance(boxes[0], (list, tuple)) else (list(boxes) * len(frames) if len(boxes) == 1 else boxes)
    halves = []
    for fr, (y1, y2, x1, x2) in zip(frames, boxes):
        halves.append(resample96(fr[:, y1:y2, x1:x2])[::-1, 48:])
    return np.stack([np.concatenate(halves[i:i + 5]) for i in range(len(frames) - 4)])


# ---- the meter's bookkeeping ----------------------------------------------------------------------------------------------------
def meter_starts(n_frames, T, fps):
    """(the mel starts of the kept windows, the number dropped): window i = frames i..i+4 pairs with mel columns s..s+15,
    s = int(80. * (i / float(fps))); a window whose slice passes the end of the T columns is dropped"""
    kept, dropped = [], 0
    for i in range(n_frames - 4):
        s = int(80. * (i / float(fps)))
        if s + 16 > T:
            dropped += 1
        else:
            kept.append(s)
    return kept, dropped


def meter_result(cos, audio_emb=None, face_emb=None, max_shift=0):
    """sync_conf, sync_loss and, with max_shift, the curve and its argmax, from per-window values (numpy float64)"""
    cos = np.asarray(cos, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        res = {"sync_conf": float(cos.mean()), "sync_loss": float(np.minimum(-np.log(cos), 100.0).mean())}
    if max_shift:
        a, f = np.asarray(audio_emb, dtype=np.float64), np.asarray(face_emb, dtype=np.float64)
        n, curve = len(cos), []
        for k in range(-max_shift, max_shift + 1):
            vals = [float((f[i] * a[i + k]).sum()) for i in range(n) if 0 <= i + k < n]
            curve.append(float(np.mean(vals)) if vals else float("nan"))
        res["curve"] = curve
        res["offset"] = int(np.nanargmax(curve)) - max_shift
    return res
