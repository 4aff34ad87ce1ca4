"""A float64 restatement of Wav2Lip's generator the way the reference's wav_models/wav2lip.py + wav_models/conv.py compute it,
written from n3dt.wav2lip's table, and an emulation of the arithmetic csrc/wav2lip.hip uses for it.  tests/golden/wav2lip.*
(tools/gen_golden_wav2lip.py, from the reference's own class in float64) pins the restatement; the GPU tests are judged against
the restatement.

  restatement   per block: convolution with the UNFOLDED weights -- a ConvTranspose2d block as the gather over parity classes the
                kernel uses, not as torch's conv_transpose2d -- then batch norm by its formula, then the block's own input for
                residual blocks, then ReLU; torch.cat((x, skip), 1) behind each decoder group; the plain output convolution and
                the sigmoid.  float64 throughout.
  emulation     per block: the weights with batch norm folded in float64 and rounded to fp32, input and weights split into two
                bf16 values each, the three products lo*hi + hi*lo + hi*hi as fp32 convolutions (fp32 accumulation), the folded
                bias, the residual, ReLU, all in fp32; the output convolution from fp32 operands in float64, rounded to fp32, and
                the sigmoid in float64, rounded to fp32.  Its distance from the reference's float64 values is the floor the GPU
                tests' bounds are 4 x of (the order of the fp32 sums differs between this and the MFMA).
  prologue      crop, bilinear resample with half-pixel centres, BGR, masked target + reference; the paste back
"""
import torch
import torch.nn.functional as F

from n3dt.wav2lip import BLOCKS, FIRST_AUDIO, HEAD, SKIP_OF, block_names

WEIGHTS_SEED = 2026
INPUT_SEED = 78
N_WINDOWS = 3
SAMPLE_STRIDE = 97
BN_EPS = 1e-5
N_BLOCKS = len(BLOCKS)


def fixture_inputs():
    """(face inputs [3,6,96,96] uint8 with rows 48..95 of channels 0..2 zero, mel windows [3,1,80,16] uint8): the network sees
    faces / 255 and mel / 32 - 4.  The faces are smooth gradients plus noise, different in every channel and window."""
    g = torch.Generator().manual_seed(INPUT_SEED)
    yy, xx = torch.meshgrid(torch.arange(96.0), torch.arange(96.0), indexing="ij")
    faces = torch.empty(N_WINDOWS, 6, 96, 96)
    for w in range(N_WINDOWS):
        for c in range(6):
            a, b, p = (torch.rand(3, generator=g) * 0.15).tolist()
            faces[w, c] = 128 + 80 * torch.sin(a * yy + b * xx + 40 * p) + 30 * torch.randn(96, 96, generator=g)
    faces_u8 = faces.clamp(0, 255).to(torch.uint8)
    faces_u8[:, :3, 48:] = 0
    mel_u8 = torch.randint(0, 256, (N_WINDOWS, 1, 80, 16), generator=g, dtype=torch.uint8)
    return faces_u8.numpy(), mel_u8.numpy()


def faces_from_u8(u8):
    return torch.as_tensor(u8).double() / 255.0


def mel_from_u8(u8):
    return torch.as_tensor(u8).double() / 32.0 - 4.0


def block_params(sd, b, dtype=torch.float64):
    name = block_names()[b]
    if b == HEAD:
        return [sd[name + ".weight"].to(dtype), sd[name + ".bias"].to(dtype)]
    keys = ("conv_block.0.weight", "conv_block.0.bias", "conv_block.1.weight", "conv_block.1.bias", "conv_block.1.running_mean",
            "conv_block.1.running_var")
    return [sd["%s.%s" % (name, k)].to(dtype) for k in keys]


def conv_transpose_gather(x, w, stride):
    """ConvTranspose2d without bias as the kernel forms it, x [n, C_in, H, W], w [C_in, C_out, 3, 3].
    stride 2 (padding 1, output_padding 1) -> [n, C_out, 2 H, 2 W]: output pixel y = 2 i - 1 + ky, so an even row takes ky = 1 from
    input row y / 2, an odd one ky = 2 from (y - 1) / 2 and ky = 0 from (y + 1) / 2 (nothing past the last row), columns alike:
    four sub-products of 1, 2, 2 and 4 taps.  stride 1 (padding 0) on a 1 x 1 map -> [n, C_out, 3, 3]: pixel (y, x) is the one
    input pixel times w[:, :, y, x]."""
    n, _, H, W = x.shape
    cout = w.shape[1]
    if stride == 1:
        assert (H, W) == (1, 1)
        out = x.new_zeros(n, cout, 3, 3)
        for y in range(3):
            for xx in range(3):
                out[:, :, y, xx] = x[:, :, 0, 0] @ w[:, :, y, xx]
        return out
    xp = F.pad(x, (0, 1, 0, 1))  # the zero row and column that (y + 1) / 2 reads behind the last odd row
    out = x.new_zeros(n, cout, 2 * H, 2 * W)
    taps = {0: ((1, 0),), 1: ((2, 0), (0, 1))}  # parity -> ((k, offset of the input row from y // 2), ...)
    for py in (0, 1):
        for px in (0, 1):
            acc = x.new_zeros(n, cout, H, W)
            for ky, dy in taps[py]:
                for kx, dx in taps[px]:
                    acc = acc + torch.einsum("nchw,co->nohw", xp[:, :, dy:dy + H, dx:dx + W], w[:, :, ky, kx])
            out[:, :, py::2, px::2] = acc
    return out


def block64(sd, b, x):
    """one block in float64: convolution -> batch norm (eval) -> + x if residual -> ReLU; the head: the plain convolution (logits)"""
    tr, _, _, _, stride, pad, _, residual = BLOCKS[b]
    x = x.double()
    if b == HEAD:
        w, bias = block_params(sd, b)
        return F.conv2d(x, w, bias)
    w, bias, gamma, beta, mean, var = block_params(sd, b)
    if tr:
        y = conv_transpose_gather(x, w, stride[0]) + bias[None, :, None, None]
    else:
        y = F.conv2d(x, w, bias, stride=stride, padding=pad)
    y = (y - mean[None, :, None, None]) / torch.sqrt(var[None, :, None, None] + BN_EPS) * gamma[None, :, None, None] + beta[None, :, None, None]
    if residual:
        y = y + x
    return torch.relu(y)


def block_input(acts, b, faces, mel):
    """what block b is fed, given the outputs of the blocks before it: the concatenation behind a decoder group"""
    if b == 0:
        return faces
    if b == FIRST_AUDIO:
        return mel
    if b - 1 in SKIP_OF:
        return torch.cat((acts[b - 1], acts[SKIP_OF[b - 1]]), dim=1)
    return acts[b - 1]


def chain(block_fn, sd, faces, mel, dtype):
    """(the 51 blocks' own outputs, the last one the logits) with `block_fn(sd, b, x)` for every block"""
    acts = []
    for b in range(N_BLOCKS):
        acts.append(block_fn(sd, b, block_input(acts, b, faces.to(dtype), mel.to(dtype))))
    return acts


def chain64(sd, faces, mel):
    """(acts, image): image = sigmoid(logits) in float64"""
    with torch.no_grad():
        acts = chain(block64, sd, faces, mel, torch.float64)
        return acts, torch.sigmoid(acts[-1])


def forward64(sd, audio_sequences, face_sequences):
    """the reference's forward in float64 with both of its input forms, its flattening and re-stacking written as it writes them"""
    B = audio_sequences.size(0)
    five = face_sequences.dim() > 4
    if five:
        audio_sequences = torch.cat([audio_sequences[:, i] for i in range(audio_sequences.size(1))], dim=0)
        face_sequences = torch.cat([face_sequences[:, :, i] for i in range(face_sequences.size(2))], dim=0)
    x = chain64(sd, face_sequences, audio_sequences)[1]
    return torch.stack(torch.split(x, B, dim=0), dim=2) if five else x


def block_inputs(acts, faces, mel):
    return [block_input(acts, b, faces, mel) for b in range(N_BLOCKS)]


# ---- the kernel's arithmetic ---------------------------------------------------------------------------------------------------
def fold(sd, b):
    """(w', b') fp32: s = gamma / sqrt(var + eps) in float64 along C_out (axis 1 of a ConvTranspose2d weight)"""
    w, bias, gamma, beta, mean, var = block_params(sd, b)
    s = gamma / torch.sqrt(var + BN_EPS)
    ws = w * (s[None, :, None, None] if BLOCKS[b][0] else s[:, None, None, None])
    return ws.float(), ((bias - mean) * s + beta).float()


def split(x):
    hi = x.bfloat16().float()
    return hi, (x - hi).bfloat16().float()


def block_emulated(sd, b, x, want_image=False):
    """one block as the kernel forms it, on x fp32"""
    tr, _, _, _, stride, pad, op, residual = BLOCKS[b]
    x = x.float()
    if b == HEAD:
        w, bias = block_params(sd, b, torch.float32)
        y = F.conv2d(x.double(), w.double(), bias.double())
        return (y.float(), torch.sigmoid(y).float()) if want_image else y.float()
    w, bias = fold(sd, b)
    (xh, xl), (wh, wl) = split(x), split(w)
    if tr:
        conv = lambda a, k: F.conv_transpose2d(a, k, None, stride=stride, padding=pad, output_padding=op)  # noqa: E731
    else:
        conv = lambda a, k: F.conv2d(a, k, None, stride=stride, padding=pad)  # noqa: E731
    y = conv(xl, wh)
    y = y + conv(xh, wl)
    y = y + conv(xh, wh)
    y = y + bias[None, :, None, None]
    if residual:
        y = y + x
    return torch.relu(y)


def chain_emulated(sd, faces, mel):
    """(acts fp32, image fp32)"""
    with torch.no_grad():
        acts = []
        for b in range(N_BLOCKS - 1):
            acts.append(block_emulated(sd, b, block_input(acts, b, faces.float(), mel.float())))
        logits, image = block_emulated(sd, HEAD, acts[-1], want_image=True)
        return acts + [logits], image


def measured_bounds(sd, faces, mel, ref_acts, ref_image):
    """The emulation's error against float64 reference values, on the CPU alone: per block max |emulated block(fp32(x_b)) - y_b|
    with x the REFERENCE's activations (each block alone, fed the fp32-rounded reference input), then the emulated chain's
    logits and image end to end."""
    inputs = block_inputs(ref_acts, faces, mel)
    with torch.no_grad():
        blocks = [float((block_emulated(sd, b, inputs[b].float()).double() - ref_acts[b]).abs().max()) for b in range(N_BLOCKS)]
    acts, image = chain_emulated(sd, faces, mel)
    return {"block": blocks, "logits": float((acts[-1].double() - ref_acts[-1]).abs().max()),
            "image": float((image.double() - ref_image).abs().max())}


def summary(act):
    """what the fixture keeps of an activation: its sum, its abs-sum and every 97th element"""
    flat = act.double().reshape(-1)
    return float(flat.sum()), float(flat.abs().sum()), flat[::SAMPLE_STRIDE].numpy().copy()


# ---- prologue and paste ----------------------------------------------------------------------------------------------------------
def _box_of(boxes, i):
    if not isinstance(boxes[0], (list, tuple)):
        return boxes
    return boxes[0] if len(boxes) == 1 else boxes[i]


def face_inputs(frames, boxes, ref_frames=None):
    """frames [F,3,H,W] (RGB, float64 tensor) -> [F,6,96,96]: F.interpolate(align_corners=False) of each crop, BGR, the target's
    rows 48.. zero, then the reference's crop (default: the frame's own)"""
    frames = torch.nan_to_num(frames.double(), nan=0.0, posinf=1.0, neginf=0.0).clamp(0.0, 1.0)
    ref = frames if ref_frames is None else torch.nan_to_num(ref_frames.double(), nan=0.0, posinf=1.0, neginf=0.0).clamp(0.0, 1.0)
    out = []
    for i in range(frames.shape[0]):
        y1, y2, x1, x2 = _box_of(boxes, i)
        parts = []
        for src, masked in ((frames, True), (ref, False)):
            crop = F.interpolate(src[i:i + 1, :, y1:y2, x1:x2], size=(96, 96), mode="bilinear", align_corners=False)[0].flip(0)
            if masked:
                crop = crop.clone()
                crop[:, 48:] = 0.0
            parts.append(crop)
        out.append(torch.cat(parts))
    return torch.stack(out)


def paste(faces, frames, boxes):
    """faces [F,3,96,96] (BGR) resampled to each box and written over a copy of frames [F,3,H,W] (RGB)"""
    out = frames.double().clone()
    for i in range(frames.shape[0]):
        y1, y2, x1, x2 = _box_of(boxes, i)
        p = F.interpolate(faces[i:i + 1].double().flip(1), size=(y2 - y1, x2 - x1), mode="bilinear", align_corners=False)[0]
        out[i, :, y1:y2, x1:x2] = p
    return out
