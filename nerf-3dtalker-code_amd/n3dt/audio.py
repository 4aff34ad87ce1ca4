"""Audio2style encoder of the reference (talker_trainer.py:407-461) on libn3dt's HIP kernels (csrc/audio_lstm.hip).

The reference co-trains it with the renderer: `audiostyle = audio2style(mel_batch)` feeds HeadNeRFNet, one backward reaches
both, and a second Adam steps the encoder (:665, :1002-1067).  What the reference computes, kept exactly here:
  * the frames of a batch are the TIME axis: mel [B, 80, 16] -> [B, 1280] -> one sequence of T = B steps, batch 1;
  * nn.LSTM(1280, 640, num_layers=2, bidirectional=True), h0 = c0 = 0, then Linear(1280, 640), Linear(640, 320),
    Linear(320, 64), each followed by LeakyReLU(0.2) and Dropout(0.5);
  * the reference never calls `.eval()` on it, so dropout is on in training, validation and fitting alike.  Training mode is
    the default here too; `eval()` turns dropout off;
  * RNNModel.fc1 is a parameter that forward never reads: it gets no gradient (`.grad` stays None), so Adam leaves it alone.
State-dict keys, shapes and (under the same torch.manual_seed) initial values are the reference's.  The LSTM and the head run
on the HIP kernels only; torch.nn.LSTM / MIOpen are never called.
"""
import ctypes
import math

import torch
from torch import nn

IN_FEATURES = 80 * 16
HIDDEN = 40 * 16
OUT_FEATURES = 64
HEAD = ((80 * 16, 40 * 16), (40 * 16, 20 * 16), (20 * 16, 64))
MAX_T = 256
N_PARAMS = 21_546_624  # n3dt.parallel.FlatBucket.AUDIO2STYLE_PARAMS


class LSTMParams(nn.Module):
    """The parameters of nn.LSTM(input_size, hidden_size, num_layers, bidirectional=True) -- same names, shapes, registration
    order and initialisation (reset_parameters: U(-1/sqrt(hidden), 1/sqrt(hidden)) over the tensors in that order) -- and
    nothing else: Audio2style's forward runs them through libn3dt, not through torch.nn.LSTM."""

    def __init__(self, input_size=IN_FEATURES, hidden_size=HIDDEN, num_layers=2):
        super().__init__()
        self.input_size, self.hidden_size, self.num_layers = input_size, hidden_size, num_layers
        self.bidirectional, self.batch_first = True, True
        for layer in range(num_layers):
            n_in = input_size if layer == 0 else 2 * hidden_size
            for suffix in ("", "_reverse"):
                for name, shape in (("weight_ih", (4 * hidden_size, n_in)), ("weight_hh", (4 * hidden_size, hidden_size)),
                                    ("bias_ih", (4 * hidden_size,)), ("bias_hh", (4 * hidden_size,))):
                    setattr(self, "%s_l%d%s" % (name, layer, suffix), nn.Parameter(torch.empty(shape)))
        self.reset_parameters()

    def reset_parameters(self):
        stdv = 1.0 / math.sqrt(self.hidden_size)
        for w in self.parameters():
            nn.init.uniform_(w, -stdv, stdv)

    def tensors(self):
        """(w_ih, w_hh, b_ih, b_hh) for k = 2 * layer + direction, the C ABI's order."""
        out = []
        for layer in range(self.num_layers):
            for suffix in ("", "_reverse"):
                out.append(tuple(getattr(self, "%s_l%d%s" % (n, layer, suffix)) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")))
        return out


class RNNModel(nn.Module):
    """The reference's RNNModel(1280, 640): `rnn` (the LSTM's parameters) and the never-used `fc1` Linear(1280, 640)."""

    def __init__(self, input_size=IN_FEATURES, hidden_size=HIDDEN, num_layers=2):
        super().__init__()
        self.nhid, self.nlayers = hidden_size, num_layers
        self.rnn = LSTMParams(input_size, hidden_size, num_layers)
        self.fc1 = nn.Linear(hidden_size * 2, hidden_size)  # a parameter of the reference that its forward never reads


def _c_params(params):
    from ._lib import A2sParams
    p = A2sParams()
    for k in range(4):
        w_ih, w_hh, b_ih, b_hh = params[4 * k:4 * k + 4]
        p.w_ih[k], p.w_hh[k], p.b_ih[k], p.b_hh[k] = w_ih.data_ptr(), w_hh.data_ptr(), b_ih.data_ptr(), b_hh.data_ptr()
    for k in range(3):
        p.lin_w[k], p.lin_b[k] = params[16 + 2 * k].data_ptr(), params[17 + 2 * k].data_ptr()
    return p


class _A2sFn(torch.autograd.Function):
    """n3dt_a2s_fwd / n3dt_a2s_bwd.  Inputs: the module, mel [T, 1280] (fp32, contiguous; no gradient), the three keep masks
    (or None) and the 22 trained tensors in the grad arena's order.  The backward writes all 22 gradients in one call."""

    @staticmethod
    def forward(ctx, mod, mel, masks, *params):
        from . import ops
        from ._lib import lib, check
        T = mel.shape[0]
        L = lib()
        sv_b, ws_b = L.n3dt_a2s_saved_bytes(T), L.n3dt_a2s_workspace_bytes(T)
        saved = torch.empty(sv_b, dtype=torch.uint8, device=mel.device)
        ws = torch.empty(ws_b, dtype=torch.uint8, device=mel.device)
        out = torch.empty(T, OUT_FEATURES, dtype=torch.float32, device=mel.device)
        m = (None, None, None) if masks is None else masks
        # the parameters are read where they live, on every call: no packed copy can go stale after an optimizer step that
        # leaves the version counters alone (a captured fused Adam)
        check(L.n3dt_a2s_fwd(T, ctypes.byref(_c_params(params)), ops._ptr(mel), ops._ptr(m[0]), ops._ptr(m[1]), ops._ptr(m[2]),
                             ops._ptr(out), ops._ptr(saved), ctypes.c_size_t(sv_b), ops._ptr(ws), ctypes.c_size_t(ws_b), ops._stream()),
              "n3dt_a2s_fwd")
        if mod.keep_layer_outputs:
            # `saved` starts with mel [T,1280], then layer 0's and layer 1's outputs [T,1280] (csrc/audio_lstm.hip, a2s_saved)
            f = saved.view(torch.float32)
            mod.last_layer_outputs = tuple(f[(i + 1) * T * IN_FEATURES:(i + 2) * T * IN_FEATURES].view(T, IN_FEATURES) for i in range(2))
        ctx.keep = (saved, [t.detach() for t in params], T)
        ctx.mod = mod
        return out

    @staticmethod
    def backward(ctx, g_out):
        from . import ops
        from ._lib import lib, check
        saved, params, T = ctx.keep
        L = lib()
        g = g_out.detach().float().contiguous()
        views = ctx.mod._hand_out_grads()
        if views is None:
            # the arena cannot be used in this pass (see FlatGrads.hand_out): one fresh flat buffer in the same layout
            flat = torch.empty(sum(t.numel() for t in params), dtype=torch.float32, device=g.device)
            views, off = [], 0
            for t in params:
                views.append(flat[off:off + t.numel()].view(t.shape))
                off += t.numel()
        else:
            flat = ctx.mod.grad_arena().flat
        ws_b = L.n3dt_a2s_workspace_bytes(T)
        ws = torch.empty(ws_b, dtype=torch.uint8, device=g.device)
        check(L.n3dt_a2s_bwd(T, ctypes.byref(_c_params(params)), ops._ptr(g), ops._ptr(saved), ctypes.c_size_t(saved.numel()),
                             ops._ptr(flat), ops._ptr(ws), ctypes.c_size_t(ws_b), ops._stream()), "n3dt_a2s_bwd")
        ctx.keep = None
        grads = [v.view(t.shape) for v, t in zip(views, params)]
        del views, flat  # the returned views must be the only references (autograd then adopts them as .grad)
        return (None, None, None, *grads)


class Audio2style(nn.Module):
    """Drop-in for the reference's Audio2style (talker_trainer.py:428-461), forward and backward on libn3dt.

        a2s = n3dt.Audio2style().cuda()          # training mode, as the reference's module always is
        audiostyle = a2s(mel_batch)               # [B, 80, 16] -> [B, 64]; the B frames are ONE sequence
        opt_a2s = torch.optim.Adam(a2s.parameters(), lr=1e-7, betas=(0.5, 0.999))

    forward(mel, dropout_masks=None): in training mode the three dropout keep masks ([T,640], [T,320], [T,64]) are drawn with
    torch's RNG on the current stream (graph-safe) unless the caller passes them; `last_masks` holds the ones used last.
    In eval mode no dropout is applied.  The gradients of the trained tensors are slices of one flat buffer (grad_arena()),
    as HeadNeRFNet's; RNNModel.fc1 has none.  `keep_layer_outputs = True` makes `last_layer_outputs` the two LSTM layers'
    [T, 1280] outputs of the last forward (for inspection)."""

    def __init__(self, hidden_size=128):
        super().__init__()  # hidden_size: the reference's signature; its module ignores it, so does this one
        self.flatten = nn.Flatten()
        self.rnn = RNNModel(IN_FEATURES, HIDDEN)
        self.linear1 = nn.Sequential(nn.Linear(*HEAD[0]), nn.LeakyReLU(0.2, True), nn.Dropout(p=0.5))
        self.linear2 = nn.Sequential(nn.Linear(*HEAD[1]), nn.LeakyReLU(0.2, True), nn.Dropout(p=0.5))
        self.linear3 = nn.Sequential(nn.Linear(*HEAD[2]), nn.LeakyReLU(0.2, True), nn.Dropout(p=0.5))
        self.use_grad_arena = True
        self._grad_arena = None
        self.last_masks = None
        self.keep_layer_outputs = False
        self.last_layer_outputs = None

    def trained_parameters(self):
        """The 22 tensors forward reads, in the C ABI's grad-arena order (every parameter except rnn.fc1)."""
        out = []
        for quad in self.rnn.rnn.tensors():
            out.extend(quad)
        for seq in (self.linear1, self.linear2, self.linear3):
            out.extend((seq[0].weight, seq[0].bias))
        return out

    def grad_arena(self):
        """The persistent flat gradient buffer (n3dt.parallel.FlatGrads) over trained_parameters() that require grad; rnn.fc1
        is not in it.  Pass it to GradReducer next to HeadNeRFNet.grad_arena()."""
        from . import parallel
        params = [p for p in self.trained_parameters() if p.requires_grad]
        a = self._grad_arena
        if a is None or not a.matches(params):
            a = self._grad_arena = parallel.FlatGrads(params)
            for p in self.trained_parameters():
                p._n3dt_arena = a if p.requires_grad else None
        return a

    def _hand_out_grads(self):
        # the kernel writes the whole C layout at once, so the arena serves only when it holds all 22 tensors (its 64-element
        # alignment then coincides with the C layout: every size is a multiple of 64)
        params = self.trained_parameters()
        if not self.use_grad_arena or not all(p.requires_grad for p in params):
            return None
        return self.grad_arena().hand_out(params)

    def _mel(self, mel):
        if not torch.is_tensor(mel):
            raise ValueError("Audio2style: mel must be a tensor, got %s" % type(mel).__name__)
        if mel.dim() < 2 or (mel.shape[0] > 0 and mel[0].numel() != IN_FEATURES):
            raise ValueError("Audio2style: mel must be [B, 80, 16] (or [B, ...] with 80 * 16 = 1280 values per frame), got %s"
                             % (tuple(mel.shape),))
        T = mel.shape[0]
        if not 1 <= T <= MAX_T:
            raise ValueError("Audio2style: the sequence length T (the batch size) must be in 1..%d, got %d" % (MAX_T, T))
        if not mel.is_cuda:
            raise ValueError("Audio2style: mel must be a GPU tensor (there is no CPU path)")
        w = self.linear1[0].weight
        if not w.is_cuda or w.device != mel.device:
            raise ValueError("Audio2style: the module lives on %s, mel on %s" % (w.device, mel.device))
        return mel.detach().reshape(T, IN_FEATURES).to(torch.float32).contiguous()

    def draw_masks(self, T, device):
        """Three fresh keep masks of Bernoulli(0.5) (torch.rand on the current stream: registered with a captured graph)."""
        return tuple((torch.rand(T, n, device=device) < 0.5).to(torch.float32) for _, n in HEAD)

    def forward(self, mel, dropout_masks=None):
        x = self._mel(mel)
        T = x.shape[0]
        if self.training:
            if dropout_masks is None:
                masks = self.draw_masks(T, x.device)
            else:
                if len(dropout_masks) != 3:
                    raise ValueError("Audio2style: dropout_masks must be three keep masks ([T,640], [T,320], [T,64])")
                masks = []
                for m, (_, n) in zip(dropout_masks, HEAD):
                    if tuple(m.shape) != (T, n) or m.device != x.device:
                        raise ValueError("Audio2style: a dropout mask must be [%d, %d] on %s, got %s on %s"
                                         % (T, n, x.device, tuple(m.shape), m.device))
                    masks.append(m.detach().to(torch.float32).contiguous())
                masks = tuple(masks)
            self.last_masks = masks
        else:
            masks = None
            self.last_masks = None
        return _A2sFn.apply(self, x, masks, *self.trained_parameters())


def clip_audiostyle(a2s, front, wav, n_frames, fps=25.0, frames_per_sequence=1):
    """From a clip's waveform to its audiostyle codes: [n_frames, 64].

    `front` (n3dt.MelFrontend) computes the mel spectrogram of `wav` ([L] fp32 at 16 kHz on the GPU) and cuts the "chunk" window
    of every video frame 0 .. n_frames - 1; `a2s` is then called on groups of `frames_per_sequence` consecutive frames (the last
    group may be shorter).  The frames of one call are ONE LSTM sequence, as in the reference: 1 is its inference use
    (one frame per call), the training batch size is the other natural value; at most MAX_T.  `a2s` is used as it stands --
    its train/eval mode, and with it the dropout of the reference's always-training module, are the caller's choice."""
    n_frames, per = int(n_frames), int(frames_per_sequence)
    if n_frames < 1:
        raise ValueError("clip_audiostyle: n_frames must be >= 1, got %d" % n_frames)
    if not 1 <= per <= MAX_T:
        raise ValueError("clip_audiostyle: frames_per_sequence must be in 1..%d, got %d" % (MAX_T, per))
    windows = front.windows(front.melspectrogram(wav), range(n_frames), fps=fps, rule="chunk")
    return torch.cat([a2s(windows[i:i + per]) for i in range(0, n_frames, per)])
