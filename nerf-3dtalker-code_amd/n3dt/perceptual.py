"""VGG16 perceptual loss term of the reference's objective (Utils/HeadNeRFLossUtils.py:23-64, 140-154) on libn3dt's HIP kernels.

The reference builds it from torchvision's pretrained `vgg16().features[:23]`.  Nothing here downloads anything: the caller passes
the weights, as a torchvision `vgg16` state dict or the path of one (`torch.load` of a local file), e.g. the checkpoint torchvision
cached wherever the reference ran.  The weights are frozen; gradients go to the predicted image only.
"""
import ctypes

import torch

from ._host import PackedCache, open_state_dict, pack, take

# torchvision vgg16().features indices of the ten 3x3 convolutions in blocks [:4], [4:9], [9:16], [16:23]
VGG_CONV_INDICES = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21)
VGG_CONV_CHANNELS = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512))


def load_vgg16_features(src):
    """The ten (weight [C_out, C_in, 3, 3], bias [C_out]) pairs of `features[:23]` from a torchvision vgg16 state dict (or the path of
    one, read with torch.load).  `classifier.*` and the later feature layers are ignored; a missing or wrongly shaped key is refused
    with its name."""
    who = "load_vgg16_features"
    src = open_state_dict(who, src, expected="a torchvision vgg16 state dict or a path to one")
    return [(take(who, src, "features.%d.weight" % idx, (cout, cin, 3, 3)), take(who, src, "features.%d.bias" % idx, (cout,)))  # not converted
            for idx, (cin, cout) in zip(VGG_CONV_INDICES, VGG_CONV_CHANNELS)]


class _VggLoss(torch.autograd.Function):
    """n3dt_vgg_loss_fwd / n3dt_vgg_loss_bwd.  Outputs: the term (a 0-d view of terms[4]) and the four block terms (no gradient)."""

    @staticmethod
    def forward(ctx, merge_img, gt, mask, bg_value, mod):
        from . import ops
        from ._lib import lib, check
        B, _, P, _ = merge_img.shape
        m = merge_img.detach().float().contiguous()
        g = gt.detach().float().contiguous()
        k = None if mask is None else mask.detach().float().contiguous()
        packed = mod._packed_for(m.device)
        L = lib()
        sv_b, ws_b = L.n3dt_vgg_saved_bytes(B, mod.prec), L.n3dt_vgg_workspace_bytes(B, P, mod.prec)
        saved = torch.empty(sv_b, dtype=torch.uint8, device=m.device)
        ws = torch.empty(ws_b, dtype=torch.uint8, device=m.device)
        terms = torch.empty(5, dtype=torch.float32, device=m.device)
        check(L.n3dt_vgg_loss_fwd(B, P, mod.prec, ops._ptr(packed), ops._ptr(m), ops._ptr(g), ops._ptr(k), ctypes.c_float(bg_value),
                                  ops._ptr(terms), ops._ptr(saved), ctypes.c_size_t(sv_b), ops._ptr(ws), ctypes.c_size_t(ws_b),
                                  ops._stream()), "n3dt_vgg_loss_fwd")
        ctx.keep = (m, saved, packed)
        ctx.mod = mod
        ctx.set_materialize_grads(False)
        blocks = terms[:4]
        ctx.mark_non_differentiable(blocks)
        return terms[4], blocks

    @staticmethod
    def backward(ctx, g_total, _g_blocks):
        from . import ops
        from ._lib import lib, check
        if g_total is None:
            return None, None, None, None, None
        m, saved, packed = ctx.keep
        mod = ctx.mod
        B, _, P, _ = m.shape
        L = lib()
        ws_b = L.n3dt_vgg_workspace_bytes(B, P, mod.prec)
        ws = torch.empty(ws_b, dtype=torch.uint8, device=m.device)
        gt_ = g_total.detach().float().reshape(1).contiguous()
        d_merge = torch.empty_like(m)
        check(L.n3dt_vgg_loss_bwd(B, P, mod.prec, ops._ptr(packed), ops._ptr(m), ops._ptr(gt_), ops._ptr(saved),
                                  ctypes.c_size_t(saved.numel()), ops._ptr(d_merge), ops._ptr(ws), ctypes.c_size_t(ws_b), ops._stream()),
                  "n3dt_vgg_loss_bwd")
        return d_merge, None, None, None, None


class VGGPerceptualLoss(object):
    """Drop-in for the reference's VGGPerceptualLoss(resize=True) with caller-supplied weights: `loss = f(input, target)`.

    weights: load_vgg16_features() output, or what it accepts (a torchvision vgg16 state dict or its path).
    precision: "fp32" (split-bf16 operands, three products: the parity mode) or "bf16" (single bf16 operands: the fast mode), the
    module's train_precision convention.  The weights are packed once per device, and again when a weight tensor's version has
    changed since (an in-place update of a float32 tensor, which is held as the caller's); `repack()` forces it.  A call on another
    stream than the pack's waits for the pack first, and the uploaded fp32 weights are released once it has run."""

    def __init__(self, weights, precision="fp32"):
        from ._lib import PRECISIONS, F32, BF16
        if precision not in ("fp32", "bf16"):
            raise ValueError("VGGPerceptualLoss: precision must be 'fp32' or 'bf16', got %r" % (precision,))
        self.prec = PRECISIONS[precision]
        assert self.prec in (F32, BF16)
        self.precision = precision
        if not (isinstance(weights, (list, tuple)) and len(weights) == len(VGG_CONV_INDICES)):
            weights = load_vgg16_features(weights)
        for i, ((w, b), (cin, cout)) in enumerate(zip(weights, VGG_CONV_CHANNELS)):
            if tuple(w.shape) != (cout, cin, 3, 3) or tuple(b.shape) != (cout,):
                raise ValueError("VGGPerceptualLoss: conv %d has weight %s / bias %s, expected (%d, %d, 3, 3) / (%d,)"
                                 % (i, tuple(w.shape), tuple(b.shape), cout, cin, cout))
        self.weights = [(w.detach().float(), b.detach().float()) for w, b in weights]
        self._packed = PackedCache(lambda: [t for pair in self.weights for t in pair], self._pack)

    def repack(self):
        self._packed.clear()

    def _pack(self, device, dev):
        from ._lib import lib, VggParams
        p = VggParams()
        for i in range(len(self.weights)):
            p.weight[i], p.bias[i] = dev[2 * i].data_ptr(), dev[2 * i + 1].data_ptr()
        return pack("n3dt_vgg_pack", lib().n3dt_vgg_packed_bytes(self.prec), device, self.prec, ctypes.byref(p)), dev

    def _packed_for(self, device):
        return self._packed.get(device)

    def conv_stage(self, layer, x, dgrad=False, gate=None, out=None, out_pad=False):
        """n3dt_vgg_conv_stage: ONE conv of the table on NHWC fp32 device maps (the tests judge the kernel a layer at a time with it).
        x [n, H+2, W+2, C] with a zero halo (forward of layers 2, 4, 7: the un-pooled [n, 2H+2, 2W+2, C]).  forward: ReLU(conv + bias)
        [n, H, W, C_out]; dgrad: the gradient of the layer's input [n, H, W, C_in], kept where gate > 0 (gate: out's layout).
        out_pad: out is [n, H+2, W+2, C], interior written only; pass `out` to choose what the halo holds."""
        from . import ops
        from ._lib import lib, check
        cin, cout = VGG_CONV_CHANNELS[layer]
        pooled = (not dgrad) and layer in (2, 4, 7)
        n, hp, wp, c = x.shape
        if c != (cout if dgrad else cin) or x.dtype != torch.float32 or not x.is_contiguous():
            raise ValueError("VGGPerceptualLoss.conv_stage: layer %d %s takes contiguous fp32 [n, H+2, W+2, %d], got %s %s"
                             % (layer, "dgrad" if dgrad else "forward", cout if dgrad else cin, x.dtype, tuple(x.shape)))
        H, W = ((hp - 2) // 2, (wp - 2) // 2) if pooled else (hp - 2, wp - 2)
        shape = (n, H + 2, W + 2, cin if dgrad else cout) if out_pad else (n, H, W, cin if dgrad else cout)
        if out is None:
            out = torch.zeros(shape, dtype=torch.float32, device=x.device)
        if tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError("VGGPerceptualLoss.conv_stage: out must be contiguous fp32 %s, got %s" % (shape, tuple(out.shape)))
        if gate is not None and (tuple(gate.shape) != shape or gate.dtype != torch.float32 or not gate.is_contiguous()):
            raise ValueError("VGGPerceptualLoss.conv_stage: gate must be contiguous fp32 %s, got %s" % (shape, tuple(gate.shape)))
        check(lib().n3dt_vgg_conv_stage(self.prec, ops._ptr(self._packed_for(x.device)), layer, int(bool(dgrad)), n, H, W, ops._ptr(x),
                                        ops._ptr(gate), ops._ptr(out), int(bool(out_pad)), ops._stream()), "n3dt_vgg_conv_stage")
        return out

    def _check(self, merge_img, gt, mask):
        if merge_img.dim() != 4 or merge_img.shape[1] != 3 or merge_img.shape[2] != merge_img.shape[3]:
            raise ValueError("VGGPerceptualLoss: images must be [B,3,P,P], got %s" % (tuple(merge_img.shape),))
        if tuple(gt.shape) != tuple(merge_img.shape):
            raise ValueError("VGGPerceptualLoss: target %s does not match input %s" % (tuple(gt.shape), tuple(merge_img.shape)))
        B, _, P, _ = merge_img.shape
        if mask is not None and tuple(mask.shape) != (B, 1, P, P):
            raise ValueError("VGGPerceptualLoss: mask must be [B,1,P,P], got %s" % (tuple(mask.shape),))
        ts = (merge_img, gt) + (() if mask is None else (mask,))
        if not (merge_img.is_cuda and all(t.device == merge_img.device for t in ts)):
            raise ValueError("VGGPerceptualLoss: all tensors must live on the same GPU (no CPU fallback)")

    def masked_terms(self, merge_img, gt, mask, bg_value):
        """(term, block terms [4]) for input = nan_to_num(merge_img), target = gt with bg_value where mask < 0.5 (mask None: gt)."""
        self._check(merge_img, gt, mask)
        return _VggLoss.apply(merge_img, gt, mask, float(bg_value), self)

    def masked(self, merge_img, gt, mask, bg_value):
        """The fused form HeadNeRFLossUtils uses (Utils/HeadNeRFLossUtils.py:148-154)."""
        return self.masked_terms(merge_img, gt, mask, bg_value)[0]

    def __call__(self, input, target, feature_layers=(0, 1, 2, 3), style_layers=()):
        """The reference's call (:41-64).  The kernel applies nan_to_num to `input` (the reference's caller does, :137); for
        finite inputs the two are the same."""
        if list(style_layers):
            raise NotImplementedError("VGGPerceptualLoss: Gram (style) layers are not built; only the reference's default style_layers=[]")
        if list(feature_layers) != [0, 1, 2, 3]:
            raise NotImplementedError("VGGPerceptualLoss: only the reference's default feature_layers=[0, 1, 2, 3] is built")
        return self.masked(input, target, None, 0.0)
