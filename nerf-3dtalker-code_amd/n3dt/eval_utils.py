"""The reference's validation metrics (Utils/Eval_utils.py) on libn3dt: SSIM, PSNR and LPIPS of rendered frames.

`calc_eval_metrics` keeps the reference's signature and quirks -- image 0 of the batch only, `mask_tensor` accepted and
ignored, the RGB image grey-converted as if it were BGR -- and `image_metrics` is the same arithmetic for every image of a
batch, left on the device.  Both run n3dt_eval_metrics (csrc/eval_metrics.hip): frames are quantised
to bytes, the 7x7 window sums and the squared error are exact integers, the rest is float64.

Quantisation: q = uint8(min(max(x * 255, 0), 255)) with the product in float32, NaN -> 0.  Inside [0, 1] that is the
reference's `(x * 255).astype(np.uint8)`; outside it numpy's cast is undefined and the clamp is this project's definition.

LPIPS (`LPIPS`, n3dt_lpips, csrc/lpips.hip) is lpips.LPIPS(net='alex') with the CALLER'S weights: AlexNet's
five convolutions and the metric's five linear layers, from a torchvision / lpips state dict.  Nothing is downloaded, the `lpips`
package is not a dependency and its pretrained weights have never been run through this code: parity is unpinned to the
dependency.  Pass the object as `lpips=`; the older host callback `lpips_fn=` keeps working.
The lip-sync score (`SyncNet`, `SyncMeter`, n3dt_syncnet_*, csrc/syncnet.hip) lives in n3dt/syncnet.py and is
re-exported here: what single-frame metrics cannot see -- whether the rendered lips follow the audio.
There is no CPU path.
"""
import ctypes

import torch

from . import ops
from ._host import PackedCache, count_or_raise, gpu_tensor, open_state_dict, pack, take, workspace
from ._lib import LPIPS_INPUT_MODES, LpipsParams, check, lib
from .syncnet import SyncMeter, SyncNet  # noqa: F401


def _pair(who, pred, gt):
    """pred and gt as contiguous float32 [B,3,H,W] GPU tensors of one shape on one device (B = 0 is the library's to refuse)"""
    for name, t in (("pred", pred), ("gt", gt)):
        gpu_tensor(who, name, t, copy=False)
        if t.dtype != torch.float32 or t.dim() != 4 or t.shape[1] != 3:
            raise ValueError("%s: %s must be float32 [B,3,H,W], got %s %s" % (who, name, t.dtype, tuple(t.shape)))
    if pred.shape != gt.shape or pred.device != gt.device:
        raise ValueError("%s: pred %s and gt %s differ in shape or device" % (who, tuple(pred.shape), tuple(gt.shape)))
    return pred.detach().contiguous(), gt.detach().contiguous()


def _metrics(pred, gt):
    """[2, B] float64 on the device: row 0 SSIM, row 1 PSNR.  Enqueues on the current stream, no synchronisation."""
    pred, gt = _pair("image_metrics", pred, gt)
    B, _, H, W = pred.shape
    L = lib()
    ws = workspace("eval_metrics", L.n3dt_eval_metrics_workspace_bytes(B, H, W), pred.device)
    out = torch.empty(2, B, dtype=torch.float64, device=pred.device)
    check(L.n3dt_eval_metrics(B, H, W, ops._ptr(pred), ops._ptr(gt), ops._ptr(out[0]), ops._ptr(out[1]), ops._ptr(ws),
                              ctypes.c_size_t(ws.numel()), ops._stream()), "n3dt_eval_metrics")
    return out


def image_metrics(pred, gt, lpips=None):
    """SSIM and PSNR of every image pair of a batch: pred, gt [B,3,H,W] float32 GPU tensors (any strides; H, W >= 7) ->
    {"SSIM": float64 [B], "PSNR": float64 [B]} on the device.  Stream-ordered, no synchronisation, bitwise reproducible.
    Values outside [0, 1] are clamped and NaN counts as 0 (see the module docstring).
    `lpips`: an `LPIPS` object; adds "LPIPS": float64 [B] (H, W >= 31)."""
    out = _metrics(pred, gt)
    res = {"SSIM": out[0], "PSNR": out[1]}
    if lpips is not None:
        res["LPIPS"] = lpips(pred, gt)
    return res


# torchvision alexnet().features: (index, C_in, C_out, kernel, stride, padding) of the five convolutions LPIPS reads; a 3 / 2
# max-pool sits in front of the second and the third (csrc/lpips_core.h holds the same geometry for the kernels)
ALEXNET_CONVS = ((0, 3, 64, 11, 4, 2), (3, 64, 192, 5, 1, 2), (6, 192, 384, 3, 1, 1), (8, 384, 256, 3, 1, 1), (10, 256, 256, 3, 1, 1))


def _lpips_keys(layer, idx):
    """the names one tensor may carry: torchvision's, then lpips's own (net.slice{k}.{idx} holds torchvision's features[idx])"""
    return ["features.%d" % idx, "net.slice%d.%d" % (layer + 1, idx)]


def load_lpips_alex(state_dict):
    """[(weight, bias, lin)] x 5 from a state dict holding AlexNet's five convolutions
    as torchvision names them (`features.{0,3,6,8,10}.{weight,bias}`) or as lpips does (`net.slice{1..5}.{0,3,6,8,10}.*`), and the
    linear layers as `lin{k}.model.1.weight` or `lins.{k}.model.1.weight` ([1, C, 1, 1] or [C]).  Other keys (`scaling_layer.*`,
    `classifier.*`) are ignored.  A missing or wrongly shaped tensor is refused with its key."""
    sd = open_state_dict("load_lpips_alex", state_dict, paths=False)

    def get(names, shapes):
        return take("load_lpips_alex", sd, names[0], shapes, names[1:]).float()  # a float32 tensor stays the caller's

    out = []
    for layer, (idx, cin, cout, k, _, _) in enumerate(ALEXNET_CONVS):
        w = get([n + ".weight" for n in _lpips_keys(layer, idx)], (cout, cin, k, k))
        b = get([n + ".bias" for n in _lpips_keys(layer, idx)], (cout,))
        lin = get(["lin%d.model.1.weight" % layer, "lins.%d.model.1.weight" % layer], [(1, cout, 1, 1), (cout,)])
        out.append((w, b, lin.reshape(cout)))  # a view of a float32 `lin`: it shares the caller's version counter
    return out


class LPIPS(object):
    """lpips.LPIPS(net='alex') on libn3dt with caller-supplied weights (see load_lpips_alex for what `state_dict` may be).

    input_mode "reference" (the default) reproduces Utils/Eval_utils.compute_LPIPS: the images are quantised to bytes, the
    [H,W,3] byte image is read as [3,H,W] by a reshape (not a transpose) and fed as values 0..255.  "standard" is the metric as
    its authors define it: channels as given, 2 clamp(x, 0, 1) - 1.
    `lpips(pred, gt)`: [B,3,H,W] float32 GPU tensors (any strides; 31 <= H, W <= 2048, B <= 64) -> float64 [B] on the device,
    stream-ordered, no synchronisation, bitwise reproducible; `lpips.layers(pred, gt)` -> the five layer values, [5, B].
    The weights are packed once per device, and again when a weight tensor's version has changed since (an in-place update);
    `repack()` forces it."""

    def __init__(self, state_dict, input_mode="reference"):
        if input_mode not in LPIPS_INPUT_MODES:
            raise ValueError("LPIPS: input_mode must be 'reference' or 'standard', got %r" % (input_mode,))
        self.input_mode = input_mode
        self.weights = load_lpips_alex(state_dict)
        self._packed = PackedCache(lambda: [t for layer in self.weights for t in layer], self._pack)

    def repack(self):
        self._packed.clear()

    def _pack(self, device, dev):
        p = LpipsParams()
        for i in range(len(self.weights)):
            p.weight[i], p.bias[i], p.lin[i] = (t.data_ptr() for t in dev[3 * i:3 * i + 3])
        return pack("n3dt_lpips_pack", lib().n3dt_lpips_packed_bytes(), device, ctypes.byref(p)), dev

    def _packed_for(self, device):
        return self._packed.get(device)

    def _run(self, pred, gt):
        """[6, B] float64: row 0 the score, rows 1..5 the layer values"""
        pred, gt = _pair("LPIPS", pred, gt)
        B, _, H, W = pred.shape
        L = lib()
        nbytes = count_or_raise(L.n3dt_lpips_workspace_bytes(B, H, W))  # a size the library refuses is refused before anything is packed
        packed = self._packed_for(pred.device)
        ws = workspace("lpips", nbytes, pred.device)
        out = torch.empty(6, B, dtype=torch.float64, device=pred.device)
        check(L.n3dt_lpips(B, H, W, LPIPS_INPUT_MODES[self.input_mode], ops._ptr(packed), ops._ptr(pred), ops._ptr(gt), ops._ptr(out[0]),
                           ops._ptr(out[1:]), ops._ptr(ws), ctypes.c_size_t(ws.numel()), ops._stream()), "n3dt_lpips")
        return out

    def __call__(self, pred, gt):
        return self._run(pred, gt)[0]

    def layers(self, pred, gt):
        return self._run(pred, gt)[1:]


def calc_eval_metrics(pred_dict, gt_rgb, mask_tensor, eye_mask_tensor=None, vis=False, lpips_fn=None, lpips=None):
    """Utils/Eval_utils.calc_eval_metrics: {"SSIM", "PSNR"} as Python floats for IMAGE 0 of
    pred_dict["coarse_dict"]["merge_img"] against gt_rgb[0]; `mask_tensor` and `eye_mask_tensor` are ignored, as the
    reference ignores them.  One synchronisation (the copy of the two numbers to the host).
    `lpips_fn(img1_u8, img2_u8) -> float`, when given, is called once with the two [H,W,3] uint8 numpy images (one more
    copy to the host) and its result is returned as "LPIPS".  `lpips`, an `LPIPS` object, computes "LPIPS" on the device
    instead, within the same single synchronisation; giving both raises.  `vis=True` raises: there is no display."""
    if vis:
        raise ValueError("calc_eval_metrics: vis=True needs a display, which this build does not have")
    if lpips is not None and lpips_fn is not None:
        raise ValueError("calc_eval_metrics: give lpips= (on the device) or lpips_fn= (a host callback), not both")
    pred = pred_dict["coarse_dict"]["merge_img"][:1]
    gt = gt_rgb[:1]
    m = _metrics(pred, gt)[:, 0]
    if lpips is not None:
        ssim, psnr, lp = torch.cat([m, lpips(pred, gt)]).tolist()
        return {"SSIM": ssim, "PSNR": psnr, "LPIPS": lp}
    ssim, psnr = m.tolist()
    res = {"SSIM": ssim, "PSNR": psnr}
    if lpips_fn is not None:
        u8 = ops.img_to_uint8(torch.cat([pred.detach(), gt.detach()])).cpu().numpy()
        res["LPIPS"] = float(lpips_fn(u8[0], u8[1]))
    return res
