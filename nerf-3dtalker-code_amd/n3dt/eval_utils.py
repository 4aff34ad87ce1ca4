"""The reference's validation metrics (Utils/Eval_utils.py) on libn3dt: SSIM and PSNR of rendered frames.

`calc_eval_metrics` keeps the reference's signature and quirks -- image 0 of the batch only, `mask_tensor` accepted and
ignored, the RGB image grey-converted as if it were BGR -- and `image_metrics` is the same arithmetic for every image of a
batch, left on the device.  Both run n3dt_eval_metrics (csrc/eval_metrics.hip): frames are quantised
to bytes, the 7x7 window sums and the squared error are exact integers, the rest is float64.

Quantisation: q = uint8(min(max(x * 255, 0), 255)) with the product in float32, NaN -> 0.  Inside [0, 1] that is the
reference's `(x * 255).astype(np.uint8)`; outside it numpy's cast is undefined and the clamp is this project's definition.

LPIPS is not built (it needs AlexNet weights and a package this project does not carry): pass `lpips_fn` to add it.
There is no CPU path.
"""
import ctypes

import torch

from . import ops
from ._lib import check, lib


def _metrics(pred, gt):
    """[2, B] float64 on the device: row 0 SSIM, row 1 PSNR.  Enqueues on the current stream, no synchronisation."""
    for name, t in (("pred", pred), ("gt", gt)):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise ValueError("image_metrics: %s must be a GPU tensor (there is no CPU path)" % name)
        if t.dtype != torch.float32 or t.dim() != 4 or t.shape[1] != 3:
            raise ValueError("image_metrics: %s must be float32 [B,3,H,W], got %s %s" % (name, t.dtype, tuple(t.shape)))
    if pred.shape != gt.shape or pred.device != gt.device:
        raise ValueError("image_metrics: pred %s and gt %s differ in shape or device" % (tuple(pred.shape), tuple(gt.shape)))
    pred, gt = pred.detach().contiguous(), gt.detach().contiguous()
    B, _, H, W = pred.shape
    L = lib()
    nbytes = L.n3dt_eval_metrics_workspace_bytes(B, H, W)
    if nbytes == 0:
        raise ValueError(L.n3dt_last_error().decode())
    ws = ops.WORKSPACE.get("eval_metrics", nbytes, pred.device)
    out = torch.empty(2, B, dtype=torch.float64, device=pred.device)
    check(L.n3dt_eval_metrics(B, H, W, ops._ptr(pred), ops._ptr(gt), ops._ptr(out[0]), ops._ptr(out[1]), ops._ptr(ws),
                              ctypes.c_size_t(ws.numel()), ops._stream()), "n3dt_eval_metrics")
    return out


def image_metrics(pred, gt):
    """SSIM and PSNR of every image pair of a batch: pred, gt [B,3,H,W] float32 GPU tensors (any strides; H, W >= 7) ->
    {"SSIM": float64 [B], "PSNR": float64 [B]} on the device.  Stream-ordered, no synchronisation, bitwise reproducible.
    Values outside [0, 1] are clamped and NaN counts as 0 (see the module docstring)."""
    out = _metrics(pred, gt)
    return {"SSIM": out[0], "PSNR": out[1]}


def calc_eval_metrics(pred_dict, gt_rgb, mask_tensor, eye_mask_tensor=None, vis=False, lpips_fn=None):
    """Utils/Eval_utils.calc_eval_metrics: {"SSIM", "PSNR"} as Python floats for IMAGE 0 of
    pred_dict["coarse_dict"]["merge_img"] against gt_rgb[0]; `mask_tensor` and `eye_mask_tensor` are ignored, as the
    reference ignores them.  One synchronisation (the copy of the two numbers to the host).
    `lpips_fn(img1_u8, img2_u8) -> float`, when given, is called once with the two [H,W,3] uint8 numpy images (one more
    copy to the host) and its result is returned as "LPIPS".  `vis=True` raises: there is no display."""
    if vis:
        raise ValueError("calc_eval_metrics: vis=True needs a display, which this build does not have")
    pred = pred_dict["coarse_dict"]["merge_img"][:1]
    gt = gt_rgb[:1]
    ssim, psnr = _metrics(pred, gt)[:, 0].tolist()
    res = {"SSIM": ssim, "PSNR": psnr}
    if lpips_fn is not None:
        u8 = ops.img_to_uint8(torch.cat([pred.detach(), gt.detach()])).cpu().numpy()
        res["LPIPS"] = float(lpips_fn(u8[0], u8[1]))
    return res
