"""Train-step harness around HeadNeRFNet (the caller side of SURVEY 8a row a12).

The reference's loop is `pred = model("train", ...)` -> data losses -> `backward()` -> two Adam steps
(talker_trainer.py:1008-1067).  The renderer's forward/backward and the fused loss tail run in libn3dt; the optimizer is
torch.optim.Adam as in the reference (make_optimizer) or the same step as one libn3dt launch (make_flat_optimizer).
"""
import torch
import torch.nn.functional as F


def disk_mask(batch, size, radius=0.35):
    """Synthetic head mask used by the benchmark / fixtures."""
    yy, xx = torch.meshgrid(torch.arange(size), torch.arange(size), indexing="ij")
    r2 = (xx - size / 2.0) ** 2 + (yy - size / 2.0) ** 2
    m = (r2 <= (radius * size) ** 2).float()
    return m.view(1, 1, size, size).repeat(batch, 1, 1, 1)


def data_losses(coarse, gt_rgb, mask, bg_value=1.0):
    """The three MSE data terms of the reference loss (Utils/HeadNeRFLossUtils.py:125-146,196-236); the VGG
    perceptual term is HeadNeRFLossUtils(vgg_weights=...) / n3dt.perceptual."""
    bg_img = coarse["bg_img"]
    bg_loss = torch.mean((bg_img - bg_value) * (bg_img - bg_value))
    res = torch.nan_to_num(coarse["merge_img"], nan=0.0)
    head = (mask >= 0.5).expand(-1, 3, -1, -1)
    nonhead = (mask < 0.5).expand(-1, 3, -1, -1)
    head_loss = F.mse_loss(res[head], gt_rgb[head])
    tv = res[nonhead] - bg_value
    nonhead_loss = torch.mean(tv * tv)
    return {"bg_loss": bg_loss, "head_loss": head_loss, "nonhead_loss": nonhead_loss}


class _FusedDataLoss(torch.autograd.Function):
    """bg / head / nonhead MSE terms and their sum in one pass over the images (n3dt_loss_fwd / n3dt_loss_bwd).
    Four scalar outputs (views of one 4-float buffer): indexing ONE output tensor instead cost the step a zeros + copy + add
    chain per term in backward.  The two image gradients are slices of one buffer, merged images first, so that the
    renderer's backward finds them adjacent and takes them as its d_img without a concatenation."""

    @staticmethod
    def forward(ctx, merge_img, bg_img, gt_rgb, mask, bg_value):
        import ctypes
        from . import ops
        from ._lib import lib, check
        B, _, P, Q = merge_img.shape
        # the kernel's contract (csrc/loss_tail.hip): ONE background image [1,3,P,P] (HeadNeRFNet.py:109 renders it at
        # batch 1), images [B,3,P,P], mask [B,1,P,P], all on the device of merge_img
        if tuple(merge_img.shape) != (B, 3, P, Q) or tuple(bg_img.shape) != (1, 3, P, Q):
            raise ValueError("fused_data_losses: merge_img must be [B,3,P,P] and bg_img [1,3,P,P], got %s and %s"
                             % (tuple(merge_img.shape), tuple(bg_img.shape)))
        if tuple(gt_rgb.shape) != tuple(merge_img.shape) or tuple(mask.shape) != (B, 1, P, Q):
            raise ValueError("fused_data_losses: gt_rgb must match merge_img and mask be [B,1,P,P], got %s and %s"
                             % (tuple(gt_rgb.shape), tuple(mask.shape)))
        if not (merge_img.is_cuda and all(t.device == merge_img.device for t in (bg_img, gt_rgb, mask))):
            raise ValueError("fused_data_losses: all tensors must live on the same GPU (no CPU fallback)")
        m, b, g, k = (t.detach().float().contiguous() for t in (merge_img, bg_img, gt_rgb, mask))
        acc = torch.empty(8, dtype=torch.float32, device=m.device)
        terms = torch.empty(4, dtype=torch.float32, device=m.device)
        check(lib().n3dt_loss_fwd(B, P * Q, ops._ptr(m), ops._ptr(b), ops._ptr(g), ops._ptr(k), ctypes.c_float(bg_value),
                                  ops._ptr(acc), ops._ptr(terms), ops._stream()), "n3dt_loss_fwd")
        ctx.keep, ctx.bg_value = (m, b, g, k, acc), bg_value
        ctx.set_materialize_grads(False)
        return terms[0], terms[1], terms[2], terms[3]

    @staticmethod
    def backward(ctx, g_bg, g_head, g_non, g_total):
        import ctypes
        from . import ops
        from ._lib import lib, check
        m, b, g, k, acc = ctx.keep
        B, _, P, Q = m.shape
        if g_bg is None and g_head is None and g_non is None and g_total is None:
            return None, None, None, None, None
        g3 = None
        if g_bg is not None or g_head is not None or g_non is not None:
            z = torch.zeros((), dtype=torch.float32, device=m.device)
            g3 = torch.stack([z if t is None else t.float() for t in (g_bg, g_head, g_non)])
        gt_ = None if g_total is None else g_total.float().contiguous()
        d_all = torch.empty(B + 1, 3, P, Q, dtype=torch.float32, device=m.device)  # [merge images..., background image]
        check(lib().n3dt_loss_bwd(B, P * Q, ops._ptr(m), ops._ptr(b), ops._ptr(g), ops._ptr(k), ctypes.c_float(ctx.bg_value),
                                  ops._ptr(acc), ops._ptr(g3), ops._ptr(gt_), ops._ptr(d_all[:B]), ops._ptr(d_all[B:]),
                                  ops._stream()), "n3dt_loss_bwd")
        return d_all[:B], d_all[B:], None, None, None


def fused_data_losses(coarse, gt_rgb, mask, bg_value=1.0):
    """Same three terms as data_losses(), computed by the fused HIP loss tail (no host synchronisation); `total_loss` is
    their sum in the reference's order ((bg + head) + nonhead), formed by the kernel."""
    t = _FusedDataLoss.apply(coarse["merge_img"], coarse["bg_img"], gt_rgb, mask, bg_value)
    return {"bg_loss": t[0], "head_loss": t[1], "nonhead_loss": t[2], "total_loss": t[3]}


class HeadNeRFLossUtils(object):
    """Drop-in for the reference's loss object (Utils/HeadNeRFLossUtils.py:66-236) on the fused HIP loss tail: same
    constructor, same `calc_total_loss(delta_cam_info, opt_code_dict, pred_dict, gt_rgb, mask_tensor, disp_pred_dict)` call,
    same result keys -- including the reference's spelling `nonhaed_loss` -- so the trainer's and the fitting script's loss lines
    (talker_trainer.py:1058, FittingSingleImage_new.py:894) stay as they are.  The VGG perceptual term (`use_vgg_loss=True`, the
    reference's default) runs on libn3dt's VGG kernels (n3dt.perceptual) with the caller's torchvision vgg16 weights: pass
    `vgg_weights` (a state dict or the path of one; nothing is downloaded).  `vgg_precision` follows train_precision: "fp32" is the
    parity mode, "bf16" the fast one."""

    def __init__(self, bg_type="white", use_vgg_loss=True, device=None, vgg_weights=None, vgg_precision="fp32"):
        if bg_type == "white":
            self.bg_value = 1.0
        elif bg_type == "black":
            self.bg_value = 0.0
        else:
            raise ValueError("Error BG type. ")  # the reference prints this and exit(0)s
        self.vgg_loss_func = None
        if use_vgg_loss:
            if vgg_weights is None:
                raise NotImplementedError("use_vgg_loss=True needs vgg_weights: pass torchvision's vgg16 state dict (or the path of its "
                                          "checkpoint) as vgg_weights -- pretrained weights are never downloaded -- or construct "
                                          "with use_vgg_loss=False")
            from .perceptual import VGGPerceptualLoss
            self.vgg_loss_func = VGGPerceptualLoss(vgg_weights, precision=vgg_precision)
        self.use_vgg_loss = bool(use_vgg_loss)
        self.device = device

    def _vgg(self, merge_img, gt_rgb, mask):
        # the reference: vgg_loss_func(nan_to_num(merge_img), gt with bg_value where mask < 0.5) (:137, :148-153)
        return self.vgg_loss_func.masked(merge_img, gt_rgb, mask, self.bg_value)

    def calc_data_loss(self, data_dict, gt_rgb, head_mask_c1b, nonhead_mask_c1b):
        """The reference passes the two boolean masks of `mask >= 0.5` / `mask < 0.5` (:200-201); the kernel takes the mask itself."""
        if not (nonhead_mask_c1b.dtype == torch.bool and head_mask_c1b.dtype == torch.bool):
            raise TypeError("calc_data_loss expects the boolean masks calc_total_loss builds")
        if bool((head_mask_c1b == nonhead_mask_c1b).any()):
            raise ValueError("head and non-head masks must be complementary (the fused kernel classifies each pixel once)")
        mask = head_mask_c1b.to(gt_rgb.dtype)
        t = fused_data_losses(data_dict, gt_rgb, mask, self.bg_value)
        res = {"bg_loss": t["bg_loss"], "head_loss": t["head_loss"], "nonhaed_loss": t["nonhead_loss"]}
        if self.use_vgg_loss:
            res["vgg"] = self._vgg(data_dict["merge_img"], gt_rgb, mask)
        return res

    def calc_total_loss(self, delta_cam_info, opt_code_dict, pred_dict, gt_rgb, mask_tensor, disp_pred_dict, eye_mask_tensor=None):
        """bg + head + non-head data terms (+ vgg) and their sum (:196-236; the camera / code / eye / displacement terms are commented
        out in the reference, so the first two and the last two arguments are accepted and unused, as there)."""
        t = fused_data_losses(pred_dict["coarse_dict"], gt_rgb, mask_tensor, self.bg_value)
        loss_dict = {"bg_loss": t["bg_loss"], "head_loss": t["head_loss"], "nonhaed_loss": t["nonhead_loss"]}
        # the reference adds the entries up in dict order (0.0 + bg + head + nonhead [+ vgg], :228-231); the kernel forms the first
        # three in the same order, so the autograd graph has one node instead of three additions
        total = t["total_loss"]
        if self.use_vgg_loss:
            loss_dict["vgg"] = self._vgg(pred_dict["coarse_dict"]["merge_img"], gt_rgb, mask_tensor)
            total = total + loss_dict["vgg"]
        loss_dict["total_loss"] = total
        return loss_dict


def make_optimizer(net, lr=1e-4):
    """Adam + StepLR as the reference builds them (talker_trainer.py:722-727)."""
    opt = torch.optim.Adam(net.parameters(), lr=lr)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=10, gamma=0.1)
    return opt, sched


def make_flat_optimizer(net, lr=1e-4, max_grad_norm=None, skip_nonfinite=False):
    """The same Adam + StepLR with the optimizer step on libn3dt (n3dt.FlatAdam: one launch over the net's gradient arena,
    version counters and packed-weight caches kept right after every step).  `max_grad_norm` / `skip_nonfinite`: FlatAdam's
    device-side global-norm clipping and non-finite step skipping (off by default)."""
    from .optim import FlatAdam
    opt = FlatAdam(net.parameters(), lr=lr, modules=[net], max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=10, gamma=0.1)
    return opt, sched


def train_step(net, optimizer, inputs, gt_rgb, mask, t_rand=None, extra_optimizers=(), fused_loss=True, loss_utils=None,
               audio2style=None):
    """One reference-shaped step: forward("train") -> losses -> zero_grad -> backward -> step.  `loss_utils`: a HeadNeRFLossUtils
    whose calc_total_loss forms the losses instead (the reference's own objective, e.g. with the VGG term).  `audio2style`: the
    co-trained encoder (n3dt.Audio2style); audiostyle = audio2style(inputs["mel_batch"]) then feeds the render
    (talker_trainer.py:1002-1008), and its optimizer belongs in `extra_optimizers`."""
    audiostyle = inputs["audiostyle"] if audio2style is None else audio2style(inputs["mel_batch"])
    pred = net("train", inputs["batch_xy"], inputs["batch_uv"], audiostyle, bg_code=None,
               shape_code=inputs["shape_code"], appea_code=inputs["appea_code"], batch_Rmats=inputs["batch_Rmats"],
               batch_Tvecs=inputs["batch_Tvecs"], batch_inv_inmats=inputs["batch_inv_inmats"], t_rand=t_rand)
    if loss_utils is not None:
        terms = loss_utils.calc_total_loss(None, None, pred, gt_rgb, mask, None)
    else:
        terms = (fused_data_losses if fused_loss else data_losses)(pred["coarse_dict"], gt_rgb, mask)
    total = terms["total_loss"] if "total_loss" in terms else terms["bg_loss"] + terms["head_loss"] + terms["nonhead_loss"]
    for o in extra_optimizers:
        o.zero_grad()
    optimizer.zero_grad()
    total.backward()
    optimizer.step()
    for o in extra_optimizers:
        o.step()
    terms["total_loss"] = total
    return pred, terms


class GraphedTrainStep:
    """One whole training step -- forward("train"), loss tail, backward, optimizer step(s) -- recorded ONCE into a hipGraph and
    replayed with one launch per step.  Every libn3dt entry point only enqueues on the caller's stream and allocates nothing, the
    autograd Functions allocate through PyTorch's caching allocator (a graph gets its private pool) and HeadNeRFNet's gradient
    arena is persistent, so the ~100 launches of a step are capturable as they are.  What the caller must provide:
      * `step_fn()` reads its inputs from tensors whose ADDRESSES do not change (refresh them with `.copy_()` before a
        replay) and takes no data-dependent Python branch;
      * optimizers built with `capturable=True` (their step counters then live on the device);
      * `zero_grad(set_to_none=True)` inside step_fn (the default), so that backward re-adopts the arena slices.
    Train-mode jitter: the forward's `torch.rand` is registered with the graph (PyTorch's graph-safe Philox offsets), so
    every replay draws fresh noise.  `warmup` eager steps run first on a side stream (allocator and optimizer state warm).
    The reference's step is launch-bound at small geometries (config 4: 2.1 of 2.6 ms is host enqueue time); a replay costs
    the host one launch."""

    def __init__(self, step_fn, warmup=3):
        self.step_fn = step_fn
        cur = torch.cuda.current_stream()
        side = torch.cuda.Stream()
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            for _ in range(warmup):
                step_fn()
        cur.wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, capture_error_mode="thread_local"):
            self.out = step_fn()

    def __call__(self):
        self.graph.replay()
        return self.out


_RENDER_KEYS = ("shape_code", "appea_code", "batch_Rmats", "batch_Tvecs", "batch_inv_inmats")


def validate(net, batches, audio2style=None, all_images=False, lpips_fn=None, lpips=None, sync=None):
    """The reference's validation pass (talker_trainer.py:1087-1150): render every held-out batch with net("test", ...) and score
    it with n3dt.eval_utils (SSIM and PSNR on the device; LPIPS only with `lpips` or `lpips_fn`, see calc_eval_metrics).
    `batches`: an iterable of dicts with the keys of synthetic.frame_inputs plus "gt_rgb" [B,3,P,P], "mask" (accepted and ignored,
    as the reference's metrics ignore it) and, for `audio2style`, "mel" (the encoder's input; audiostyle = audio2style(mel) then
    replaces the batch's own, talker_trainer.py:1113-1119; the encoder's train / eval mode is the caller's).
    all_images=False is the reference: image 0 of each batch, the mean over batches.  all_images=True averages every image.
    Returns {"SSIM", "PSNR", "count"}, `count` being the number of images scored.  With `lpips_fn(img1_u8, img2_u8) -> float`
    also "LPIPS": its mean over the SAME images (one call per scored image, on [P,P,3] uint8 arrays), at the cost of one copy to
    the host and one synchronisation per batch.  With `lpips`, an eval_utils.LPIPS object, "LPIPS" is computed on the device
    and accumulated there with the other two: still one synchronisation.  Giving both raises.
    With `sync`, an eval_utils.SyncMeter over the sequence's mel spectrogram, every rendered batch's merge_img is pushed to it in
    order -- ALL images of the batch, whatever `all_images` says; the batches must then be consecutive frames -- and the result
    gains "SYNC_conf", "SYNC_loss" and "SYNC_windows" (the meter's sync_conf, sync_loss and n_windows, over everything pushed to
    it so far; the meter is the caller's and is not reset).  Still one synchronisation.
    net.invalidate_packed() runs first, so weights written through `.data` or by a replayed training graph since the last
    render are the ones rendered; the metrics accumulate on the device and the host synchronises once, at the end.
    The reference calls model.eval() first and never switches back; the "test" forward does not read net.training, so this
    function does not touch it: net.training is left as it was found."""
    from . import eval_utils, ops
    if lpips is not None and lpips_fn is not None:
        raise ValueError("validate: give lpips= (on the device) or lpips_fn= (a host callback), not both")
    net.invalidate_packed()
    total, count, lpips_sum = None, 0, 0.0
    with torch.no_grad():
        for b in batches:
            audiostyle = b["audiostyle"] if audio2style is None else audio2style(b["mel"])
            pred = net("test", b["batch_xy"], b["batch_uv"], audiostyle, bg_code=None, **{k: b[k] for k in _RENDER_KEYS})
            merge, gt = pred["coarse_dict"]["merge_img"], b["gt_rgb"]
            if sync is not None:
                sync.push(merge)
            if not all_images:
                merge, gt = merge[:1], gt[:1]
            m = eval_utils._metrics(merge, gt).sum(dim=1)  # [2]: this batch's sums of SSIM and PSNR
            if lpips is not None:
                m = torch.cat([m, lpips(merge, gt).sum(dim=0, keepdim=True)])  # [3]: and of LPIPS
            total = m if total is None else total + m
            n = merge.shape[0]
            count += n
            if lpips_fn is not None:
                u8 = ops.img_to_uint8(torch.cat([merge, gt])).cpu().numpy()
                lpips_sum += sum(float(lpips_fn(u8[i], u8[n + i])) for i in range(n))
    if count == 0:
        raise ValueError("validate: no batches")
    if sync is not None:
        n_img = total.shape[0]
        means = torch.cat([total / count, sync._device_result()]).tolist()  # the one synchronisation
        means, synced = means[:n_img], sync._finish(means[n_img:])
    else:
        means = (total / count).tolist()
    res = {"SSIM": means[0], "PSNR": means[1], "count": count}
    if sync is not None:
        res["SYNC_conf"], res["SYNC_loss"], res["SYNC_windows"] = synced["sync_conf"], synced["sync_loss"], synced["n_windows"]
    if lpips is not None:
        res["LPIPS"] = means[2]
    if lpips_fn is not None:
        res["LPIPS"] = lpips_sum / count
    return res
