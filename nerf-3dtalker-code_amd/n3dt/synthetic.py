"""Parameter inventory and seeded synthetic inputs for the head-render path.

The reference ships neither checkpoints nor camera intrinsics (SURVEY.md
header), so every number this repo produces is on seeded random weights and a
synthetic camera.  This module is the single source of those inputs: the golden
fixture generator (tools/gen_golden.py) loads `make_state_dict()` into the
reference module with a strict `load_state_dict`, and the tests / bench feed the
same tensors to the HIP path.  Everything is generated on the CPU with an
explicit `torch.Generator`, so it is identical here and on the GPU box.

Reference shapes followed (not copied):
  MLP layer shapes / init rules ....... NetWorks/models.py:29-59
  neural renderer layer shapes ........ NetWorks/neural_renderer.py:49-69
  pixel-shuffle block shapes .......... NetWorks/PixelShuffleUpsample.py:29-33
  ray grid ............................ Utils/RenderUtils.py:31-43
  inverse intrinsics form ............. XGaze_utils/data_loader_xgaze_new.py:1092-1097
  default camera ...................... Utils/RenderUtils.py:53-99
"""
import math
from collections import OrderedDict

import torch

PE_FREQS = 10
PE_DIM = 3 + 6 * PE_FREQS  # 63 (reference: HeadNeRFNet.py:27-28,50)


def n_blocks(opt):
    return int(math.log2(opt.pred_img_size) - math.log2(opt.featmap_size))


def mlp_dims(opt, include_gaze=False, eye_gaze_dim=2, audio_dim=64, include_vd=False):
    """Channel bookkeeping of the latent-conditioned MLP.  include_vd: RGB_layer_1 takes 27 more channels (the
    4-frequency encoding of the ray direction, NetWorks/HeadNeRFNet.py:56-63), between RGB_layer_0's output and the appearance code."""
    shape_dim = opt.iden_code_dims + opt.expr_code_dims + (eye_gaze_dim if include_gaze else 0)
    appea_dim = opt.text_code_dims + opt.illu_code_dims
    vp = PE_DIM + shape_dim
    return {
        "H": opt.mlp_hidden_nchannels,
        "C": opt.featmap_nc,
        "shape_dim": shape_dim,
        "appea_dim": appea_dim,
        "audio_dim": audio_dim,
        "vp": vp,
        "in0": vp + audio_dim,
        "in5": vp + opt.mlp_hidden_nchannels,
        "in_rgb1": opt.mlp_hidden_nchannels + (27 if include_vd else 0) + appea_dim,
    }


def param_specs(opt, include_gaze=False, eye_gaze_dim=2, audio_dim=64, hier_sampling=False, include_vd=False):
    """Ordered name -> (shape, init_kind, is_buffer).

    init_kind: "xavier" | "default_w" | "default_b" | "zero" | "ones" | "blur"
    Key names are the reference module's state-dict keys.
    """
    d = mlp_dims(opt, include_gaze, eye_gaze_dim, audio_dim, include_vd)
    H, C = d["H"], d["C"]
    specs = OrderedDict()

    def conv(prefix, cin, cout, w_init, b_init="default_b"):
        specs[prefix + ".weight"] = ((cout, cin, 1, 1), w_init, False)
        specs[prefix + ".bias"] = ((cout,), b_init, False)

    p = "fg_CD_predictor."
    conv(p + "FeaExt_module_0", d["in0"], H, "default_w")
    for i in range(1, 8):
        conv(p + "FeaExt_module_%d" % i, d["in5"] if i == 5 else H, H, "xavier")
    conv(p + "density_module", H, 1, "xavier", "zero")
    conv(p + "RGB_layer_0", H, H, "xavier")
    conv(p + "RGB_layer_1", d["in_rgb1"], H // 2, "default_w")
    conv(p + "RGB_layer_2", H // 2, C, "default_w")

    nb = n_blocks(opt)
    fs = opt.featmap_size
    q = "neural_render."
    specs[q + "bg_featmap"] = ((1, C, fs, fs), "ones" if opt.bg_type == "white" else "zero", False)
    for i in range(nb):
        ci = max(C // (2 ** i), 32)
        conv(q + "feat_upsample_list.%d.layer_1" % i, ci, ci * 2, "default_w")
        conv(q + "feat_upsample_list.%d.layer_2" % i, ci * 2, ci * 4, "default_w")
        specs[q + "feat_upsample_list.%d.blur_layer.f" % i] = ((3,), "blur", True)
    specs[q + "rgb_upsample.1.f"] = ((3,), "blur", True)
    conv(q + "feat_2_rgb_list.0", C, 3, "default_w")
    for i in range(nb):
        conv(q + "feat_2_rgb_list.%d" % (i + 1), max(C // (2 ** (i + 1)), 32), 3, "default_w")
    for i in range(nb):
        conv(q + "feat_layers.%d" % i, max(C // (2 ** i), 32), max(C // (2 ** (i + 1)), 32), "default_w")
    if hier_sampling:
        # the second network of the hierarchical pass (NetWorks/HeadNeRFNet.py:72-74).  Listed last so that the seeded
        # values of every other tensor do not depend on this flag.
        p = "fine_fg_CD_predictor."
        conv(p + "FeaExt_module_0", d["in0"], H, "default_w")
        for i in range(1, 8):
            conv(p + "FeaExt_module_%d" % i, d["in5"] if i == 5 else H, H, "xavier")
        conv(p + "density_module", H, 1, "xavier", "zero")
        conv(p + "RGB_layer_0", H, H, "xavier")
        conv(p + "RGB_layer_1", d["in_rgb1"], H // 2, "default_w")
        conv(p + "RGB_layer_2", H // 2, C, "default_w")
    return specs


def init_tensor(shape, kind, gen, fan_in_of_weight=None):
    """One tensor under the reference's init rule for its layer."""
    if kind == "zero":
        return torch.zeros(shape)
    if kind == "ones":
        return torch.ones(shape)
    if kind == "blur":
        return torch.tensor([1.0, 2.0, 1.0])
    if kind == "xavier":
        cout, cin = shape[0], shape[1]
        a = math.sqrt(6.0 / (cin + cout))
    elif kind == "default_w":  # kaiming_uniform(a=sqrt(5)) == U(-1/sqrt(fan_in), 1/sqrt(fan_in))
        a = 1.0 / math.sqrt(shape[1])
    elif kind == "default_b":
        a = 1.0 / math.sqrt(fan_in_of_weight)
    else:
        raise ValueError(kind)
    return (torch.rand(shape, generator=gen) * 2.0 - 1.0) * a


def make_state_dict(opt, seed=0, include_gaze=False, eye_gaze_dim=2, audio_dim=64, bg_noise=0.0, hier_sampling=False, include_vd=False):
    """Seeded random weights with the reference's per-layer init distributions.

    bg_noise > 0 perturbs the learned background feature map away from its
    all-ones initial value so that the merge seam is exercised non-trivially.
    """
    gen = torch.Generator().manual_seed(seed)
    sd = OrderedDict()
    last_fan_in = None
    fine = OrderedDict()
    for name, (shape, kind, _buf) in param_specs(opt, include_gaze, eye_gaze_dim, audio_dim, hier_sampling, include_vd).items():
        if name.startswith("fine_"):
            fine[name] = (shape, kind)
            continue
        if name.endswith(".weight"):
            last_fan_in = shape[1]
        sd[name] = init_tensor(shape, kind, gen, last_fan_in)
    if bg_noise > 0.0:
        k = "neural_render.bg_featmap"
        sd[k] = sd[k] + bg_noise * torch.randn(sd[k].shape, generator=gen)
    for name, (shape, kind) in fine.items():  # drawn after everything else (see param_specs)
        if name.endswith(".weight"):
            last_fan_in = shape[1]
        sd[name] = init_tensor(shape, kind, gen, last_fan_in)
    return sd


def contrast_state_dict(opt, seed=0, density_gain=400.0, density_bias=-60.0, feat_gain=40.0):
    """Seeded weights that stress the 16-bit modes (fixture `contrast`): the density head is scaled (and biased negative)
    so that alpha saturates on part of the rays and vanishes on others -- sharp weights, front-most samples carrying the
    whole ray -- and RGB_layer_2 is scaled so that features are O(10)."""
    sd = make_state_dict(opt, seed=seed, bg_noise=0.1)
    p = "fg_CD_predictor."
    sd[p + "density_module.weight"] = sd[p + "density_module.weight"] * density_gain
    sd[p + "density_module.bias"] = sd[p + "density_module.bias"] + density_bias
    sd[p + "RGB_layer_2.weight"] = sd[p + "RGB_layer_2.weight"] * feat_gain
    sd[p + "RGB_layer_2.bias"] = sd[p + "RGB_layer_2.bias"] * feat_gain
    return sd


def state_dict_checksum(sd):
    """Cheap drift detector stored next to every fixture."""
    tot, asum = 0.0, 0.0
    for v in sd.values():
        v64 = v.double()
        tot += float(v64.sum())
        asum += float(v64.abs().sum())
    return [tot, asum]


def ray_grid(fs, n_side=None):
    """Integer pixel-centre ray grid, x = i % w, y = i // w (no +0.5).

    Returns batch_xy [1,2,N_r] float32 and batch_uv [1,N_r,2] (unused by the net).
    n_side lets the 'literal' reading cast rays on an n_side x n_side grid while
    keeping intrinsics expressed in that grid's pixel units.
    """
    w = n_side or fs
    idx = torch.arange(w * w)
    x = (idx % w).float()
    y = torch.div(idx, w, rounding_mode="floor").float()
    xy = torch.stack([x, y], dim=0).unsqueeze(0)
    uv = torch.stack([x / float(w), y / float(w)], dim=-1).unsqueeze(0)
    return xy, uv


def inv_intrinsics(grid, batch):
    """K^-1 for focal 1200*grid/512 and principal point grid/2."""
    f = 1200.0 * grid / 512.0
    c = grid / 2.0
    k = torch.tensor([[1.0 / f, 0.0, -c / f], [0.0, 1.0 / f, -c / f], [0.0, 0.0, 1.0]])
    return k.unsqueeze(0).repeat(batch, 1, 1).contiguous()


def cameras(batch, yaw_range=0.3, seed=99):
    """c2w rotation diag(1,-1,-1) (optionally yawed about world y) and T=(0,0,12)."""
    gen = torch.Generator().manual_seed(seed)
    base = torch.diag(torch.tensor([1.0, -1.0, -1.0]))
    Rs, Ts = [], []
    for _ in range(batch):
        yaw = (torch.rand((), generator=gen).item() * 2.0 - 1.0) * yaw_range
        cy, sy = math.cos(yaw), math.sin(yaw)
        Ry = torch.tensor([[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]])
        Rs.append(Ry @ base)
        # keep the camera on the orbit sphere so the head stays in the slab
        Ts.append(Ry @ torch.tensor([[0.0], [0.0], [12.0]]))
    return torch.stack(Rs).contiguous(), torch.stack(Ts).contiguous()


def latents(batch, shape_dim=179, appea_dim=127, audio_dim=64, first_frame=0):
    """0.5*N(0,1) codes, one generator per frame index (seed 1234+frame)."""
    sh, ap, au = [], [], []
    for b in range(batch):
        gen = torch.Generator().manual_seed(1234 + first_frame + b)
        sh.append(0.5 * torch.randn(shape_dim, generator=gen))
        ap.append(0.5 * torch.randn(appea_dim, generator=gen))
        au.append(0.5 * torch.randn(max(audio_dim, 1), generator=gen)[:audio_dim])
    return torch.stack(sh), torch.stack(ap), torch.stack(au)


def stratified_noise(batch, n_rays, n_samples, seed=7):
    """The per-edge jitter tensor the train mode consumes."""
    gen = torch.Generator().manual_seed(seed)
    return torch.rand(batch, n_rays, n_samples + 1, generator=gen)


def frame_inputs(opt, batch, n_side=None, yaw_range=0.3, include_gaze=False, eye_gaze_dim=2,
                 audio_dim=64, first_frame=0):
    """All forward() inputs for `batch` synthetic frames, keyed by the reference's kwarg names."""
    grid = n_side or opt.featmap_size
    d = mlp_dims(opt, include_gaze, eye_gaze_dim, audio_dim)
    xy, uv = ray_grid(opt.featmap_size, n_side)
    R, T = cameras(batch, yaw_range)
    sh, ap, au = latents(batch, d["shape_dim"], d["appea_dim"], audio_dim, first_frame)
    return {
        "batch_xy": xy.expand(batch, -1, -1),
        "batch_uv": uv.expand(batch, -1, -1),
        "audiostyle": au,
        "bg_code": None,
        "shape_code": sh,
        "appea_code": ap,
        "batch_Rmats": R,
        "batch_Tvecs": T,
        "batch_inv_inmats": inv_intrinsics(grid, batch),
    }


def sharp_target(batch, size, radius=0.35, seed=4321):
    """Training target of train_sharp_head: inside a disk a smooth seeded colour pattern in [0.1, 0.9], outside white (the
    reference's white background, Utils/HeadNeRFLossUtils.py:77-80).  Returns (gt [B,3,P,P], mask [B,1,P,P])."""
    gen = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(size, dtype=torch.float32), torch.arange(size, dtype=torch.float32), indexing="ij")
    r2 = (xx - size / 2.0) ** 2 + (yy - size / 2.0) ** 2
    m = (r2 <= (radius * size) ** 2).float()
    gts = []
    for _ in range(batch):
        ch = []
        for _c in range(3):
            fx, fy, ph = (torch.rand(3, generator=gen) * torch.tensor([3.0, 3.0, 6.28])).tolist()
            ch.append(0.5 + 0.4 * torch.sin(6.2832 * (fx * xx + fy * yy) / size + ph))
        g = torch.stack(ch)
        gts.append(g * m + (1.0 - m))
    return torch.stack(gts), m.view(1, 1, size, size).repeat(batch, 1, 1, 1)


def train_sharp_head(opt, dev, steps=400, lr=1e-3, batch=2, train_precision="fp32", seed=0, want_share=0.2, check_every=25,
                     log_every=0, log=None):
    """A head made sharp by the build's OWN trainer (the released checkpoints are absent, so what a trained network
    looks like to the 16-bit arithmetic is answered by training one): seed-`seed` weights, `steps` Adam steps (at most) of the
    differentiable path (`train_precision`, exact fp32 by default) on `batch` synthetic frames against sharp_target() with the
    reference's three data terms, stopping once alpha has saturated on `want_share` of the rays in both senses: the ray is opaque
    (bg_alpha < 0.01) AND one sample carries it (compositing weight > 0.9: a hard surface, what stresses 16-bit arithmetic).
    Measured at config 4's geometry, lr 1e-3, B = 2: 20 % one-sample rays after ~100 steps, 30 % after ~200 (3 - 4 s; the loss has
    fallen 180-fold), 46 % after 800; every ray is opaque from step 25 on.  Returns (net, info); info carries the alpha statistics."""
    from . import HeadNeRFNet
    from .train import fused_data_losses
    net = HeadNeRFNet(opt, include_vd=False, hier_sampling=False, precision="fp32", train_precision=train_precision).to(dev)
    net.load_state_dict(make_state_dict(opt, seed=seed, bg_noise=0.1), strict=True)
    d = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in frame_inputs(opt, batch).items()}
    gt, mask = sharp_target(batch, opt.pred_img_size)
    gt, mask = gt.to(dev), mask.to(dev)
    optim = torch.optim.Adam(net.parameters(), lr=lr)
    args = (d["batch_xy"], d["batch_uv"], d["audiostyle"], None, d["shape_code"], d["appea_code"], d["batch_Rmats"], d["batch_Tvecs"],
            d["batch_inv_inmats"])

    def stats():
        with torch.no_grad():
            o = net.render_features(d["batch_xy"], d["audiostyle"], d["shape_code"], d["appea_code"], d["batch_Rmats"], d["batch_Tvecs"],
                                    d["batch_inv_inmats"], want_merge=False, want_weight=True, precision="fp32")
        ba = o["bg_alpha"].float()
        w = o["weight"].float()
        return {"alpha_saturated_ray_share": float((ba < 0.01).float().mean()), "transparent_ray_share": float((ba > 0.5).float().mean()),
                "one_sample_rays_share": float((w.max(dim=-1).values > 0.9).float().mean()),  # one sample carries the ray: a hard surface
                "weight_max": float(w.max()), "fg_feat_abs_max": float(o["fg_feat"].abs().max())}

    loss0 = lossv = None
    done = 0
    st = stats()
    for it in range(steps):
        out = net("train", *args)
        t = fused_data_losses(out["coarse_dict"], gt, mask)
        optim.zero_grad()
        t["total_loss"].backward()
        optim.step()
        done = it + 1
        if it == 0:
            loss0 = float(t["total_loss"].detach())
        if done % check_every == 0 or done == steps:
            st = stats()
            lossv = float(t["total_loss"].detach())
            if log is not None and log_every and done % log_every == 0:
                log("step %4d  loss %.5f  %s" % (done, lossv, st))
            if st["alpha_saturated_ray_share"] >= want_share and st["one_sample_rays_share"] >= want_share:
                break
    net.zero_grad(set_to_none=True)
    info = dict(st)
    info.update({"steps": done, "lr": lr, "batch": batch, "train_precision": train_precision, "loss_first": loss0, "loss_last": lossv,
                 "target": "disk of a seeded colour pattern on white, bg + head + nonhead MSE terms"})
    return net, info


# torchvision vgg16 (configuration "D") feature extractor: conv widths, "M" = 2x2 max-pool
VGG16_CFG = (64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M")


def vgg16_features_state_dict(seed=0):
    """Seeded stand-in for torchvision's pretrained vgg16 `features.*` weights (the real ones cannot be fetched offline): the
    13 convolutions at torchvision's indices, He-normal weights std = sqrt(2 / (9 C_in)) and small non-zero biases."""
    gen = torch.Generator().manual_seed(seed)
    sd, idx, cin = {}, 0, 3
    for v in VGG16_CFG:
        if v == "M":
            idx += 1
            continue
        std = math.sqrt(2.0 / (9 * cin))
        sd["features.%d.weight" % idx] = torch.randn(v, cin, 3, 3, generator=gen) * std
        sd["features.%d.bias" % idx] = (torch.rand(v, generator=gen) - 0.5) * 0.02
        idx += 2  # conv, ReLU
        cin = v
    return sd


def lpips_alex_state_dict(seed=0):
    """Seeded stand-in for the weights lpips.LPIPS(net='alex') loads (neither torchvision's pretrained AlexNet nor the package's
    linear layers can be fetched offline): the five convolutions under torchvision's names `features.{0,3,6,8,10}.{weight,bias}`,
    He-normal with std = sqrt(2 / (C_in k^2)) and biases in +-0.01, and the 1x1 linear layers under lpips's names
    `lin{k}.model.1.weight` [1, C, 1, 1] as |randn| (the trained ones are non-negative)."""
    from .eval_utils import ALEXNET_CONVS
    gen = torch.Generator().manual_seed(seed)
    sd = {}
    for idx, cin, cout, k, _, _ in ALEXNET_CONVS:
        sd["features.%d.weight" % idx] = torch.randn(cout, cin, k, k, generator=gen) * math.sqrt(2.0 / (cin * k * k))
        sd["features.%d.bias" % idx] = (torch.rand(cout, generator=gen) - 0.5) * 0.02
    for layer, (_, _, cout, _, _, _) in enumerate(ALEXNET_CONVS):
        sd["lin%d.model.1.weight" % layer] = torch.randn(1, cout, 1, 1, generator=gen).abs()
    return sd


def syncnet_state_dict(seed=0):
    """Seeded stand-in for the weights of Wav2Lip's lip-sync expert (`lipsync_expert.pth` cannot be fetched offline), under the
    reference's keys for `SyncNet_color` (n3dt.syncnet.load_syncnet): every convolution with torch's default initialisation
    (kaiming_uniform_(a = sqrt(5)) weights and the matching uniform bias, i.e. both U(-1 / sqrt(fan_in), 1 / sqrt(fan_in))), and
    non-trivial batch-norm tensors: running_mean ~ N(0, 0.1), running_var ~ U(0.5, 1.5), weight ~ U(0.5, 1.5), bias ~ N(0, 0.1).
    With these the class keeps O(1) activations through all its blocks."""
    from .syncnet import BLOCKS, block_names
    gen = torch.Generator().manual_seed(seed)
    sd = {}
    for name, (cin, cout, (kh, kw), _, _, _) in zip(block_names(), BLOCKS):
        bound = 1.0 / math.sqrt(cin * kh * kw)
        sd[name + ".conv_block.0.weight"] = (torch.rand(cout, cin, kh, kw, generator=gen) * 2.0 - 1.0) * bound
        sd[name + ".conv_block.0.bias"] = (torch.rand(cout, generator=gen) * 2.0 - 1.0) * bound
        sd[name + ".conv_block.1.weight"] = torch.rand(cout, generator=gen) + 0.5
        sd[name + ".conv_block.1.bias"] = torch.randn(cout, generator=gen) * 0.1
        sd[name + ".conv_block.1.running_mean"] = torch.randn(cout, generator=gen) * 0.1
        sd[name + ".conv_block.1.running_var"] = torch.rand(cout, generator=gen) + 0.5
        sd[name + ".conv_block.1.num_batches_tracked"] = torch.tensor(0, dtype=torch.int64)
    return sd


WAV2LIP_HEAD_WEIGHT_SCALE = 16.0
WAV2LIP_HEAD_BIAS_SCALE = 2.0


def wav2lip_state_dict(seed=0):
    """Seeded stand-in for the weights of Wav2Lip's generator (`wav2lip.pth` cannot be fetched offline), under the reference's
    keys for `Wav2Lip` (n3dt.wav2lip.load_wav2lip), by syncnet_state_dict's rules: every convolution U(-1 / sqrt(fan_in),
    1 / sqrt(fan_in)) in weights and bias -- for a ConvTranspose2d weight [C_in, C_out, kh, kw] the fan-in is C_in kh kw with C_in
    on axis 0 -- and non-trivial batch-norm tensors.  With these the class keeps O(1) activations through all 51 blocks, but its
    logits stay within +-0.21: too flat to test a sigmoid.  The plain output convolution's weights are therefore scaled by
    WAV2LIP_HEAD_WEIGHT_SCALE and its bias by WAV2LIP_HEAD_BIAS_SCALE, chosen so that the image of the fixture's windows spans
    [0.2, 0.8] with at most 1 % of it outside (0.02, 0.98)."""
    from .wav2lip import BLOCKS, HEAD, block_names
    gen = torch.Generator().manual_seed(seed)
    sd = {}
    for b, (name, (tr, cin, cout, (kh, kw), _, _, _, _)) in enumerate(zip(block_names(), BLOCKS)):
        bound = 1.0 / math.sqrt(cin * kh * kw)
        shape = (cin, cout, kh, kw) if tr else (cout, cin, kh, kw)
        weight = (torch.rand(shape, generator=gen) * 2.0 - 1.0) * bound
        bias = (torch.rand(cout, generator=gen) * 2.0 - 1.0) * bound
        if b == HEAD:
            sd[name + ".weight"] = weight * WAV2LIP_HEAD_WEIGHT_SCALE
            sd[name + ".bias"] = bias * WAV2LIP_HEAD_BIAS_SCALE
            continue
        sd[name + ".conv_block.0.weight"] = weight
        sd[name + ".conv_block.0.bias"] = bias
        sd[name + ".conv_block.1.weight"] = torch.rand(cout, generator=gen) + 0.5
        sd[name + ".conv_block.1.bias"] = torch.randn(cout, generator=gen) * 0.1
        sd[name + ".conv_block.1.running_mean"] = torch.randn(cout, generator=gen) * 0.1
        sd[name + ".conv_block.1.running_var"] = torch.rand(cout, generator=gen) + 0.5
        sd[name + ".conv_block.1.num_batches_tracked"] = torch.tensor(0, dtype=torch.int64)
    return sd


S3FD_INPUT_SCALE = 1.0 / 64.0
S3FD_CONF_SCALE = 6.0
S3FD_LOC_SCALE = 2.0
S3FD_FACE_BIAS = (-6.988, -8.967, -3.788, -18.223, -4.062, 0.819)
S3FD_EMPTY_FACE_BIAS = (-60.0,) * 6


def s3fd_state_dict(seed=0, face_bias=S3FD_FACE_BIAS):
    """Seeded stand-in for the weights of the S3FD face detector (`s3fd-619a316812.pth` cannot be fetched offline), under the keys
    of the reference's `net_s3fd.s3fd` (n3dt.s3fd.load_s3fd).  He-scaled -- N(0, 2 / fan_in) weights, biases N(0.1, 0.05^2) -- so
    that 19 ReLU layers keep O(1) activations; conv1_1, which sees 255 u - mean, is scaled by S3FD_INPUT_SCALE on top.  L2Norm
    weights are the reference's scales (10, 8, 5) times U(0.75, 1.25).  The heads are N(0, 1 / fan_in) times S3FD_CONF_SCALE /
    S3FD_LOC_SCALE with N(0, 0.5^2) biases, and `face_bias[l]` is added to the bias of level l's face channel (the last conf
    channel): S3FD_FACE_BIAS leaves a few per cent of the head positions above the 0.5 score threshold on the fixture's frames,
    S3FD_EMPTY_FACE_BIAS none.  Never stored."""
    from .s3fd import CONVS, LEVEL_C, LEVEL_CONF, LEVEL_SOURCES, NORMS
    gen = torch.Generator().manual_seed(seed)
    sd = {}
    for i, (name, cin, cout, k, _, _, _, _) in enumerate(CONVS):
        std = math.sqrt(2.0 / (cin * k * k)) * (S3FD_INPUT_SCALE if i == 0 else 1.0)
        sd[name + ".weight"] = torch.randn(cout, cin, k, k, generator=gen) * std
        sd[name + ".bias"] = 0.1 + 0.05 * torch.randn(cout, generator=gen)
    for name, c, scale in zip(NORMS, LEVEL_C, (10.0, 8.0, 5.0)):
        sd[name + ".weight"] = scale * (0.75 + 0.5 * torch.rand(c, generator=gen))
    for src, c, conf, fb in zip(LEVEL_SOURCES, LEVEL_C, LEVEL_CONF, face_bias):
        std = math.sqrt(1.0 / (c * 9))
        sd[src + "_mbox_conf.weight"] = torch.randn(conf, c, 3, 3, generator=gen) * std * S3FD_CONF_SCALE
        bias = 0.5 * torch.randn(conf, generator=gen)
        bias[conf - 1] += fb
        sd[src + "_mbox_conf.bias"] = bias
        sd[src + "_mbox_loc.weight"] = torch.randn(4, c, 3, 3, generator=gen) * std * S3FD_LOC_SCALE
        sd[src + "_mbox_loc.bias"] = 0.5 * torch.randn(4, generator=gen)
    return sd


FACE_RECON_BN3_GAMMA = 0.5
FACE_RECON_HEAD_SCALE = 1.0


def face_recon_state_dict(seed=0):
    """Seeded stand-in for the weights of the 3-D face reconstruction net (the pretrained `net_recon` checkpoint cannot be fetched
    offline), under the keys of the reference's `ReconNetWrapper('resnet50', use_last_fc=False)` (n3dt.face_recon.load_face_recon).
    Convolutions are He-scaled, N(0, 2 / fan_in).  BatchNorm statistics are near the identity -- running_mean N(0, 0.1^2),
    running_var U(0.75, 1.25), beta N(0.1, 0.1^2), gamma U(0.75, 1.25) -- except that the last BatchNorm of a residual branch and a
    downsample branch's carry gamma times FACE_RECON_BN3_GAMMA and sqrt(1 - FACE_RECON_BN3_GAMMA^2): sixteen residual additions
    then neither blow the activations up nor let the branch die.  The seven final_layers, which the reference initialises to
    zero, are N(0, 1 / 2048) times FACE_RECON_HEAD_SCALE with N(0, 0.5^2) biases.  Never stored."""
    from .face_recon import CONVS, FEAT, HEAD_COLS
    gen = torch.Generator().manual_seed(seed)
    sd = {}
    for conv, bn, cin, cout, k, _, _, role, _ in CONVS:
        sd[conv + ".weight"] = torch.randn(cout, cin, k, k, generator=gen) * math.sqrt(2.0 / (cin * k * k))
        gamma = 0.75 + 0.5 * torch.rand(cout, generator=gen)
        if role == 3:
            gamma = gamma * FACE_RECON_BN3_GAMMA
        elif role == 4:
            gamma = gamma * math.sqrt(1.0 - FACE_RECON_BN3_GAMMA ** 2)
        sd[bn + ".weight"] = gamma
        sd[bn + ".bias"] = 0.1 + 0.1 * torch.randn(cout, generator=gen)
        sd[bn + ".running_mean"] = 0.1 * torch.randn(cout, generator=gen)
        sd[bn + ".running_var"] = 0.75 + 0.5 * torch.rand(cout, generator=gen)
        sd[bn + ".num_batches_tracked"] = torch.tensor(0, dtype=torch.int64)
    for i, cols in enumerate(HEAD_COLS):
        sd["final_layers.%d.weight" % i] = torch.randn(cols, FEAT, 1, 1, generator=gen) * (FACE_RECON_HEAD_SCALE / math.sqrt(FEAT))
        sd["final_layers.%d.bias" % i] = 0.5 * torch.randn(cols, generator=gen)
    return sd


FAN_BRANCH_SCALE = 0.35
FAN_HEAT_SCALE = 1.0
FAN_COORD_SCALE = 0.1
FAN_CALIBRATION_IMAGES = 2
FAN_BOUNDARY_MEAN = 0.95


def _fan_calibrate(sd, num_modules):
    """Walk the network in float64 over FAN_CALIBRATION_IMAGES seeded noise images and, in front of every BatchNorm, set its running
    statistics to those of its input, as training would have left them.  The statistics are quantised to float16 precision, so
    that a last-bit difference between two machines' float64 sums does not reach the weights."""
    import torch.nn.functional as F
    from .fan import HG_BLOCKS, coords
    gen = torch.Generator().manual_seed(977)
    x = torch.rand(FAN_CALIBRATION_IMAGES, 3, 256, 256, generator=gen).double()
    w = lambda k: sd[k].double()  # noqa: E731

    def bn(name, t, relu=True):
        sd[name + ".running_mean"] = t.mean(dim=(0, 2, 3)).to(torch.float16).float()
        sd[name + ".running_var"] = t.var(dim=(0, 2, 3), unbiased=False).clamp(1e-4, 6e4).to(torch.float16).float()
        g = w(name + ".weight") / torch.sqrt(w(name + ".running_var") + 1e-5)
        y = (t - w(name + ".running_mean")[None, :, None, None]) * g[None, :, None, None] + w(name + ".bias")[None, :, None, None]
        return torch.relu(y) if relu else y

    def cb(name, t):
        o1 = F.conv2d(bn(name + ".bn1", t), w(name + ".conv1.weight"), None, 1, 1)
        o2 = F.conv2d(bn(name + ".bn2", o1), w(name + ".conv2.weight"), None, 1, 1)
        o3 = F.conv2d(bn(name + ".bn3", o2), w(name + ".conv3.weight"), None, 1, 1)
        res = t
        if name + ".downsample.2.weight" in sd:
            res = F.conv2d(bn(name + ".downsample.0", t), w(name + ".downsample.2.weight"))
        return torch.cat((o1, o2, o3), 1) + res

    def hourglass(s, level, t):
        up1 = cb("m%d.b1_%d" % (s, level), t)
        low = cb("m%d.b2_%d" % (s, level), F.avg_pool2d(t, 2, 2))
        low = hourglass(s, level - 1, low) if level > 1 else cb("m%d.b2_plus_1" % s, low)
        low = cb("m%d.b3_%d" % (s, level), low)
        return up1 + F.interpolate(low, scale_factor=2, mode="nearest")

    assert len(HG_BLOCKS) == 13
    n = x.shape[0]
    c256, c64 = coords(256).double()[None].expand(n, -1, -1, -1), coords(64).double()[None].expand(n, -1, -1, -1)
    y = bn("bn1", F.conv2d(torch.cat((x, c256), 1), w("conv1.conv.weight"), w("conv1.conv.bias"), 2, 3))
    previous = cb("conv4", cb("conv3", F.avg_pool2d(cb("conv2", y), 2, 2)))
    tmp = None
    for s in range(num_modules):
        t = torch.cat((previous, c64), 1)
        if s > 0:
            gate = (torch.clamp(tmp[:, -1:].float(), 0.0, 1.0) > 0.05).double()
            t = torch.cat((t, gate * c64[:, :2]), 1)
        t = F.conv2d(t, w("m%d.coordconv.conv.weight" % s), w("m%d.coordconv.conv.bias" % s))
        ll = cb("top_m_%d" % s, hourglass(s, 4, t))
        ll = bn("bn_end%d" % s, F.conv2d(ll, w("conv_last%d.weight" % s), w("conv_last%d.bias" % s)))
        tmp = F.conv2d(ll, w("l%d.weight" % s), w("l%d.bias" % s))
        # the boundary channel's bias: its mean FAN_BOUNDARY_MEAN standard deviations above the gate, so that both sides of the gate
        # are populated and few cells lie right on it
        shift = (0.05 + FAN_BOUNDARY_MEAN * tmp[:, -1].std() - tmp[:, -1].mean()).to(torch.float16).float()
        sd["l%d.bias" % s][-1] += shift
        tmp[:, -1] += shift.double()
        if s < num_modules - 1:
            previous = previous + F.conv2d(ll, w("bl%d.weight" % s), w("bl%d.bias" % s)) + F.conv2d(tmp, w("al%d.weight" % s), w("al%d.bias" % s))


def fan_state_dict(seed=0, num_modules=4, num_landmarks=98):
    """Seeded stand-in for the weights of the AWing FAN landmark detector (the pretrained alignment_WFLW_4HG.pth cannot be fetched
    offline), under the keys of the reference's `FAN(num_modules, num_landmarks=...)` (n3dt.fan.load_fan).  Default initialisation
    is useless here: its heat maps are smooth and peak on the border, because every ReLU leaves a positive mean that the zero
    padding removes along the border only.  Here
    * every convolution's weights are centred over their input channels per (output, tap) -- with like channels the means cancel
      tap by tap, on the border too; the stem's image kernels sum to zero, its and the hourglass CoordConvs' coordinate channels
      carry FAN_COORD_SCALE of the weight of a feature channel;
    * a ConvBlock's convolutions are N(0, 2 / fan_in) times FAN_BRANCH_SCALE, so that a block adds about half its input's
      magnitude to the residual and 59 of them neither blow the activations up nor leave a branch dead; l is N(0, 1 / 256) times
      FAN_HEAT_SCALE;
    * gamma is U(0.9, 1.1), beta N(0.1, 0.05^2), and every BatchNorm's running statistics are those of its input over
      FAN_CALIBRATION_IMAGES seeded noise images (_fan_calibrate), as training leaves them: the channels in front of every ReLU are
      alike, the heat maps noise-like with peaks all over the map; the boundary channel's bias puts its mean FAN_BOUNDARY_MEAN
      standard deviations above the 0.05 gate: both sides of the gate are populated, and few cells lie on it.
    Takes a few seconds (one float64 forward).  Never stored."""
    from .fan import state_dict_keys
    gen = torch.Generator().manual_seed(seed)
    sd = {}
    for key, shape in state_dict_keys(num_modules, num_landmarks).items():
        name, part = key.rsplit(".", 1)
        leaf = name.rsplit(".", 1)[-1]
        if part == "num_batches_tracked":
            sd[key] = torch.tensor(0, dtype=torch.int64)
        elif len(shape) == 4:
            cout, cin, k, _ = shape
            w = torch.randn(shape, generator=gen)
            feat = 3 if name == "conv1.conv" else 256 if "coordconv" in name else cin  # the channels in front of the coordinates'
            if k == 3:
                scale = FAN_BRANCH_SCALE * math.sqrt(2.0 / (cin * 9))
            elif name == "conv1.conv":
                scale = math.sqrt(2.0 / (3 * 49))
            elif name[0] == "l" and name[1:].isdigit():
                scale = FAN_HEAT_SCALE * math.sqrt(1.0 / cin)
            elif name[:2] in ("al", "bl"):
                scale = 0.25 * math.sqrt(1.0 / cin)
            else:  # downsample.2, conv_last, coordconv
                scale = math.sqrt(1.0 / feat)
            w[:, feat:] *= FAN_COORD_SCALE
            if name == "conv1.conv":
                w[:, :3] -= w[:, :3].mean(dim=(1, 2, 3), keepdim=True)
            else:
                w[:, :feat] -= w[:, :feat].mean(dim=1, keepdim=True)
            sd[key] = w * scale
        elif part == "weight":  # a BatchNorm's gamma
            sd[key] = 0.9 + 0.2 * torch.rand(shape, generator=gen)
        elif part == "bias" and (leaf.startswith("bn") or leaf == "0"):
            sd[key] = 0.1 + 0.05 * torch.randn(shape, generator=gen)
        elif part == "bias":
            sd[key] = 0.05 * torch.randn(shape, generator=gen)
        elif part == "running_mean":
            sd[key] = torch.zeros(shape)
        else:
            sd[key] = torch.ones(shape)
    _fan_calibrate(sd, num_modules)
    return sd


HEAD_MASK_BN2_GAMMA = 0.5
HEAD_MASK_HEAD_SCALE = 8.0
HEAD_MASK_CALIBRATION_IMAGES = 2


def _head_mask_mids(sd, x):
    """the inputs of the three heads' last 1 x 1 convolutions, float64, for x [n,3,H,W]"""
    import torch.nn.functional as F
    w = lambda k: sd[k].double()  # noqa: E731

    def bn(name, t):
        g = w(name + ".weight") / torch.sqrt(w(name + ".running_var") + 1e-5)
        return (t - w(name + ".running_mean")[None, :, None, None]) * g[None, :, None, None] + w(name + ".bias")[None, :, None, None]

    def cbr(name, t, pad=1):
        return torch.relu(bn(name + ".bn", F.conv2d(t, w(name + ".conv.weight"), None, 1, pad)))

    def arm(name, t):
        f = cbr(name + ".conv", t)
        return f * torch.sigmoid(bn(name + ".bn_atten", F.conv2d(f.mean((2, 3), keepdim=True), w(name + ".conv_atten.weight"))))

    r = "cp.resnet."
    t = F.max_pool2d(torch.relu(bn(r + "bn1", F.conv2d(x, w(r + "conv1.weight"), None, 2, 3))), 3, 2, 1)
    feats = []
    for layer in range(1, 5):
        for b in range(2):
            p = "%slayer%d.%d." % (r, layer, b)
            s = 2 if (layer > 1 and b == 0) else 1
            y = torch.relu(bn(p + "bn1", F.conv2d(t, w(p + "conv1.weight"), None, s, 1)))
            y = bn(p + "bn2", F.conv2d(y, w(p + "conv2.weight"), None, 1, 1))
            sc = bn(p + "downsample.1", F.conv2d(t, w(p + "downsample.0.weight"), None, s, 0)) if p + "downsample.0.weight" in sd else t
            t = torch.relu(sc + y)
        feats.append(t)
    _, f8, f16, f32 = feats
    s32 = arm("cp.arm32", f32) + cbr("cp.conv_avg", f32.mean((2, 3), keepdim=True), 0)
    cp16 = cbr("cp.conv_head32", F.interpolate(s32, f16.shape[2:], mode="nearest"))
    cp8 = cbr("cp.conv_head16", F.interpolate(arm("cp.arm16", f16) + cp16, f8.shape[2:], mode="nearest"))
    f = cbr("ffm.convblk", torch.cat([f8, cp8], 1), 0)
    a = torch.sigmoid(F.conv2d(torch.relu(F.conv2d(f.mean((2, 3), keepdim=True), w("ffm.conv1.weight"))), w("ffm.conv2.weight")))
    return cbr("conv_out.conv", f * a + f), cbr("conv_out16.conv", cp8), cbr("conv_out32.conv", cp16)


def head_mask_state_dict(seed=0, n_classes=19):
    """Seeded stand-in for the weights of the face parser (faceparsing_model.pth cannot be fetched offline), under the keys of the
    reference's `BiSeNet(n_classes)` (n3dt.head_mask.load_head_mask).  Convolutions are He-scaled; BatchNorm statistics are near the
    identity as in face_recon_state_dict, a residual branch's last BatchNorm and a downsample branch's carry gamma times
    HEAD_MASK_BN2_GAMMA and sqrt(1 - HEAD_MASK_BN2_GAMMA^2).  The heads have no bias, and the features in front of them are
    positive: as drawn, one class would win everywhere.  So each head's last 1 x 1 convolution, N(0, HEAD_MASK_HEAD_SCALE^2 /
    C_in), is made orthogonal to the mean of its input over HEAD_MASK_CALIBRATION_IMAGES seeded noise images (float64; the
    direction is quantised to float16 so that a last-bit difference between two machines' sums does not reach the weights): the
    logits are then centred and every class wins somewhere.  Never stored."""
    from .head_mask import CONVS, SKIP_BLOCKS
    gen = torch.Generator().manual_seed(seed)
    sd = {}
    for j, (conv, bn, cin, cout, k, _, _, _, _) in enumerate(CONVS):
        cout = cout or n_classes
        scale = math.sqrt(2.0 / (cin * k * k)) if bn is not None else (HEAD_MASK_HEAD_SCALE if conv.endswith("conv_out") else 1.0) / math.sqrt(cin)
        sd[conv + ".weight"] = torch.randn(cout, cin, k, k, generator=gen) * scale
        if bn is None:
            continue
        gamma = 0.75 + 0.5 * torch.rand(cout, generator=gen)
        if j in SKIP_BLOCKS:
            gamma = gamma * HEAD_MASK_BN2_GAMMA
        elif "downsample" in conv:
            gamma = gamma * math.sqrt(1.0 - HEAD_MASK_BN2_GAMMA ** 2)
        sd[bn + ".weight"] = gamma
        sd[bn + ".bias"] = 0.1 + 0.1 * torch.randn(cout, generator=gen)
        sd[bn + ".running_mean"] = 0.1 * torch.randn(cout, generator=gen)
        sd[bn + ".running_var"] = 0.75 + 0.5 * torch.rand(cout, generator=gen)
        sd[bn + ".num_batches_tracked"] = torch.tensor(0, dtype=torch.int64)
    x = torch.rand(HEAD_MASK_CALIBRATION_IMAGES, 3, 128, 128, generator=torch.Generator().manual_seed(991)).double()
    x = (x - torch.tensor([0.485, 0.456, 0.406]).double()[None, :, None, None]) / torch.tensor([0.229, 0.224, 0.225]).double()[None, :, None, None]
    with torch.no_grad():
        mids = _head_mask_mids(sd, x)
    for head, mid in zip(("conv_out", "conv_out16", "conv_out32"), mids):
        mu = mid.mean((0, 2, 3))
        u = (mu / mu.norm()).to(torch.float16).double()
        wgt = sd[head + ".conv_out.weight"].double().flatten(1)
        wgt = wgt - (wgt @ u)[:, None] * u[None, :] / (u @ u)
        sd[head + ".conv_out.weight"] = wgt.float().reshape(n_classes, -1, 1, 1).contiguous()
    return sd


def face_recon_lm3d():
    """A stand-in for the [5,3] standard landmarks the reference's load_lm3d reads from its BFM folder (left eye, right eye, nose,
    left and right mouth corner; float64): a plausible face for smoke runs and timing, NOT the reference's values -- those the
    caller supplies."""
    return torch.tensor([[-0.31, 0.29, 0.03], [0.31, 0.29, 0.03], [0.0, 0.03, 0.45], [-0.25, -0.33, 0.12], [0.25, -0.33, 0.12]],
                        dtype=torch.float64).numpy()


def mel_batch(B, seed=0):
    """Seeded stand-in for the mel windows the reference's data loader hands Audio2style: [B, 80, 16] float32 in [-4, 4) (the
    range of Wav2Lip's normalised log-mel), quantised to 1/32 so that the values are exact in every precision."""
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (B, 80, 16), generator=gen, dtype=torch.uint8).float() / 32.0 - 4.0
