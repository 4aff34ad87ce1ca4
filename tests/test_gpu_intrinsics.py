"""Gradients to the other two inputs of ray generation, batch_inv_inmats and batch_xy, on the GPU: against
the reference's float64 autograd (tests/golden/intrinsics.*), as directional derivatives, fused bf16 against exact fp32, the
autograd plumbing around them, and single-image fitting of a focal length through them.

With c = Kinv [x, y, 1] and gc = R^T dL/d(R c) per ray, the camera backward kernels add d Kinv = sum over rays of gc [x, y, 1]^T
and d (x, y) = the first two columns of Kinv against gc to the d R, d T they already formed."""
import numpy as np
import pytest
import torch

from conftest import load_golden, synthetic_case

pytestmark = pytest.mark.gpu

CAM = ("batch_inv_inmats", "batch_xy", "batch_Rmats", "batch_Tvecs")


def dev():
    return torch.device("cuda:0")


def to_dev(inp):
    return {k: (v.to(dev()) if torch.is_tensor(v) else v) for k, v in inp.items()}


def build_net(opt, sd, include_vd=False, hier=False, precision="fp32", frozen=False):
    from n3dt import HeadNeRFNet
    net = HeadNeRFNet(opt, include_vd=include_vd, hier_sampling=hier, train_precision=precision).to(dev())
    net.load_state_dict(sd, strict=True)
    if frozen:
        for p in net.parameters():
            p.requires_grad_(False)
    return net


def total_loss(net, mode, d, B, size, t_rand=None, fine=False):
    from n3dt.train import data_losses, disk_mask
    out = net(mode, d["batch_xy"], d["batch_uv"], d["audiostyle"], bg_code=None, shape_code=d["shape_code"], appea_code=d["appea_code"],
              batch_Rmats=d["batch_Rmats"], batch_Tvecs=d["batch_Tvecs"], batch_inv_inmats=d["batch_inv_inmats"], t_rand=t_rand)
    mask = disk_mask(B, size).to(dev())
    total = 0.0
    for k in ("coarse_dict", "fine_dict") if fine else ("coarse_dict",):
        t = data_losses(out[k], torch.full_like(out[k]["merge_img"], 0.5), mask)
        total = total + t["bg_loss"] + t["head_loss"] + t["nonhead_loss"]
    return total


def with_grad(d, names):
    d = dict(d)
    for k in names:
        d[k] = d[k].clone().requires_grad_(True)
    return d


def directional_check(loss_of, d, names, seed, h=1e-6):
    """d[names] carry .grad of loss_of(d): (analytic, numeric) derivative along one random direction.
    The direction is N(0, 1) times the tensor's mean magnitude, as the renderer's finite-difference tests scale theirs: the same
    relative step for Kinv (entries ~ 0.04 .. 1) and xy (pixels, ~ 6).  An unscaled N(0, 1) step of 1e-6 in Kinv moves the
    far sample points by 1e-6 * 12 px * 12 units, 0.07 rad of the encoder's 2^9 frequency: the central difference is then 3 %
    of the gradient's scale off (measured at fs 8, 12, 16), more than the whole derivative where the direction cancels.
    The difference is taken over the step that float32 really makes (x + h u rounds: at |xy| ~ 8 a step of 6e-6 is 12 ulps)."""
    gen = torch.Generator().manual_seed(seed)
    base = {k: d[k].detach().clone() for k in names}
    dirs = {k: torch.randn(base[k].shape, generator=gen).to(dev()) * base[k].abs().mean() for k in names}
    analytic, vals = 0.0, []
    plus = {k: base[k] + h * dirs[k] for k in names}
    minus = {k: base[k] - h * dirs[k] for k in names}
    for k in names:
        assert torch.isfinite(d[k].grad).all(), k
        analytic += float((d[k].grad.double() * (plus[k].double() - minus[k].double()) / (2 * h)).sum())
    with torch.no_grad():
        for pert in (plus, minus):
            dd = dict(d)
            dd.update(pert)
            vals.append(float(loss_of(dd).double()))
    return analytic, (vals[0] - vals[1]) / (2 * h)


@pytest.mark.parametrize("name", ["tiny_test", "tiny_train", "vd_train"])
def test_intrinsics_and_ray_gradients_match_reference_autograd(name):
    """Exact fp32 path against the reference's float64 autograd: d Kinv and d xy within the bound
    test_gradients_match_reference_autograd applies to camera tensors (5e-2 of max|ref|), and in the same call d R and d T
    still within that test's bound against that test's fixture."""
    from n3dt import synthetic as syn
    ref, _ = load_golden("intrinsics")
    g0, m = load_golden(name)
    opt, sd, inp = synthetic_case(m)
    net = build_net(opt, sd, include_vd=bool(m.get("include_vd", False)))
    B = m["batch"]
    t_rand = syn.stratified_noise(B, opt.featmap_size ** 2, opt.num_sample_coarse, m["t_rand_seed"]).to(dev()) if m["mode"] == "train" else None
    d = with_grad(to_dev(inp), CAM)
    total_loss(net, m["mode"], d, B, opt.pred_img_size, t_rand).backward()
    for k in CAM:
        assert d[k].grad is not None, k
        want = ref["%s.grad_in.%s" % (name, k)] if k in CAM[:2] else g0["grad_in." + k]
        got = d[k].grad.cpu().numpy()
        assert got.shape == want.shape, k
        err = np.abs(got - want).max() / np.abs(want).max()
        print("%s %s: max|diff| / max|ref| = %.3e" % (name, k, err))
        assert err <= 5e-2, (k, err)


def test_intrinsics_and_ray_gradient_is_the_directional_derivative():
    """Frozen network, "test" mode, fs 12 -> 144 rays (not a multiple of any rays-per-workgroup choice of the camera kernels:
    their tail runs), 16 samples: d loss / d(Kinv, xy) along a random direction against a central finite difference, with the
    step and tolerance of test_camera_gradient_is_the_directional_derivative."""
    from n3dt import BaseOptions, synthetic as syn
    opt = BaseOptions({"featmap_size": 12, "featmap_nc": 256, "pred_img_size": 48, "num_sample_coarse": 16})
    net = build_net(opt, syn.make_state_dict(opt, seed=3, bg_noise=0.1), frozen=True)
    B = 2
    d = with_grad(to_dev(syn.frame_inputs(opt, B)), CAM[:2])
    loss_of = lambda dd: total_loss(net, "test", dd, B, opt.pred_img_size)  # noqa: E731
    loss_of(d).backward()
    analytic, numeric = directional_check(loss_of, d, CAM[:2], seed=5)
    print("directional derivative: analytic %.5e numeric %.5e" % (analytic, numeric))
    assert abs(numeric - analytic) <= 0.15 * abs(analytic) + 2e-2, (numeric, analytic)


def _grads(opt, sd, B, precision, t_rand):
    net = build_net(opt, sd, precision=precision)
    net.neural_render.train_precision = "fp32"  # isolate the volumetric stage
    from n3dt import synthetic as syn
    d = with_grad(to_dev(syn.frame_inputs(opt, B)), CAM)
    total_loss(net, "train", d, B, opt.pred_img_size, t_rand).backward()
    return {k: d[k].grad.detach().clone() for k in CAM}


def bf16_band():
    """(geometry, tensor) -> (max|fp32 - bf16| / max|fp32|, cosine) of the camera gradients, fused bf16 against exact fp32."""
    from n3dt import BaseOptions, synthetic as syn
    out = {}
    for fs, ns, B in ((8, 8, 2), (16, 64, 2)):
        opt = BaseOptions({"featmap_size": fs, "featmap_nc": 256, "pred_img_size": fs * 4, "num_sample_coarse": ns})
        sd = syn.make_state_dict(opt, seed=0, bg_noise=0.1)
        t_rand = syn.stratified_noise(B, fs * fs, ns, 7).to(dev())
        g32, g16 = _grads(opt, sd, B, "fp32", t_rand), _grads(opt, sd, B, "bf16", t_rand)
        for k in CAM:
            a, b = g32[k].double().flatten(), g16[k].double().flatten()
            out[((fs, ns, B), k)] = (float((a - b).abs().max() / a.abs().max()), float((a * b).sum() / (a.norm() * b.norm() + 1e-30)))
    return out


def test_fused_bf16_intrinsics_and_ray_gradients_against_the_fp32_path():
    """d Kinv and d xy of the fused bf16 path against the exact path at (fs, N_s, B) = (8, 8, 2) and (16, 64, 2) (two 32-sample
    blocks per ray), under the bounds test_fused_bf16_camera_gradients_against_the_fp32_path applies to batch_Rmats: they are
    the same per-ray gw that d R sums, through R^T instead of against c."""
    for (geo, k), (err, cos) in bf16_band().items():
        print("bf16 vs fp32 %s %s: max|diff| / max|fp32| = %.4f cosine = %.5f" % (geo, k, err, cos))
        if k in CAM[:2]:
            assert err <= 0.35 and cos >= 0.98, (geo, k, err, cos)


def _tiny_train():
    from n3dt import synthetic as syn
    _, m = load_golden("tiny_train")
    opt, sd, inp = synthetic_case(m)
    t_rand = syn.stratified_noise(m["batch"], opt.featmap_size ** 2, opt.num_sample_coarse, m["t_rand_seed"]).to(dev())
    return m["batch"], opt, sd, to_dev(inp), t_rand


def test_broadcast_ray_grid_receives_the_sum_over_frames():
    """batch_xy handed over as base.expand(B, -1, -1) (stride 0 over the frames): autograd reduces the kernel's [B, 2, N_r] onto
    the base tensor.  Same kernels as with a dense batch_xy, so only the order of the last sum differs: 1e-6 relative."""
    B, opt, sd, inp, t_rand = _tiny_train()
    net = build_net(opt, sd)
    assert float((inp["batch_xy"] - inp["batch_xy"][:1]).abs().max()) == 0.0  # the frames do share one grid
    dense = with_grad(inp, ["batch_xy"])
    total_loss(net, "train", dense, B, opt.pred_img_size, t_rand).backward()
    base = inp["batch_xy"][:1].clone().requires_grad_(True)
    shared = dict(inp)
    shared["batch_xy"] = base.expand(B, -1, -1)
    assert shared["batch_xy"].stride(0) == 0
    total_loss(net, "train", shared, B, opt.pred_img_size, t_rand).backward()
    want = dense["batch_xy"].grad.sum(0, keepdim=True)
    assert base.grad.shape == want.shape and float(want.abs().max()) > 0
    assert float((base.grad - want).abs().max()) <= 1e-6 * float(want.abs().max())


def test_intrinsics_alone_receive_a_gradient():
    """Only batch_inv_inmats requires grad; R, T, the codes and the network are frozen."""
    B, opt, sd, inp, t_rand = _tiny_train()
    net = build_net(opt, sd, frozen=True)
    d = with_grad(inp, ["batch_inv_inmats"])
    total_loss(net, "train", d, B, opt.pred_img_size, t_rand).backward()
    g = d["batch_inv_inmats"].grad
    assert g is not None and g.shape == (B, 3, 3) and torch.isfinite(g).all() and float(g.abs().min()) > 0
    assert all(d[k].grad is None for k in ("batch_xy", "batch_Rmats", "batch_Tvecs", "shape_code"))


def test_intrinsics_and_ray_gradients_through_the_hierarchical_pass():
    """hier_sampling=True at the hier_train geometry (fs 8, 16 + 24 samples, B = 2): finite gradients for both tensors in both
    precisions, and the fp32 result is the directional derivative of the loss on both images.  The fine planes come from the
    DETACHED coarse weights (NetWorks/utils.py:219): constants of the backward, so the finite difference holds them at their
    values of the unperturbed point."""
    _, m = load_golden("hier_train")
    opt, sd, inp = synthetic_case(m)
    B = m["batch"]
    inp = to_dev(inp)
    for precision in ("bf16", "fp32"):
        net = build_net(opt, sd, hier=True, precision=precision, frozen=True)
        d = with_grad(inp, CAM[:2])
        planes, orig = [], net.fine_planes

        def record(*a, **kw):
            planes.append(orig(*a, **kw))
            return planes[-1]
        net.fine_planes = record
        loss_of = lambda dd: total_loss(net, "test", dd, B, opt.pred_img_size, fine=True)  # noqa: E731
        loss_of(d).backward()
        for k in CAM[:2]:
            assert d[k].grad is not None and torch.isfinite(d[k].grad).all() and float(d[k].grad.abs().max()) > 0, (precision, k)
    net.fine_planes = lambda *a, **kw: planes[-1]  # (net, d, loss_of: the fp32 pass; the forward without grad asks for them too)
    analytic, numeric = directional_check(loss_of, d, CAM[:2], seed=6)
    print("hierarchical directional derivative: analytic %.5e numeric %.5e" % (analytic, numeric))
    assert abs(numeric - analytic) <= 0.15 * abs(analytic) + 2e-2, (numeric, analytic)


def test_render_bwd_cam_without_the_new_outputs_equals_render_bwd():
    """Neither new gradient asked for: d R, d T and an MLP weight gradient from n3dt_render_bwd_cam are bit for bit what
    n3dt_render_bwd returns on the same saved buffers (that entry point is now a call to the new one with both NULL).
    Four rays per frame: ONE workgroup of the camera kernels per frame, so its atomics meet zeroed memory in a fixed order.
    (With the 64 rays of the tiny cases 16 workgroups add to each address, and two calls of n3dt_render_bwd itself differ
    in the last bit: 1e-7 relative, measured.)  1024 / 64 points stay under the split of the weight-gradient sums."""
    from n3dt import _lib, ops
    B, opt, sd, inp, t_rand = _tiny_train()
    net = build_net(opt, sd)
    rays = torch.tensor([0, 21, 42, 63], device=dev())
    for precision in ("fp32", "bf16"):
        prec = _lib.PRECISIONS[precision]
        xy = inp["batch_xy"][:, :, rays].contiguous()
        tr = t_rand[:, rays].contiguous()
        geom = net._geom(B, len(rays), xy)
        params, ws, bs = net._mlp_params()
        packed = net._packed(geom, prec, params, ws, bs)
        R, T, Kinv = ops._f32c(inp["batch_Rmats"]), ops._f32c(inp["batch_Tvecs"]).view(B, 3), ops._f32c(inp["batch_inv_inmats"])
        shape, appea, audio = ops._f32c(inp["shape_code"]), ops._f32c(inp["appea_code"]), ops._f32c(inp["audiostyle"])
        bg = net.neural_render.bg_featmap.detach().reshape(opt.featmap_nc, -1)[:, rays].contiguous()
        out, saved = ops.render_train_fwd(geom, packed, params, xy, R, T, Kinv, shape, appea, audio, tr, bg, prec)
        d_merge = torch.randn(out["merge_feat"].shape, generator=torch.Generator().manual_seed(9)).to(dev())
        res = []
        for cam_grads in (None, ("R", "T")):
            gws, gbs = [torch.zeros_like(w) for w in ws], [torch.zeros_like(b) for b in bs]
            r = ops.render_bwd(geom, params, ops.mlp_params(gws, gbs), shape, appea, audio, bg, d_merge, saved,
                               cam=(xy, R, T, Kinv, tr), precision=prec, cam_grads=cam_grads)
            # (the weight gradients of the exact path only: a sum that is not split; the code gradients' column sums and the
            # fused path's weight gradients leave through atomics of many workgroups and differ between any two calls)
            res.append((r[4], r[5]) + ((gws[3], gws[0]) if precision == "fp32" else ()))
            if cam_grads is not None:
                assert len(r) == 8 and r[6] is None and r[7] is None
        torch.cuda.synchronize()
        for a, b in zip(*res):
            assert float(a.abs().max()) > 0 and torch.equal(a, b), precision
        # asking for the new outputs leaves the old ones where they were (same sums, same order)
        r = ops.render_bwd(geom, params, None, shape, appea, audio, bg, d_merge, saved, cam=(xy, R, T, Kinv, tr), precision=prec,
                           frozen=True, cam_grads=("R", "T", "Kinv", "xy"))
        assert torch.equal(r[4], res[0][0]) and torch.equal(r[5], res[0][1]), precision
        assert r[6].shape == (B, 3, 3) and r[7].shape == (B, 2, len(rays)) and torch.isfinite(r[6]).all() and torch.isfinite(r[7]).all()


def test_fitting_recovers_a_focal_length():
    """Single-image fitting with the intrinsics among the variables (fs 16 -> 64^2, 32 samples, one frame, exact path, frozen
    network): the target is this network's own render at focal 1.05 f0; FittingState(opt_intrinsics=True, opt_cam=False)
    starts from f0 with the loop of n3dt.fitting.  After 40 iterations the loss is below its first value and f is nearer
    1.05 f0 than f0 was -- two orderings, no rate.  Only the intrinsics group is stepped (Adam at the rate make_optimizer gives
    it): the codes are the target's own, and 306 free code offsets at 15 times that rate absorb a focal change of this
    network before the focal length moves (measured with every group stepping: the loss rose 25-fold within 8 iterations and f
    went to 0.997 f0), which is a property of fitting a random network, not of the gradient under test.

    The scene must make that a well-posed fit.  With the plain seeded weights it is not: the encoder's 2^9 frequency turns a
    1 % change of focal length into an unrelated image, and on the CPU restatement of the forward (oracle/) the loss against
    the target is flat noise between f0 and 1.05 f0 (9.7e-6, 2.1e-5, 1.2e-5, 9.9e-6 at steps of 1.25 %).  So the two layers
    that read the encoding get its 2^k columns scaled by 4^-k, a field as smooth as a trained one, and the test first checks
    on the CPU restatement that the loss then falls from f0 over 1.025 f0 to its zero at 1.05 f0 (a bowl: 1.2e-6, 3.0e-7, 0)."""
    from n3dt import BaseOptions, synthetic as syn, fitting
    from oracle import oracle as orc
    opt = BaseOptions({"featmap_size": 16, "featmap_nc": 256, "pred_img_size": 64, "num_sample_coarse": 32})
    sd = syn.make_state_dict(opt, seed=0, bg_noise=0.1)
    for name in ("fg_CD_predictor.FeaExt_module_0.weight", "fg_CD_predictor.FeaExt_module_5.weight"):
        for k in range(10):  # columns [p, sin(2^0 p), cos(2^0 p), sin(2^1 p), ...] lead both layers' inputs (NetWorks/models.py:69-76)
            sd[name][:, 3 + 6 * k:9 + 6 * k] *= 4.0 ** -k
    inp = syn.frame_inputs(opt, 1, yaw_range=0.0)
    K0 = inp["batch_inv_inmats"]
    f0 = 1.0 / float(K0[0, 0, 0])

    def K_at(scale):  # focal f0 * scale, same principal point
        K = K0.clone()
        K[:, 0, 0] /= scale
        K[:, 1, 1] /= scale
        K[:, :2, 2] /= scale
        return K

    def cpu_img(scale):
        return torch.from_numpy(orc.forward(sd, opt, dict(inp, batch_inv_inmats=K_at(scale)))["merge_img"])
    gt_cpu = cpu_img(1.05)
    shape = [float(((cpu_img(s) - gt_cpu) ** 2).mean()) for s in (1.0, 1.025)]
    print("CPU restatement, image MSE against the 1.05 f0 target at f0, 1.025 f0: %.3e %.3e" % tuple(shape))
    assert shape[0] > 2.0 * shape[1] > 0.0

    net = build_net(opt, sd, frozen=True)
    d = to_dev(inp)
    cam0 = {k: d[k] for k in ("batch_Rmats", "batch_Tvecs", "batch_inv_inmats")}
    with torch.no_grad():
        gt = net("test", d["batch_xy"], d["batch_uv"], d["audiostyle"], None, d["shape_code"], d["appea_code"], cam0["batch_Rmats"],
                 cam0["batch_Tvecs"], K_at(1.05).to(dev()))["coarse_dict"]["merge_img"].detach().clone()
    st = fitting.FittingState(d["shape_code"], d["appea_code"], cam0, opt_cam=False, opt_intrinsics=True)
    rate = st.make_optimizer()[0].param_groups[-1]["lr"]
    optim = torch.optim.Adam([st.delta_logf, st.delta_center], lr=rate, betas=(0.9, 0.999))
    sched = torch.optim.lr_scheduler.LambdaLR(optim, lr_lambda=lambda epoch: 0.1 ** (epoch / 300))
    image_mse = lambda pred, gt_, mask_: {"total_loss": ((pred["merge_img"] - gt_) ** 2).mean()}  # noqa: E731
    losses, focals = [], []
    for _ in range(40):
        _, _, total = fitting.fit_step(net, st, optim, sched, d["batch_xy"], d["batch_uv"], d["audiostyle"], gt, None, image_mse)
        losses.append(float(total))
        focals.append(float(st.focal().detach()[0]) / f0)
    print("fitting the focal length: loss", ["%.3e" % v for v in losses[::8] + losses[-1:]], "f / f0", ["%.4f" % v for v in focals[::8] + focals[-1:]])
    assert torch.isfinite(st.delta_logf.grad).all() and torch.isfinite(st.delta_center.grad).all()
    assert losses[-1] < losses[0]
    assert abs(focals[-1] - 1.05) < 0.05
