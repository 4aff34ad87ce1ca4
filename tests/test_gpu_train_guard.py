"""The guarded FlatAdam step through train.train_step at the smallest renderer (featmap 8, 16 samples, 64 x 64 image, B = 1), both
training precisions: make_flat_optimizer(net, max_grad_norm=..., skip_nonfinite=True).

A clean step: opt.grad_norm is the 2-norm of the very gradients backward left in p.grad (the step does not rewrite them), taken by
torch.linalg.vector_norm over float64 copies, within 2^-23 relative (double accumulation; the sqrt and one rounding to fp32 are
all that is inexact); the parameters move.  A step whose gt_rgb holds one NaN (the loss tail's nan_to_num covers merge_img, not
the target): every parameter bit-identical afterwards, skipped_steps == 1, the next forward("test") reproduces the pre-step image
bit for bit (version bumps and invalidate_packed() still ran: the re-packed caches hold the same weights), and a following clean
step trains again."""
import pytest
import torch

pytestmark = pytest.mark.gpu

IMG = 64


def dev():
    return torch.device("cuda:0")


def _setup(precision):
    from n3dt import BaseOptions, HeadNeRFNet, synthetic as syn
    from n3dt.train import disk_mask
    opt = BaseOptions({"featmap_size": 8, "featmap_nc": 256, "pred_img_size": IMG, "num_sample_coarse": 16})
    net = HeadNeRFNet(opt, False, False, train_precision=precision).to(dev())
    net.load_state_dict(syn.make_state_dict(opt, seed=0, bg_noise=0.1), strict=True)
    d = {k: (v.to(dev()) if torch.is_tensor(v) else v) for k, v in syn.frame_inputs(opt, 1).items()}
    gt = torch.full((1, 3, IMG, IMG), 0.5, device=dev())
    mask = disk_mask(1, IMG).to(dev())
    t_rand = syn.stratified_noise(1, 64, 16, seed=3).to(dev())
    return net, d, gt, mask, t_rand


def _render(net, d):
    with torch.no_grad():
        out = net("test", d["batch_xy"], d["batch_uv"], d["audiostyle"], bg_code=None, shape_code=d["shape_code"],
                  appea_code=d["appea_code"], batch_Rmats=d["batch_Rmats"], batch_Tvecs=d["batch_Tvecs"],
                  batch_inv_inmats=d["batch_inv_inmats"])
    return out["coarse_dict"]["merge_img"].clone()


def _bits(params):
    return [p.detach().clone().view(torch.int32) for p in params]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_clean_step_trains_and_a_nan_target_is_skipped(precision):
    from n3dt.train import train_step, make_flat_optimizer
    net, d, gt, mask, t_rand = _setup(precision)
    params = [p for p in net.parameters() if p.requires_grad]
    optim, _ = make_flat_optimizer(net, lr=1e-4, max_grad_norm=1.0, skip_nonfinite=True)

    # a clean step
    start = _bits(params)
    train_step(net, optim, d, gt, mask, t_rand=t_rand)
    grads = [p.grad for p in params if p.grad is not None]
    assert grads
    want = float(torch.linalg.vector_norm(torch.cat([g.detach().double().reshape(-1) for g in grads])))
    got = float(optim.grad_norm)
    rel = abs(got - want) / want
    print("%s: grad_norm %.9g, float64 norm of p.grad %.17g, relative difference %.3e (bound %.3e), clip_coef %.6g"
          % (precision, got, want, rel, 2.0 ** -23, float(optim.clip_coef)))
    assert want > 0.0 and rel <= 2.0 ** -23
    assert int(optim.skipped_steps) == 0 and int(optim.state[params[0]]["step"]) == 1
    after_clean = _bits(params)
    assert not _same(after_clean, start)

    # one NaN in the target
    img0 = _render(net, d)
    bad = gt.clone()
    bad[0, 1, IMG // 2, IMG // 2] = float("nan")
    versions = [p._version for p in params]
    train_step(net, optim, d, bad, mask, t_rand=t_rand)
    assert _same(_bits(params), after_clean), "a skipped step changed a parameter"
    assert int(optim.skipped_steps) == 1 and int(optim.state[params[0]]["step"]) == 1
    assert not bool(torch.isfinite(optim.grad_norm))
    assert all(p._version > v for p, v in zip(params, versions) if p.grad is not None)  # the host does not know: caches are rebuilt
    assert torch.equal(_render(net, d).view(torch.int32), img0.view(torch.int32))

    # and training goes on
    train_step(net, optim, d, gt, mask, t_rand=t_rand)
    assert int(optim.skipped_steps) == 1 and int(optim.state[params[0]]["step"]) == 2
    assert bool(torch.isfinite(optim.grad_norm))
    assert not _same(_bits(params), after_clean)
    assert all(bool(torch.isfinite(p).all()) for p in params)
