"""The VGG16 perceptual term on the MI355X (csrc/vgg_loss.hip through n3dt.perceptual and n3dt.train.HeadNeRFLossUtils): against the
fixture the reference's own HeadNeRFLossUtils emitted (tests/golden/vgg), against the tests' float64 restatement at other geometries,
exact zeros on identical images, bit-reproducible backward, NaN pixels, side streams, a training step and its hipGraph replay.

Tolerances, all set on the CPU (tools/vgg_bf16_band.py, profiles/vgg_bf16_band.json):
  fp32 (split-bf16 operands, three products): every term relative <= 1e-4.  d_merge: twice the error of the restatement run in
       plain float32 on the fixture's inputs (relative L2 8.7e-3, per entry 6.2e-2 x max|d_merge|).  The gradient is discontinuous
       -- the L1 sign at each block end, every ReLU gate, every pool arg-max -- and fp32 rounding alone flips enough of them that no
       fp32 computation holds the 1e-3 / 1e-2 first proposed for it (PyTorch's own float32 misses it on both fixture cases).  At the
       other geometries the fp32 d_merge band is computed the same way on the case's own inputs.
  bf16: twice the error of the bf16-rounded float64 restatement on the fixture's inputs (term 2.4e-3, d_merge relative L2 0.161,
       per entry 0.197 x max|d_merge|).
"""
import numpy as np
import pytest
import torch

from test_vgg_cpu import vgg_term_reference, fixture_case, fixture_weights, d_merge_at

pytestmark = pytest.mark.gpu

TOL = {
    "fp32": {"term": 1e-4, "d_l2": 1.75e-2, "d_max": 0.125},
    "bf16": {"term": 4.8e-3, "d_l2": 0.32, "d_max": 0.39},
}


def dev():
    return torch.device("cuda:0")


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / np.abs(np.asarray(b, np.float64))))


def _check_d(got, want, tol, what=""):
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    l2 = float(np.linalg.norm(got - want) / np.linalg.norm(want))
    mx = float(np.abs(got - want).max() / np.abs(want).max())
    assert l2 <= tol["d_l2"] and mx <= tol["d_max"], (what, l2, mx)


def _random_case(B, P, seed, nan=3):
    g = torch.Generator().manual_seed(seed)
    merge = torch.rand(B, 3, P, P, generator=g)
    merge.view(-1)[torch.randperm(merge.numel(), generator=g)[:nan]] = float("nan")
    gt = torch.rand(B, 3, P, P, generator=g)
    yy, xx = torch.meshgrid(torch.arange(P), torch.arange(P), indexing="ij")
    r = ((yy - P / 2.0) ** 2 + (xx - P / 2.0) ** 2).sqrt() / P
    mask = ((0.35 - r) * 8 + 0.5).clamp(0, 1).view(1, 1, P, P).repeat(B, 1, 1, 1)
    return merge, gt, mask


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["a", "b"])
def test_loss_object_matches_the_reference_fixture(golden, name, prec):
    """HeadNeRFLossUtils(vgg_weights=...).calc_total_loss: the reference's keys in its order, every term, the four block terms and
    d(total_loss)/d(merge_img) against the reference's float64 run (tools/gen_golden_vgg.py)."""
    from n3dt.train import HeadNeRFLossUtils
    g, m = golden("vgg")
    sd, _ = fixture_weights(m)
    merge, gt, bg, mask, bgv, case = fixture_case(g, m, name)
    tol = TOL[prec]
    lu = HeadNeRFLossUtils(bg_type=case["bg_type"], use_vgg_loss=True, device=dev(), vgg_weights=sd, vgg_precision=prec)
    x = merge.to(dev()).requires_grad_(True)
    res = lu.calc_total_loss(None, None, {"coarse_dict": {"merge_img": x, "bg_img": bg.to(dev())}}, gt.to(dev()), mask.to(dev()), None)
    assert list(res.keys()) == case["keys"] == ["bg_loss", "head_loss", "nonhaed_loss", "vgg", "total_loss"]
    k = name + "."
    got = [float(res[n]) for n in case["keys"]]
    assert _rel(got[3:], g[k + "terms"][3:]) <= tol["term"], (got, g[k + "terms"])
    np.testing.assert_allclose(got[:3], g[k + "terms"][:3], rtol=2e-6)
    _, blocks = lu.vgg_loss_func.masked_terms(x.detach(), gt.to(dev()), mask.to(dev()), bgv)
    assert _rel(blocks.cpu().numpy(), g[k + "blocks"]) <= tol["term"], (blocks, g[k + "blocks"])
    res["total_loss"].backward()
    d = x.grad.cpu().numpy()
    want, have = d_merge_at(g, name, d)
    _check_d(have, want, tol, name + prec)
    assert np.all(d.reshape(-1)[g[k + "nan_idx"]] == 0.0)


@pytest.mark.parametrize("B,P", [(1, 128), (3, 128), (1, 512), (3, 512), (1, 1024), (3, 1024)])
def test_term_matches_the_restatement_across_geometries(B, P):
    from n3dt import synthetic as syn
    from n3dt.perceptual import VGGPerceptualLoss, load_vgg16_features
    sd = syn.vgg16_features_state_dict(5)
    weights = load_vgg16_features(sd)
    merge, gt, mask = _random_case(B, P, seed=100 + B * 7 + P)
    xr = merge.double().requires_grad_(True)
    ref, ref_blocks = vgg_term_reference(weights, xr, gt, mask, 1.0)
    ref.backward()
    # fp32's d_merge band at this geometry: twice what plain float32 does on the same inputs (the module docstring says why)
    x32 = merge.clone().requires_grad_(True)
    vgg_term_reference(weights, x32, gt, mask, 1.0, dtype=torch.float32)[0].backward()
    e32 = x32.grad.double().numpy().reshape(-1) - xr.grad.numpy().reshape(-1)
    want = xr.grad.numpy().reshape(-1)
    band = {"fp32": dict(TOL["fp32"], d_l2=2 * float(np.linalg.norm(e32) / np.linalg.norm(want)),
                         d_max=2 * float(np.abs(e32).max() / np.abs(want).max())), "bf16": TOL["bf16"]}
    precs = ["fp32", "bf16"] if (B, P) == (3, 512) else ["fp32"]
    for prec in precs:
        f = VGGPerceptualLoss(sd, precision=prec)
        x = merge.to(dev()).requires_grad_(True)
        t, blocks = f.masked_terms(x, gt.to(dev()), mask.to(dev()), 1.0)
        t.backward()
        tol = band[prec]
        assert _rel([float(t)] + blocks.tolist(), [float(ref)] + [float(b) for b in ref_blocks]) <= tol["term"], (prec, float(t), float(ref))
        _check_d(x.grad.cpu().numpy(), xr.grad.numpy(), tol, "%s B=%d P=%d" % (prec, B, P))


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_identical_images_give_exactly_zero(prec):
    """Prediction == target (mask 1): every image of the 2B batch runs the same code in the same order, so the term and its
    gradient are exactly 0 -- whatever the image's position in the batch."""
    from n3dt import synthetic as syn
    from n3dt.perceptual import VGGPerceptualLoss
    f = VGGPerceptualLoss(syn.vgg16_features_state_dict(6), precision=prec)
    img = torch.rand(3, 3, 96, 96, generator=torch.Generator().manual_seed(8)).to(dev())
    x = img.clone().requires_grad_(True)
    t, blocks = f.masked_terms(x, img, torch.ones(3, 1, 96, 96, device=dev()), 1.0)
    t.backward()
    assert float(t) == 0.0 and float(blocks.abs().max()) == 0.0
    assert float(x.grad.abs().max()) == 0.0
    x.grad = None
    t = f(x, img)  # the reference's call form: target used as given
    t.backward()
    assert float(t) == 0.0 and float(x.grad.abs().max()) == 0.0


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_backward_is_bit_reproducible_and_nan_pixels_get_zero(prec):
    from n3dt import synthetic as syn
    from n3dt.perceptual import VGGPerceptualLoss
    f = VGGPerceptualLoss(syn.vgg16_features_state_dict(7), precision=prec)
    merge, gt, mask = _random_case(2, 200, seed=9, nan=11)
    x = merge.to(dev()).requires_grad_(True)
    grads, terms = [], []
    for _ in range(2):
        x.grad = None
        t = f.masked(x, gt.to(dev()), mask.to(dev()), 0.0)
        t.backward()
        grads.append(x.grad.clone())
        terms.append(float(t))
    assert terms[0] == terms[1]
    assert torch.equal(grads[0], grads[1])
    nan = torch.isnan(merge).view(-1).to(dev())
    assert int(nan.sum()) == 11
    assert float(grads[0].view(-1)[nan].abs().max()) == 0.0
    assert float(grads[0].abs().max()) > 0.0


def test_side_stream_gives_the_same_result_while_the_default_stream_is_busy():
    from n3dt import synthetic as syn
    from n3dt.perceptual import VGGPerceptualLoss
    f = VGGPerceptualLoss(syn.vgg16_features_state_dict(10), precision="bf16")
    merge, gt, mask = _random_case(2, 256, seed=12)
    merge, gt, mask = merge.to(dev()), gt.to(dev()), mask.to(dev())
    x = merge.clone().requires_grad_(True)
    t0 = f.masked(x, gt, mask, 1.0)
    t0.backward()
    g0, v0 = x.grad.clone(), float(t0)
    big = torch.randn(4096, 4096, device=dev())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    for _ in range(20):
        big = big @ big  # keeps the default stream busy
        big = big / big.norm()
    with torch.cuda.stream(side):
        x2 = merge.clone().requires_grad_(True)
        t1 = f.masked(x2, gt, mask, 1.0)
        t1.backward()
    side.synchronize()
    torch.cuda.synchronize()
    assert float(t1) == v0
    assert torch.equal(x2.grad, g0)


def _train_setup(B, loss_utils_fn, graph=False):
    from n3dt import BaseOptions, HeadNeRFNet, synthetic as syn
    from n3dt.train import disk_mask
    opt = BaseOptions({"featmap_size": 16, "featmap_nc": 256, "pred_img_size": 64, "num_sample_coarse": 32})
    sd = syn.make_state_dict(opt, seed=0, bg_noise=0.1)
    inp = syn.frame_inputs(opt, B)
    d = {k: (v.to(dev()) if torch.is_tensor(v) else v) for k, v in inp.items()}
    net = HeadNeRFNet(opt, False, False, train_precision="bf16").to(dev())
    net.load_state_dict(sd, strict=True)
    gt = syn.sharp_target(B, 64)[0].to(dev())
    mask = disk_mask(B, 64).to(dev())
    t_rand = syn.stratified_noise(B, 16 * 16, 32, seed=3).to(dev())
    return net, d, gt, mask, t_rand


def test_train_step_with_the_term_matches_the_restated_term():
    """train_step(loss_utils=HeadNeRFLossUtils(vgg_weights=...)) against the same step whose vgg gradient is the restatement's (float64
    on the CPU, on the same merge_img): the network's parameter gradients agree within the bf16 band."""
    from n3dt import synthetic as syn
    from n3dt.perceptual import load_vgg16_features
    from n3dt.train import HeadNeRFLossUtils, train_step, fused_data_losses
    sd = syn.vgg16_features_state_dict(13)
    weights = load_vgg16_features(sd)
    lu = HeadNeRFLossUtils(bg_type="white", use_vgg_loss=True, device=dev(), vgg_weights=sd, vgg_precision="fp32")
    net, d, gt, mask, t_rand = _train_setup(2, None)
    sgd = torch.optim.SGD(net.parameters(), lr=0.0)
    _, terms = train_step(net, sgd, d, gt, mask, t_rand=t_rand, loss_utils=lu)
    assert "vgg" in terms and float(terms["vgg"]) > 0.0
    ga = {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None}
    # the same step, the vgg term formed by the restatement on the GPU in float64
    pred = net("train", d["batch_xy"], d["batch_uv"], d["audiostyle"], bg_code=None, shape_code=d["shape_code"],
               appea_code=d["appea_code"], batch_Rmats=d["batch_Rmats"], batch_Tvecs=d["batch_Tvecs"],
               batch_inv_inmats=d["batch_inv_inmats"], t_rand=t_rand)
    t = fused_data_losses(pred["coarse_dict"], gt, mask)
    merge = pred["coarse_dict"]["merge_img"]
    xr = merge.detach().cpu().double().requires_grad_(True)
    vgg, _ = vgg_term_reference(weights, xr, gt.cpu(), mask.cpu(), 1.0)
    vgg.backward()
    assert abs(float(vgg) - float(terms["vgg"])) <= 1e-4 * float(vgg)
    sgd.zero_grad()
    torch.autograd.backward([t["total_loss"], merge], [None, xr.grad.float().to(dev())])
    worst = 0.0
    for n, p in net.named_parameters():
        if n not in ga:
            continue
        ref = p.grad.detach()
        nrm = float(ref.norm())
        if nrm == 0.0:
            continue
        worst = max(worst, float((ga[n] - ref).norm()) / nrm)
    assert worst <= TOL["bf16"]["d_l2"], worst


def test_graphed_train_step_with_the_term_replays_like_the_eager_step():
    from n3dt import synthetic as syn
    from n3dt.train import HeadNeRFLossUtils, GraphedTrainStep
    sd = syn.vgg16_features_state_dict(14)
    lu = HeadNeRFLossUtils(bg_type="white", use_vgg_loss=True, device=dev(), vgg_weights=sd, vgg_precision="bf16")
    net, d, gt, mask, t_rand = _train_setup(2, None)

    def step():
        pred = net("train", d["batch_xy"], d["batch_uv"], d["audiostyle"], bg_code=None, shape_code=d["shape_code"],
                   appea_code=d["appea_code"], batch_Rmats=d["batch_Rmats"], batch_Tvecs=d["batch_Tvecs"],
                   batch_inv_inmats=d["batch_inv_inmats"], t_rand=t_rand)
        res = lu.calc_total_loss(None, None, pred, gt, mask, None)
        for p in net.parameters():
            p.grad = None
        res["total_loss"].backward()
        return res["vgg"].detach(), res["total_loss"].detach()

    eager_vgg, eager_total = (float(v) for v in step())
    g = GraphedTrainStep(step, warmup=2)
    vgg, total = g()
    torch.cuda.synchronize()
    # no optimizer step: the weights do not move, so a replay recomputes the eager step (up to the renderer's atomic ordering)
    assert abs(float(vgg) - eager_vgg) <= 1e-4 * eager_vgg, (float(vgg), eager_vgg)
    assert abs(float(total) - eager_total) <= 1e-4 * eager_total
