"""The validation metrics on the GPU: n3dt.image_metrics / calc_eval_metrics / train.validate (n3dt_eval_metrics) against the
float64 restatement (tests/eval_restatement.py) and its recorded fixtures (tests/golden/eval_metrics.*).

Tolerances (both 1e-9) are bounds, not measurements: the kernel's window sums and squared error are exact integers, so it and
the restatement differ only in float64 rounding -- below 1e-11 per window in S (the worst term, cov_norm (uxx - ux^2) with
uxx <= 65 025, has an ulp of 7.3e-12 and is divided by C2 = 58.5), and below 2^20 * 2^-53 = 1.2e-10 in the mean of up to 2^20
values of |S| <= 1 added in another order; PSNR is the same integer through sqrt and log10 on values <= 362."""
import math

import numpy as np
import pytest
import torch

import eval_restatement as er

pytestmark = pytest.mark.gpu

TOL = 1e-9
C1 = (0.01 * 255.0) ** 2
PSNR_IDENTICAL = 20.0 * math.log10(255.0 / 2.220446049250313e-16)


def dev():
    return torch.device("cuda:0")


def run(pred, gt):
    """image_metrics on host arrays -> (ssim, psnr) float64 numpy"""
    from n3dt import image_metrics
    m = image_metrics(torch.as_tensor(pred).to(dev()), torch.as_tensor(gt).to(dev()))
    assert m["SSIM"].dtype == torch.float64 and m["SSIM"].is_cuda and m["SSIM"].shape == (len(pred),) == m["PSNR"].shape
    return m["SSIM"].cpu().numpy(), m["PSNR"].cpu().numpy()


def close(got, want, what):
    err = float(np.abs(np.asarray(got) - np.asarray(want)).max())
    print("%s: max |error| %.3e" % (what, err))
    assert err <= TOL, what


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("eval_metrics")


@pytest.fixture(scope="module")
def big():
    """One 512x512 random pair and its restatement, computed once; nothing writes to it."""
    rng = np.random.default_rng(11)
    pred, gt = rng.random((1, 3, 512, 512), dtype=np.float32), rng.random((1, 3, 512, 512), dtype=np.float32)
    return pred, gt, er.batch_metrics(pred, gt)


def test_every_fixture_case(fixture):
    """A single window (7x7), sizes below one tile, tiles cut on both edges with halos crossing tile boundaries (37x53), and
    batches of different images, so that a wrong image index shows."""
    data, manifest = fixture
    for c in manifest["cases"]:
        ssim, psnr = run(data[c["name"] + "/pred"], data[c["name"] + "/gt"])
        close(ssim, data[c["name"] + "/ssim"], c["name"] + " SSIM")
        close(psnr, data[c["name"] + "/psnr"], c["name"] + " PSNR")


def test_real_size_random_pair(big):
    """512x512: 256 partials per image through the finalise kernel, the integer ranges at real size."""
    pred, gt, (ssim_ref, psnr_ref) = big
    ssim, psnr = run(pred, gt)
    close(ssim, ssim_ref, "512^2 SSIM")
    close(psnr, psnr_ref, "512^2 PSNR")


def test_extreme_and_identical_images():
    zeros, ones = np.zeros((1, 3, 64, 64), np.float32), np.ones((1, 3, 64, 64), np.float32)
    ssim, psnr = run(zeros, ones)  # the largest sums: every window 49 * 255^2, every difference 255
    close(ssim, [C1 / (65025.0 + C1)], "0 vs 1 SSIM")
    close(psnr, [0.0], "0 vs 1 PSNR")
    a = np.random.default_rng(3).random((2, 3, 40, 33), dtype=np.float32)
    ssim, psnr = run(a, a.copy())
    assert ssim.tolist() == [1.0, 1.0]  # exactly
    close(psnr, [PSNR_IDENTICAL] * 2, "identical PSNR")


def test_strided_inputs_and_repeated_calls_give_the_same_bits(big):
    from n3dt import image_metrics
    pred, gt = torch.as_tensor(big[0]).to(dev()), torch.as_tensor(big[1]).to(dev())
    pred, gt = pred[:, :, :70, :45].contiguous(), gt[:, :, :70, :45].contiguous()
    first = image_metrics(pred, gt)
    again = image_metrics(pred, gt)
    assert torch.equal(first["SSIM"], again["SSIM"]) and torch.equal(first["PSNR"], again["PSNR"])
    # an expand()ed batch: stride 0 over the images
    ex = image_metrics(pred.expand(3, -1, -1, -1), gt.expand(3, -1, -1, -1))
    assert not pred.expand(3, -1, -1, -1).is_contiguous()
    assert torch.equal(ex["SSIM"], first["SSIM"].expand(3)) and torch.equal(ex["PSNR"], first["PSNR"].expand(3))
    # channel-last storage viewed back as [B,3,H,W]
    cl_pred, cl_gt = pred.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2), gt.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert not cl_pred.is_contiguous()
    cl = image_metrics(cl_pred, cl_gt)
    assert torch.equal(cl["SSIM"], first["SSIM"]) and torch.equal(cl["PSNR"], first["PSNR"])


def test_out_of_range_values_follow_the_documented_clamp():
    rng = np.random.default_rng(7)
    pred, gt = rng.random((1, 3, 20, 27), dtype=np.float32), rng.random((1, 3, 20, 27), dtype=np.float32)
    pred[0, 0, 5, 5], pred[0, 1, 9, 14], pred[0, 2, 10, 3], gt[0, 1, 12, 20] = np.nan, -0.1, 1.3, 1.3
    ssim, psnr = run(pred, gt)
    ssim_ref, psnr_ref = er.batch_metrics(np.clip(np.nan_to_num(pred, nan=0.0), 0.0, 1.0), np.clip(gt, 0.0, 1.0))
    close(ssim, ssim_ref, "clamped SSIM")
    close(psnr, psnr_ref, "clamped PSNR")


def test_graph_capture_replays_bit_equal(big):
    """One single-stream capture of image_metrics: the path synchronises nothing and allocates only through the caching allocator."""
    from n3dt import image_metrics
    pred, gt = torch.as_tensor(big[0]).to(dev())[:, :, :96, :80].contiguous(), torch.as_tensor(big[1]).to(dev())[:, :, :96, :80].contiguous()
    eager = image_metrics(pred, gt)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = image_metrics(pred, gt)
    out["SSIM"].zero_()
    out["PSNR"].zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out["SSIM"], eager["SSIM"]) and torch.equal(out["PSNR"], eager["PSNR"])


def test_calc_eval_metrics_keeps_the_reference_quirks():
    from n3dt import calc_eval_metrics
    rng = np.random.default_rng(9)
    pred, gt = rng.random((2, 3, 32, 32), dtype=np.float32), rng.random((2, 3, 32, 32), dtype=np.float32)
    ssim_ref, psnr_ref = er.batch_metrics(pred, gt)
    d = {"coarse_dict": {"merge_img": torch.as_tensor(pred).to(dev())}}
    g = torch.as_tensor(gt).to(dev())
    m = calc_eval_metrics(d, g, torch.ones(2, 1, 32, 32, device=dev()))
    assert sorted(m) == ["PSNR", "SSIM"] and all(type(v) is float for v in m.values())
    close([m["SSIM"], m["PSNR"]], [ssim_ref[0], psnr_ref[0]], "image 0 only")
    assert abs(m["SSIM"] - ssim_ref[1]) > 1e-6  # and not image 1
    assert calc_eval_metrics(d, g, torch.zeros(2, 1, 32, 32, device=dev())) == m  # the mask changes nothing
    calls = []

    def lpips_fn(a, b):
        calls.append((a, b))
        return 0.25
    m2 = calc_eval_metrics(d, g, None, lpips_fn=lpips_fn)
    assert m2 == dict(m, LPIPS=0.25) and len(calls) == 1
    a, b = calls[0]
    assert a.dtype == np.uint8 and b.dtype == np.uint8 and a.shape == (32, 32, 3) == b.shape
    assert np.array_equal(a, er.quantise(pred[0].transpose(1, 2, 0))) and np.array_equal(b, er.quantise(gt[0].transpose(1, 2, 0)))
    with pytest.raises(ValueError, match="display"):
        calc_eval_metrics(d, g, None, vis=True)


RENDER_KEYS = ("shape_code", "appea_code", "batch_Rmats", "batch_Tvecs", "batch_inv_inmats")


@pytest.fixture(scope="module")
def head():
    """The smoke geometry (featmap 8 -> 32x32, 32 samples, seed-0 weights with bg_noise 0.1) and two batches of two frames
    against synthetic.sharp_target.  A test that writes to the net's weights puts them back."""
    from n3dt import BaseOptions, HeadNeRFNet, synthetic as syn
    opt = BaseOptions({"featmap_size": 8, "featmap_nc": 256, "pred_img_size": 32, "num_sample_coarse": 32})
    net = HeadNeRFNet(opt, include_vd=False, hier_sampling=False).to(dev())
    net.load_state_dict(syn.make_state_dict(opt, seed=0, bg_noise=0.1), strict=True)
    batches = []
    for i in range(2):
        b = {k: (v.to(dev()) if torch.is_tensor(v) else v) for k, v in syn.frame_inputs(opt, 2, first_frame=2 * i).items()}
        gt, mask = syn.sharp_target(2, 32, seed=4321 + i)
        b["gt_rgb"], b["mask"] = gt.to(dev()), mask.to(dev())
        batches.append(b)
    return net, batches


def renders(net, batches, audiostyles=None):
    """per batch (merge_img, gt_rgb) on the host: the net's own renders"""
    out = []
    with torch.no_grad():
        for i, b in enumerate(batches):
            audio = b["audiostyle"] if audiostyles is None else audiostyles[i]
            img = net("test", b["batch_xy"], b["batch_uv"], audio, bg_code=None, **{k: b[k] for k in RENDER_KEYS})["coarse_dict"]["merge_img"]
            out.append((img.cpu().numpy(), b["gt_rgb"].cpu().numpy()))
    return out


def check_validate(res, res_all, exp, what):
    """exp: per batch (ssim [2], psnr [2]) of the restatement"""
    assert res["count"] == 2 and res_all["count"] == 4
    close([res["SSIM"], res["PSNR"]], [np.mean([s[0] for s, _ in exp]), np.mean([p[0] for _, p in exp])], what + ", image 0 of each batch")
    close([res_all["SSIM"], res_all["PSNR"]], [np.mean([s for s, _ in exp]), np.mean([p for _, p in exp])], what + ", every image")


def test_validate_scores_the_nets_own_renders(head):
    """train.validate, two batches of two frames: both modes equal the restatement applied to the net's own merge_img; weights
    written through .data (which moves no version counter) are the ones the next validate() renders."""
    from n3dt import validate
    net, batches = head
    exp = [er.batch_metrics(img, gt) for img, gt in renders(net, batches)]
    for mode in (True, False):
        net.train(mode)
        res, res_all = validate(net, batches), validate(net, batches, all_images=True)
        assert net.training is mode
        check_validate(res, res_all, exp, "validate")
    assert abs(res["SSIM"] - res_all["SSIM"]) > 1e-6  # the two modes are different numbers here

    w = net.fg_CD_predictor.RGB_layer_2.weight
    version, saved = w._version, w.detach().clone()
    try:
        w.data.mul_(1.01)
        assert w._version == version  # nothing tells the packed-weight cache: only invalidate_packed() does
        res2, res2_all = validate(net, batches), validate(net, batches, all_images=True)
        net.invalidate_packed()
        exp2 = [er.batch_metrics(img, gt) for img, gt in renders(net, batches)]
        check_validate(res2, res2_all, exp2, "validate after a .data write")
        print("PSNR before %.6f, after %.6f" % (res_all["PSNR"], res2_all["PSNR"]))
        assert res2_all["PSNR"] != res_all["PSNR"]
    finally:
        w.data.copy_(saved)
        net.invalidate_packed()


def test_validate_lpips_covers_the_images_the_other_metrics_cover(head):
    """`lpips_fn` is called once per SCORED image -- image 0 of each batch, or every image with all_images=True -- with that
    image's own uint8 pair, and "LPIPS" is the mean over those calls."""
    from n3dt import validate
    net, batches = head
    pairs = [(er.quantise(img.transpose(0, 2, 3, 1)), er.quantise(gt.transpose(0, 2, 3, 1))) for img, gt in renders(net, batches)]

    def stub(a, b):
        assert a.dtype == np.uint8 and b.dtype == np.uint8 and a.shape == (32, 32, 3) == b.shape
        calls.append((a.copy(), b.copy()))
        return float(np.abs(a.astype(np.float64) - b.astype(np.float64)).mean())  # a figure that depends on both images

    for all_images, picked in ((False, [(0, 0), (1, 0)]), (True, [(0, 0), (0, 1), (1, 0), (1, 1)])):
        calls = []
        res = validate(net, batches, all_images=all_images, lpips_fn=stub)
        assert res["count"] == len(picked) == len(calls)
        for (a, b), (batch, image) in zip(calls, picked):
            assert np.array_equal(a, pairs[batch][0][image]) and np.array_equal(b, pairs[batch][1][image]), (batch, image)
        want = np.mean([stub(pairs[batch][0][image], pairs[batch][1][image]) for batch, image in picked])
        assert abs(res["LPIPS"] - want) <= 1e-12 * want, (all_images, res["LPIPS"], want)
        plain = validate(net, batches, all_images=all_images)
        assert "LPIPS" not in plain and {k: res[k] for k in plain} == plain  # the other figures do not move


def test_validate_takes_audiostyle_from_the_encoder(head):
    """With `audio2style`, audiostyle = audio2style(batch["mel"]) replaces the batch's own: the batches here carry an audiostyle
    (all 5) that renders differently, and validate() must score the encoder's renders, not those."""
    from n3dt import Audio2style, synthetic as syn, validate
    net, batches = head
    torch.manual_seed(0)
    enc = Audio2style().to(dev()).eval()
    with_mel = [dict(b, mel=syn.mel_batch(2, seed=i).to(dev()), audiostyle=torch.full_like(b["audiostyle"], 5.0)) for i, b in enumerate(batches)]
    seen = []

    def encoder(mel):
        seen.append(mel)
        return enc(mel)
    with torch.no_grad():
        styles = [enc(b["mel"]) for b in with_mel]
    assert styles[0].shape == (2, 64)
    exp = [er.batch_metrics(img, gt) for img, gt in renders(net, with_mel, styles)]
    own = [er.batch_metrics(img, gt) for img, gt in renders(net, with_mel)]
    assert max(float(np.abs(e[1] - o[1]).max()) for e, o in zip(exp, own)) > 1e-6  # the batch's own audiostyle renders differently
    res, res_all = validate(net, with_mel, audio2style=encoder), validate(net, with_mel, audio2style=encoder, all_images=True)
    assert len(seen) == 4 and all(m is b["mel"] for m, b in zip(seen, with_mel + with_mel))
    check_validate(res, res_all, exp, "validate with the encoder")
