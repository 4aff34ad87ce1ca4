"""LPIPS on the GPU: n3dt.LPIPS / image_metrics / calc_eval_metrics / train.validate (n3dt_lpips, csrc/lpips.hip) against the
float64 restatement (tests/lpips_restatement.py) and its recorded fixtures (tests/golden/lpips.*), with the seeded stand-in
weights of n3dt.synthetic.lpips_alex_state_dict.

Tolerances.  The kernels form every convolution from split-bf16 operands (hi*hi + hi*lo + lo*hi) with fp32 accumulation and the
distance in float64.  tools/lpips_band.py measures, on the CPU and over exactly these cases, the relative error against the
float64 restatement of (a) the restatement in plain float32 and (b) the restatement with that operand split and an fp32
accumulator per 16-wide K step; profiles/lpips_band.json holds the result: floors of 2.855e-6 for the scores and 3.175e-5 for the
layer values (the worst is a layer of the 31 x 31 case, which is a single pixel).  The bounds below are 4 x those floors, the
project's convention; tests/test_lpips_cpu.py checks the constants against the file."""
import numpy as np
import pytest
import torch

import lpips_restatement as lr

pytestmark = pytest.mark.gpu

SCORE_TOL = 1.142e-5   # 4 x 2.855e-6, relative
LAYER_TOL = 1.270e-4   # 4 x 3.175e-5, relative


def dev():
    return torch.device("cuda:0")


def gpu(a):
    return torch.as_tensor(a).to(dev())


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("lpips")


@pytest.fixture(scope="module")
def weights():
    from n3dt import synthetic as syn
    return syn.lpips_alex_state_dict(lr.WEIGHTS_SEED)


@pytest.fixture(scope="module")
def metric(weights):
    from n3dt import LPIPS
    return {"reference": LPIPS(weights), "standard": LPIPS(weights, input_mode="standard")}


def run(lp, pred, gt):
    """(score [B], layers [5,B]) float64 numpy of host arrays"""
    p, g = gpu(pred), gpu(gt)
    score, layers = lp(p, g), lp.layers(p, g)
    assert score.dtype == torch.float64 and score.is_cuda and score.shape == (len(pred),) and layers.shape == (5, len(pred))
    return score.cpu().numpy(), layers.cpu().numpy()


def close(got, want, what):
    """score and layers against the restatement, each by its relative bound; the figures are printed before they are judged"""
    (score, layers), (want_s, want_l) = got, want
    es, el = float(np.abs(score / want_s - 1.0).max()), float(np.abs(layers / want_l - 1.0).max())
    print("%s: max relative error, score %.3e (bound %.3e), layers %.3e (bound %.3e)" % (what, es, SCORE_TOL, el, LAYER_TOL))
    assert es <= SCORE_TOL and el <= LAYER_TOL, what


@pytest.mark.parametrize("mode", ["reference", "standard"])
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("case", [c[0] for c in lr.SMALL_CASES])
def test_small_shapes_against_the_restatement(fixture, metric, case, batch, mode):
    """31x31: every late map is 1x1, one partial wave, M < 64.  35x47 and 67x61: non-square, conv1's floor is not exact and a
    pool drops a row.  B = 3: different images, so that a wrong image index shows; B = 1: the first of them alone."""
    data, _ = fixture
    pred, gt = lr.to_float(data[case + "/pred_u8"][:batch]), lr.to_float(data[case + "/gt_u8"][:batch])
    want = data["%s/%s/score" % (case, mode)][:batch], data["%s/%s/layers" % (case, mode)][:, :batch]
    close(run(metric[mode], pred, gt), want, "%s B=%d %s" % (case, batch, mode))


@pytest.mark.parametrize("case", [c[0] for c in lr.BIG_CASES])
def test_real_geometry_against_the_restatement(fixture, metric, case):
    """256^2 and 512^2 at B = 1 (512^2: maps of 127^2, 63^2, 31^2): the images come from their seeds, the expected values from
    the fixture."""
    data, manifest = fixture
    c = next(c for c in manifest["cases"] if c["name"] == case)
    pred, gt = (lr.to_float(t) for t in lr.case_images_u8(c["index"], c["height"], c["width"], c["n"]))
    close(run(metric["reference"], pred, gt), (data[case + "/reference/score"], data[case + "/reference/layers"]), case)


@pytest.mark.parametrize("case", ["odd_35x47", "odd_67x61"])
def test_bitwise_properties(fixture, metric, case):
    data, _ = fixture
    lp = metric["reference"]
    a, b = gpu(lr.to_float(data[case + "/pred_u8"])), gpu(lr.to_float(data[case + "/gt_u8"]))
    first = torch.cat([lp(a, b)[None], lp.layers(a, b)])  # [6, 3]
    assert (first > 0).all()
    # two runs give the same bits
    assert torch.equal(first, torch.cat([lp(a, b)[None], lp.layers(a, b)]))
    # an identical pair is exactly 0.0, in every layer, wherever it sits in the batch
    mixed = torch.cat([a[:1], b[1:2], a[2:]])
    same = torch.cat([lp(mixed, a)[None], lp.layers(mixed, a)])
    assert same[:, 0].tolist() == [0.0] * 6 and same[:, 2].tolist() == [0.0] * 6 and torch.equal(same[:, 1], first[:, 1])
    # symmetry
    assert torch.equal(torch.cat([lp(b, a)[None], lp.layers(b, a)]), first)
    # a pair's value depends neither on its position in the batch nor on the batch size
    order = [2, 0, 1]
    assert torch.equal(torch.cat([lp(a[order], b[order])[None], lp.layers(a[order], b[order])]), first[:, order])
    for i in range(3):
        assert torch.equal(lp(a[i:i + 1], b[i:i + 1]), first[0, i:i + 1]), i
    five = [0, 1, 2, 1, 0]
    assert torch.equal(lp(a[five], b[five]), first[0, five])


def test_graph_capture_replays_bit_equal(fixture, metric):
    """One single-stream capture of the whole launch sequence: nothing synchronises and memory comes from the caching allocator.
    Default queue settings; nothing about how graphs replay is changed."""
    data, _ = fixture
    lp = metric["reference"]
    a, b = gpu(lr.to_float(data["odd_67x61/pred_u8"])), gpu(lr.to_float(data["odd_67x61/gt_u8"]))
    eager_s, eager_l = lp(a, b), lp.layers(a, b)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = lp._run(a, b)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], eager_s) and torch.equal(out[1:], eager_l)


def test_first_use_on_one_stream_then_a_call_on_another(fixture, weights):
    """The weights are packed on the stream of the first call; a call on another stream right after it waits for that pack."""
    from n3dt import LPIPS
    data, _ = fixture
    a, b = gpu(lr.to_float(data["odd_35x47/pred_u8"])), gpu(lr.to_float(data["odd_35x47/gt_u8"]))
    want = data["odd_35x47/reference/score"]
    lp = LPIPS(weights)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    first = lp(a[:1], b[:1])  # packs on the current stream
    with torch.cuda.stream(side):
        second = lp(a, b)
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(second[:1], first) and float(np.abs(second.cpu().numpy() / want - 1.0).max()) <= SCORE_TOL


def test_inputs_outside_the_unit_range_and_strided_tensors(fixture, metric, weights):
    """Values outside [0, 1] and NaN follow the quantiser's definition (clamp, NaN -> 0) in both input modes; tensors of any
    strides are accepted and give the bits of their contiguous copies."""
    data, _ = fixture
    pred, gt = lr.to_float(data["odd_35x47/pred_u8"][:1]).copy(), lr.to_float(data["odd_35x47/gt_u8"][:1]).copy()
    pred[0, 0, 5, 5], pred[0, 1, 9, 14], pred[0, 2, 10, 3], gt[0, 1, 12, 20], gt[0, 2, 30, 40] = np.nan, -0.1, 1.3, 1.3, -np.inf
    for mode in ("reference", "standard"):
        want = lr.lpips_batch(pred, gt, weights, mode)
        clean = lr.lpips_batch(np.clip(np.nan_to_num(pred, nan=0.0), 0.0, 1.0), np.clip(gt, 0.0, 1.0), weights, mode)
        assert np.array_equal(want[0], clean[0])
        close(run(metric[mode], pred, gt), want, "out of range, " + mode)
    lp = metric["reference"]
    a, b = gpu(lr.to_float(data["odd_35x47/pred_u8"])), gpu(lr.to_float(data["odd_35x47/gt_u8"]))
    first = lp(a, b)
    cl_a, cl_b = a.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2), b.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert not cl_a.is_contiguous() and torch.equal(lp(cl_a, cl_b), first)
    ex_a, ex_b = a[:1].expand(3, -1, -1, -1), b[:1].expand(3, -1, -1, -1)
    assert not ex_a.is_contiguous() and torch.equal(lp(ex_a, ex_b), first[:1].expand(3))
    wide = torch.zeros(3, 3, 40, 60, device=dev())
    wide[:, :, 2:37, 5:52] = a
    assert torch.equal(lp(wide[:, :, 2:37, 5:52], b), first)


def test_argument_errors(metric):
    lp = metric["reference"]
    ok = torch.rand(1, 3, 31, 31, device=dev())
    assert lp(ok, ok).tolist() == [0.0]
    for shape, what in (((1, 3, 30, 64), ">= 31"), ((1, 3, 64, 30), ">= 31"), ((65, 3, 31, 31), "batch")):
        x = torch.rand(*shape, device=dev())
        with pytest.raises(ValueError, match=what):
            lp(x, x)
    with pytest.raises(ValueError, match="GPU"):
        lp(ok.cpu(), ok)
    with pytest.raises(ValueError, match="GPU"):
        lp(ok, ok.cpu())
    with pytest.raises(ValueError, match="differ"):
        lp(ok, torch.rand(1, 3, 31, 32, device=dev()))
    with pytest.raises(ValueError, match="float32"):
        lp(ok.double(), ok.double())


def test_image_metrics_and_calc_eval_metrics_add_lpips(fixture, metric):
    from n3dt import calc_eval_metrics, image_metrics
    data, _ = fixture
    lp = metric["reference"]
    a, b = gpu(lr.to_float(data["square_64/pred_u8"])), gpu(lr.to_float(data["square_64/gt_u8"]))
    plain, with_lp = image_metrics(a, b), image_metrics(a, b, lpips=lp)
    assert sorted(with_lp) == ["LPIPS", "PSNR", "SSIM"] and "LPIPS" not in plain
    assert torch.equal(with_lp["LPIPS"], lp(a, b)) and torch.equal(with_lp["SSIM"], plain["SSIM"]) and torch.equal(with_lp["PSNR"], plain["PSNR"])
    d = {"coarse_dict": {"merge_img": a}}
    m, m_plain = calc_eval_metrics(d, b, None, lpips=lp), calc_eval_metrics(d, b, None)
    assert sorted(m) == ["LPIPS", "PSNR", "SSIM"] and all(type(v) is float for v in m.values())
    assert m["LPIPS"] == float(lp(a[:1], b[:1])[0]) and m["LPIPS"] != float(lp(a[1:2], b[1:2])[0])  # image 0, not image 1
    assert abs(m["LPIPS"] / data["square_64/reference/score"][0] - 1.0) <= SCORE_TOL
    assert {k: m[k] for k in m_plain} == m_plain
    with pytest.raises(ValueError, match="not both"):
        calc_eval_metrics(d, b, None, lpips=lp, lpips_fn=lambda x, y: 0.0)
    assert calc_eval_metrics(d, b, None, lpips_fn=lambda x, y: 0.25) == dict(m_plain, LPIPS=0.25)  # the callback still works


RENDER_KEYS = ("shape_code", "appea_code", "batch_Rmats", "batch_Tvecs", "batch_inv_inmats")


@pytest.fixture(scope="module")
def head():
    """The smoke geometry (featmap 8 -> 32x32, 32 samples, seed-0 weights with bg_noise 0.1) and two batches of two frames
    against synthetic.sharp_target.  Nothing writes to the net."""
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


def count_syncs(fn):
    """(result, number of synchronising calls torch saw while fn ran): torch's sync debug mode warns at every TORCH-level call that
    makes the host wait for the device (.tolist(), .cpu(), .item() ...).  That is all this counter can see: a stream synchronise
    inside libn3dt would not be counted here; it would break test_graph_capture_replays_bit_equal instead, since a capture
    refuses one."""
    import warnings
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            res = fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return res, sum("synchroniz" in str(w.message) for w in seen)


def test_validate_accumulates_lpips_on_the_device(head, metric):
    """validate(..., lpips=): the mean of the per-batch values over the images the other metrics cover, the same SSIM / PSNR as
    without it, and still ONE synchronisation -- the callback form pays one per batch on top."""
    from n3dt import validate
    net, batches = head
    lp = metric["reference"]
    with torch.no_grad():
        imgs = [net("test", b["batch_xy"], b["batch_uv"], b["audiostyle"], bg_code=None, **{k: b[k] for k in RENDER_KEYS})["coarse_dict"]["merge_img"]
                for b in batches]
    per_batch = [lp(img, b["gt_rgb"]).cpu().numpy() for img, b in zip(imgs, batches)]
    assert min(v.min() for v in per_batch) > 0.0
    for all_images in (False, True):
        plain, n_plain = count_syncs(lambda: validate(net, batches, all_images=all_images))
        res, n_res = count_syncs(lambda: validate(net, batches, all_images=all_images, lpips=lp))
        want = np.mean([v if all_images else v[:1] for v in per_batch])
        print("all_images=%s: LPIPS %.9f, mean of the per-batch calls %.9f; synchronisations %d (without lpips: %d)"
              % (all_images, res["LPIPS"], want, n_res, n_plain))
        assert abs(res["LPIPS"] - want) <= 1e-14 * want
        assert "LPIPS" not in plain and {k: res[k] for k in plain} == plain
        assert n_res == 1 and n_plain == 1
    _, n_fn = count_syncs(lambda: validate(net, batches, lpips_fn=lambda a, b: 0.5))
    assert n_fn == 1 + len(batches)  # the detector sees the callback's copies: one per batch
    with pytest.raises(ValueError, match="not both"):
        validate(net, batches, lpips=lp, lpips_fn=lambda a, b: 0.5)
