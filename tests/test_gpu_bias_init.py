"""The fused render kernel's tile biases: staged into per-wave LDS slots and placed in the accumulator as the C operand of a
tile's first weight MFMA (csrc/nerf_fwd_x16.hip: X16BiasLds, X16TileInit).  bf16 and fp16 `render_features` against the CPU
oracle at the tolerances tests/test_gpu_round2.py uses for these precisions, on shapes chosen for what this path can get
wrong: workgroups whose eight waves cover two frames (per-wave tables), ragged blocks with dead lanes, a network that is
nothing but biases (the row mapping of the LDS reads), the per-ray table of include_vd, and back-to-back launches."""
import functools

import numpy as np
import pytest
import torch

from test_gpu_parity import dev, to_dev, feats, FEAT_TOL

pytestmark = pytest.mark.gpu

RAYS = [0, 9, 18, 27, 36, 45, 63]  # a free set of 7 rays of the 8 x 8 grid


def _opt(n_samples):
    from n3dt import BaseOptions
    return BaseOptions({"featmap_size": 8, "featmap_nc": 256, "pred_img_size": 32, "num_sample_coarse": n_samples})


def _inputs(opt, batch, first_frame=0):
    from n3dt import synthetic as syn
    inp = syn.frame_inputs(opt, batch, first_frame=first_frame)
    inp["batch_xy"] = inp["batch_xy"].index_select(2, torch.tensor(RAYS)).contiguous()  # [B, 2, 7]
    del inp["batch_uv"]  # (of the full grid; the volumetric stage does not read it)
    return inp


def _net(opt, sd, precision, include_vd=False):
    from n3dt import HeadNeRFNet
    net = HeadNeRFNet(opt, include_vd=include_vd, hier_sampling=False, precision=precision).to(dev())
    net.load_state_dict(sd, strict=True)
    return net


def _oracle(sd, opt, inp, include_vd=False):
    from oracle import oracle as orc
    ref = orc.forward(sd, opt, inp, skip_neural_render=True, include_vd=include_vd)
    return ref["fg_feat"], ref["bg_alpha"]


def _check(f, ref, precision):
    fg, ba = ref
    np.testing.assert_allclose(f["fg_feat"].permute(0, 2, 1).cpu().numpy(), fg, atol=FEAT_TOL[precision])
    np.testing.assert_allclose(f["bg_alpha"].cpu().numpy()[:, None], ba, atol=FEAT_TOL[precision])


@functools.lru_cache(maxsize=None)
def _spanning_case(n_samples):
    from n3dt import synthetic as syn
    opt = _opt(n_samples)
    sd = syn.make_state_dict(opt, seed=3, bg_noise=0.1)
    inp = _inputs(opt, 3)
    return opt, sd, inp, _oracle(sd, opt, inp)


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
@pytest.mark.parametrize("n_samples", [40, 32])
def test_workgroups_that_span_frames_and_ragged_blocks(n_samples, precision):
    """7 rays x 3 frames with different latent codes.  N_s = 40: two blocks per ray, the second with 8 live samples -- 42
    blocks, so the eight waves of a workgroup cover two frames (each wave stages ITS frame's tables) and dead lanes and dead
    waves exist.  N_s = 32: one full block per ray, 21 blocks."""
    opt, sd, inp, ref = _spanning_case(n_samples)
    assert float(np.abs(ref[0][0] - ref[0][1]).max()) > 10 * FEAT_TOL[precision]  # the frames do differ
    _check(feats(_net(opt, sd, precision), to_dev(inp), want_merge=False), ref, precision)


@functools.lru_cache(maxsize=None)
def _bias_only_case():
    from n3dt import synthetic as syn
    opt = _opt(40)
    sd = syn.make_state_dict(opt, seed=0, bg_noise=0.1)
    layer = 0
    for k in sorted(sd):
        if not k.startswith("fg_CD_predictor."):
            continue
        if k.endswith(".weight") and "RGB_layer_2" not in k:
            sd[k] = torch.zeros_like(sd[k])
        elif k.endswith(".bias"):
            i = torch.arange(sd[k].numel(), dtype=torch.float64)
            sd[k] = ((((37 * i + 13 * layer) % 101) - 50) / 64 + i * 2.0 ** -12).to(torch.float32).view_as(sd[k])
            layer += 1
    sd["fg_CD_predictor.density_module.bias"] = torch.full((1,), 0.75 + 2.0 ** -12)  # relu(density) must not be 0
    inp = _inputs(opt, 2)
    for k in ("shape_code", "appea_code", "audiostyle"):
        inp[k] = torch.zeros_like(inp[k])
    return opt, sd, inp, _oracle(sd, opt, inp)


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_a_network_of_biases_only(precision):
    """Every weight matrix the fused kernel multiplies by is zero (RGB_layer_2, applied per ray behind it, keeps its weights
    so that the 192 composited values stay visible), the latent codes are zero, and every bias is a distinct value per row
    with more than 8 mantissa bits: ((37 i + 13 layer) % 101 - 50) / 64 + i 2^-12.  The output is then relu(bias of
    RGB_layer_1) times the density bias's compositing weights: a wrong row mapping of the LDS reads (lane half, 16-byte
    group, register) moves whole values instead of hiding in random weights."""
    opt, sd, inp, ref = _bias_only_case()
    assert float(np.abs(ref[0]).max()) > 0.1 and float(ref[1].max()) < 0.9
    _check(feats(_net(opt, sd, precision), to_dev(inp), want_merge=False), ref, precision)


@functools.lru_cache(maxsize=None)
def _vd_case():
    from n3dt import synthetic as syn
    opt = _opt(32)
    sd = syn.make_state_dict(opt, seed=4, bg_noise=0.1, include_vd=True)
    inp = _inputs(opt, 3)
    return opt, sd, inp, _oracle(sd, opt, inp, include_vd=True)


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_per_ray_bias_of_include_vd_through_the_lds_slot(precision):
    """include_vd: the merged RGB stage's table is per RAY (frame entry + view-direction term), 7 rays x 3 frames, N_s = 32."""
    opt, sd, inp, ref = _vd_case()
    _check(feats(_net(opt, sd, precision, include_vd=True), to_dev(inp), want_merge=False), ref, precision)


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_consecutive_launches_on_different_frames(precision):
    """Two launches through one network, on different frames, give what each gives alone (a network of its own): nothing of
    the first launch's bias tables survives into the second."""
    from n3dt import synthetic as syn
    opt = _opt(40)
    sd = syn.make_state_dict(opt, seed=3, bg_noise=0.1)
    a, b = to_dev(_inputs(opt, 2, first_frame=0)), to_dev(_inputs(opt, 2, first_frame=2))
    net = _net(opt, sd, precision)
    got_a = {k: v.clone() for k, v in feats(net, a, want_merge=False).items() if torch.is_tensor(v)}
    got_b = {k: v.clone() for k, v in feats(net, b, want_merge=False).items() if torch.is_tensor(v)}
    alone_a = feats(_net(opt, sd, precision), a, want_merge=False)
    alone_b = feats(_net(opt, sd, precision), b, want_merge=False)
    assert not torch.equal(got_a["fg_feat"], got_b["fg_feat"])
    for k in ("fg_feat", "bg_alpha"):
        assert torch.equal(got_a[k], alone_a[k]), k
        assert torch.equal(got_b[k], alone_b[k]), k
    _check(got_b, _oracle(sd, opt, _inputs(opt, 2, first_frame=2)), precision)
