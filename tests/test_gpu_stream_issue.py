"""The weight stream's issue schedule (csrc/x16_core.h: X16Issue, WeightStream): where in a chunk a wave issues the LDS-DMA
pieces of the chunk two ahead.  A piece issued too early overwrites a ring buffer that a slower wave still reads; one whose
wait is miscounted is read before it has landed.  Both show as a run-to-run difference before they show as a parity failure,
so next to the oracle comparisons at tests/test_gpu_parity.py's tolerances the same launch is repeated and compared bit for
bit.  Shapes: ragged blocks with dead waves and dead lanes and workgroups of two frames; 32 full workgroups; the whole
forward("test") at the smallest geometry the suite uses for it (the renderer's block kernels read the same stream)."""
import functools

import numpy as np
import pytest
import torch

from test_gpu_parity import dev, to_dev, feats, fwd, FEAT_TOL, RGB_TOL

pytestmark = pytest.mark.gpu

RAYS = [0, 9, 18, 27, 36, 45, 63]  # 7 rays of the 8 x 8 grid


def _opt(n_samples, pred=32):
    from n3dt import BaseOptions
    return BaseOptions({"featmap_size": 8, "featmap_nc": 256, "pred_img_size": pred, "num_sample_coarse": n_samples})


def _net(opt, sd, precision):
    from n3dt import HeadNeRFNet
    net = HeadNeRFNet(opt, include_vd=False, hier_sampling=False, precision=precision).to(dev())
    net.load_state_dict(sd, strict=True)
    return net


def _oracle_feats(sd, opt, inp):
    from oracle import oracle as orc
    ref = orc.forward(sd, opt, inp, skip_neural_render=True)
    return ref["fg_feat"], ref["bg_alpha"]


def _check(f, ref, precision):
    fg, ba = ref
    e_f = float(np.abs(f["fg_feat"].permute(0, 2, 1).cpu().numpy() - fg).max())
    e_a = float(np.abs(f["bg_alpha"].cpu().numpy()[:, None] - ba).max())
    print("%s: fg_feat max|err| %.3e, bg_alpha max|err| %.3e (bound %.1e)" % (precision, e_f, e_a, FEAT_TOL[precision]))
    assert e_f <= FEAT_TOL[precision] and e_a <= FEAT_TOL[precision]


@functools.lru_cache(maxsize=None)
def _ragged_case(n_samples):
    from n3dt import synthetic as syn
    opt = _opt(n_samples)
    sd = syn.make_state_dict(opt, seed=3, bg_noise=0.1)
    inp = syn.frame_inputs(opt, 3)
    inp["batch_xy"] = inp["batch_xy"].index_select(2, torch.tensor(RAYS)).contiguous()  # [B, 2, 7]
    del inp["batch_uv"]  # (of the full grid; the volumetric stage does not read it)
    return opt, sd, inp, _oracle_feats(sd, opt, inp)


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
@pytest.mark.parametrize("n_samples", [40, 32])
def test_ragged_blocks_dead_waves_and_two_frames_per_workgroup(n_samples, precision):
    """7 rays x 3 frames.  N_s = 40: 42 blocks, the second of a ray with 8 live samples; N_s = 32: 21 blocks.  Workgroups
    with dead waves (which still issue their share of every chunk) and dead lanes, and tables of two frames in one workgroup."""
    opt, sd, inp, ref = _ragged_case(n_samples)
    _check(feats(_net(opt, sd, precision), to_dev(inp), want_merge=False), ref, precision)


@functools.lru_cache(maxsize=None)
def _full_case():
    from n3dt import synthetic as syn
    opt = _opt(64)
    sd = syn.make_state_dict(opt, seed=5, bg_noise=0.1)
    inp = syn.frame_inputs(opt, 2)
    return opt, sd, inp, _oracle_feats(sd, opt, inp)


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_full_workgroups_repeat_bit_for_bit(precision):
    """The full 8 x 8 grid, N_s = 64, B = 2: 256 blocks = 32 workgroups of eight live waves.  The same launch eight times:
    every repeat equals the first bit for bit (a stale ring read is a run-to-run difference), the first equals the oracle."""
    opt, sd, inp, ref = _full_case()
    net, d = _net(opt, sd, precision), to_dev(inp)
    first = {k: v.clone() for k, v in feats(net, d, want_merge=False).items() if torch.is_tensor(v)}
    for n in range(1, 8):
        again = feats(net, d, want_merge=False)
        for k in ("fg_feat", "bg_alpha"):
            assert torch.equal(first[k], again[k]), "%s differs in repeat %d" % (k, n)
    _check(first, ref, precision)


@functools.lru_cache(maxsize=None)
def _forward_case():
    from n3dt import synthetic as syn
    from oracle import oracle as orc
    opt = _opt(16, pred=64)
    sd = syn.make_state_dict(opt, seed=0, bg_noise=0.1)
    inp = syn.frame_inputs(opt, 3)
    ref = orc.forward(sd, opt, inp)
    return opt, sd, inp, (ref["merge_img"], ref["bg_img"])


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_forward_against_the_oracle(precision):
    """forward("test") at fs 8 / 16 samples / 64^2, B = 3: the fused kernel and the renderer's block kernels behind it."""
    opt, sd, inp, (ref_merge, ref_bg) = _forward_case()
    net, d = _net(opt, sd, precision), to_dev(inp)
    out = fwd(net, d)
    e_m = float(np.abs(out["merge_img"].cpu().numpy() - ref_merge).max())
    e_b = float(np.abs(out["bg_img"].cpu().numpy() - ref_bg).max())
    print("%s forward: merge_img max|err| %.3e, bg_img max|err| %.3e (bound %.1e)" % (precision, e_m, e_b, RGB_TOL[precision]))
    assert e_m <= RGB_TOL[precision] and e_b <= RGB_TOL[precision]
