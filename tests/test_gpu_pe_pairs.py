"""The fused 16-bit kernels' positional encoder handles every (octave, axis) once, sine and cosine together, by octave half,
and scatters the values to their MFMA fragment slots through the wave's LDS copy (csrc/x16_core.h: pe_encode).  The seam
n3dt_x16_pe_probe runs it on its own (form 0) next to the per-channel encoder it replaced (form 1, kept in the probe kernel).

* form 0 == form 1, bit for bit, on 32 768 seeded random points in [-4, 4]^3 and on a structured set of at most 4 096 points:
  +-0; for each of the 10 octaves and 3 axes the fp32 neighbours (-2 .. +2 ulp) of points where 2^k p / 2 pi is a multiple of
  1/4 (where the phase fold changes branch), both signs; 1e-30 and a subnormal; 1e4; +-inf and NaN (NaN results: both NaN).
  Form 1 is the code the kernels ran before, so no tolerance is involved: zero differing entries.
* the fragment layout the header documents: form 0 decoded channel by channel against float64 sin / cos of the fp32 points.
* end to end: forward("test") twice at the smallest geometry the suite uses for the fused kernel (fs 8, 16 samples, 64^2,
  B = 3) against the CPU oracle at test_gpu_parity's RGB_TOL, same bits both times; render_features on ragged input (7 rays x
  3 frames, N_s = 40: dead lanes, a workgroup spanning frames) against the oracle at FEAT_TOL.
"""
import functools

import numpy as np
import pytest
import torch

from n3dt import ops
from test_gpu_parity import RGB_TOL, feats, to_dev
from test_gpu_pack_pairs import _oracle_images
from test_gpu_step_tail import dev, fwd, make
from test_gpu_stream_issue import _check, _net, _ragged_case

pytestmark = pytest.mark.gpu

NAN_ABOVE = {"bf16": 0x7F80, "fp16": 0x7C00}


@functools.lru_cache(maxsize=None)
def _random_points():
    return np.random.RandomState(20261019).uniform(-4.0, 4.0, size=(32768, 3)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _structured_points():
    rng = np.random.RandomState(1019)
    rows = []

    def on_axis(axis, values):
        p = rng.uniform(-4.0, 4.0, size=(len(values), 3)).astype(np.float32)
        p[:, axis] = values
        rows.append(p)

    for k in range(10):
        step = np.pi / 2.0 ** (k + 1)                                 # 2^k p / 2 pi = m / 4  <=>  p = m pi / 2^(k+1)
        m_max = int(4.0 / step)
        m = np.concatenate([np.arange(1, 9), rng.randint(9, max(m_max, 10) + 1, size=4)]).astype(np.float64)
        centre = (m * step).astype(np.float32).view(np.int32)
        near = np.concatenate([centre + d for d in (-2, -1, 0, 1, 2)]).view(np.float32)  # positive floats: +-1 on the bits is +-1 ulp
        for axis in range(3):
            on_axis(axis, np.concatenate([near, -near]))
    special = np.array([0.0, -0.0, 1e-30, -1e-30, 1e-40, -1e-40, 1e4, -1e4, np.inf, -np.inf, np.nan], dtype=np.float32)
    for axis in range(3):
        on_axis(axis, special)
    rows.append(np.repeat(special[:, None], 3, axis=1))               # and on all three axes at once
    p = np.concatenate(rows).astype(np.float32)
    assert len(p) <= 4096
    return np.concatenate([p, np.zeros(((-len(p)) % 32, 3), dtype=np.float32)])


def _encode(points, prec, form):
    x = torch.from_numpy(points).to(dev())
    out = ops.x16_pe_probe(x, prec, form)
    torch.cuda.synchronize()
    assert out.shape == (len(points) // 32, 4, 64, 8)
    return out.view(torch.int16).cpu().numpy().view(np.uint16)


def _channels(frags):
    """[waves, 4, 64, 8] fragments -> [points, 64] channels: piece ks, lane (c, h), element j is channel
    16 ks + 8 (j >> 2) + 4 h + (j & 3) of the wave's point c"""
    w = frags.shape[0]
    f = frags.reshape(w, 4, 2, 32, 2, 4)                              # ks, h, c, j >> 2, j & 3
    return f.transpose(0, 3, 1, 4, 2, 5).reshape(w * 32, 64)          # point, then ks, j >> 2, h, j & 3 = the channel's bits


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_pair_encoder_equals_the_per_channel_encoder(prec):
    for what, p, nan_ok in (("32 768 random points", _random_points(), False), ("structured set", _structured_points(), True)):
        a, b = _encode(p, prec, 0), _encode(p, prec, 1)
        na, nb = (a & 0x7FFF) > NAN_ABOVE[prec], (b & 0x7FFF) > NAN_ABOVE[prec]
        bad = (na != nb) | (~na & (a != b))
        n = int(bad.sum())
        print("%s %s: %d values, %d NaN results, %d differ" % (prec, what, a.size, int(na.sum()), n))
        if not nan_ok:
            assert not na.any() and not nb.any()
        if n:
            pt, ch = np.argwhere(_channels(bad))[0]
            raise AssertionError("%s: %d differ, first: point %r channel %d -> 0x%04x against 0x%04x" % (
                what, n, p[pt].tolist(), ch, int(_channels(a)[pt, ch]), int(_channels(b)[pt, ch])))


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_fragments_hold_the_documented_channels(prec):
    """Channels 0-2 the point, 3 + 6 k + d the sine and 3 + 6 k + 3 + d the cosine of 2^k p_d, 63 zero.  Bound: half a unit in
    the last place of the 16-bit format for values up to 1 (2^-9 / 2^-12; for the raw coordinates up to 4: 2^-7 / 2^-10) plus
    the encoder's own fp32 error (below 1e-6, tests/test_gpu_x16_stagewise.py), asserted at twice the half-ulp."""
    p = _random_points()[:4096]
    dt = torch.bfloat16 if prec == "bf16" else torch.float16
    got = torch.from_numpy(_channels(_encode(p, prec, 0)).view(np.int16).copy()).view(dt).to(torch.float64).numpy()
    p64 = p.astype(np.float64)
    want = np.zeros((len(p), 64))
    want[:, :3] = p64
    for k in range(10):
        want[:, 3 + 6 * k:6 + 6 * k] = np.sin(2.0 ** k * p64)
        want[:, 6 + 6 * k:9 + 6 * k] = np.cos(2.0 ** k * p64)
    half_ulp = 2.0 ** -9 if prec == "bf16" else 2.0 ** -12
    e_raw, e_enc = float(np.abs(got[:, :3] - want[:, :3]).max()), float(np.abs(got[:, 3:] - want[:, 3:]).max())
    print("%s: raw coordinates max|err| %.3e (bound %.3e), encoded channels %.3e (bound %.3e)" % (prec, e_raw, 8 * half_ulp, e_enc, 2 * half_ulp))
    assert e_raw <= 8 * half_ulp and e_enc <= 2 * half_ulp
    assert not got[:, 63].any()


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_forward_twice_against_the_oracle(prec):
    ref_merge, ref_bg = _oracle_images()
    net, d, _ = make(prec, B=3)
    outs = []
    for _ in range(2):
        o = fwd(net, d)["coarse_dict"]
        outs.append({k: o[k].clone() for k in ("merge_img", "bg_img")})
    for n, o in enumerate(outs):
        e_m = float(np.abs(o["merge_img"].cpu().numpy() - ref_merge).max())
        e_b = float(np.abs(o["bg_img"].cpu().numpy() - ref_bg).max())
        print("%s forward %d: merge_img max|err| %.3e, bg_img max|err| %.3e (bound %.1e)" % (prec, n + 1, e_m, e_b, RGB_TOL[prec]))
        assert e_m <= RGB_TOL[prec] and e_b <= RGB_TOL[prec]
    assert torch.equal(outs[0]["merge_img"], outs[1]["merge_img"]) and torch.equal(outs[0]["bg_img"], outs[1]["bg_img"])


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_ragged_blocks_against_the_oracle(prec):
    """7 rays x 3 frames, N_s = 40: the second block of a ray has 8 live samples (dead lanes still encode and scatter: their
    LDS rows are their own), 42 blocks leave dead waves, and a workgroup's eight waves cover two frames."""
    opt, sd, inp, ref = _ragged_case(40)
    _check(feats(_net(opt, sd, prec), to_dev(inp), want_merge=False), ref, prec)
