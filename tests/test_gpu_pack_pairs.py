"""X16<PREC>::pack converts accumulator values two at a time (one v_cvt_pk_bf16_f32 / v_cvt_pk_f16_f32 per packed dword, both
sources live).  The seam n3dt_x16_pack_probe runs that pack on its own (form 0) next to a copy of the element-wise cast it used to
be (form 1, kept in the probe kernel only).

* form 0 == form 1, bit for bit (NaN results: both NaN), on 2^20 float bit patterns from a fixed seed and on a structured set:
  for 4 096 random 16-bit targets (2 048 with an even, 2 048 with an odd bit pattern -- both tie directions) the exact midpoint
  between the target and its neighbour one step up in magnitude, and the floats one ulp either side of that midpoint; +-0, +-inf,
  +-the largest finite float, fp16's overflow threshold 65 520 and its neighbours, values that round into fp16's subnormal range,
  NaNs (quiet, signalling, payload in the low 16 bits only).
* the structured set against the host's round-to-nearest-even (`tensor.to(torch.bfloat16 / torch.float16)` on the CPU), on
  every input that is normal in fp32 and whose result is normal, zero or infinite in the 16-bit format: there the two cannot
  legitimately differ (subnormal inputs and results depend on the denormal mode of the kernel, NaN payloads on the hardware).
* end to end at the smallest geometry the suite uses for the fused kernel (tests/test_gpu_step_tail.py: fs 8, 16 samples, 64^2,
  B = 3): forward("test") twice on the same inputs, merge_img and bg_img against the CPU oracle at test_gpu_parity's RGB_TOL.
"""
import functools

import numpy as np
import pytest
import torch

from n3dt import ops, synthetic as syn
from test_gpu_parity import RGB_TOL
from test_gpu_step_tail import dev, fwd, make

pytestmark = pytest.mark.gpu

FMT = {  # torch dtype, mantissa bits, the 16-bit pattern of +inf
    "bf16": (torch.bfloat16, 7, 0x7F80),
    "fp16": (torch.float16, 10, 0x7C00),
}


def _midpoints(prec, rng):
    """Midpoints (and their two float neighbours) above 4 096 random finite 16-bit targets, half of them even, half odd."""
    _dt, _mant, inf16 = FMT[prec]
    mag = rng.randint(0, inf16, size=4096).astype(np.uint32)          # finite magnitudes: 0 .. inf16 - 1
    mag = (mag & ~np.uint32(1)) | np.repeat(np.array([0, 1], dtype=np.uint32), 2048)  # parity of the LOWER neighbour
    sign = rng.randint(0, 2, size=4096).astype(np.uint32)
    if prec == "bf16":
        mid = (mag << 16) | np.uint32(0x8000)                       # bf16 is the float's upper half: the midpoint is exact
    else:
        lo = mag.astype(np.uint16).view(np.float16).astype(np.float64)
        up = (mag + 1).astype(np.uint16).view(np.float16).astype(np.float64)
        up[mag + 1 == inf16] = 65536.0                                # above the largest finite value: the overflow threshold 65 520
        m32 = ((lo + up) / 2).astype(np.float32)
        assert np.array_equal(m32.astype(np.float64), (lo + up) / 2)  # 12 significant bits at most: exact in fp32
        mid = m32.view(np.uint32)
    assert (mid & 0x7FFFFFFF).min() > 0
    mid = np.concatenate([mid - 1, mid, mid + 1])                     # sign-magnitude: +-1 on the pattern is +-1 ulp
    return mid | np.tile(sign << 31, 3)


@functools.lru_cache(maxsize=None)
def _structured(prec):
    rng = np.random.RandomState(20261018)
    both = lambda a: np.concatenate([np.asarray(a, dtype=np.uint32), np.asarray(a, dtype=np.uint32) | np.uint32(0x80000000)])  # noqa: E731
    f = lambda *v: np.array(v, dtype=np.float32).view(np.uint32)      # noqa: E731
    around = lambda u: np.concatenate([u - 1, u, u + 1])              # noqa: E731
    parts = [
        _midpoints(prec, rng),
        both([0x00000000, 0x7F800000, 0x7F7FFFFF]),                   # 0, inf, the largest finite float
        both(around(f(65520.0, 65504.0, 65536.0))),                   # fp16's overflow threshold, its largest value, 2^16
        # fp16's subnormal range [2^-24, 2^-14) and its edges: 2^-14 (smallest normal), 2^-24 (smallest subnormal), 2^-25 (the
        # tie to zero), 2^-26, plus 2 048 random floats in [2^-26, 2^-14)
        both(around(f(2.0 ** -14, 2.0 ** -15, 2.0 ** -24, 2.0 ** -25, 2.0 ** -26, 3 * 2.0 ** -25, 1023.5 * 2.0 ** -24))),
        both(rng.randint(0x32800000, 0x38800000, size=2048).astype(np.uint32)),
        # NaNs: quiet, signalling, full payload, payload in the low 16 bits only (the bits bf16 drops)
        both([0x7FC00000, 0x7F800001, 0x7FFFFFFF, 0x7FA00000, 0x7F80FFFF, 0x7F808000, 0x7FC00001]),
    ]
    u = np.concatenate(parts).astype(np.uint32)
    pad = (-len(u)) % 512
    return np.concatenate([u, np.zeros(pad, dtype=np.uint32)])


@functools.lru_cache(maxsize=None)
def _random_patterns():
    return np.random.RandomState(7).randint(0, 2 ** 32, size=1 << 20, dtype=np.uint64).astype(np.uint32)


def _pack(u32, prec, form):
    x = torch.from_numpy(u32.view(np.int32).copy()).to(dev()).view(torch.float32)
    out = ops.x16_pack_probe(x, prec, form)
    torch.cuda.synchronize()
    assert out.dtype == FMT[prec][0] and out.shape == x.shape
    return out.view(torch.int16).cpu().numpy().view(np.uint16)


def _is_nan16(u16, prec):
    return (u16 & 0x7FFF) > FMT[prec][2]


def _same_bits_or_both_nan(a, b, prec, src, what):
    na, nb = _is_nan16(a, prec), _is_nan16(b, prec)
    bad = (na != nb) | (~na & (a != b))
    n = int(bad.sum())
    i = int(np.argmax(bad))
    print("%s %s: %d values, %d NaN results, %d differ" % (prec, what, a.size, int(na.sum()), n))
    assert n == 0, "%s: %d differ, first: float bits 0x%08x -> 0x%04x against 0x%04x" % (what, n, int(src[i]), int(a[i]), int(b[i]))


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_pairwise_pack_equals_the_element_wise_cast(prec):
    for what, u in (("2^20 random bit patterns", _random_patterns()), ("structured set", _structured(prec))):
        assert u.size % 512 == 0
        _same_bits_or_both_nan(_pack(u, prec, 0), _pack(u, prec, 1), prec, u, what)


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_pack_is_the_hosts_round_to_nearest_even(prec):
    dt, mant, inf16 = FMT[prec]
    u = _structured(prec)
    got = _pack(u, prec, 0)
    host = torch.from_numpy(u.view(np.int32).copy()).view(torch.float32).to(dt).view(torch.int16).numpy().view(np.uint16)
    e32 = (u >> 23) & 0xFF
    in_normal = (e32 >= 1) & (e32 <= 254)
    hmag = host & 0x7FFF
    res_ok = (hmag == 0) | (hmag == inf16) | ((hmag >= (1 << mant)) & (hmag < inf16))  # zero, infinite, normal
    sel = in_normal & res_ok
    n_inf, n_zero = int((hmag[sel] == inf16).sum()), int((hmag[sel] == 0).sum())
    print("%s against the host: %d of %d inputs compared (%d round to inf, %d to zero), %d differ" % (
        prec, int(sel.sum()), u.size, n_inf, n_zero, int((got[sel] != host[sel]).sum())))
    assert int(sel.sum()) > 3 * 2048 and n_inf > 0  # the midpoints are in it, and so is the overflow edge
    if prec == "fp16":
        assert n_zero > 0
    bad = sel & (got != host)
    i = int(np.argmax(bad))
    assert not bad.any(), "first: float bits 0x%08x -> 0x%04x, host 0x%04x" % (int(u[i]), int(got[i]), int(host[i]))


@functools.lru_cache(maxsize=None)
def _oracle_images():
    from oracle import oracle as orc
    _net, _d, opt = make("bf16", B=3)
    sd = syn.make_state_dict(opt, seed=0, bg_noise=0.1, hier_sampling=False)
    ref = orc.forward(sd, opt, syn.frame_inputs(opt, 3))
    return ref["merge_img"], ref["bg_img"]


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
