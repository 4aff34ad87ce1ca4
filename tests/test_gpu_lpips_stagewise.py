"""The kernels of csrc/lpips.hip pinned stage by stage on the MI355X through the two buffers they leave behind: n3dt_lpips_pack's
caller-owned packed buffer and n3dt_lpips' caller-owned workspace, both pre-filled by the test and read back whole -- see
tests/lpips_stagewise.py for the restated layouts, the float64 references (each stage from its own STORED input), the rules and the
floors, which come from the CPU alone (test_lpips_stagewise_cpu.py).  No kernel changed and there is no debug entry.

  pack        byte for byte over a 0xA5 prefill, the bytes behind the buffer included
  in0         bitwise against float32 numpy, both input modes, NaN / -0.0 / out-of-range / between-bytes inputs; halo +0
  conv1..5    every float of every map: |got - ref| <= 4 floor_l S per entry, halos +0
  pool1, 2    bitwise, halo +0
  partials    per (layer, pair, part) within 1e-13 S_p; parts without a pixel and identical pairs exactly +0
  layers out  bitwise from the stored partials
  untouched   every other workspace byte keeps the prefill; a 0xFF (NaN) and a zero prefill give the bits of the 0xA5 run

                conv1     conv2     conv3     conv4     conv5
  CPU floor     3.5e-6    1.7e-6    2.5e-6    2.5e-6    3.35e-6
  bound (x 4)   1.4e-5    6.8e-6    1.0e-5    1.0e-5    1.34e-5
Each test prints every family's largest error / bound before judging it (pytest -s); DESIGN section 4 records what one MI355X showed."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import lpips_stagewise as ls

pytestmark = pytest.mark.gpu

BOUND = tuple(ls.MARGIN * f for f in ls.FLOOR)
TAIL = 256


def dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def packed():
    """(the packed buffer on the device with TAIL bytes behind it, its bytes on the host), packed once over a 0xA5 prefill"""
    from n3dt import ops
    from n3dt._lib import LpipsParams, check, lib
    total = lib().n3dt_lpips_packed_bytes()
    dev_w = [tuple(torch.from_numpy(t).to(dev()).contiguous() for t in layer) for layer in ls.weights()[0]]
    p = LpipsParams()
    for i, (w, b, lin) in enumerate(dev_w):
        p.weight[i], p.bias[i], p.lin[i] = w.data_ptr(), b.data_ptr(), lin.data_ptr()
    buf = torch.full((total + TAIL,), ls.PREFILL, dtype=torch.uint8, device=dev())
    assert buf.data_ptr() % 256 == 0
    check(lib().n3dt_lpips_pack(ctypes.byref(p), ops._ptr(buf), ops._stream()), "n3dt_lpips_pack")
    torch.cuda.synchronize()
    return buf, buf.cpu().numpy()


def call(case, mode, prefill):
    """one n3dt_lpips on a workspace filled with `prefill`: (workspace bytes with TAIL behind them, out [B], layers [5, B])"""
    from n3dt import ops
    from n3dt._lib import LPIPS_INPUT_MODES, check, lib
    B, H, W = ls.CASES[case]
    pred, gt = (torch.from_numpy(a).to(dev()).contiguous() for a in ls.images(case, mode))
    nbytes = lib().n3dt_lpips_workspace_bytes(B, H, W)
    assert nbytes == ls.ws_layout(B, H, W)[2]
    ws = torch.full((nbytes + TAIL,), prefill, dtype=torch.uint8, device=dev())
    res = torch.full((6, B), float("nan"), dtype=torch.float64, device=dev())
    assert ws.data_ptr() % 256 == 0
    check(lib().n3dt_lpips(B, H, W, LPIPS_INPUT_MODES[mode], ops._ptr(packed()[0]), ops._ptr(pred), ops._ptr(gt), ops._ptr(res[0]), ops._ptr(res[1:]),
                           ops._ptr(ws), ctypes.c_size_t(nbytes), ops._stream()), "n3dt_lpips")
    torch.cuda.synchronize()
    res = res.cpu().numpy()
    return ws.cpu().numpy(), res[0], res[1:]


def test_pack_is_held_byte_for_byte():
    total = ls.pack_layout()[4]
    got = packed()[1]
    assert got.size == total + TAIL
    msg = ls.judge_pack(got, ls.weights()[0])
    print("pack: %d bytes, %s" % (total, msg or "every byte as restated, the %d bytes behind the buffer keep the prefill" % TAIL))
    assert msg is None, msg


@pytest.mark.parametrize("case,mode", ls.RUNS)
def test_every_stage_from_its_stored_input(case, mode):
    B, H, W = ls.CASES[case]
    ws, out, layers = call(case, mode, ls.PREFILL)
    worst, fails = ls.judge(case, mode, ws, out, layers)
    print("%s %s, largest error / bound: " % (case, mode) + "  ".join("%s %.3g" % kv for kv in worst.items()))
    assert not fails, "\n" + "\n".join(m for _, m in fails)
    for prefill in (0xFF, 0x00):        # read-before-write: NaN everywhere, then zeros
        ws2, out2, layers2 = call(case, mode, prefill)
        diff = ls.same_results(ws, ws2, B, H, W)
        assert diff is None, "%s %s: %s differs in bits over a 0x%02X prefill" % (case, mode, diff, prefill)
        assert ls.same_bits(out, out2) and ls.same_bits(layers, layers2)
    assert np.isfinite(out).all() and np.isfinite(layers).all()
