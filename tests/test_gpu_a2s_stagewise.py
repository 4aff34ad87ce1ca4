"""The Audio2style encoder's kernels (csrc/audio_lstm.hip: a2s_step_fwd, a2s_step_bwd, the dropout and column-sum kernels, and the
fp32 kernel of gemm32.hip at M = T and at K = T, T - 1 with both operands k-major) pinned one stage at a time from what
n3dt_a2s_fwd / n3dt_a2s_bwd leave in `saved`, their two workspaces and the grad arena -- see tests/a2s_stagewise.py for the
layouts, the comparison rule and the bounds, all of which come from the CPU alone (every bound is 4 x a floor
test_a2s_stagewise_cpu.py re-measures).

One synchronised forward + backward per case through ctypes on this file's own buffers (the forward and the backward get a
workspace each, so XP[l] and DG[l], which share floats, both survive).  Cases:
  t1    T = 1, seeded weights: no recurrent term, the dW_hh memset, M = 1, db equals DG
  t2    T = 2, sharp weights: dW_hh with K = 1
  t5    T = 5, seeded weights, no masks (eval): S = 1 everywhere
  t17   T = 17, sharp: K = 17 is one past a 16-wide staging step, K - 1 = 16 exactly one
  t33   T = 33, seeded: K = 33 and K = 32
  t130  T = 130, sharp: two 128-row tiles with two live rows in the second; K = 130 = 8 x 16 + 2; about 520 short launches"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import a2s_stagewise as a2

pytestmark = pytest.mark.gpu

ALL = list(a2.CASES)
FORWARD = ("X0", "XP", "G[", "C[", "H[", "A[", "S[", "Y[", "out")
HEAD_BWD = ("DZ3", "DY2", "DY1", "DH1", "dW1", "dW2", "dW3", "db1", "db2", "db3")
BPTT = ("DC[", "DG[", "DH0")
LSTM_GRADS = ("dW_ih", "dW_hh", "db_ih", "db_hh")


def dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def run(name, fill=0, repeat=0):
    """-> (inp, rec): one forward + backward of a case; saved, both workspaces and the arena prefilled with the byte `fill`
    (`repeat` only distinguishes cached runs)"""
    from n3dt import _lib
    L = _lib.lib()
    inp = a2.case_inputs(name, 0)
    T = inp["T"]
    saved_bytes, ws_bytes = a2.library_totals(T)
    assert saved_bytes == 4 * a2.saved_layout(T)["total"] and ws_bytes == 4 * a2.ws_layout(T)["total"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev())  # noqa: E731
    keep = {k: [t(a) for a in inp[k]] for k in ("w_ih", "w_hh", "b_ih", "b_hh", "lin_w", "lin_b")}
    p = _lib.A2sParams()
    for f, arr in keep.items():
        for i, x in enumerate(arr):
            getattr(p, f)[i] = x.data_ptr()
    mel, cot = t(inp["mel"]), t(inp["cot"])
    masks = [None] * 3 if inp["masks"] is None else [t(m) for m in inp["masks"]]
    buf = lambda n: torch.full((n,), fill, dtype=torch.uint8, device=dev())  # noqa: E731
    saved, wsf, wsb, arena, out = buf(saved_bytes), buf(ws_bytes), buf(ws_bytes), buf(4 * a2.GRAD_FLOATS), buf(4 * 64 * T)
    ptr = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())  # noqa: E731
    _lib.check(L.n3dt_a2s_fwd(T, ctypes.byref(p), ptr(mel), ptr(masks[0]), ptr(masks[1]), ptr(masks[2]), ptr(out), ptr(saved), saved_bytes,
                              ptr(wsf), ws_bytes, None), "n3dt_a2s_fwd")
    _lib.check(L.n3dt_a2s_bwd(T, ctypes.byref(p), ptr(cot), ptr(saved), saved_bytes, ptr(arena), ptr(wsb), ws_bytes, None), "n3dt_a2s_bwd")
    torch.cuda.synchronize()
    n = lambda x: x.cpu().numpy().view(np.float32)  # noqa: E731
    rec = {"saved": a2.Saved(n(saved), T), "wsf": a2.Workspace(n(wsf), T), "wsb": a2.Workspace(n(wsb), T), "arena": a2.Arena(n(arena)),
           "out": n(out).reshape(T, 64)}
    return inp, rec


@functools.lru_cache(maxsize=None)
def evaluated(name):
    inp, rec = run(name)
    return a2.failures(inp, rec, name, quiet=True)


def check(name, prefixes):
    bad, _, evs = evaluated(name)
    mine = [e for e in evs if e["tag"].startswith(prefixes)]
    assert mine
    worst = {}
    for e in mine:
        a2.report(name, e)
        if not e["exact"]:
            worst[e["family"]] = max(worst.get(e["family"], 0.0), e["ratio"])
    print("%s: largest error per family, in units of its bound: %s" % (name, "  ".join("%s %.3f (%.2e of S, bound %.2e)" % (f, v / a2.bound(f), v, a2.bound(f)) for f, v in sorted(worst.items()))))
    assert [e["tag"] for e in mine if e["bad"]] == []
    return mine


@pytest.mark.parametrize("name", ALL)
def test_forward_stages(name):
    """X0 (bitwise), XP[l][d], the gates, C, H of both layers and directions at every step, A[k], and S[k], Y[k], out (bitwise)."""
    check(name, FORWARD)
    inp, rec = run(name)
    if inp["masks"] is None:
        assert all(np.all(s == 1) for s in rec["saved"].S)


@pytest.mark.parametrize("name", ALL)
def test_head_backward_stages(name):
    """DZ3 (bitwise), DY2 and DY1 with their gates applied in place, DH1, and the head's three dW and db."""
    check(name, HEAD_BWD)


@pytest.mark.parametrize("name", ALL)
def test_bptt_stages(name):
    """DC and the four gate blocks of DG of both layers and directions at every step, teacher-forced from the stored G, C, DG[tn],
    DC[tn] and DH1 / DH0; DH0 as both direction products summed."""
    check(name, BPTT)


@pytest.mark.parametrize("name", ALL)
def test_lstm_gradient_stages(name):
    """dW_ih[k] (K = T), dW_hh[k] (K = T - 1; exactly zero at T = 1), db_ih[k], and db_hh[k] bitwise equal to it."""
    mine = check(name, LSTM_GRADS)
    inp, rec = run(name)
    if inp["T"] == 1:
        assert all(not np.any(w) for w in rec["arena"].W_hh)
        assert all(np.array_equal(rec["arena"].b_ih[2 + d], rec["wsb"].DG[1][d, 0]) for d in range(2))
    else:
        assert all(np.any(w) for w in rec["arena"].W_hh)
    assert len(mine) == 16


@pytest.mark.parametrize("name", ALL)
def test_every_laid_out_float_is_compared(name):
    """The compared entries number exactly N3DT_A2S_GRAD_FLOATS in the arena, every float of `saved`, of the backward's workspace,
    of `out`, and of what the forward uses of its workspace (XP of both layers; the rest of it is the backward's)."""
    inp, _ = run(name)
    _, _, evs = evaluated(name)
    T = inp["T"]
    assert a2.compared_floats(evs) == {"saved": a2.saved_layout(T)["total"], "wsf": 2 * 2 * a2.G * T, "wsb": a2.ws_layout(T)["total"],
                                       "arena": a2.GRAD_FLOATS, "out": 64 * T}


def _bits(rec):
    return [np.ascontiguousarray(x).view(np.uint32) for x in (rec["saved"].buf, rec["wsf"].buf, rec["wsb"].buf, rec["arena"].buf, rec["out"])]


@pytest.mark.parametrize("name", ["t1", "t17"])
def test_two_runs_give_the_same_bits(name):
    (_, a), (_, b) = run(name), run(name, 0, 1)
    for x, y in zip(_bits(a), _bits(b)):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("name", ["t1", "t17"])
def test_a_0xff_prefill_gives_the_bits_of_a_zero_prefill_and_nothing_is_left_unwritten(name):
    """saved, both workspaces, the arena and out prefilled with 0xFF bytes (NaN as floats): every laid-out float is overwritten --
    the forward's workspace beyond XP is not its to write and keeps the prefill -- and the results have the bits of the run over
    zeros, so nothing is accumulated into and nothing read before it is written."""
    (inp, a), (_, b) = run(name), run(name, 0xFF)
    T = inp["T"]
    xp = 2 * 2 * a2.G * T
    for i, (x, y) in enumerate(zip(_bits(a), _bits(b))):
        if i == 1:
            assert np.all(y[xp:] == 0xFFFFFFFF) and np.all(x[xp:] == 0)
            x, y = x[:xp], y[:xp]
        assert np.array_equal(x, y)
    for x in (b["saved"].buf, b["wsf"].buf[:xp], b["wsb"].buf, b["arena"].buf, b["out"]):
        assert np.all(np.isfinite(x))
