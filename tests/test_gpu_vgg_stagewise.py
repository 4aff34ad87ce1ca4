"""The nine kernels of csrc/vgg_loss.hip pinned stage by stage on the MI355X against the float64 restatement of tests/vgg_stagewise.py
-- see that module for the restatement, the comparison rule (per entry, relative to S = sum |a| |w| + |bias|; the end-to-end
gradient per entry relative to max |ref| and in relative L2) and the floors, which come from the CPU alone
(test_vgg_stagewise_cpu.py).  Every bound is 4 x the floor of its stage family and precision; every comparison is over ALL entries.

The gates, signs and arg-maxes of a backward are read from the `saved` buffer the kernel itself reads, so there is no gate band: the
backward is linear in g and the float64 restatement with the same gates is exact.  In bf16 mode the reference rounds both operands of
every product to bf16 first (forward: activation and weight; backward: incoming gradient and weight).

  (a) n3dt_vgg_conv_stage, all ten layers forward and dgrad, at (n_img, H, W) = (2, 5, 7) (3, 12, 10) (1, 16, 16) (2, 1, 3)
  (b) one n3dt_vgg_loss_fwd (B = 1, P = 64, mask, NaN pixels), teacher-forced: in0 from the workspace, map l from map l - 1 AS STORED,
      the five terms from the stored block ends; halos exactly 0.  B = 2 (fp32): terms and map 9, for the batch offsets
  (c) n3dt_vgg_loss_bwd on that `saved`, g_total = 0.37, then the same `saved` under merge images of P = 16 .. 1000 (the resize adjoint)
  (d) `saved` written by the test (fp32): one block at a time, positive ties in pool windows with x == y entries, scattered live entries
  (e) the stage entry is bit-reproducible and independent of the image's position in the batch

                  fp32 floor   bound      bf16 floor   bound
  prologue        7.5e-6       3.0e-5     7.5e-6       3.0e-5      (float32 arithmetic in both modes)
  conv forward    8.4e-6       3.4e-5     2.6e-7       1.0e-6
  conv dgrad      1.9e-6       7.6e-6     8.4e-8       3.4e-7
  terms           6.7e-8       2.7e-7     6.7e-8       2.7e-7      (float32 sums in both modes)
  d_merge / max   6.8e-5       2.7e-4     4.4e-3       1.8e-2      (the un-forced bands of test_gpu_vgg.py: 0.125 and 0.39)
  d_merge L2      5.7e-5       2.3e-4     4.0e-3       1.6e-2      (1.75e-2 and 0.32)
The largest error / bound seen on the MI355X per family is printed by each test (pytest -s) and recorded in DESIGN 3.10."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import vgg_stagewise as vs

pytestmark = pytest.mark.gpu

BOUND = {prec: {fam: vs.MARGIN * floor for fam, floor in vs.FLOOR[prec].items()} for prec in vs.PRECISIONS}
SENTINEL = 7.25
TAIL = 256


def dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def loss(prec):
    from n3dt.perceptual import VGGPerceptualLoss
    return VGGPerceptualLoss(vs.weights()[1], precision=prec)


def report(tag, worst, bnd):
    print("%-44s largest %.3g  bound %.3g  (%.2f of it)" % (tag, worst, bnd, worst / bnd))


def check(fails):
    assert not fails, "\n" + "\n".join(fails)


# ---- (a), (e): the stage entry ---------------------------------------------------------------------------------------------------
def stage_call(prec, layer, transpose, x, gate=None, out_pad=True):
    """one n3dt_vgg_conv_stage on interior NHWC numpy maps: (result interior, the whole output buffer with halo and tail)"""
    xd = torch.from_numpy(vs.padded(x)).to(dev())
    n, H, Wd = x.shape[:3]
    if not transpose and vs.POOL_IN[layer]:
        H, Wd = H // 2, Wd // 2
    C = vs.CIN[layer] if transpose else vs.COUT[layer]
    shape = (n, H + 2, Wd + 2, C) if out_pad else (n, H, Wd, C)
    numel = int(np.prod(shape))
    buf = torch.full((numel + TAIL,), SENTINEL, dtype=torch.float32, device=dev())
    gd = None
    if gate is not None:   # the gate has the output's layout; its halo is live (1), so a write there would show
        gd = torch.from_numpy(np.pad(gate, ((0, 0), (1, 1), (1, 1), (0, 0)), constant_values=1.0) if out_pad else gate).to(dev()).contiguous()
    loss(prec).conv_stage(layer, xd, dgrad=transpose, gate=gd, out=buf[:numel].view(shape), out_pad=out_pad)
    torch.cuda.synchronize()
    whole = buf.cpu().numpy()
    out = whole[:numel].reshape(shape)
    return (vs.interior(out) if out_pad else out), whole, shape


def untouched(whole, shape, out_pad):
    """the tail behind the output, and the halo of a padded output, still hold the sentinel"""
    numel = int(np.prod(shape))
    ok = bool(np.all(whole[numel:] == SENTINEL))
    if out_pad:
        halo = np.array(whole[:numel].reshape(shape), copy=True)
        halo[:, 1:-1, 1:-1, :] = SENTINEL
        ok = ok and bool(np.all(halo == SENTINEL))
    return ok


@pytest.mark.parametrize("geom", vs.STAGE_GEOMETRIES)
@pytest.mark.parametrize("transpose", [False, True], ids=["forward", "dgrad"])
@pytest.mark.parametrize("prec", vs.PRECISIONS)
def test_conv_stage_matches_the_restatement_at_awkward_geometries(prec, transpose, geom):
    fam = "conv_dgrad" if transpose else "conv_fwd"
    fails, worst = [], 0.0
    for layer in range(10):
        x, gate = vs.stage_case(layer, transpose, geom)
        ref, S = vs.stage_reference(layer, transpose, geom, prec)
        for out_pad in ((True, False) if layer == 0 or not transpose else (True,)):
            tag = "%s layer %d %s (n, H, W) = %s out_pad %d" % (fam, layer, prec, geom, out_pad)
            got, whole, shape = stage_call(prec, layer, transpose, x, gate, out_pad)
            w, msg = vs.compare(got, ref, S, BOUND[prec][fam], tag)
            worst = max(worst, w)
            if msg:
                fails.append(msg)
            if not untouched(whole, shape, out_pad):
                fails.append(tag + ": the halo or the floats behind the output were written")
            if transpose and np.any(got[gate <= 0] != 0.0):
                fails.append(tag + ": an entry whose gate is <= 0 is not exactly 0")
    report("%s %s %s" % (fam, prec, geom), worst, BOUND[prec][fam])
    check(fails)


@pytest.mark.parametrize("prec", vs.PRECISIONS)
def test_conv_stage_is_bit_reproducible_and_batch_position_independent(prec):
    for layer, transpose in ((0, False), (2, False), (5, False), (0, True), (4, True), (9, True)):
        x, gate = vs.stage_case(layer, transpose, (3, 12, 10))
        a, _, _ = stage_call(prec, layer, transpose, x, gate)
        b, _, _ = stage_call(prec, layer, transpose, x, gate)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (layer, transpose, "two calls differ")
        for i in range(3):
            one, _, _ = stage_call(prec, layer, transpose, x[i:i + 1], None if gate is None else gate[i:i + 1])
            assert np.array_equal(one.view(np.uint32), a[i:i + 1].view(np.uint32)), (layer, transpose, "image %d depends on its position" % i)


# ---- (b): the production forward, teacher-forced ---------------------------------------------------------------------------------
def raw_forward(prec, merge, gt, mask, bg):
    """n3dt_vgg_loss_fwd on sentinel-filled buffers: (terms, saved, workspace) as float32 numpy"""
    from n3dt import ops
    from n3dt._lib import lib, check as ck
    f = loss(prec)
    B, _, P, _ = merge.shape
    L = lib()
    sv_b, ws_b = L.n3dt_vgg_saved_bytes(B, f.prec), L.n3dt_vgg_workspace_bytes(B, P, f.prec)
    saved = torch.full((sv_b // 4,), SENTINEL, dtype=torch.float32, device=dev())
    ws = torch.full((ws_b // 4,), SENTINEL, dtype=torch.float32, device=dev())
    terms = torch.empty(5, dtype=torch.float32, device=dev())
    m, g, k = (torch.from_numpy(a).to(dev()).contiguous() for a in (merge, gt, mask))
    ck(L.n3dt_vgg_loss_fwd(B, P, f.prec, ops._ptr(f._packed_for(dev())), ops._ptr(m), ops._ptr(g), ops._ptr(k), ctypes.c_float(bg),
                           ops._ptr(terms), ops._ptr(saved), ctypes.c_size_t(sv_b), ops._ptr(ws), ctypes.c_size_t(ws_b), ops._stream()),
       "n3dt_vgg_loss_fwd")
    torch.cuda.synchronize()
    return terms.cpu().numpy(), saved.cpu().numpy(), ws.cpu().numpy()


def raw_backward(prec, merge, saved, g_total):
    from n3dt import ops
    from n3dt._lib import lib, check as ck
    f = loss(prec)
    B, _, P, _ = merge.shape
    L = lib()
    ws_b = L.n3dt_vgg_workspace_bytes(B, P, f.prec)
    ws = torch.full((ws_b // 4,), SENTINEL, dtype=torch.float32, device=dev())
    sv = torch.from_numpy(np.ascontiguousarray(saved, dtype=np.float32)).to(dev())
    m = torch.from_numpy(merge).to(dev()).contiguous()
    g = torch.tensor([g_total], dtype=torch.float32, device=dev())
    d = torch.full_like(m, SENTINEL)
    ck(L.n3dt_vgg_loss_bwd(B, P, f.prec, ops._ptr(f._packed_for(dev())), ops._ptr(m), ops._ptr(g), ops._ptr(sv), ctypes.c_size_t(sv.numel() * 4),
                           ops._ptr(d), ops._ptr(ws), ctypes.c_size_t(ws_b), ops._stream()), "n3dt_vgg_loss_bwd")
    torch.cuda.synchronize()
    return d.cpu().numpy()


@functools.lru_cache(maxsize=None)
def run(prec, B=1):
    merge, gt, mask = vs.production_case(B=B)
    terms, saved, ws = raw_forward(prec, merge, gt, mask, vs.PRODUCTION["bg"])
    return merge, gt, mask, terms, saved, ws


@functools.lru_cache(maxsize=None)
def stored(prec, B=1):
    return [np.ascontiguousarray(vs.interior(p)) for p in vs.saved_maps(run(prec, B)[4], B)]


@functools.lru_cache(maxsize=None)
def reference_backward(prec):
    """the gate-forced float64 backward on the maps the kernel stored, once per precision"""
    return vs.backward(stored(prec), vs.weights()[0], vs.PRODUCTION["g_total"], run(prec)[0], vs.reference_q(prec))


def check_terms(prec, B, terms, fails):
    ends = [stored(prec, B)[l] for l in vs.BLOCK_END]
    want = vs.l1_terms(ends, B)
    names = ["block term %d" % b for b in range(4)] + ["sum"]
    worst = 0.0
    for nm, got, ref in zip(names, terms, want):
        w, msg = vs.compare(np.array([got]), np.array([ref]), np.array([ref]), BOUND[prec]["terms"], "terms %s B=%d: %s" % (prec, B, nm))
        worst = max(worst, w)
        if msg:
            fails.append(msg)
    report("terms %s B=%d" % (prec, B), worst, BOUND[prec]["terms"])


@pytest.mark.parametrize("prec", vs.PRECISIONS)
def test_production_forward_teacher_forced(prec):
    W = vs.weights()[0]
    merge, gt, mask, terms, saved, ws = run(prec)
    fails = []
    in0, _ = vs.workspace_views(ws, 1)
    ref = vs.prologue(merge, gt, mask, vs.PRODUCTION["bg"])
    w, msg = vs.compare(vs.interior(in0), ref, vs.prologue(merge, gt, mask, vs.PRODUCTION["bg"], mag=True), BOUND[prec]["prologue"], "prologue %s in0" % prec)
    report("prologue %s" % prec, w, BOUND[prec]["prologue"])
    fails += [msg] if msg else []
    if not vs.halo_is_zero(in0):
        fails.append("prologue %s: the halo of in0 is not exactly 0" % prec)
    maps = vs.saved_maps(saved, 1)
    worst = 0.0
    for l in range(10):
        src = vs.interior(in0) if l == 0 else vs.interior(maps[l - 1])
        ref, S = vs.conv_stage(src, W[l][0], W[l][1], vs.POOL_IN[l], vs.reference_q(prec))
        w, msg = vs.compare(vs.interior(maps[l]), ref, S, BOUND[prec]["conv_fwd"], "conv_fwd layer %d %s (production loop, map %d from stored map %d)" % (l, prec, l, l - 1))
        worst = max(worst, w)
        fails += [msg] if msg else []
        if not vs.halo_is_zero(maps[l]):
            fails.append("conv_fwd layer %d %s: the halo of the stored map is not exactly 0" % (l, prec))
    report("conv_fwd %s production" % prec, worst, BOUND[prec]["conv_fwd"])
    check_terms(prec, 1, terms, fails)
    check(fails)


def test_production_forward_batch_offsets():
    """B = 2, fp32: the terms and map 9, which sit behind every B-dependent offset (act_ptr, the target half at B img)"""
    W = vs.weights()[0]
    prec, B = "fp32", 2
    terms = run(prec, B)[3]
    maps = stored(prec, B)
    fails = []
    ref, S = vs.conv_stage(maps[8], W[9][0], W[9][1], False)
    w, msg = vs.compare(maps[9], ref, S, BOUND[prec]["conv_fwd"], "conv_fwd layer 9 fp32 B=2")
    report("conv_fwd fp32 B=2 map 9", w, BOUND[prec]["conv_fwd"])
    fails += [msg] if msg else []
    assert vs.halo_is_zero(vs.saved_maps(run(prec, B)[4], B)[9])
    check_terms(prec, B, terms, fails)
    check(fails)


# ---- (c): the production backward, gates forced ------------------------------------------------------------------------------------
def check_gradient(prec, got, ref, merge, tag, fails):
    mx, l2, msg = vs.compare_gradient(got, ref, BOUND[prec]["d_merge_max"], BOUND[prec]["d_merge_l2"], tag)
    print("%-44s per entry %.3g (bound %.3g)  L2 %.3g (bound %.3g)" % (tag, mx, BOUND[prec]["d_merge_max"], l2, BOUND[prec]["d_merge_l2"]))
    fails += [msg] if msg else []
    if np.any(got[~np.isfinite(merge)] != 0.0):
        fails.append(tag + ": a non-finite pixel of merge has a non-zero gradient")


@pytest.mark.parametrize("prec", vs.PRECISIONS)
def test_production_backward_with_forced_gates(prec):
    merge, saved = run(prec)[0], run(prec)[4]
    ref = reference_backward(prec)
    fails = []
    got = raw_backward(prec, merge, saved, vs.PRODUCTION["g_total"])
    assert int((~np.isfinite(merge)).sum()) == 5 and float(np.abs(ref["d_merge"]).max()) > 0
    check_gradient(prec, got, ref["d_merge"], merge, "d_merge %s B=1 P=64" % prec, fails)
    check(fails)


@pytest.mark.parametrize("P", vs.RESIZE_SIZES)
@pytest.mark.parametrize("prec", vs.PRECISIONS)
def test_resize_backward_across_image_sizes(prec, P):
    """the backward reads merge for its size and finiteness only: the same `saved` under a merge image of another size sweeps
    vgg_resize_bwd_kernel alone (d_in0 of the reference is computed once)"""
    merge = vs.resize_merge(P)
    ref = vs.resize_adjoint(reference_backward(prec)["d_in0"], merge)
    got = raw_backward(prec, merge, run(prec)[4], vs.PRODUCTION["g_total"])
    fails = []
    check_gradient(prec, got, ref, merge, "d_merge %s resize P=%d" % (prec, P), fails)
    if P == 1000:
        dead = ~(vs.resize_matrix(P) != 0).any(axis=0)
        if np.any(got[:, :, dead, :] != 0.0) or np.any(got[:, :, :, dead] != 0.0):
            fails.append("d_merge %s resize P=1000: a source pixel that no output samples is not exactly 0" % prec)
    check(fails)


# ---- (d): `saved` written by the test ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", vs.CRAFTED)
def test_backward_on_crafted_saved(kind):
    prec = "fp32"
    merge = run(prec)[0]
    maps = vs.crafted_maps(stored(prec), kind)
    ref = vs.backward(maps, vs.weights()[0], vs.PRODUCTION["g_total"], merge)
    got = raw_backward(prec, merge, vs.build_saved(maps, 1), vs.PRODUCTION["g_total"])
    fails = []
    assert float(np.abs(ref["d_merge"]).max()) > 0
    check_gradient(prec, got, ref["d_merge"], merge, "d_merge fp32 crafted %s" % kind, fails)
    check(fails)


def test_backward_on_equal_block_ends_is_exactly_zero():
    merge = run("fp32")[0]
    got = raw_backward("fp32", merge, vs.build_saved(vs.crafted_maps(stored("fp32"), "equal"), 1), vs.PRODUCTION["g_total"])
    assert not got.any()
