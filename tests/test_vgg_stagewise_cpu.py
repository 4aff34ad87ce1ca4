"""CPU checks of the stage-wise restatement of the VGG perceptual term (tests/vgg_stagewise.py): the stages composed against the
tests' float64 oracle and its autograd, the pool arg-max and sign rules against PyTorch, the resize adjoint against autograd of
F.interpolate, the layout helpers against the library's size queries, the refusals of n3dt_vgg_conv_stage, and the floors the GPU
bounds of test_gpu_vgg_stagewise.py are derived from (4 x FLOOR, never a GPU figure)."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vgg_stagewise as vs
from test_vgg_cpu import vgg_term_reference

EINVAL = -1


def torch_weights():
    W, _ = vs.weights()
    return [(torch.from_numpy(w), torch.from_numpy(b)) for w, b in W]


# ---- layout ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2, 3])
def test_layout_helpers_mirror_the_library(B):
    from n3dt import _lib
    L = _lib.lib()
    off, total = vs.saved_offsets(B)
    assert total * 4 == L.n3dt_vgg_saved_bytes(B, _lib.F32) == L.n3dt_vgg_saved_bytes(B, _lib.BF16)
    assert all(o % 64 == 0 for o in off)
    n0 = 2 * B * 226 * 226 * 3
    assert (vs.rup64(n0) + 4 * vs.L1_BLOCKS) * 4 <= L.n3dt_vgg_workspace_bytes(B, 64, _lib.F32)
    if B == 1:
        rng = np.random.RandomState(0)
        maps = [rng.rand(2, vs.SIDE[l], vs.SIDE[l], vs.COUT[l]).astype(np.float32) + 1 for l in range(10)]
        saved = vs.build_saved(maps, B)
        back = vs.saved_maps(saved, B)
        for l in range(10):
            assert vs.halo_is_zero(back[l]) and np.array_equal(vs.interior(back[l]), maps[l])
        assert np.count_nonzero(saved) == sum(m.size for m in maps)   # padding between segments stays zero


# ---- the restatement against the oracle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2])
def test_stages_compose_to_the_reference_and_its_autograd(B):
    """prologue -> ten conv stages -> L1 equals vgg_term_reference in float64 (1e-12 relative), and the gate-forced backward run on
    the restatement's own activations equals autograd's d_merge (1e-12 x max; NaN pixels exactly 0) -- with a mask and NaN pixels."""
    W, _ = vs.weights()
    merge, gt, mask = vs.production_case(B=B, P=64, seed=40 + B, nan=4)
    x = torch.from_numpy(merge).double().requires_grad_(True)
    ref, blocks = vgg_term_reference(torch_weights(), x, torch.from_numpy(gt), torch.from_numpy(mask), 1.0)
    g = 0.37
    (g * ref).backward()
    in0, maps, terms = vs.forward(merge, gt, mask, 1.0, W)
    want = np.array([float(b.detach()) for b in blocks] + [float(ref.detach())])
    assert np.all(np.abs(terms - want) <= 1e-12 * np.abs(want)), (terms, want)
    bw = vs.backward(maps, W, g, merge)
    d, dref = bw["d_merge"], x.grad.numpy()
    err = float(np.abs(d - dref).max())
    print("B=%d: max |d_merge - autograd| = %.3g of max %.3g" % (B, err, np.abs(dref).max()))
    assert err <= 1e-12 * np.abs(dref).max()
    assert np.all(d[np.isnan(merge)] == 0.0) and int(np.isnan(merge).sum()) == 4
    assert set(bw) == {"dz%d" % l for l in range(10)} | {"dpool0", "dpool1", "dpool2", "d_in0", "d_merge"}
    # the same backward from the float32-stored maps and a rebuilt `saved` (what the GPU tests do)
    stored = [vs.interior(p) for p in vs.saved_maps(vs.build_saved(maps, B), B)]
    assert all(np.array_equal(s, m.astype(np.float32)) for s, m in zip(stored, maps))


def test_arg_max_and_sign_rules_match_pytorch():
    """A hand-made map with positive ties in pool windows and x == y entries: route_pool against F.max_pool2d's own arg-max (and its
    autograd), junction's sign against torch.sign."""
    rng = np.random.RandomState(3)
    H = Wd = 16
    C = 8
    k = (np.arange(H // 2)[:, None] * (Wd // 2) + np.arange(Wd // 2)[None, :]) % 8
    pat = vs.TIE_PATTERNS[k].reshape(H // 2, Wd // 2, 2, 2).transpose(0, 2, 1, 3).reshape(H, Wd)
    x = (pat[None, :, :, None] * (1 + np.arange(C) % 3)[None, None, None, :]).astype(np.float64)
    x = np.concatenate([x, np.round(np.maximum(rng.standard_normal((1, H, Wd, C)), 0) * 2) / 2])   # quantised: many ties
    dpool = rng.standard_normal((2, H // 2, Wd // 2, C))
    xt = torch.from_numpy(x).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    pooled, idx = F.max_pool2d(xt, 2, 2, return_indices=True)
    pooled.backward(torch.from_numpy(dpool).permute(0, 3, 1, 2).contiguous())
    got = vs.route_pool(dpool, x)
    assert np.array_equal(got, xt.grad.permute(0, 2, 3, 1).numpy())
    # the indices themselves: first maximum in row-major order
    want = np.zeros((2, C, H * Wd))
    np.put_along_axis(want, idx.reshape(2, C, -1).numpy(), dpool.transpose(0, 3, 1, 2).reshape(2, C, -1), axis=-1)
    assert np.array_equal(got, want.reshape(2, C, H, Wd).transpose(0, 2, 3, 1))
    # every tie pattern puts its gradient on the expected element
    first = [0, 0, 0, 0, 1, 1, 2, 0]
    for p, f in zip(vs.TIE_PATTERNS, first):
        r = vs.route_pool(np.ones((1, 1, 1, 1)), p.reshape(1, 2, 2, 1).astype(np.float64)).reshape(4)
        assert list(r) == [1.0 if i == f else 0.0 for i in range(4)], (p, r)
    # sign: x == y contributes nothing; the ReLU gate kills x == 0
    y = np.where(rng.rand(*x.shape) < 0.5, x, x + rng.choice([-0.5, 0.5], size=x.shape))
    act = np.concatenate([x, y])
    dz = vs.junction(act, None, 0.37, 2)
    want = 0.37 * torch.sign(torch.from_numpy(x - y)).numpy() / x.size * (x > 0)
    assert np.array_equal(dz, want) and np.all(dz[x == y] == 0) and np.any(dz != 0)


@pytest.mark.parametrize("P", vs.RESIZE_SIZES)
def test_resize_adjoint_matches_autograd_of_interpolate(P):
    rng = np.random.RandomState(P)
    d_in0 = rng.standard_normal((1, 224, 224, 3))
    merge = vs.resize_merge(P)
    x = torch.from_numpy(np.nan_to_num(merge)).double().requires_grad_(True)
    std = torch.tensor(vs.STD).double().view(1, 3, 1, 1)      # float32 constants widened, as the reference's
    mean = torch.tensor(vs.MEAN).double().view(1, 3, 1, 1)
    out = F.interpolate((x - mean) / std, size=(224, 224), mode="bilinear", align_corners=False)
    out.backward(torch.from_numpy(d_in0).permute(0, 3, 1, 2))
    want = np.where(np.isfinite(merge), x.grad.numpy(), 0.0)
    got = vs.resize_adjoint(d_in0, merge)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    assert np.all(got[~np.isfinite(merge)] == 0.0)
    A = vs.resize_matrix(P)
    if P == 1000:   # source pixels that no output samples
        dead = ~(A != 0).any(axis=0)
        assert dead.sum() > 300
        assert np.all(got[:, :, dead, :] == 0.0) and np.all(got[:, :, :, dead] == 0.0)
    if P == 224:    # the identity times 1 / std
        assert np.array_equal(A, np.eye(224))
        ident = d_in0.transpose(0, 3, 1, 2) / np.asarray(vs.STD, np.float32).astype(np.float64).reshape(1, 3, 1, 1)
        assert np.array_equal(got, np.where(np.isfinite(merge), ident, 0.0))
    # the prologue is the same matrix: resized = A v A^T
    v = rng.rand(2, 3, P, P)
    assert np.abs(vs._bilinear(v, np.float64) - np.einsum("oy,ncyx,px->nopc", A, v, A, optimize=True)).max() <= 1e-13


# ---- the stage entry ---------------------------------------------------------------------------------------------------------------
def test_vgg_conv_stage_refuses_bad_arguments_before_any_launch():
    """NULLs, layers outside 0..9, precisions other than N3DT_F32 / N3DT_BF16, H or W outside 1..224, n_img outside 1..128, a direction
    or out_pad that is not 0 / 1, a gate on a forward call, misaligned pointers: N3DT_EINVAL and a message naming the entry, before
    the first HIP call (the pointers below are never dereferenced)."""
    from n3dt import _lib
    L = _lib.lib()
    P = ctypes.c_void_p(4096)

    def stage(prec=_lib.BF16, packed=P, layer=3, dgrad=1, n=2, H=5, W=7, x=P, gate=P, out=P, pad=1):
        return L.n3dt_vgg_conv_stage(prec, packed, layer, dgrad, n, H, W, x, gate, out, pad, None)

    def refused(what, **kw):
        assert stage(**kw) == EINVAL, kw
        msg = L.n3dt_last_error()
        assert what in msg and b"n3dt_vgg_conv_stage" in msg, (kw, msg)

    for p in (2, 3, -1):
        refused(b"precision", prec=p)
    for l in (-1, 10, 13):
        refused(b"layer", layer=l)
    for d in (-1, 2):
        refused(b"direction", dgrad=d)
    for n in (0, -3, 129):
        refused(b"n_img", n=n)
    for h in (0, -1, 225):
        refused(b"H, W", H=h)
        refused(b"H, W", W=h)
    refused(b"out_pad", pad=2)
    for k in ("packed", "x", "out"):
        refused(b"NULL", **{k: None})
    refused(b"gate", dgrad=0)                       # a gate goes with dgrad only
    refused(b"16-byte", x=ctypes.c_void_p(4100))
    refused(b"16-byte", gate=ctypes.c_void_p(4104))
    refused(b"256-byte", packed=ctypes.c_void_p(4096 + 64))


def test_conv_stage_wrapper_refuses_wrong_shapes():
    from n3dt.perceptual import VGGPerceptualLoss
    _, sd = vs.weights()
    f = VGGPerceptualLoss(sd)
    with pytest.raises(ValueError, match="layer 3 forward"):
        f.conv_stage(3, torch.zeros(1, 6, 6, 64))       # layer 3 takes 128 channels
    with pytest.raises(ValueError, match="out must be"):
        f.conv_stage(1, torch.zeros(1, 6, 6, 64), out=torch.zeros(1, 4, 4, 32))
    with pytest.raises(ValueError, match="gate must be"):
        f.conv_stage(1, torch.zeros(1, 6, 6, 64), dgrad=True, gate=torch.zeros(1, 4, 4, 3))


# ---- the emulation and the floors ------------------------------------------------------------------------------------------------
def test_emulations_agree_with_each_other_and_with_float64():
    """conv_seq16 and conv_emulated form the same products in two accumulation orders; both sit within 2^-14 of S of float64 in
    fp32 mode (three products of 8-bit halves leave ~2^-16 per term), and within float32 accumulation error of the bf16-rounded
    float64 product in bf16 mode.  The weight matrices are the pack's: forward [tap C_in + ci, co], dgrad flipped and transposed."""
    W, _ = vs.weights()
    for layer, transpose in ((1, False), (2, False), (3, True), (0, True), (0, False)):
        x, gate = vs.stage_case(layer, transpose, (2, 5, 7))
        for prec in vs.PRECISIONS:
            if transpose:
                ref, S = vs.dgrad(x, W[layer][0], None, vs.reference_q(prec))
                a, b = vs.conv_seq16(x, W[layer][0], prec, True), vs.conv_emulated(x, W[layer][0], prec, True)
            else:
                xi = vs.pool2(x) if vs.POOL_IN[layer] else x
                ref = F.conv2d(vs._t(vs.reference_q(prec)(xi.astype(np.float64)), torch.float64),
                               torch.from_numpy(vs.reference_q(prec)(W[layer][0].astype(np.float64))), padding=1)
                ref = vs._n(ref)
                S = vs.conv_stage(x, W[layer][0], 0 * W[layer][1], vs.POOL_IN[layer], vs.reference_q(prec))[1]
                a, b = vs.conv_seq16(xi, W[layer][0], prec), vs.conv_emulated(xi, W[layer][0], prec)
            cap = 2.0 ** -14 if prec == "fp32" else 2.0 ** -19
            for got in (a, b):
                assert vs.ratio(got, ref, S).max() <= cap, (layer, transpose, prec, vs.ratio(got, ref, S).max())
    # dropping the lo products (a bf16-mode result judged as fp32) is far outside 4 x any fp32 floor
    x, _ = vs.stage_case(1, False, (2, 5, 7))
    ref, S = vs.conv_stage(x, W[1][0], W[1][1])
    bad = vs.conv_stage_emulated(x, W[1][0], W[1][1], False, "bf16")
    assert vs.ratio(bad, ref, S).max() > 10 * vs.bound("fp32", "conv_fwd")


@functools.lru_cache(maxsize=None)
def measure_floors():
    """the emulation's largest error under the comparison rule, per precision and stage family, over every case of the GPU tests"""
    W, _ = vs.weights()
    floors = {p: dict.fromkeys(vs.FLOOR[p], 0.0) for p in vs.PRECISIONS}

    def up(prec, fam, v):
        floors[prec][fam] = max(floors[prec][fam], float(v))

    # (a) single stages, the MFMA loop's K order
    for prec in vs.PRECISIONS:
        for geom in vs.STAGE_GEOMETRIES:
            for layer in range(10):
                for transpose in (False, True):
                    ref, S = vs.stage_reference(layer, transpose, geom, prec)
                    up(prec, "conv_dgrad" if transpose else "conv_fwd", vs.ratio(vs.stage_emulated(layer, transpose, geom, prec), ref, S).max())
    # (b) the production forward, teacher-forced on the stored (float32) maps
    P = vs.PRODUCTION
    for B in (1, 2):
        merge, gt, mask = vs.production_case(B=B)
        in0, maps, _ = vs.forward(merge, gt, mask, P["bg"], W)
        stored = [m.astype(np.float32) for m in maps]
        pro = vs.ratio(vs.prologue(merge, gt, mask, P["bg"], np.float32), in0, vs.prologue(merge, gt, mask, P["bg"], mag=True)).max()
        ends = [stored[l] for l in vs.BLOCK_END]
        t64, t32 = vs.l1_terms(ends, B), vs.l1_terms_emulated(ends, B)
        for prec in vs.PRECISIONS:
            up(prec, "prologue", pro)
            up(prec, "terms", (np.abs(t32 - t64) / t64).max())
        if B == 2:
            continue
        x = in0.astype(np.float32)
        for prec in vs.PRECISIONS:
            for l in range(10):
                src = x if l == 0 else stored[l - 1]
                ref, S = vs.conv_stage(src, W[l][0], W[l][1], vs.POOL_IN[l], vs.reference_q(prec))
                got = vs.conv_stage_emulated(src, W[l][0], W[l][1], vs.POOL_IN[l], prec, conv=vs.conv_emulated)
                up(prec, "conv_fwd", vs.ratio(got, ref, S).max())
        # (c), (d) the backward on those maps, gates forced; the resize sweep reuses d_in0
        for prec in vs.PRECISIONS:
            for kind in (None,) + (vs.CRAFTED if prec == "fp32" else ()):
                mp = stored if kind is None else vs.crafted_maps(stored, kind, B)
                ref = vs.backward(mp, W, P["g_total"], merge, vs.reference_q(prec))
                emu = vs.backward_emulated(mp, W, P["g_total"], merge, prec)
                mx, l2, _ = vs.compare_gradient(emu["d_merge"], ref["d_merge"], np.inf, np.inf, "")
                up(prec, "d_merge_max", mx)
                up(prec, "d_merge_l2", l2)
                if kind is None:
                    for size in vs.RESIZE_SIZES:
                        m = vs.resize_merge(size)
                        mx, l2, _ = vs.compare_gradient(vs.resize_adjoint(emu["d_in0"], m, np.float32), vs.resize_adjoint(ref["d_in0"], m),
                                                        np.inf, np.inf, "")
                        up(prec, "d_merge_max", mx)
                        up(prec, "d_merge_l2", l2)
    return floors


def test_floors_have_not_moved_up():
    """FLOOR re-measured.  The GPU bounds are MARGIN x FLOOR (vs.bound); a measured floor above its constant, or a constant more than
    a quarter above what is measured, fails."""
    floors = measure_floors()
    for prec in vs.PRECISIONS:
        print(prec, "  ".join("%s %.3g" % kv for kv in floors[prec].items()))
    for prec in vs.PRECISIONS:
        for fam, v in floors[prec].items():
            c = vs.FLOOR[prec][fam]
            assert v <= c <= 1.25 * v, (prec, fam, v, c)
            assert vs.bound(prec, fam) == 4.0 * c


def test_gpu_bounds_are_the_floors_times_four():
    """the bounds written in the GPU test module are the ones derived from FLOOR, and far below the end-to-end bands they tighten"""
    import test_gpu_vgg_stagewise as g
    assert vs.MARGIN == 4.0
    for prec in vs.PRECISIONS:
        for fam in vs.FLOOR[prec]:
            assert g.BOUND[prec][fam] == vs.MARGIN * vs.FLOOR[prec][fam] > 0.0
    assert g.BOUND["fp32"]["d_merge_max"] < 0.125 / 100 and g.BOUND["bf16"]["d_merge_max"] < 0.39 / 4


def test_crafted_equal_maps_give_exactly_zero():
    """with the target half of every block-end map equal to the prediction half nothing enters the backward"""
    W, _ = vs.weights()
    rng = np.random.RandomState(1)
    maps = [np.maximum(rng.standard_normal((2, vs.SIDE[l], vs.SIDE[l], vs.COUT[l])), 0).astype(np.float32) if l in vs.BLOCK_END or l == 0
            else np.ones((2, vs.SIDE[l], vs.SIDE[l], vs.COUT[l]), np.float32) for l in range(10)]
    bw = vs.backward(vs.crafted_maps(maps, "equal"), W, 0.37, vs.resize_merge(100))
    assert not bw["d_merge"].any() and not bw["d_in0"].any()
