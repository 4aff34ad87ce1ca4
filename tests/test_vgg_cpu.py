"""CPU checks of the VGG16 perceptual term (n3dt.perceptual, n3dt_vgg_* of include/n3dt.h): size queries, argument refusal before any
launch, the torchvision key mapping, the weights requirement of HeadNeRFLossUtils, and the tests' own float64 restatement of the
reference's term against the fixture the reference emitted (tests/golden/vgg, tools/gen_golden_vgg.py)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

EINVAL, EWS = -1, -2

# ---- the tests' oracle: the reference's term restated with torch.nn.functional -------------------------------------------------
# Utils/HeadNeRFLossUtils.py:137 (nan_to_num), :148-151 (target = gt with bg_value where mask < 0.5), :44-49 (ImageNet normalisation,
# bilinear resize to 224^2, align_corners=False), :27-30 + :52-58 (vgg16().features[:4], [4:9], [9:16], [16:23] and l1_loss per block)
VGG_BLOCKS = (("c", "c"), ("p", "c", "c"), ("p", "c", "c", "c"), ("p", "c", "c", "c"))


def _bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


def vgg_term_reference(weights, merge, gt, mask, bg_value, round_bf16=False, dtype=torch.float64):
    """(term, [four block terms]) with autograd to `merge`.  weights: the ten (w, b) pairs of n3dt.perceptual.load_vgg16_features.
    round_bf16: round activations and weights to bf16 before every conv (the gradient entering each conv then rounds too) -- the
    emulation of the N3DT_BF16 kernels that sets their tolerance (tools/vgg_bf16_band.py)."""
    x = torch.nan_to_num(merge.to(dtype), nan=0.0)
    y = gt.to(dtype)
    if mask is not None:
        y = torch.where((mask.to(dtype) >= 0.5).expand_as(y), y, torch.full_like(y, bg_value))
    mean = torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1).to(dtype)
    std = torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1).to(dtype)
    x = F.interpolate((x - mean) / std, size=(224, 224), mode="bilinear", align_corners=False)
    y = F.interpolate((y - mean) / std, size=(224, 224), mode="bilinear", align_corners=False)
    q = _bf16 if round_bf16 else (lambda t: t)
    it = iter(weights)
    loss, blocks = 0.0, []
    for ops in VGG_BLOCKS:
        for op in ops:
            if op == "p":
                x, y = F.max_pool2d(x, 2, 2), F.max_pool2d(y, 2, 2)
            else:
                w, b = next(it)
                w, b = q(w.to(dtype)), b.to(dtype)
                x = F.relu(F.conv2d(q(x), w, b, padding=1))
                y = F.relu(F.conv2d(q(y), w, b, padding=1))
        t = F.l1_loss(x, y)
        blocks.append(t)
        loss = loss + t
    return loss, blocks


def fixture_case(g, m, name):
    """(merge with NaNs, gt, bg, mask, bg_value, case manifest) of one case of tests/golden/vgg, float32."""
    case = next(c for c in m["cases"] if c["name"] == name)
    k = name + "."
    merge = torch.from_numpy(g[k + "merge_u8"]).float() / 255.0
    merge.view(-1)[torch.from_numpy(g[k + "nan_idx"])] = float("nan")
    gt = torch.from_numpy(g[k + "gt_u8"]).float() / 255.0
    bg = torch.from_numpy(g[k + "bg_u8"]).float() / 255.0
    mask = torch.from_numpy(g[k + "mask_q"]).float() / 4.0
    return merge, gt, bg, mask, (1.0 if case["bg_type"] == "white" else 0.0), case


def fixture_weights(m):
    from n3dt import synthetic as syn
    from n3dt.perceptual import load_vgg16_features
    sd = syn.vgg16_features_state_dict(m["weights_seed"])
    assert np.allclose(syn.state_dict_checksum(sd), m["weights_checksum"], rtol=1e-9, atol=1e-6), "vgg weight generator drifted"
    return sd, load_vgg16_features(sd)


def d_merge_at(g, name, d):
    """The fixture's d_merge entries and the same entries of a full gradient `d` (flattened)."""
    k = name + "."
    d = d.reshape(-1)
    if k + "d_idx" in g:
        return g[k + "d_merge"].astype(np.float64), d[g[k + "d_idx"]].astype(np.float64)
    return g[k + "d_merge"].reshape(-1).astype(np.float64), d.astype(np.float64)


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------
def test_vgg_size_queries_accept_and_refuse_geometries():
    from n3dt import _lib
    L = _lib.lib()
    for prec in (_lib.F32, _lib.BF16):
        assert L.n3dt_vgg_packed_bytes(prec) > 0
        assert L.n3dt_vgg_saved_bytes(2, prec) > L.n3dt_vgg_saved_bytes(1, prec) > 0
        assert L.n3dt_vgg_workspace_bytes(1, 16, prec) > 0 and L.n3dt_vgg_workspace_bytes(64, 2048, prec) > 0
    # the split-operand mode carries a lo half of every weight matrix
    assert L.n3dt_vgg_packed_bytes(_lib.F32) > L.n3dt_vgg_packed_bytes(_lib.BF16) > 2 * 7_600_000
    for prec in (2, 3, 7):
        assert L.n3dt_vgg_packed_bytes(prec) == 0 and b"precision" in L.n3dt_last_error()
    assert L.n3dt_vgg_saved_bytes(0, _lib.F32) == 0 and b"batch" in L.n3dt_last_error()
    assert L.n3dt_vgg_saved_bytes(65, _lib.F32) == 0 and b"batch" in L.n3dt_last_error()
    assert L.n3dt_vgg_workspace_bytes(1, 15, _lib.BF16) == 0 and b"img_size" in L.n3dt_last_error()
    assert L.n3dt_vgg_workspace_bytes(1, 2049, _lib.BF16) == 0 and b"img_size" in L.n3dt_last_error()


def test_vgg_entry_points_refuse_bad_arguments_before_any_launch():
    """Every n3dt_vgg_* call answers a NULL, an undersized saved buffer or workspace, an img_size out of 16..2048 or a precision other
    than N3DT_F32 / N3DT_BF16 with its error code and a message naming itself -- before the first HIP call (the pointers below are
    never dereferenced)."""
    from n3dt import _lib
    L = _lib.lib()
    P = ctypes.c_void_p(4096)
    vp = _lib.VggParams()
    for i in range(_lib.VGG_CONVS):
        vp.weight[i] = vp.bias[i] = 4096
    B, S, prec = 2, 64, _lib.BF16
    sv, ws = L.n3dt_vgg_saved_bytes(B, prec), L.n3dt_vgg_workspace_bytes(B, S, prec)

    def fwd(b=B, s=S, p=prec, packed=P, merge=P, gt=P, mask=P, terms=P, saved=P, sv_b=sv, w=P, ws_b=ws):
        return L.n3dt_vgg_loss_fwd(b, s, p, packed, merge, gt, mask, ctypes.c_float(1.0), terms, saved, ctypes.c_size_t(sv_b), w,
                                   ctypes.c_size_t(ws_b), None)

    def bwd(b=B, s=S, p=prec, packed=P, merge=P, g=P, saved=P, sv_b=sv, d=P, w=P, ws_b=ws):
        return L.n3dt_vgg_loss_bwd(b, s, p, packed, merge, g, saved, ctypes.c_size_t(sv_b), d, w, ctypes.c_size_t(ws_b), None)

    for call, who in ((fwd, b"n3dt_vgg_loss_fwd"), (bwd, b"n3dt_vgg_loss_bwd")):
        for p in (2, 3):
            assert call(p=p) == EINVAL and b"precision" in L.n3dt_last_error() and who in L.n3dt_last_error()
        for s in (15, 2049):
            assert call(s=s) == EINVAL and b"img_size" in L.n3dt_last_error() and who in L.n3dt_last_error()
        assert call(b=0) == EINVAL and b"batch" in L.n3dt_last_error()
        assert call(packed=None) == EINVAL and b"NULL" in L.n3dt_last_error() and who in L.n3dt_last_error()
        assert call(merge=None) == EINVAL and b"NULL" in L.n3dt_last_error()
        assert call(saved=None) == EINVAL and b"NULL" in L.n3dt_last_error()
        assert call(w=None) == EINVAL and b"NULL" in L.n3dt_last_error()
        assert call(sv_b=sv - 1) == EWS and b"saved buffer too small" in L.n3dt_last_error() and who in L.n3dt_last_error()
        assert call(ws_b=ws - 1) == EWS and b"workspace too small" in L.n3dt_last_error() and who in L.n3dt_last_error()
    for k in ("gt", "terms"):
        assert fwd(**{k: None}) == EINVAL and b"NULL" in L.n3dt_last_error()
    for k in ("g", "d"):
        assert bwd(**{k: None}) == EINVAL and b"NULL" in L.n3dt_last_error()
    # pack: precision, NULLs
    assert L.n3dt_vgg_pack(2, ctypes.byref(vp), P, None) == EINVAL and b"precision" in L.n3dt_last_error()
    assert L.n3dt_vgg_pack(3, ctypes.byref(vp), P, None) == EINVAL and b"precision" in L.n3dt_last_error()
    assert L.n3dt_vgg_pack(prec, None, P, None) == EINVAL and b"n3dt_vgg_pack" in L.n3dt_last_error()
    assert L.n3dt_vgg_pack(prec, ctypes.byref(vp), None, None) == EINVAL and b"NULL" in L.n3dt_last_error()
    vp.bias[4] = None
    assert L.n3dt_vgg_pack(prec, ctypes.byref(vp), P, None) == EINVAL and b"NULL parameter" in L.n3dt_last_error()


# ---- Python ---------------------------------------------------------------------------------------------------------------------
def test_load_vgg16_features_maps_torchvision_keys_and_refuses_bad_ones(tmp_path):
    from n3dt import synthetic as syn
    from n3dt.perceptual import load_vgg16_features, VGG_CONV_INDICES
    sd = syn.vgg16_features_state_dict(3)
    sd["classifier.0.weight"] = torch.zeros(4096, 25088)  # ignored, as are features.24.. (past features[:23])
    pairs = load_vgg16_features(sd)
    assert len(pairs) == 10
    for (w, b), idx in zip(pairs, VGG_CONV_INDICES):
        assert w is not None and torch.equal(w, sd["features.%d.weight" % idx]) and torch.equal(b, sd["features.%d.bias" % idx])
    path = tmp_path / "vgg16.pth"
    torch.save(sd, str(path))
    for (w, b), (w2, b2) in zip(pairs, load_vgg16_features(str(path))):
        assert torch.equal(w, w2) and torch.equal(b, b2)
    bad = dict(sd)
    del bad["features.12.bias"]
    with pytest.raises(KeyError, match="features.12.bias"):
        load_vgg16_features(bad)
    bad = dict(sd)
    bad["features.7.weight"] = torch.zeros(128, 64, 3, 3)
    with pytest.raises(ValueError, match="features.7.weight"):
        load_vgg16_features(bad)
    with pytest.raises(TypeError):
        load_vgg16_features(42)


def test_vgg_loss_without_weights_is_refused():
    from n3dt.train import HeadNeRFLossUtils
    with pytest.raises(NotImplementedError, match="vgg_weights"):
        HeadNeRFLossUtils(bg_type="white", use_vgg_loss=True)
    with pytest.raises(NotImplementedError, match="vgg_weights"):
        HeadNeRFLossUtils(bg_type="black", use_vgg_loss=True, device="cpu")
    assert HeadNeRFLossUtils(bg_type="white", use_vgg_loss=False).vgg_loss_func is None


def test_vgg_loss_object_refuses_style_layers_and_cpu_tensors():
    from n3dt import synthetic as syn
    from n3dt.perceptual import VGGPerceptualLoss
    f = VGGPerceptualLoss(syn.vgg16_features_state_dict(0))
    x = torch.rand(1, 3, 32, 32)
    with pytest.raises(NotImplementedError, match="style"):
        f(x, x, style_layers=[0])
    with pytest.raises(ValueError, match="no CPU fallback"):
        f(x, x)
    with pytest.raises(ValueError):
        VGGPerceptualLoss(syn.vgg16_features_state_dict(0), precision="fp16")


@pytest.mark.parametrize("name", ["a", "b"])
def test_restated_term_equals_the_reference_fixture(golden, name):
    """The tests' float64 restatement of the term (vgg_term_reference) against what the reference's own HeadNeRFLossUtils emitted
    (tools/gen_golden_vgg.py): the four block terms, the `vgg` key, and d(vgg)/d(merge_img) -- the reference's gradient minus the
    three MSE terms' share, which is formed here in float64 as well."""
    g, m = golden("vgg")
    _, weights = fixture_weights(m)
    merge, gt, bg, mask, bgv, case = fixture_case(g, m, name)
    merge = merge.double().requires_grad_(True)
    loss, blocks = vgg_term_reference(weights, merge, gt, mask, bgv)
    k = name + "."
    np.testing.assert_allclose([float(b) for b in blocks], g[k + "blocks"], rtol=1e-10)
    assert case["keys"] == ["bg_loss", "head_loss", "nonhaed_loss", "vgg", "total_loss"]
    np.testing.assert_allclose(float(loss), g[k + "terms"][3], rtol=1e-10)
    # the MSE terms restated (Utils/HeadNeRFLossUtils.py:125-146) so that the total and its gradient can be compared too
    res = torch.nan_to_num(merge, nan=0.0)
    head = (mask.double() >= 0.5).expand(-1, 3, -1, -1)
    bg64 = bg.double()
    t_bg = torch.mean((bg64 - bgv) ** 2)
    t_head = F.mse_loss(res[head], gt.double()[head])
    t_non = torch.mean((res[~head] - bgv) ** 2)
    total = (((0.0 + t_bg) + t_head) + t_non) + loss
    np.testing.assert_allclose([float(t_bg), float(t_head), float(t_non), float(total)], g[k + "terms"][[0, 1, 2, 4]], rtol=1e-10)
    total.backward()
    want, got = d_merge_at(g, name, merge.grad.numpy())
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-6 * np.abs(want).max())
    assert np.all(merge.grad.view(-1)[torch.from_numpy(g[k + "nan_idx"])].numpy() == 0.0)
