"""The 3-D face reconstruction net on the GPU: n3dt.FaceRecon (n3dt_face_recon_*, csrc/face_recon.hip) against the float64
restatement (tests/face_recon_restatement.py), which tests/test_face_recon_cpu.py pins to the fixture recorded from the reference's
own class and functions and from PIL (tests/golden/face_recon*), with the seeded stand-in weights of
n3dt.synthetic.face_recon_state_dict.

Tolerances.  The kernels form every convolution from split-bf16 operands with fp32 accumulation.  The manifests hold, per block,
for the 257 coefficients and for the expressions end to end from the frames, the absolute error of the restatement's EMULATION of
that arithmetic against the reference's float64 values, measured on the CPU alone (tools/gen_golden_face_recon.py).  The bounds
here are 4 x those figures (the MFMA sums a K block in another order than the emulation), the factor the SyncNet, Wav2Lip and S3FD
pins use.  Blocks are judged one at a time, each fed the restatement's fp32-rounded input (and skip) for that block, then the chain
end to end.  The aligner's byte crops are compared with PIL's bytes: at most 1e-3 of them differ, none by more than one level;
unrounded crops within 4 x the restatement's own measured distance from PIL's bytes / 255; the integers w, h, left, up exactly.
Every figure is printed before it is judged.  Everything else is asserted bitwise."""
import numpy as np
import pytest
import torch

import face_recon_restatement as fr

pytestmark = pytest.mark.gpu

GPU_FACTOR = 4.0
BYTE_CAP = 1e-3


def dev():
    return torch.device("cuda:0")


def gpu(a):
    return torch.as_tensor(a).to(dev())


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("face_recon")


@pytest.fixture(scope="module")
def aligned(golden):
    return golden("face_recon_align")


@pytest.fixture(scope="module")
def weights(fixture):
    from n3dt import synthetic as syn
    assert fixture[1]["weights_seed"] == fr.WEIGHTS_SEED
    return syn.face_recon_state_dict(fr.WEIGHTS_SEED)


@pytest.fixture(scope="module")
def net(weights, aligned):
    from n3dt import FaceRecon
    return FaceRecon(weights, aligned[0]["lm3d_std"])


@pytest.fixture(scope="module")
def bounds(fixture, aligned):
    b, a = fixture[1]["bounds"], aligned[1]["bounds"]
    assert b["gpu_factor"] == GPU_FACTOR == a["gpu_factor"]
    return {"block": [GPU_FACTOR * v for v in b["block"]], "coeffs": GPU_FACTOR * b["coeffs"], "expressions": GPU_FACTOR * a["expressions"],
            "unquantized": GPU_FACTOR * a["unquantized"]}


@pytest.fixture(scope="module")
def chains(fixture, weights):
    """the float64 restatement of the three small cases, computed once and pinned to the fixture's coefficients"""
    data, _ = fixture
    out = {}
    for case in fr.SMALL_CASES:
        ins, skips, outs = fr.chain(weights, fr.fixture_images(case))
        assert np.abs(outs[-1].numpy() - data[case + "/coeffs"]).max() <= 1e-12 * np.abs(data[case + "/coeffs"]).max()
        out[case] = (ins, skips, outs)
    return out


@pytest.fixture(scope="module")
def tiny():
    """65 distinct images of 32 x 32, the smallest legal size (compared bit for bit with themselves)"""
    g = torch.Generator().manual_seed(5)
    return gpu(torch.rand(65, 3, 32, 32, generator=g))


def _landmarks(data, case):
    """the fixture's landmarks as align takes them: (tensor [n,points,2] per group of frames with the same point count, indices)"""
    pts, lm = data[case + "/points"], data[case + "/landmarks"]
    return [(int(p), [i for i in range(len(pts)) if pts[i] == p]) for p in sorted(set(pts.tolist()))], lm


def _align_case(net, data, case, quantize):
    """align on the fixture's frames, the 68- and the 5-point frames in a call each -> crops, trans, status, geom in frame order"""
    frames = gpu(fr.frames_f32(data[case + "/frames_u8"]))
    groups, lm = _landmarks(data, case)
    n = frames.shape[0]
    crops = torch.empty(n, 3, 224, 224, device=dev())
    trans = torch.empty(n, 5, dtype=torch.float64, device=dev())
    status = torch.empty(n, dtype=torch.int32, device=dev())
    geom = torch.empty(n, 4, dtype=torch.int32, device=dev())
    for points, idx in groups:
        c, t, s = net.align(frames[idx], gpu(lm[idx][:, :points]), quantize=quantize)
        crops[idx], trans[idx], status[idx], geom[idx] = c, t, s, net.last_geometry
    return frames, crops, trans, status, geom


@pytest.mark.parametrize("case", fr.SMALL_CASES)
def test_every_block_alone_against_the_restatement(net, chains, bounds, case):
    from n3dt.face_recon import block_names
    ins, skips, outs = chains[case]
    worst = []
    for b, name in enumerate(block_names()):
        got = net.block(b, gpu(ins[b].float()), None if skips[b] is None else gpu(skips[b].float()))
        assert got.shape == outs[b].shape
        err = float((got.double().cpu() - outs[b]).abs().max())
        print("%s block %2d %-34s %s  max|err| %.3e  bound %.3e" % (case, b, name, tuple(got.shape), err, bounds["block"][b]))
        if not err <= bounds["block"][b]:
            worst.append((b, name, err, bounds["block"][b]))
    assert not worst, worst


@pytest.mark.parametrize("case", list(fr.CASES))
def test_coefficients_end_to_end(net, fixture, bounds, case):
    data, _ = fixture
    x = gpu(fr.fixture_images(case).float())
    y = net.forward(x)
    want = data[case + "/coeffs"]
    assert tuple(y.shape) == want.shape == (fr.CASES[case][0], 257)
    err = float(np.abs(y.double().cpu().numpy() - want).max())
    print("%s coefficients max|err| %.3e  bound %.3e  (max |value| %.3g)" % (case, err, bounds["coeffs"], np.abs(want).max()))
    assert err <= bounds["coeffs"]
    assert torch.equal(net(x), y)
    parts = net.coeffs(x)
    assert [tuple(parts[k].shape[1:]) for k in ("id", "exp", "tex", "angle", "gamma", "trans")] == [(80,), (64,), (80,), (3,), (27,), (3,)]
    assert torch.equal(torch.cat([parts[k] for k in ("id", "exp", "tex", "angle", "gamma", "trans")], dim=1), y)


@pytest.mark.parametrize("case", list(fr.ALIGN_CASES))
def test_align_against_pil_and_the_reference(net, aligned, bounds, case):
    data, m = aligned
    ref_status, ref_geom, ref_trans = data[case + "/status"], data[case + "/geom"], data[case + "/trans_params"]
    pil = data[case + "/crops_u8"].astype(np.int64).transpose(0, 3, 1, 2)
    frames, crops, trans, status, geom = _align_case(net, data, case, True)
    _, unrounded, _, _, _ = _align_case(net, data, case, False)
    assert np.array_equal(status.cpu().numpy(), ref_status)
    trans, geom, crops, unrounded = trans.cpu().numpy(), geom.cpu().numpy(), crops.double().cpu().numpy(), unrounded.double().cpu().numpy()
    differing = total = 0
    for i in range(len(ref_status)):
        if ref_status[i]:
            # a frame the reference has no path for: zeros, and the status says so
            assert not crops[i].any() and not unrounded[i].any() and not geom[i].any()
            continue
        rel = np.abs(trans[i] - ref_trans[i]) / np.maximum(np.abs(ref_trans[i]), 1.0)
        print("%s frame %d: trans_params relative error %.3e, geometry %s (reference %s)" % (case, i, rel.max(), geom[i].tolist(), ref_geom[i].tolist()))
        assert rel.max() <= 1e-12
        fallback = float(np.mean(data[case + "/landmarks"][i][:int(data[case + "/points"][i])])) == -1.0
        if fallback:
            # the reference's fallback puts one truncation's argument on an integer (tests/face_recon_restatement.fixture_landmarks):
            # the arguments the manifest names may fall to either side, every other integer is exact
            loose = m["conditions"]["fallback_on_integer"]
            assert np.array_equal(geom[i][:2], ref_geom[i][:2]), (geom[i], ref_geom[i])  # w and h: exact, whatever the manifest names
            for k, name in ((2, "left"), (3, "up")):
                assert geom[i][k] == ref_geom[i][k] or (name in loose and abs(int(geom[i][k]) - int(ref_geom[i][k])) == 1), (name, geom[i], ref_geom[i])
            want_u8 = np.floor(fr.crop(frames[i].cpu().numpy(), tuple(int(v) for v in geom[i]), True) * 255.0 + 0.5).astype(np.int64)
            want_unrounded = None  # the unrounded bound is measured against PIL, which holds the reference's own geometry
            if np.array_equal(geom[i], ref_geom[i]):
                want_u8, want_unrounded = pil[i], pil[i] / 255.0
        else:
            assert np.array_equal(geom[i], ref_geom[i]), (geom[i], ref_geom[i])
            want_u8, want_unrounded = pil[i], pil[i] / 255.0
        got = crops[i] * 255.0
        assert np.abs(got - np.round(got)).max() < 1e-4  # quantize=True gives bytes / 255
        d = np.abs(np.round(got).astype(np.int64) - want_u8)
        assert d.max() <= 1, "a byte differs by more than one level"
        differing, total = differing + int((d != 0).sum()), total + d.size
        if want_unrounded is not None:
            err = float(np.abs(unrounded[i] - want_unrounded).max())
            print("%s frame %d: unrounded crop max|err| %.3e against PIL's bytes / 255, bound %.3e" % (case, i, err, bounds["unquantized"]))
            assert err <= bounds["unquantized"]
    print("%s: %d of %d bytes differ from PIL's" % (case, differing, total))
    assert differing <= BYTE_CAP * total
    # landmarks=None is the fallback for every frame: the -1 frame's result wherever a frame of -1 stands
    n = frames.shape[0]
    c_none, t_none, s_none = net.align(frames)
    c_neg, t_neg, s_neg = net.align(frames, gpu(np.full((n, 68, 2), -1.0)))
    assert torch.equal(c_none, c_neg) and torch.equal(t_none, t_neg) and torch.equal(s_none, s_neg) and int(s_none.max()) == 0


def test_status_frames(net, aligned):
    data, _ = aligned
    frames = gpu(fr.frames_f32(data["p/frames_u8"]))[:1]
    good = gpu(data["p/landmarks"][:1])
    for bad in (good * float("inf"), good * 1e-4, good * 0.0 + 7.0, good * 4000.0):  # non-finite; s above 16; coincident points; s below 1/16
        crops, trans, status = net.align(frames, bad)
        assert int(status[0]) == 1 and not bool(crops.any()) and not bool(net.last_geometry.any()), bad[0, :2]
    crops, trans, status = net.align(frames, good)
    assert int(status[0]) == 0 and bool(crops.any())


def test_expressions_against_the_reference(net, aligned, bounds):
    data, _ = aligned
    for case in fr.ALIGN_CASES:
        frames = gpu(fr.frames_f32(data[case + "/frames_u8"]))
        groups, lm = _landmarks(data, case)
        ok = data[case + "/status"] == 0
        want = data[case + "/coeffs"][:, 80:144]
        got = np.zeros_like(want)
        for points, idx in groups:
            e = net.expressions(frames[idx], gpu(lm[idx][:, :points]))
            assert e.is_cuda and tuple(e.shape) == (len(idx), 64)
            got[idx] = e.double().cpu().numpy()
        err = float(np.abs(got[ok] - want[ok]).max())
        print("%s expressions max|err| %.3e  bound %.3e" % (case, err, bounds["expressions"]))
        assert err <= bounds["expressions"]


def test_bitwise_properties(net, tiny):
    from n3dt import ops
    a = gpu(fr.fixture_images("b").float())
    y = net.forward(a)
    # an image alone equals the same image inside a batch
    for i in range(a.shape[0]):
        assert torch.equal(net.forward(a[i:i + 1])[0], y[i])
    # 65 images of 32 x 32 as one call and as 1 + 3 + 61, and chunked
    whole = net.forward(tiny)
    parts = [net.forward(tiny[s:e]) for s, e in ((0, 1), (1, 4), (4, 65))]
    assert torch.equal(whole, torch.cat(parts))
    assert torch.equal(whole, net.forward(tiny, chunk=7)) and torch.equal(whole, net.forward(tiny, chunk=64))
    # replay, and a workspace filled with 0xFF: nothing is read before it is written
    for buf in ops.WORKSPACE.buf.values():
        buf.fill_(0xFF)
    assert torch.equal(net.forward(tiny), whole)
    for buf in ops.WORKSPACE.buf.values():
        buf.fill_(0xFF)
    assert torch.equal(net.forward(a), y)
    # the aligner: a frame alone equals the frame inside a batch, and a replay
    frames = torch.rand(4, 3, 48, 40, generator=torch.Generator().manual_seed(2)).to(dev())
    lm = gpu(np.random.default_rng(4).uniform(8.0, 36.0, size=(4, 5, 2)))
    crops, trans, status = net.align(frames, lm)
    again = net.align(frames, lm)
    assert torch.equal(crops, again[0]) and torch.equal(trans, again[1]) and torch.equal(status, again[2])
    for i in range(4):
        c1, t1, s1 = net.align(frames[i:i + 1], lm[i:i + 1])
        assert torch.equal(c1[0], crops[i]) and torch.equal(t1[0], trans[i]) and torch.equal(s1[0], status[i])


def test_repack_follows_a_weight_update(weights, aligned, tiny):
    from n3dt import FaceRecon
    sd = {k: v.clone() for k, v in weights.items()}
    net = FaceRecon(sd, aligned[0]["lm3d_std"])
    before = net.forward(tiny[:2])
    original = sd["backbone.layer3.2.bn2.running_var"].clone()
    sd["backbone.layer3.2.bn2.running_var"].mul_(1.5)
    after = net.forward(tiny[:2])
    assert not torch.equal(before, after)
    sd["backbone.layer3.2.bn2.running_var"].copy_(original)
    assert torch.equal(net.forward(tiny[:2]), before)
    sd["final_layers.1.bias"].add_(0.25)
    moved = net.forward(tiny[:2])
    assert torch.equal(moved[:, :80], before[:, :80]) and torch.equal(moved[:, 144:], before[:, 144:]) and not torch.equal(moved[:, 80:144], before[:, 80:144])


def test_strict_load_refusals(weights, aligned, tiny):
    from n3dt import FaceRecon, load_face_recon
    lm3d = aligned[0]["lm3d_std"]
    with pytest.raises(KeyError):
        FaceRecon({k: v for k, v in weights.items() if k != "backbone.layer4.0.downsample.1.running_mean"}, lm3d)
    with pytest.raises(KeyError):
        FaceRecon(dict(weights, **{"backbone.fc.weight": torch.zeros(257, 2048)}), lm3d)
    with pytest.raises(ValueError):
        FaceRecon(dict(weights, **{"final_layers.1.weight": torch.zeros(64, 2048)}), lm3d)
    with pytest.raises(ValueError):
        FaceRecon(weights, np.zeros((5, 2)))
    # num_batches_tracked may be absent; a checkpoint holding the state dict under 'net_recon' is unwrapped
    bare = {k: v for k, v in weights.items() if not k.endswith("num_batches_tracked")}
    assert len(load_face_recon({"net_recon": bare})[0]) == 53
    assert torch.equal(FaceRecon({"net_recon": bare}, lm3d).forward(tiny[:1]), FaceRecon(weights, lm3d).forward(tiny[:1]))
    net = FaceRecon(weights, lm3d)
    with pytest.raises(ValueError):
        net.forward(tiny.cpu())
    with pytest.raises(ValueError):
        net.forward(tiny[:, :, :31])
    with pytest.raises(ValueError):
        net.align(tiny, torch.zeros(65, 68, 2))  # landmarks on the CPU
    with pytest.raises(ValueError):
        net.block(3, tiny[:1, :, :8, :8].repeat(1, 64, 1, 1)[:, :64])  # a third convolution without its skip


def test_wav2lip_hand_off(net):
    """frames shaped like Wav2LipClip.generate's output go in unchanged, [F,64] comes out on the device"""
    from n3dt import Wav2Lip, Wav2LipClip, synthetic as syn
    g = torch.Generator().manual_seed(9)
    clip = gpu(torch.rand(5, 3, 64, 96, generator=g))
    boxes = [(8, 56, 20, 76)] * 5
    mel = gpu(torch.randn(80, 60, generator=g))
    out = Wav2LipClip(Wav2Lip(syn.wav2lip_state_dict(1))).generate(clip, boxes, mel, 25.0)
    assert out.shape == clip.shape and out.dtype == torch.float32 and out.is_cuda
    lm = gpu(np.random.default_rng(6).uniform(20.0, 60.0, size=(5, 68, 2)))
    exp = net.expressions(out, lm)
    assert exp.is_cuda and tuple(exp.shape) == (5, 64) and bool(torch.isfinite(exp).all())
    assert torch.equal(exp, net.expressions(out, lm))
    crops, _, status = net.align(out, lm)
    assert torch.equal(exp, net.forward(crops)[:, 80:144]) and int(status.max()) == 0
