"""The head-mask generator on the GPU (n3dt.head_mask over csrc/head_mask.hip) against tests/golden/head_mask*.{npz,json}: the
reference's BiSeNet in float64 (tools/gen_golden_head_mask.py), within 4 x the bounds the generator measured on the CPU with the
restatement's emulation of the kernel's arithmetic; the labels exactly outside the recorded low-margin pixels; the integer
post-process exactly against the restatement; and the bitwise properties of the interface."""
import json
import os

import numpy as np
import pytest
import torch

import head_mask_restatement as hr

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
DEV = "cuda:0"


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(GOLDEN, "head_mask.json")) as f:
        return np.load(os.path.join(GOLDEN, "head_mask.npz")), json.load(f)


@pytest.fixture(scope="module")
def weights():
    from n3dt import synthetic as syn
    return syn.head_mask_state_dict(hr.WEIGHTS_SEED, hr.N_CLASSES)


@pytest.fixture(scope="module")
def net(weights):
    from n3dt import HeadMask
    return HeadMask(weights, n_classes=hr.N_CLASSES, size=None)


@pytest.fixture(scope="module")
def chains(weights):
    """the restatement's float64 chain per small case, computed once"""
    return {case: hr.chain(weights, hr.normalise(hr.fixture_frames(case)).double()) for case in hr.BLOCK_CASES}


def _gpu(v):
    return v.float().to(DEV).contiguous() if torch.is_tensor(v) else v


@pytest.mark.parametrize("case", hr.BLOCK_CASES)
def test_every_block_alone(net, fixture, chains, case):
    _, m = fixture
    ins, outs = chains[case]
    factor, bound = m["bounds"]["gpu_factor"], m["bounds"]["block"]
    worst = []
    for b in range(hr.N_BLOCKS):
        a = ins[b]
        got = net.block(b, _gpu(a["x"]), aux=_gpu(a.get("aux")), scale=_gpu(a.get("scale")), addvec=_gpu(a.get("addvec")), size=a.get("size"))
        err = float((got.double().cpu() - outs[b]).abs().max())
        worst.append((b, err, factor * bound[b]))
    print(case, " ".join("%d:%.2g/%.2g" % w for w in worst))
    bad = [w for w in worst if not w[1] <= w[2]]
    assert not bad, bad


def _check_logits(data, m, case, o, got):
    bound = m["bounds"]["gpu_factor"] * m["bounds"]["logits"][o]
    got = got.double().cpu()
    key = "%s/logits%d/" % (case, o)
    if key + "full" in data.files:
        err = float((got - torch.as_tensor(data[key + "full"])).abs().max())
    else:
        err = float((got.reshape(-1)[::hr.SAMPLE_STRIDE] - torch.as_tensor(data[key + "sample"])).abs().max())
        s, sa = data[key + "sums"]
        assert abs(float(got.abs().sum()) - sa) <= bound * got.numel()
    print("%s logits%d: %.3g (allowed %.3g)" % (case, o, err, bound))
    assert err <= bound


@pytest.mark.parametrize("case", list(hr.CASES))
def test_logits_and_labels(net, fixture, case):
    """the three low-resolution logit maps within 4 x the recorded bound; the labels of output 2 equal to the reference's outside
    the recorded low-margin pixels, which are at most 1 %"""
    data, m = fixture
    n, H, W = hr.CASES[case]
    u8 = hr.fixture_frames(case)
    x = hr.normalise(u8).to(DEV)
    for o in range(3):
        _check_logits(data, m, case, o, net.logits(x, o))
    lab = net.parse(torch.as_tensor(u8).to(DEV)).cpu().numpy()
    ref = hr.unpack_labels(data[case + "/labels_packed"], n * H * W).reshape(n, H, W)
    skip = np.zeros(n * H * W, dtype=bool)
    skip[data[case + "/low_margin"]] = True
    assert skip.mean() <= 0.01
    wrong = (lab != ref).reshape(-1) & ~skip
    print("%s labels: %d pixels skipped of %d, %d differ inside the skipped set" % (case, skip.sum(), skip.size, ((lab != ref).reshape(-1) & skip).sum()))
    assert not wrong.any(), int(wrong.sum())


@pytest.mark.parametrize("case", ["a", "b"])
def test_forward_gives_the_upsampled_maps(net, fixture, case):
    data, m = fixture
    n, H, W = hr.CASES[case]
    x = hr.normalise(hr.fixture_frames(case)).to(DEV)
    outs = net.forward(x)
    for o in range(3):
        want = hr.upsample(torch.as_tensor(data["%s/logits%d/full" % (case, o)]), H, W)
        assert tuple(outs[o].shape) == (n, hr.N_CLASSES, H, W)
        assert float((outs[o].double().cpu() - want).abs().max()) <= m["bounds"]["gpu_factor"] * m["bounds"]["logits"][o]


def test_output_2_does_not_depend_on_the_other_branches(net):
    x = hr.normalise(hr.fixture_frames("b")).to(DEV)
    alone = net.logits(x, 2)
    together = net._run(x, 7, False, None)[2]
    assert torch.equal(alone, together)
    assert torch.equal(net.logits(x, 1), net._run(x, 3, False, None)[1])


# ---- the post-process: hand-made label maps -----------------------------------------------------------------------------------------
def _spiral(H, W):
    """a one-pixel-wide inward spiral: one long chain for the union-find"""
    m = np.zeros((H, W), dtype=np.uint8)
    y, x, dy, dx = 1, 1, 0, 1
    m[y, x] = 1
    while True:
        for _ in range(2):  # straight on, else one turn to the right
            ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if 1 <= ny < H - 1 and 1 <= nx < W - 1 and not m[ny, nx] and not (0 <= ay < H and 0 <= ax < W and m[ay, ax]):
                y, x = ny, nx
                m[y, x] = 1
                break
            dy, dx = dx, -dy
        else:
            return m


def label_maps(H, W):
    maps = {}
    maps["spiral"] = _spiral(H, W)
    d = np.zeros((H, W), dtype=np.uint8)
    d[4:20, 4:20] = 1
    d[20:30, 20:34] = 17            # touches the first block at one corner only
    d[40:44, 40:50] = 2             # a smaller free block
    maps["diagonal"] = d
    t = np.zeros((H, W), dtype=np.uint8)
    t[30:40, 5:15] = 3              # the later block in raster order ...
    t[10:20, 30:40] = 7             # ... and the earlier one, of equal area: the tie
    maps["tie"] = t
    b = np.zeros((H, W), dtype=np.uint8)
    b[H // 2, :] = 1
    b[:, W // 2] = 17
    b[3:8, 3:8] = 10
    maps["borders"] = b
    maps["empty"] = np.full((H, W), 16, dtype=np.uint8)   # a label the LUT sends to 0
    h = np.zeros((H, W), dtype=np.uint8)
    h[8:40, 8:30] = 1
    h[20, 30:44] = 17               # a one-pixel hair bridge the erosion cuts ...
    h[12:30, 44:56] = 13            # ... to a far side the second component pass then drops
    h[0:6, 0:H // 2] = 17           # hair along the border (the zero-border rule)
    h[6:8, 8:20] = 17               # joined to the face
    maps["bridge"] = h
    e = np.zeros((H, W), dtype=np.uint8)
    e[0:H - 4, 0:W - 6] = 1
    e[0:3, 0:3] = 4                 # eyes at two corners: the dilation leaves the map
    e[H - 8:H - 4, W - 10:W - 6] = 5
    e[30:34, 30:36] = 4
    maps["eyes"] = e
    return maps


def label_rgb(H, W, seed):
    rng = np.random.default_rng(seed)
    rgb = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    rgb[10:30, 12:28] = (20, 200, 30)      # green pixels inside the head
    rgb[32:36, 30:40] = (200, 30, 20)
    return rgb


@pytest.mark.parametrize("size", [(64, 64), (96, 80)])
def test_postprocess_is_exact_on_hand_made_maps(net, size):
    H, W = size
    maps = label_maps(H, W)
    names = sorted(maps)
    labels = np.stack([maps[k] for k in names])
    rgb = np.stack([label_rgb(H, W, 5 + i) for i in range(len(names))])
    head, eye = net.postprocess(torch.as_tensor(labels).to(DEV), torch.as_tensor(rgb).to(DEV))
    head, eye = head.cpu().numpy(), eye.cpu().numpy()
    kept = {}
    for i, k in enumerate(names):
        want_head, want_eye = hr.postprocess(labels[i], rgb[i])
        assert np.array_equal(head[i], want_head), k
        assert np.array_equal(eye[i], want_eye), k
        kept[k] = int((want_head != 0).sum())
    # the maps do what they were made for
    assert kept["empty"] == 0 and kept["spiral"] > 0 and kept["eyes"] > 0
    lut = hr.default_lut()
    first = hr.largest_component(lut[maps["tie"]])
    assert first[10:20, 30:40].all() and not first[30:40, 5:15].any()
    assert hr.largest_component(lut[maps["diagonal"]])[20:30, 20:34].all()
    cut = hr.largest_component(hr.erode_hair(hr.largest_component(lut[maps["bridge"]]), 7))
    assert hr.largest_component(lut[maps["bridge"]])[12:30, 44:56].all() and not cut[12:30, 44:56].any()


def test_green_is_exact_on_all_colours(net):
    c = np.arange(1 << 24, dtype=np.uint32)
    rgb = np.stack([(c >> 16) & 255, (c >> 8) & 255, c & 255], axis=1).astype(np.uint8).reshape(1, 4096, 4096, 3)
    got = net.green(torch.as_tensor(rgb).to(DEV)).cpu().numpy()
    want = np.where(hr.green(rgb[0]), 255, 0).astype(np.uint8)
    assert np.array_equal(got[0], want)
    assert 0 < (want != 0).mean() < 0.5


@pytest.mark.parametrize("case", ["a", "c", "real"])
def test_masks_are_the_restatement_of_the_devices_own_labels(net, case):
    """the glue: masks() against the restatement's post-process fed the labels the device parsed"""
    u8 = hr.fixture_frames(case)
    frames = torch.as_tensor(u8).to(DEV)
    lab = net.parse(frames).cpu().numpy()
    head, eye = net.masks(frames)
    assert head.dtype == torch.uint8 and tuple(head.shape) == tuple(lab.shape) and head.is_cuda
    for i in range(lab.shape[0]):
        want_head, want_eye = hr.postprocess(lab[i], u8[i])
        assert np.array_equal(head[i].cpu().numpy(), want_head) and np.array_equal(eye[i].cpu().numpy(), want_eye)
    assert set(np.unique(head.cpu().numpy())) <= {0, 255}


def test_frames_of_another_size_go_through_the_byte_resize(weights):
    """size=64 on 48 x 72 frames: the resize is exact against the restatement, the masks are the restatement of the device's own
    labels at 64 x 64 resized back to the frame's (H, W)"""
    from n3dt import HeadMask
    net64 = HeadMask(weights, n_classes=hr.N_CLASSES, size=64)
    rng = np.random.default_rng(3)
    u8 = rng.integers(0, 256, size=(2, 48, 72, 3), dtype=np.uint8)
    frames = torch.as_tensor(u8).to(DEV)
    small = net64.resize(frames, 64, 64).cpu().numpy()
    lab = net64.parse(frames).cpu().numpy()
    head, eye = net64.masks(frames)
    assert tuple(lab.shape) == (2, 64, 64) and tuple(head.shape) == (2, 48, 72) and tuple(eye.shape) == (2, 48, 72)
    for i in range(2):
        assert np.array_equal(small[i], hr.resize_bytes(u8[i], 64, 64))
        want_head, want_eye = hr.postprocess(lab[i], small[i])
        assert np.array_equal(head[i].cpu().numpy(), hr.resize_bytes(want_head, 48, 72))
        assert np.array_equal(eye[i].cpu().numpy(), hr.resize_bytes(want_eye, 48, 72))
    assert torch.equal(net64.resize(frames, 48, 72), frames)


def test_bitwise_properties(net):
    from n3dt import ops
    u8 = hr.fixture_frames("d")
    frames = torch.as_tensor(u8).to(DEV)
    x = hr.normalise(u8).to(DEV)
    full = net.logits(x, 2)
    head, eye = net.masks(frames)
    # replay
    assert torch.equal(net.logits(x, 2), full)
    # batch position and batch size: 65 = 1 + 3 + 61
    parts = torch.cat([net.logits(x[0:1], 2), net.logits(x[1:4], 2), net.logits(x[4:], 2)])
    assert torch.equal(parts, full)
    assert torch.equal(net.logits(x[7:8], 2), full[7:8])
    # chunking
    assert torch.equal(net.logits(x, 2, chunk=7), full)
    h2, e2 = net.masks(frames, chunk=9)
    assert torch.equal(h2, head) and torch.equal(e2, eye)
    h3, e3 = net.masks(frames[5:6])
    assert torch.equal(h3, head[5:6]) and torch.equal(e3, eye[5:6])
    # the workspaces' contents do not matter
    for buf in ops.WORKSPACE.buf.values():
        buf.fill_(0xFF)
    assert torch.equal(net.logits(x, 2), full)
    h4, e4 = net.masks(frames)
    assert torch.equal(h4, head) and torch.equal(e4, eye)
    # float frames equal their byte frames
    as_float = (frames.permute(0, 3, 1, 2).float() / 255.0).contiguous()
    rgb_f, x_f = net.frames(as_float)
    rgb_b, x_b = net.frames(frames)
    assert torch.equal(rgb_f, rgb_b) and torch.equal(x_f, x_b) and torch.equal(x_b, x)
    h5, e5 = net.masks(as_float)
    assert torch.equal(h5, head) and torch.equal(e5, eye)
