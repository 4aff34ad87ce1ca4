"""Wav2Lip's generator on the GPU: n3dt.Wav2Lip / n3dt.Wav2LipClip (n3dt_wav2lip_*, csrc/wav2lip.hip) against the float64 restatement
(tests/wav2lip_restatement.py), which tests/test_wav2lip_cpu.py pins to the fixture recorded from the reference's own class
(tests/golden/wav2lip.*), with the seeded stand-in weights of n3dt.synthetic.wav2lip_state_dict.

Tolerances.  The kernels form every convolution from split-bf16 operands with fp32 accumulation.  The fixture's manifest holds, per
block, for the logits and for the image, the absolute error of the restatement's EMULATION of that arithmetic against the
reference's float64 values, measured on the CPU alone (tools/gen_golden_wav2lip.py).  The bounds here are 4 x those figures (the
MFMA sums a K block in another order than the emulation), the factor the SyncNet and LPIPS pins use.  Blocks are judged one at a
time, each fed the restatement's fp32-rounded input for that block, then the chain end to end.  Every figure is printed before
it is judged.  Prologue and paste are float64 interpolations rounded once to fp32: 1e-6 against torch's F.interpolate.
Everything else is asserted bitwise."""
import numpy as np
import pytest
import torch

import wav2lip_restatement as wr

pytestmark = pytest.mark.gpu

GPU_FACTOR = 4.0


def dev():
    return torch.device("cuda:0")


def gpu(a):
    return torch.as_tensor(a).to(dev())


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("wav2lip")


@pytest.fixture(scope="module")
def weights():
    from n3dt import synthetic as syn
    return syn.wav2lip_state_dict(wr.WEIGHTS_SEED)


@pytest.fixture(scope="module")
def net(weights):
    from n3dt import Wav2Lip
    return Wav2Lip(weights)


@pytest.fixture(scope="module")
def bounds(fixture):
    b = fixture[1]["bounds"]
    assert b["gpu_factor"] == GPU_FACTOR
    return {"block": [GPU_FACTOR * v for v in b["block"]], "logits": GPU_FACTOR * b["logits"], "image": GPU_FACTOR * b["image"]}


@pytest.fixture(scope="module")
def three(fixture, weights):
    """the fixture's three windows and their float64 restatement, computed once"""
    data, _ = fixture
    faces, mel = wr.faces_from_u8(data["faces_u8"]), wr.mel_from_u8(data["mel_u8"])
    acts, image = wr.chain64(weights, faces, mel)
    assert np.abs(image.numpy() - data["image"]).max() <= 1e-12  # pinned to the reference's class
    return {"faces": faces, "mel": mel, "acts": acts, "image": image}


@pytest.fixture(scope="module")
def many(three):
    """65 distinct windows on the device (no reference needed: they are compared bit for bit with themselves): the fixture's
    three, shifted and mixed.  65 crosses a 64-row tile on the 1 x 1 maps and, with 9 cells a window, on the 3 x 3 ones."""
    faces, mel = three["faces"].float(), three["mel"].float()
    fs, ms = [], []
    for i in range(65):
        f = torch.roll(faces[i % 3], shifts=i // 3, dims=2) * (0.5 + 0.5 * ((i * 7) % 11) / 10.0)
        f[:3, 48:] = 0.0
        fs.append(f)
        ms.append(torch.roll(mel[(i + 1) % 3], shifts=i // 3, dims=2))
    return gpu(torch.stack(ms)), gpu(torch.stack(fs))


@pytest.mark.parametrize("n", [1, 3])
def test_every_block_alone_against_the_restatement(net, three, bounds, n):
    """Each of the 51 blocks through the single-block entry on the restatement's fp32-rounded input for that block.  n = 1 makes
    M = 1 in the 1 x 1 blocks; n = 3 is the fixture, and a wrong window index shows.  A block that ends in a concatenation gets its
    skip feature: the block's own channels are judged, the rest must be the skip feature bit for bit."""
    from n3dt.wav2lip import SKIP_OF
    inputs = wr.block_inputs(three["acts"], three["faces"], three["mel"])
    worst = []
    for b in range(51):
        x = gpu(inputs[b][:n].float())
        want = three["acts"][b][:n]
        if b in SKIP_OF:
            skip = gpu(three["acts"][SKIP_OF[b]][:n].float())
            both = net.block(b, x, skip)
            assert tuple(both.shape) == (n, want.shape[1] + skip.shape[1]) + tuple(want.shape[2:]), b
            assert torch.equal(both[:, want.shape[1]:], skip), b
            got = both[:, :want.shape[1]]
            assert torch.equal(got, net.block(b, x)), b
        else:
            got = net.block(b, x)
        assert got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape), b
        err = float((got.cpu().double() - want).abs().max())
        print("block %2d n=%d: max |error| %.3e (bound %.3e, max |value| %.3f)" % (b, n, err, bounds["block"][b], float(want.abs().max())))
        worst.append(err / bounds["block"][b])
    assert max(worst) <= 1.0, "block %d" % int(np.argmax(worst))


def test_logits_and_image_end_to_end(net, three, bounds):
    mel, faces = gpu(three["mel"].float()), gpu(three["faces"].float())
    image = net(mel, faces)
    layers = net.layers(mel, faces)
    assert image.dtype == torch.float32 and tuple(image.shape) == (3, 3, 96, 96) and len(layers) == 51
    e_logits = float((layers[-1].cpu().double() - three["acts"][-1]).abs().max())
    e_image = float((image.cpu().double() - three["image"]).abs().max())
    print("n=3: max |error| logits %.3e (bound %.3e), image %.3e (bound %.3e)" % (e_logits, bounds["logits"], e_image, bounds["image"]))
    assert e_logits <= bounds["logits"] and e_image <= bounds["image"]
    assert float(image.min()) <= 0.2 and float(image.max()) >= 0.8  # a sigmoid that is exercised
    # the chained single-block entry holds what the fused call holds: the image is the sigmoid of those logits, rounded once
    assert float((torch.sigmoid(layers[-1].double()) - image.double()).abs().max()) <= 2.0 ** -23
    assert [tuple(x.shape[1:]) for x in layers] == [tuple(x.shape[1:]) for x in three["acts"]]


def test_window_position_replay_and_five_d_are_bitwise(net, three):
    mel, faces = gpu(three["mel"].float()), gpu(three["faces"].float())
    first = net(mel, faces)
    assert torch.equal(first, net(mel, faces))  # replay
    idx = [0, 1, 0]
    moved = net(mel[idx], faces[idx])
    assert torch.equal(moved[0], moved[2]) and torch.equal(moved[0], first[0]) and torch.equal(moved[1], first[1])
    five = net(mel[None], faces.permute(1, 0, 2, 3)[None])  # [1,3,1,80,16], [1,6,3,96,96]
    assert tuple(five.shape) == (1, 3, 3, 96, 96) and torch.equal(five[0].permute(1, 0, 2, 3), first)
    # B = 2, T = 3: the reference's time-major flattening
    a = torch.stack([mel, mel.flip(0)])                                   # [2,3,1,80,16]
    f = torch.stack([faces, faces.flip(0)]).permute(0, 2, 1, 3, 4)         # [2,6,3,96,96]
    out = net(a, f)
    flat = net(torch.cat([a[:, i] for i in range(3)]), torch.cat([f[:, :, i] for i in range(3)]))
    assert tuple(out.shape) == (2, 3, 3, 96, 96) and torch.equal(out, torch.stack(torch.split(flat, 2, dim=0), dim=2))
    assert torch.equal(out[0, :, 1], first[1]) and torch.equal(out[1, :, 0], first[2])


def test_batch_size_independence_and_the_write_once_workspace(net, many):
    """65 windows in one call equal the same windows in calls of 1, 3 and 61, bit for bit; and the result does not change when
    every byte of the workspace is 0xFF (NaNs everywhere) before the call: no kernel reads what no kernel wrote."""
    mel, faces = many
    whole = net(mel, faces)
    assert tuple(whole.shape) == (65, 3, 96, 96) and bool(torch.isfinite(whole).all())
    parts = torch.cat([net(mel[a:b], faces[a:b]) for a, b in ((0, 1), (1, 4), (4, 65))])
    assert torch.equal(whole, parts)
    ws = net._workspace(65, dev())
    ws.fill_(255)
    dirty = net(mel, faces)
    ws.zero_()
    clean = net(mel, faces)
    assert torch.equal(dirty, whole) and torch.equal(clean, whole)
    ws.fill_(255)
    assert torch.equal(net(mel[:3], faces[:3]), whole[:3])
    for b, x in ((32, torch.rand(2, 1024, 1, 1)), (46, torch.rand(2, 160, 48, 48))):  # the transposed blocks' halo and classes too
        x = gpu(x)
        ws.fill_(255)
        dirty = net.block(b, x)
        ws.zero_()
        assert torch.equal(dirty, net.block(b, x)) and bool(torch.isfinite(dirty).all()), b


@pytest.mark.parametrize("b,n", [(49, 128), (1, 65), (16, 65), (34, 65), (50, 65)])
def test_single_block_entry_at_large_n_equals_the_window_alone(net, b, n):
    """The single-block entry lays a block's input out where the chain holds it: for a block that reads a concatenation buffer (1,
    16, 34 and 49, whose [80,98,98] input is larger than either alternating map) in that buffer.  At a batch whose workgroups
    cannot all be resident, a layout that overlapped the output map would be overwritten before it is read: every window must
    equal the same window in a call of its own, bit for bit, with the workspace full of NaNs beforehand."""
    from n3dt.wav2lip import block_shapes
    shape = block_shapes()[b][0]
    g = torch.Generator().manual_seed(100 + b)
    x = gpu(torch.rand((3,) + tuple(shape), generator=g))
    x = x[torch.arange(n, device=x.device) % 3] * (1.0 + (torch.arange(n, device=x.device) // 3)[:, None, None, None].float() / 64.0)
    net._workspace(n, dev()).fill_(255)
    whole = net.block(b, x)
    assert whole.shape[0] == n and bool(torch.isfinite(whole).all())
    for i in (0, n // 2, n - 2, n - 1):
        assert torch.equal(whole[i:i + 1], net.block(b, x[i:i + 1].contiguous())), (b, i)


def test_repack_follows_the_weights_version(weights, three):
    from n3dt import Wav2Lip
    sd = {k: v.clone() for k, v in weights.items()}
    net = Wav2Lip(sd)
    mel, faces = gpu(three["mel"][:1].float()), gpu(three["faces"][:1].float())
    before = net(mel, faces)
    sd["output_block.1.bias"].add_(0.5)  # in place: the version counter moves, the next call packs again
    after = net(mel, faces)
    assert not torch.equal(before, after) and torch.equal(after, Wav2Lip(sd)(mel, faces))


FRAME_BOXES = [(7, 68, 20, 77), (0, 72, 0, 88), (40, 72, 50, 88), (3, 35, 5, 37), (50, 51, 60, 61), (0, 10, 80, 88), (11, 72, 0, 9)]


@pytest.fixture(scope="module")
def clip():
    """7 frames of 72 x 88 with values in [0, 0.5] inside a buffer whose neighbouring frames are all ones: a read outside a frame,
    or outside the box's rows and columns at the frame's edge, would show in the comparison with the restatement"""
    g = torch.Generator().manual_seed(11)
    big = torch.ones(9, 3, 72, 88)
    big[1:8] = torch.rand(7, 3, 72, 88, generator=g) * 0.5
    ref = torch.rand(7, 3, 72, 88, generator=g)
    big = gpu(big)
    return big[1:8], gpu(ref)


def test_face_inputs_against_torchs_interpolate(clip):
    from n3dt.wav2lip import face_inputs
    frames, ref = clip
    assert frames.is_contiguous()
    for boxes, refs in ((FRAME_BOXES, ref), (FRAME_BOXES, None), ((0, 72, 0, 88), ref)):
        got = face_inputs(frames, boxes, refs)
        want = wr.face_inputs(frames.cpu().double(), boxes, None if refs is None else refs.cpu().double())
        assert got.dtype == torch.float32 and tuple(got.shape) == (7, 6, 96, 96)
        assert bool((got[:, :3, 48:] == 0).all()) and float(got[:, :3, :48].abs().max()) > 0.1 and float(got[:, 3:, 48:].abs().max()) > 0.1
        err = float((got.cpu().double() - want).abs().max())
        print("face_inputs: max |error| %.3e" % err)
        assert err <= 1e-6
    # BGR: channel 0 of the target is the frame's blue plane
    whole = face_inputs(frames, (0, 72, 0, 88))
    blue = wr.face_inputs(frames.cpu().double()[:, 2:3].expand(-1, 3, -1, -1), (0, 72, 0, 88))
    assert float((whole[:, 0].cpu().double() - blue[:, 0]).abs().max()) <= 1e-6 and torch.equal(whole[:, :3, :48], whole[:, 3:, :48])
    dirty = frames.clone()
    dirty[0, 0, 3, 3], dirty[1, 1, 4, 4], dirty[2, 2, 5, 5], dirty[3, 0, 6, 6] = float("nan"), -0.5, 1.5, float("inf")
    cleaned = torch.nan_to_num(dirty, nan=0.0, posinf=1.0).clamp(0.0, 1.0)
    assert torch.equal(face_inputs(dirty, FRAME_BOXES), face_inputs(cleaned, FRAME_BOXES))


def test_paste_is_exact_outside_the_box(clip):
    from n3dt.wav2lip import paste
    frames, _ = clip
    g = torch.Generator().manual_seed(12)
    faces = gpu(torch.rand(7, 3, 96, 96, generator=g))
    for boxes in (FRAME_BOXES, (5, 70, 9, 80)):
        got = paste(faces, frames, boxes)
        want = wr.paste(faces.cpu(), frames.cpu(), boxes)
        assert got.dtype == torch.float32 and got.shape == frames.shape
        for i in range(7):
            y1, y2, x1, x2 = wr._box_of(boxes, i)
            mask = torch.ones(72, 88, dtype=torch.bool)
            mask[y1:y2, x1:x2] = False
            assert torch.equal(got[i].cpu()[:, mask], frames[i].cpu()[:, mask]), i  # bit for bit
            err = float((got[i, :, y1:y2, x1:x2].cpu().double() - want[i, :, y1:y2, x1:x2]).abs().max())
            assert err <= 1e-6, (i, err)
    # BGR back to RGB: a face that is its blue plane alone lands in the frame's blue channel
    only_b = torch.zeros_like(faces)
    only_b[:, 0] = 1.0
    out = paste(only_b, frames, (0, 72, 0, 88))
    assert bool((out[:, 2] == 1.0).all()) and bool((out[:, :2] == 0.0).all())


def test_clip_generate_is_prologue_module_and_paste(net, clip):
    from n3dt import Wav2LipClip
    from n3dt.wav2lip import chunk, face_inputs, paste
    frames, ref = clip
    g = torch.Generator().manual_seed(13)
    mel = gpu(torch.rand(80, 30, generator=g) * 8.0 - 4.0)  # 30 columns: frames 5 and 6 take the last 16
    runner = Wav2LipClip(net)
    for refs in (None, ref):
        got = runner.generate(frames, FRAME_BOXES, mel, 25.0, ref_frames=refs)
        windows = torch.stack([chunk(mel, i, 25.0) for i in range(7)])[:, None]
        assert torch.equal(windows, runner.mel_windows(mel, 0, 7, 25.0)) and torch.equal(windows[6], mel[None, :, 14:])
        by_hand = paste(net(windows.contiguous(), face_inputs(frames, FRAME_BOXES, refs)), frames, FRAME_BOXES)
        assert torch.equal(got, by_hand) and bool(torch.isfinite(got).all())
    assert not torch.equal(got, frames)
