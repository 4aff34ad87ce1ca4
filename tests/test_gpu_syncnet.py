"""The lip-sync metric on the GPU: n3dt.SyncNet / n3dt.SyncMeter / train.validate(sync=) (n3dt_syncnet_*, csrc/syncnet.hip) against
the float64 restatement (tests/syncnet_restatement.py), which tests/test_syncnet_cpu.py pins to the fixture recorded from the
reference's own class (tests/golden/syncnet.*), with the seeded stand-in weights of n3dt.synthetic.syncnet_state_dict.

Tolerances.  The kernels form every convolution from split-bf16 operands (hi*hi + hi*lo + lo*hi) with fp32 accumulation.  The
fixture's manifest holds, per block, for the embeddings and for the cosine, the absolute error of the restatement's EMULATION of
that arithmetic against the reference's float64 values, measured on the CPU alone (tools/gen_golden_syncnet.py).  The bounds here
are 4 x those figures (the MFMA sums a K block in another order than the emulation), the factor the LPIPS pin uses.  Blocks are
judged one at a time, each fed the restatement's fp32-rounded input for that block, then the chain end to end.  Every figure is
printed before it is judged.  The prologue and the meter's curve have bounds of their own, reasoned where they are used."""
import math

import numpy as np
import pytest
import torch

import syncnet_restatement as sr

pytestmark = pytest.mark.gpu

GPU_FACTOR = 4.0


def dev():
    return torch.device("cuda:0")


def gpu(a):
    return torch.as_tensor(a).to(dev())


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("syncnet")


@pytest.fixture(scope="module")
def weights():
    from n3dt import synthetic as syn
    return syn.syncnet_state_dict(sr.WEIGHTS_SEED)


@pytest.fixture(scope="module")
def net(weights):
    from n3dt import SyncNet
    return SyncNet(weights)


@pytest.fixture(scope="module")
def bounds(fixture):
    b = fixture[1]["bounds"]
    assert b["gpu_factor"] == GPU_FACTOR
    return {"block": [GPU_FACTOR * v for v in b["block"]], "embedding": GPU_FACTOR * b["embedding"], "cos": GPU_FACTOR * b["cos"]}


@pytest.fixture(scope="module")
def nine(fixture, weights):
    """Nine windows and their float64 restatement, computed once: the fixture's three; the same with frames 0 and 3 of the five
    swapped; the same with the mel window moved by one column (the last column comes round)."""
    data, _ = fixture
    faces, mel = sr.faces_from_u8(data["faces_u8"]), sr.mel_from_u8(data["mel_u8"])
    swapped = faces.clone()
    swapped[:, 0:3], swapped[:, 9:12] = faces[:, 9:12], faces[:, 0:3]
    faces9 = torch.cat([faces, swapped, faces])
    mel9 = torch.cat([mel, mel, torch.roll(mel, -1, dims=3)])
    acts, a, f, cos = sr.chain64(weights, faces9, mel9)
    assert np.abs(cos[:3].numpy() - data["cos"]).max() <= 1e-12  # the first three are the fixture's, pinned to the reference's class
    return {"faces": faces9, "mel": mel9, "acts": acts, "audio": a, "face": f, "cos": cos}


@pytest.mark.parametrize("n", [1, 3])
def test_every_block_alone_against_the_restatement(net, nine, bounds, n):
    """Each of the 31 blocks through the single-block entry on the restatement's fp32-rounded input for that block: no block's
    error hides in or inherits from another's.  n = 1 makes M = 1 in the 1x1 blocks and 9 in the 3x3 ones; n = 3 spans several
    windows, so that a wrong window index shows.  Values are compared, not sign patterns: a ReLU may flip within the bound of 0."""
    inputs = sr.block_inputs(nine["acts"], nine["faces"], nine["mel"])
    worst = []
    for b in range(31):
        x = inputs[b][:n].float()
        got = net.block(b, gpu(x))
        want = nine["acts"][b][:n]
        assert got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape), b
        err = float((got.cpu().double() - want).abs().max())
        print("block %2d n=%d: max |error| %.3e (bound %.3e, max |value| %.3f)" % (b, n, err, bounds["block"][b], float(want.abs().max())))
        worst.append(err / bounds["block"][b])
    assert max(worst) <= 1.0, "block %d" % int(np.argmax(worst))


def run(net, nine, idx):
    mel, faces = gpu(nine["mel"][idx].float()), gpu(nine["faces"][idx].float())
    a, f = net(mel, faces)
    cos = net.cos(mel, faces)
    assert a.dtype == f.dtype == torch.float32 and cos.dtype == torch.float64 and a.shape == f.shape == (len(idx), 512) and cos.shape == (len(idx),)
    return a, f, cos


@pytest.mark.parametrize("n", [1, 3, 9])
def test_embeddings_and_cosine_end_to_end(net, nine, bounds, n):
    idx = list(range(n))
    a, f, cos = run(net, nine, idx)
    ea = float((a.cpu().double() - nine["audio"][idx]).abs().max())
    ef = float((f.cpu().double() - nine["face"][idx]).abs().max())
    ec = float((cos.cpu() - nine["cos"][idx]).abs().max())
    print("n=%d: max |error| audio %.3e, face %.3e (bound %.3e), cos %.3e (bound %.3e)" % (n, ea, ef, bounds["embedding"], ec, bounds["cos"]))
    assert max(ea, ef) <= bounds["embedding"] and ec <= bounds["cos"]
    norms = torch.stack([a.double().norm(dim=1), f.double().norm(dim=1)])
    assert float((norms - 1.0).abs().max()) <= 1e-6  # unit norm, up to the fp32 rounding of 512 entries
    # the chained single-block entry ends in the vectors the fused call normalises
    layers = net.layers(gpu(nine["mel"][idx].float()), gpu(nine["faces"][idx].float()))
    assert len(layers) == 31 and tuple(layers[16].shape) == (n, 512, 1, 1) and tuple(layers[0].shape) == (n, 32, 48, 96)
    for raw, emb in ((layers[16], f), (layers[30], a)):
        raw = raw.reshape(n, 512).double()
        assert float((raw / raw.norm(dim=1, keepdim=True) - emb.double()).abs().max()) <= 2.0 ** -24  # entries <= 0.25, rounded once to fp32


def test_a_changed_input_changes_the_output_far_beyond_the_bound(net, nine, bounds):
    """Two of a window's five frames swapped move the face embedding, a mel window moved by one column moves the audio embedding,
    each by far more than the bound; the other encoder's embedding keeps its bits."""
    a, f, cos = run(net, nine, list(range(9)))
    face_move = float((f[3:6] - f[0:3]).abs().max())
    audio_move = float((a[6:9] - a[0:3]).abs().max())
    want_face = float((nine["face"][3:6] - nine["face"][0:3]).abs().max())
    want_audio = float((nine["audio"][6:9] - nine["audio"][0:3]).abs().max())
    print("frames swapped: face embedding moves %.3e (restatement %.3e); mel shifted: audio embedding moves %.3e (restatement %.3e); bound %.3e"
          % (face_move, want_face, audio_move, want_audio, bounds["embedding"]))
    assert min(face_move, audio_move, want_face, want_audio) >= 100.0 * bounds["embedding"]
    assert float((cos[3:6] - cos[0:3]).abs().min()) >= 10.0 * bounds["cos"] and float((cos[6:9] - cos[0:3]).abs().min()) >= 10.0 * bounds["cos"]
    assert torch.equal(a[3:6], a[0:3]) and torch.equal(f[6:9], f[0:3])


def test_bitwise_properties(net, nine):
    a, f, cos = run(net, nine, list(range(9)))
    again = run(net, nine, list(range(9)))
    assert all(torch.equal(x, y) for x, y in zip((a, f, cos), again))  # two calls
    for k in (0, 4, 8):  # window k of a batch of 9 equals the same window alone
        one = run(net, nine, [k])
        assert torch.equal(one[0][0], a[k]) and torch.equal(one[1][0], f[k]) and torch.equal(one[2][0], cos[k]), k
    order = [5, 0, 8, 2]
    moved = run(net, nine, order)
    assert torch.equal(moved[0], a[order]) and torch.equal(moved[1], f[order]) and torch.equal(moved[2], cos[order])
    # more windows than one launch sequence takes: the same bits again
    from n3dt import syncnet
    many = [i % 9 for i in range(syncnet.MAX_CALL + 5)]
    big = run(net, nine, many)
    assert torch.equal(big[2], cos[many]) and torch.equal(big[1], f[many])


def test_graph_capture_replays_bit_equal(net, nine):
    """One single-stream capture of the whole launch sequence after a first call: nothing synchronises and memory comes from the
    caching allocator.  Default queue settings; nothing about how graphs replay is changed."""
    mel, faces = gpu(nine["mel"][:3].float()), gpu(nine["faces"][:3].float())
    eager = net._run(mel, faces)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = net._run(mel, faces)
    for t in out:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(out, eager))


def test_first_use_on_one_stream_then_a_call_on_another(weights, nine, bounds):
    """The weights are packed (batch norm folded) on the stream of the first call; a call on another stream right after it waits
    for that pack."""
    from n3dt import SyncNet
    fresh = SyncNet(weights)
    mel, faces = gpu(nine["mel"][:3].float()), gpu(nine["faces"][:3].float())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    first = fresh.cos(mel[:1], faces[:1])  # packs on the current stream
    with torch.cuda.stream(side):
        second = fresh.cos(mel, faces)
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(second[:1], first) and float((second.cpu() - nine["cos"][:3]).abs().max()) <= bounds["cos"]
    fresh.repack()
    assert torch.equal(fresh.cos(mel, faces), second)


# ---- the prologue ------------------------------------------------------------------------------------------------------------------
FACE_TOL = 2.0 ** -24  # float64 on the device, rounded once to fp32: half an ulp of a value <= 1 is 2^-25; the rest is float64 order


@pytest.fixture(scope="module")
def frames160():
    g = torch.Generator().manual_seed(11)
    yy, xx = torch.meshgrid(torch.arange(160.0), torch.arange(160.0), indexing="ij")
    out = torch.empty(7, 3, 160, 160)
    for i in range(7):
        for c in range(3):
            p, q, r = torch.rand(3, generator=g).tolist()
            out[i, c] = 0.5 + 0.35 * torch.sin(0.05 * (1 + p) * yy + 0.07 * (1 + q) * xx + 6 * r) + 0.1 * torch.randn(160, 160, generator=g)
    return out.clamp(0.0, 1.0)


def test_face_windows_against_the_restatement(net, frames160):
    """An odd 131 x 117 box, the whole frame, a box touching the frame's corner, one box per frame, a 3x upsampling box"""
    fr = gpu(frames160)
    per_frame = [(7, 138, 20, 137), (0, 160, 0, 160), (100, 160, 90, 160), (1, 33, 2, 34), (159, 160, 0, 160), (0, 97, 63, 160), (5, 6, 7, 8)]
    for boxes in ((7, 138, 20, 137), (0, 160, 0, 160), (100, 160, 90, 160), per_frame):
        got = net.face_windows(fr, boxes)
        want = sr.face_windows(frames160.numpy(), boxes)
        assert got.dtype == torch.float32 and tuple(got.shape) == (3, 15, 48, 96)
        err = float(np.abs(got.cpu().double().numpy() - want).max())
        print("boxes %s: max |error| %.3e (bound %.3e)" % (boxes if len(boxes) == 4 else "per frame", err, FACE_TOL))
        assert err <= FACE_TOL
    one = net.face_windows(fr, (7, 138, 20, 137))
    assert torch.equal(net.face_windows(fr, [(7, 138, 20, 137)] * 7), one)
    assert torch.equal(net.face_windows(fr, torch.tensor([[7, 138, 20, 137]], dtype=torch.int32, device=dev())), one)
    # window i is frames i .. i + 4: the windows of a sub-sequence are the sub-sequence of the windows
    assert torch.equal(net.face_windows(fr[1:6], (7, 138, 20, 137)), one[1:2])


def test_face_windows_strided_frames_and_values_outside_the_unit_range(net, frames160):
    fr = gpu(frames160)
    box = (7, 138, 20, 137)
    first = net.face_windows(fr, box)
    cl = fr.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert not cl.is_contiguous() and torch.equal(net.face_windows(cl, box), first)
    wide = torch.zeros(7, 3, 170, 200, device=dev())
    wide[:, :, 3:163, 11:171] = fr
    assert torch.equal(net.face_windows(wide[:, :, 3:163, 11:171], box), first)
    ex = fr[:1].expand(7, -1, -1, -1)
    assert not ex.is_contiguous() and torch.equal(net.face_windows(ex, box), net.face_windows(fr[[0] * 7], box))
    dirty = frames160.clone()
    dirty[0, 0, 50, 50], dirty[1, 1, 60, 70], dirty[2, 2, 80, 90], dirty[3, 0, 100, 100], dirty[4, 1, 120, 30] = float("nan"), -0.25, 1.75, float("inf"), float("-inf")
    clean = torch.nan_to_num(dirty, nan=0.0, posinf=1.0, neginf=0.0).clamp(0.0, 1.0)
    got = net.face_windows(gpu(dirty), box)
    assert torch.equal(got, net.face_windows(gpu(clean), box)) and not torch.equal(got, first)
    assert float(np.abs(got.cpu().double().numpy() - sr.face_windows(dirty.numpy(), box)).max()) <= FACE_TOL
    # the fused path (frames and boxes straight into the network) gives the bits of the two-step path
    mel = gpu(sr.mel_from_u8(sr.fixture_inputs()[1]).float())
    assert torch.equal(net.cos(mel, frames=fr, boxes=box), net.cos(mel, first))


def test_argument_errors_by_name(net, nine):
    mel, faces = gpu(nine["mel"][:2].float()), gpu(nine["faces"][:2].float())
    fr = torch.rand(6, 3, 40, 40, device=dev())
    for call, what in (
            (lambda: net(mel.cpu(), faces), "mel_windows must be a GPU"), (lambda: net(mel, faces.cpu()), "face_windows must be a GPU"),
            (lambda: net(mel.double(), faces), "mel_windows must be float32"), (lambda: net(mel, faces[:, :14]), "face_windows must be float32 .n,15,48,96"),
            (lambda: net(mel[:, :, :79], faces), "mel_windows must be float32 .n,1,80,16"), (lambda: net(mel, faces[:1]), "differ in windows"),
            (lambda: net.cos(mel), "face_windows or frames"), (lambda: net.cos(mel, faces, frames=fr, boxes=(0, 40, 0, 40)), "face_windows or frames"),
            (lambda: net.cos(mel, frames=fr[:5], boxes=(0, 40, 0, 40)), "2 windows need 6 frames"),
            (lambda: net.face_windows(fr[:4], (0, 40, 0, 40)), "5 consecutive frames"), (lambda: net.face_windows(fr, (0, 41, 0, 40)), "does not lie inside"),
            (lambda: net.face_windows(fr, (5, 5, 0, 40)), "does not lie inside"), (lambda: net.face_windows(fr, [(0, 40, 0, 40)] * 3), "one box or one per frame"),
            (lambda: net.face_windows(fr, (0, 40, 0)), "four integers"), (lambda: net.face_windows(fr[:, :2], (0, 40, 0, 40)), r"float32 .F,3,H,W"),
            (lambda: net.block(31, faces), "0..30"), (lambda: net.block(1, faces), r"x must be float32 .n,32,48,96"),
            (lambda: net.block(0, torch.zeros(1025, 15, 48, 96, device=dev())), "n outside 1..1024")):
        with pytest.raises(ValueError, match=what):
            call()
    assert tuple(net(mel.reshape(2, 80, 16), faces)[0].shape) == (2, 512)  # [n,80,16] is taken as [n,1,80,16]


# ---- the meter ---------------------------------------------------------------------------------------------------------------------
BOX = (4, 36, 2, 38)


@pytest.fixture(scope="module")
def sequence(weights):
    """12 frames of 40 x 40 and a mel spectrogram of 60 columns: 8 windows at 25 fps (starts 0, 3, 6, 9, 12, 16, 19, 22), and their
    float64 restatement from the fp32-rounded face windows the device forms"""
    g = torch.Generator().manual_seed(21)
    yy, xx = torch.meshgrid(torch.arange(40.0), torch.arange(40.0), indexing="ij")
    frames = torch.empty(12, 3, 40, 40)
    for i in range(12):
        for c in range(3):
            p, q, r = torch.rand(3, generator=g).tolist()
            frames[i, c] = 0.5 + 0.4 * torch.sin(0.2 * (1 + p) * yy + 0.3 * (1 + q) * xx + 6 * r + 0.4 * i)
    frames = frames.clamp(0.0, 1.0)
    mel = torch.randint(0, 256, (80, 60), generator=g, dtype=torch.uint8).float() / 32.0 - 4.0
    starts, dropped = sr.meter_starts(12, 60, 25.0)
    assert starts == [0, 3, 6, 9, 12, 16, 19, 22] and dropped == 0
    faces = torch.as_tensor(sr.face_windows(frames.numpy(), BOX)).float().double()
    mels = torch.stack([mel[:, s:s + 16] for s in starts])[:, None].double()
    _, a, f, cos = sr.chain64(weights, faces, mels)
    return {"frames": frames, "mel": mel, "audio": a, "face": f, "cos": cos}


def meter_run(net, sequence, sizes, mel=None, **kw):
    from n3dt import SyncMeter
    meter = SyncMeter(net, gpu(sequence["mel"] if mel is None else mel), fps=25.0, box=BOX, **kw)
    frames, at = gpu(sequence["frames"]), 0
    for size in sizes:
        meter.push(frames[at:at + size])
        at += size
    assert at == 12
    return meter.result()


def test_meter_does_not_depend_on_the_pushes_and_matches_the_restatement(net, sequence, bounds):
    results = [meter_run(net, sequence, sizes, max_shift=2) for sizes in ((1,) * 12, (4, 5, 3), (12,), (0, 7, 0, 5))]
    for r in results[1:]:
        assert r == results[0]  # bit for bit: Python floats from the same doubles
    res = results[0]
    want = sr.meter_result(sequence["cos"].numpy(), sequence["audio"].numpy(), sequence["face"].numpy(), max_shift=2)
    assert res["n_windows"] == 8 and res["n_dropped"] == 0 and sorted(res) == ["curve", "n_dropped", "n_windows", "offset", "sync_conf", "sync_loss"]
    # -log is 1 / cos steep: cos is about 0.3 here, so 4 x its bound covers the loss
    print("sync_conf %.9f (restatement %.9f), sync_loss %.9f (%.9f), bound %.3e" % (res["sync_conf"], want["sync_conf"], res["sync_loss"], want["sync_loss"],
                                                                                   bounds["cos"]))
    assert abs(res["sync_conf"] - want["sync_conf"]) <= bounds["cos"] and abs(res["sync_loss"] - want["sync_loss"]) <= 4.0 * bounds["cos"]
    # a dot product of two unit 512-vectors, each entry off by at most e: |error| <= 2 sqrt(512) e; e = the embedding bound + fp32 rounding
    curve_tol = 2.0 * math.sqrt(512.0) * (bounds["embedding"] + 2.0 ** -24)
    err = max(abs(x - y) for x, y in zip(res["curve"], want["curve"]))
    print("curve %s, restatement %s, max |error| %.3e (bound %.3e)" % (res["curve"], want["curve"], err, curve_tol))
    assert len(res["curve"]) == 5 and err <= curve_tol and abs(res["curve"][2] - res["sync_conf"]) <= curve_tol
    top = sorted(want["curve"])
    if top[-1] - top[-2] > 2.0 * curve_tol:  # the argmax is decided beyond the bound
        assert res["offset"] == want["offset"]
    plain = meter_run(net, sequence, (12,))
    assert sorted(plain) == ["n_dropped", "n_windows", "sync_conf", "sync_loss"] and plain["sync_conf"] == res["sync_conf"] and plain["sync_loss"] == res["sync_loss"]


def test_meter_counts_the_windows_dropped_at_the_mels_end(net, sequence, bounds):
    """36 mel columns: window 7 would read columns 22 .. 37 and is dropped, as the reference's get_segmented_mels gives up there"""
    full = meter_run(net, sequence, (12,))
    res = meter_run(net, sequence, (5, 7), mel=sequence["mel"][:, :36].contiguous())
    assert res["n_windows"] == 7 and res["n_dropped"] == 1 and sr.meter_starts(12, 36, 25.0)[1] == 1
    want = sr.meter_result(sequence["cos"].numpy()[:7])
    assert abs(res["sync_conf"] - want["sync_conf"]) <= bounds["cos"] and res["sync_conf"] != full["sync_conf"]
    none = meter_run(net, sequence, (12,), mel=sequence["mel"][:, :15].contiguous())
    assert none["n_windows"] == 0 and none["n_dropped"] == 8 and math.isnan(none["sync_conf"]) and math.isnan(none["sync_loss"])
    short = meter_run(net, sequence, (12,), mel=sequence["mel"][:, :16].contiguous())
    assert short["n_windows"] == 1 and short["n_dropped"] == 7 and abs(short["sync_conf"] - float(sequence["cos"][0])) <= bounds["cos"]


def test_meter_offset_follows_a_shifted_mel(weights):
    """The meter's pairing of face window i with audio window i + k, on an expert whose embeddings say which window they saw: frame j
    is filled with j / 64 and mel column c with c / 16, the face embedding is one-hot at the window's first frame and the audio
    embedding one-hot at start / 4 (20 fps: the stride is exactly 4 columns).  In sync the curve peaks at 0; with the mel cut by
    one window's stride in front, audio window i is what window i + 1 was, and the peak moves to -1; with a stride of silence put
    in front it moves to +1."""
    from n3dt import SyncMeter, SyncNet

    class Telltale(SyncNet):
        def _run(self, mel_windows, face_windows=None, frames=None, boxes=None):
            n = mel_windows.shape[0]
            a_id = (mel_windows[:, 0, 0, 0] * 16.0 / 4.0).round().long()
            f_id = (frames[:n, 0, 0, 0] * 64.0).round().long()
            a = torch.nn.functional.one_hot(a_id, 512).float()
            f = torch.nn.functional.one_hot(f_id, 512).float()
            return a, f, (a.double() * f.double()).sum(dim=1)

    tell = Telltale(weights)
    # audio id of window i is (20 + 4 i) / 4 = 5 + i: the frames count from 5, so that face id i + 5 is in step
    frames = ((torch.arange(20.0) + 5.0) / 64.0)[:, None, None, None].expand(20, 3, 8, 8).contiguous()
    cols = 20 + torch.arange(100.0)
    mel = (cols / 16.0)[None, :].expand(80, 100).contiguous()

    def offset(m, sizes=(20,)):
        meter = SyncMeter(tell, gpu(m), fps=20.0, max_shift=2)
        at = 0
        for s in sizes:
            meter.push(gpu(frames[at:at + s]))
            at += s
        return meter.result()

    sync = offset(mel)
    assert sync["n_windows"] == 16 and sync["curve"] == [0.0, 0.0, 1.0, 0.0, 0.0] and sync["offset"] == 0 and sync["sync_conf"] == 1.0 and sync["sync_loss"] == 0.0
    early = offset(mel[:, 4:].contiguous(), (3, 9, 8))
    assert early["curve"] == [0.0, 1.0, 0.0, 0.0, 0.0] and early["offset"] == -1 and early["sync_conf"] == 0.0 and early["sync_loss"] == 100.0
    late = offset(torch.cat([mel[:, :4] - 0.25, mel], dim=1).contiguous())
    assert late["curve"] == [0.0, 0.0, 0.0, 1.0, 0.0] and late["offset"] == 1


# ---- validate ----------------------------------------------------------------------------------------------------------------------
RENDER_KEYS = ("shape_code", "appea_code", "batch_Rmats", "batch_Tvecs", "batch_inv_inmats")


@pytest.fixture(scope="module")
def head():
    """The smoke geometry (featmap 8 -> 32 x 32, 32 samples, seed-0 weights with bg_noise 0.1) and four batches of two consecutive
    frames each.  Nothing writes to the net."""
    from n3dt import BaseOptions, HeadNeRFNet, synthetic as syn
    opt = BaseOptions({"featmap_size": 8, "featmap_nc": 256, "pred_img_size": 32, "num_sample_coarse": 32})
    model = HeadNeRFNet(opt, include_vd=False, hier_sampling=False).to(dev())
    model.load_state_dict(syn.make_state_dict(opt, seed=0, bg_noise=0.1), strict=True)
    batches = []
    for i in range(4):
        b = {k: (v.to(dev()) if torch.is_tensor(v) else v) for k, v in syn.frame_inputs(opt, 2, first_frame=2 * i).items()}
        gt, mask = syn.sharp_target(2, 32, seed=4321 + i)
        b["gt_rgb"], b["mask"] = gt.to(dev()), mask.to(dev())
        batches.append(b)
    return model, batches


def test_validate_pushes_every_render_to_the_meter(head, net, sequence):
    """validate(sync=meter): the crop of the 32 x 32 render is upsampled to 96; the three new keys equal pushing the same renders by
    hand, all images of every batch whatever all_images says; still ONE synchronisation; without sync= exactly today's dict."""
    from n3dt import SyncMeter, validate
    from test_gpu_lpips import count_syncs
    model, batches = head
    mel = gpu(sequence["mel"])
    with torch.no_grad():
        imgs = [model("test", b["batch_xy"], b["batch_uv"], b["audiostyle"], bg_code=None, **{k: b[k] for k in RENDER_KEYS})["coarse_dict"]["merge_img"]
                for b in batches]
    by_hand = SyncMeter(net, mel, box=(8, 32, 4, 28))
    for img in imgs:
        by_hand.push(img)
    want = by_hand.result()
    assert want["n_windows"] == 4 and 0.0 < want["sync_conf"] < 1.0
    for all_images in (False, True):
        plain, n_plain = count_syncs(lambda: validate(model, batches, all_images=all_images))
        meter = SyncMeter(net, mel, box=(8, 32, 4, 28))
        res, n_res = count_syncs(lambda: validate(model, batches, all_images=all_images, sync=meter))
        print("all_images=%s: SYNC_conf %.9f, SYNC_loss %.9f, %d windows; synchronisations %d (without sync: %d)"
              % (all_images, res["SYNC_conf"], res["SYNC_loss"], res["SYNC_windows"], n_res, n_plain))
        assert sorted(res) == sorted(list(plain) + ["SYNC_conf", "SYNC_loss", "SYNC_windows"]) and sorted(plain) == ["PSNR", "SSIM", "count"]
        assert {k: res[k] for k in plain} == plain
        assert (res["SYNC_conf"], res["SYNC_loss"], res["SYNC_windows"]) == (want["sync_conf"], want["sync_loss"], 4)
        assert n_res == 1 and n_plain == 1
        assert meter.result() == want  # the meter is the caller's: it holds what validate pushed
