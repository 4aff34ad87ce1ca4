"""The S3FD face detector on the GPU: n3dt.S3FD (n3dt_s3fd_*, csrc/s3fd.hip) against the float64 restatement
(tests/s3fd_restatement.py), which tests/test_s3fd_cpu.py pins to the fixture recorded from the reference's own class and functions
(tests/golden/s3fd*), with the seeded stand-in weights of n3dt.synthetic.s3fd_state_dict.

Tolerances.  The kernels form every convolution from split-bf16 operands with fp32 accumulation.  The fixture's manifest holds, per
block, for the twelve head maps, for the scores and for the box coordinates, the absolute error of the restatement's EMULATION of
that arithmetic against the reference's float64 values, measured on the CPU alone (tools/gen_golden_s3fd.py).  The bounds here are
4 x those figures (the MFMA sums a K block in another order than the emulation), the factor the SyncNet and Wav2Lip pins use.
Blocks are judged one at a time, each fed the restatement's fp32-rounded input for that block, then the chain end to end.  Every
figure is printed before it is judged.  Integer box coordinates are compared exactly, except where the reference's real value
lies within the box bound of an integer: at most 2 % of them, none of a top box.  Everything else is asserted bitwise."""
import numpy as np
import pytest
import torch

import s3fd_restatement as sr

pytestmark = pytest.mark.gpu

GPU_FACTOR = 4.0


def dev():
    return torch.device("cuda:0")


def gpu(a):
    return torch.as_tensor(a).to(dev())


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("s3fd")


@pytest.fixture(scope="module")
def weights(fixture):
    from n3dt import synthetic as syn
    assert fixture[1]["weights_seed"] == sr.WEIGHTS_SEED
    return syn.s3fd_state_dict(sr.WEIGHTS_SEED)


@pytest.fixture(scope="module")
def det(weights):
    from n3dt import S3FD
    return S3FD(weights)


@pytest.fixture(scope="module")
def empty_det():
    from n3dt import S3FD, synthetic as syn
    return S3FD(syn.s3fd_state_dict(sr.WEIGHTS_SEED, syn.S3FD_EMPTY_FACE_BIAS))


@pytest.fixture(scope="module")
def bounds(fixture):
    b = fixture[1]["bounds"]
    assert b["gpu_factor"] == GPU_FACTOR
    return {"block": [GPU_FACTOR * v for v in b["block"]], "heads": [GPU_FACTOR * v for v in b["heads"]], "score": GPU_FACTOR * b["score"],
            "box": GPU_FACTOR * b["box"]}


@pytest.fixture(scope="module")
def chains(fixture, weights):
    """the float64 restatement of cases a, b, c on the bytes the reference read, computed once and pinned to the fixture"""
    from n3dt.s3fd import MEANS
    data, _ = fixture
    out = {}
    for case in ("a", "b", "c"):
        x = torch.as_tensor(data[case + "/frames_u8"]).permute(0, 3, 1, 2).double() - torch.tensor(MEANS, dtype=torch.float64)[None, :, None, None]
        ins, outs = sr.chain(weights, x)
        for k, mp in enumerate(sr.head_maps(outs)):
            assert np.abs(mp.numpy() - data["%s/head%02d" % (case, k)]).max() <= 1e-12
        out[case] = (ins, outs)
    return out


@pytest.fixture(scope="module")
def frames(fixture):
    return {case: gpu(sr.frames_f32(fixture[0][case + "/frames_u8"])) for case in sr.CASES}


@pytest.fixture(scope="module")
def tiny():
    """65 distinct frames of 32 x 32, the smallest legal size (compared bit for bit with themselves)"""
    g = torch.Generator().manual_seed(5)
    return gpu(torch.rand(65, 3, 32, 32, generator=g))


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_every_block_alone_against_the_restatement(det, chains, bounds, case):
    from n3dt.s3fd import block_names
    ins, outs = chains[case]
    worst = []
    for b, name in enumerate(block_names()):
        got = det.block(b, gpu(ins[b].float()))
        assert got.shape == outs[b].shape
        err = float((got.double().cpu() - outs[b]).abs().max())
        print("%s block %2d %-22s %s  max|err| %.3e  bound %.3e" % (case, b, name, tuple(got.shape), err, bounds["block"][b]))
        if not err <= bounds["block"][b]:
            worst.append((b, name, err, bounds["block"][b]))
    assert not worst, worst


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_head_maps_end_to_end(det, fixture, frames, bounds, case):
    data, _ = fixture
    x = gpu(sr.prologue(frames[case].cpu(), torch.float32))
    maps = det.forward(x)
    assert len(maps) == 12
    bad = []
    for k, mp in enumerate(maps):
        want = data["%s/head%02d" % (case, k)]
        assert tuple(mp.shape) == want.shape
        err = float(np.abs(mp.double().cpu().numpy() - want).max())
        print("%s %s%d max|err| %.3e  bound %.3e" % (case, "cls" if k % 2 == 0 else "reg", k // 2 + 1, err, bounds["heads"][k]))
        if not err <= bounds["heads"][k]:
            bad.append((k, err, bounds["heads"][k]))
    assert not bad, bad
    again = det(x)
    assert all(torch.equal(a, b) for a, b in zip(maps, again))


def _compare_detections(data, case, dets, count, bounds, tally):
    ref_dets, ref_count, rects = data[case + "/dets"], data[case + "/count"], data[case + "/rects"]
    assert np.array_equal(count, ref_count), (case, count, ref_count)
    for i in range(len(count)):
        k = int(count[i])
        err = np.abs(dets[i, :k] - ref_dets[i, :k])
        print("%s image %d: %d kept, max|coordinate err| %.3e (bound %.3e), max|score err| %.3e (bound %.3e)"
              % (case, i, k, err[:, :4].max(), bounds["box"], err[:, 4].max(), bounds["score"]))
        assert err[:, :4].max() <= bounds["box"] and err[:, 4].max() <= bounds["score"]
        assert np.all(dets[i, k:] == 0.0) and np.all(np.diff(dets[i, :k, 4]) < 0)
        for j in range(k):
            real = np.clip(ref_dets[i, j, :4], 0, None)
            mine = np.clip(dets[i, j, :4], 0, None).astype(np.int64)
            for c in range(4):
                near = abs(real[c] - round(real[c])) <= bounds["box"] and real[c] > bounds["box"]
                tally["compared"] += 1
                if near:
                    assert j > 0, "a top box's coordinate may not be skipped"
                    tally["skipped"] += 1
                else:
                    assert mine[c] == int(real[c]), (case, i, j, c, mine[c], real[c])
        assert tuple(np.clip(dets[i, 0, :4], 0, None).astype(np.int64)) == tuple(rects[i])


def test_scores_and_detections_against_the_reference(det, fixture, frames, bounds):
    data, m = fixture
    tally = {"compared": 0, "skipped": 0}
    for case in sr.CASES:
        dets, count, score, left = det.detect(frames[case], sr.MAX_FACES, scores=True)
        err = float(np.abs(score.cpu().numpy() - data[case + "/score"]).max())
        print("%s scores max|err| %.3e  bound %.3e" % (case, err, bounds["score"]))
        assert err <= bounds["score"]
        assert int(left.max()) == 0
        _compare_detections(data, case, dets.cpu().numpy(), count.cpu().numpy(), bounds, tally)
        lists = det.detect_from_batch(frames[case])
        assert [len(l) for l in lists] == list(data[case + "/count"]) and all(np.array_equal(l[0], dets[i, 0].cpu().numpy()) for i, l in enumerate(lists))
    print("coordinates compared %d, skipped %d" % (tally["compared"], tally["skipped"]))
    assert tally["skipped"] <= 0.02 * tally["compared"]
    # the cap: the first two of the same descending list, and the number left standing
    dets, count, _, left = det.detect(frames["a"], 2, scores=True)
    full, full_count = det.detect(frames["a"], sr.MAX_FACES)
    assert torch.equal(dets, full[:, :2]) and torch.equal(count, full_count.clamp(max=2))
    assert torch.equal(left > 0, full_count > 2)


def test_clip_boxes_against_the_reference(det, fixture, frames):
    data, m = fixture
    clip = frames["clip"]
    for F_ in m["smooth_cases"]:
        boxes = det.boxes(clip[:F_], pads=m["pads"], smooth=m["smooth"])
        assert boxes.dtype == torch.int32 and boxes.is_cuda
        want = data["clip/smoothed%d" % F_][:, [1, 3, 0, 2]]
        assert np.array_equal(boxes.cpu().numpy(), want), (F_, boxes.cpu().numpy(), want)
        raw = det.boxes(clip[:F_], pads=m["pads"], smooth=0)
        assert np.array_equal(raw.cpu().numpy(), data["clip/padded%d" % F_][:, [1, 3, 0, 2]])
    # the smoothing alone, on boxes that move: the kernel against the restatement the CPU tests pin to the reference's function
    from n3dt import _lib, ops
    g = torch.Generator().manual_seed(3)
    for F_, T in ((1, 5), (2, 5), (4, 5), (5, 5), (6, 5), (300, 5), (7, 1), (9, 64)):
        x1 = torch.randint(0, 40, (F_,), generator=g)
        y1 = torch.randint(0, 30, (F_,), generator=g)
        rect = torch.stack((x1, y1, x1 + torch.randint(5, 50, (F_,), generator=g), y1 + torch.randint(5, 30, (F_,), generator=g)), dim=1)
        dets = torch.cat((rect.double() + 0.75, torch.ones(F_, 1, dtype=torch.float64)), dim=1).reshape(F_, 1, 5)
        count = torch.ones(F_, dtype=torch.int32)
        count[F_ // 2] = 0 if F_ > 2 else 1
        rects = [tuple(int(v) for v in r) if count[i] else None for i, r in enumerate(rect)]
        want, want_found = sr.crop_boxes(rects, 64, 96, (3, 10, -2, 1), T)
        out = torch.empty(F_, 4, dtype=torch.int32, device=dev())
        found = torch.empty(F_, dtype=torch.int32, device=dev())
        scratch = torch.empty(F_, 8, dtype=torch.int32, device=dev())
        d_dets, d_count = gpu(dets), gpu(count)  # held: the call only enqueues
        _lib.check(_lib.lib().n3dt_s3fd_boxes(F_, 64, 96, 1, ops._ptr(d_dets), ops._ptr(d_count), 3, 10, -2, 1, T, ops._ptr(out), ops._ptr(found),
                                              ops._ptr(scratch), ops._stream()), "n3dt_s3fd_boxes")
        assert out.cpu().tolist() == want and found.cpu().tolist() == [int(f) for f in want_found], (F_, T)


def test_bitwise_properties(det, frames, tiny):
    from n3dt import ops
    a = frames["a"]
    dets, count, score, left = det.detect(a, sr.MAX_FACES, scores=True)
    # an image alone equals the same image inside a batch
    for i in range(a.shape[0]):
        d1, c1, s1, _ = det.detect(a[i:i + 1], sr.MAX_FACES, scores=True)
        assert torch.equal(d1[0], dets[i]) and torch.equal(c1[0], count[i]) and torch.equal(s1[0], score[i])
    maps = det.forward(a)
    for i in range(a.shape[0]):
        assert all(torch.equal(m1[0], m[i]) for m1, m in zip(det.forward(a[i:i + 1]), maps))
    # 65 frames of 32 x 32 as one call and as 1 + 3 + 61
    whole = det.detect(tiny, sr.MAX_FACES, scores=True)
    parts = [det.detect(tiny[s:e], sr.MAX_FACES, scores=True) for s, e in ((0, 1), (1, 4), (4, 65))]
    for k in range(4):
        assert torch.equal(whole[k], torch.cat([p[k] for p in parts])), k
    # replay, and a workspace filled with 0xFF: nothing is read before it is written
    for buf in ops.WORKSPACE.buf.values():
        buf.fill_(0xFF)
    again = det.detect(tiny, sr.MAX_FACES, scores=True)
    assert all(torch.equal(x, y) for x, y in zip(whole, again))
    for buf in ops.WORKSPACE.buf.values():
        buf.fill_(0xFF)
    assert all(torch.equal(x, y) for x, y in zip(det.detect(a, sr.MAX_FACES, scores=True), (dets, count, score, left)))
    # boxes() does not depend on the chunking
    clip = frames["clip"]
    assert torch.equal(det.boxes(clip), det.boxes(clip, chunk=2)) and torch.equal(det.boxes(clip), det.boxes(clip, chunk=4))
    b1, f1 = det.boxes(tiny, strict=False)
    b2, f2 = det.boxes(tiny, strict=False, chunk=7)
    assert torch.equal(b1, b2) and torch.equal(f1, f2)


def test_repack_follows_a_weight_update(weights, frames):
    from n3dt import S3FD
    sd = {k: v.clone() for k, v in weights.items()}
    d = S3FD(sd)
    before = d.detect(frames["c"], 4, scores=True)[2]
    original = sd["conv3_3_norm_mbox_conf.bias"].clone()
    sd["conv3_3_norm_mbox_conf.bias"].add_(0.25)
    after = d.detect(frames["c"], 4, scores=True)[2]
    assert not torch.equal(before, after)
    sd["conv3_3_norm_mbox_conf.bias"].copy_(original)
    assert torch.equal(d.detect(frames["c"], 4, scores=True)[2], before)


def test_strict_and_the_empty_case(det, empty_det, fixture, frames):
    data, m = fixture
    fr = frames[m["empty_case"]]
    _, H, W = sr.CASES[m["empty_case"]]
    dets, count, score, left = empty_det.detect(fr, sr.MAX_FACES, scores=True)
    assert float(score.max()) < 0.5 and int(count.max()) == 0 and int(left.max()) == 0 and float(dets.abs().max()) == 0.0
    assert empty_det.detect_from_batch(fr) == [[] for _ in range(fr.shape[0])]
    with pytest.raises(ValueError, match="Face not detected! Ensure the video contains a face in all the frames.*frame 0"):
        empty_det.boxes(fr)
    boxes, found = empty_det.boxes(fr, strict=False)
    assert found.cpu().tolist() == [0] * fr.shape[0] and boxes.cpu().tolist() == [[0, H, 0, W]] * fr.shape[0]
    boxes, found = det.boxes(fr, strict=False)
    assert found.cpu().tolist() == [1] * fr.shape[0] and torch.equal(boxes, det.boxes(fr))


def test_wav2lip_hand_off(det, frames):
    """Wav2LipClip.generate takes the detector's device boxes as they are: the same bits as the same boxes passed as host tuples"""
    from n3dt import Wav2Lip, Wav2LipClip, synthetic as syn
    clip = frames["clip"]
    boxes = det.boxes(clip)
    gen = Wav2LipClip(Wav2Lip(syn.wav2lip_state_dict(1)))
    g = torch.Generator().manual_seed(9)
    mel = gpu(torch.randn(80, 60, generator=g))
    out = gen.generate(clip, boxes, mel, 25.0)
    host = gen.generate(clip, [tuple(b) for b in boxes.cpu().tolist()], mel, 25.0)
    assert out.shape == clip.shape and torch.equal(out, host)
    assert not torch.equal(out, clip)
