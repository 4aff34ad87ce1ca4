"""The AWing FAN landmark detector on the GPU (n3dt.FAN, csrc/fan.hip) against the float64 restatement
(tests/fan_restatement.py), which tests/test_fan_cpu.py holds to the fixture recorded from the reference's own classes.  Bounds:
the manifest's CPU-measured emulation errors times 4 (tools/gen_golden_fan.py), per block alone on that block's fp32 input and per
heat map end to end.  The decode, the glue and every bitwise property are exact.  Every figure is printed before it is judged."""
import numpy as np
import pytest
import torch

import fan_restatement as fr
from test_fan_cpu import ref_gates, weights

pytestmark = pytest.mark.gpu
F = fr.GPU_FACTOR


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("fan")


@pytest.fixture(scope="module")
def nets():
    from n3dt import FAN
    return {M: FAN(weights(M), num_modules=M) for M in (1, 2, 4)}


@pytest.fixture(scope="module")
def chains(fixture):
    """{case: (heat maps, record)}: the float64 restatement with the reference's gates forced, once"""
    data, _ = fixture
    out = {}
    for case, (M, N, n) in fr.CASES.items():
        rec = {}
        heats, _ = fr.forward(weights(M, N), fr.fixture_images(case), M, N, gates=ref_gates(data, case), record=rec)
        out[case] = (heats, rec)
    return out


def on_dev(t, dtype=torch.float32):
    return None if t is None else t.to(dtype).to(dev())


def test_every_block_alone_at_the_chain_sizes(fixture, nets, chains):
    """every block of the two-stack chain on that block's fp32 input, with its skip and the reference's gates supplied"""
    _, m = fixture
    M, N, n = fr.CASES["m2"]
    sd, rec = weights(M), chains["m2"][1]
    assert sorted(rec) == sorted(b for b in nets[M].block_names() if b not in ("avg_pool", "upsample_add"))
    worst = 0.0
    for name, (xin, skip, gate, _) in rec.items():
        x32, s32 = xin.float(), None if skip is None else skip.float()
        want = fr.run_block(sd, name, x32, s32, gate)
        got = nets[M].block(name, x32.to(dev()), skip=on_dev(s32), gates=on_dev(gate, torch.uint8)).double().cpu()
        err, bound = float((got - want).abs().max()), F * m["bounds"]["block"]["m2/" + name]
        print("%-14s err %.3e bound %.3e" % (name, err, bound))
        worst = max(worst, err / bound)
        assert got.shape == want.shape and err <= bound, name
    print("worst err / bound %.3f" % worst)


def test_convblocks_pool_and_upsample_on_small_maps(fixture, nets):
    """n = 3 on 12 x 10 (120 rows: a full 64-row tile and a tail), n = 1 on 4 x 4 (16 rows); the pool and the upsample-add at 8 x 6"""
    _, m = fixture
    sd, net = weights(2), nets[2]
    names = ["conv2", "conv3", "conv4"] + ["m%d.%s" % (s, b) for s in range(2) for b in fr.HG_BLOCKS] + ["top_m_0", "top_m_1"]
    for name in names:
        cin = sd[name + ".bn1.weight"].shape[0]
        for shape in fr.BLOCK_SHAPES:
            x = fr.block_input(name, shape, cin)
            got = net.block(name, x.to(dev())).double().cpu()
            err = float((got - fr.run_block(sd, name, x)).abs().max())
            bound = F * m["bounds"]["block"]["small/%s/%dx%dx%d" % ((name,) + shape)]
            print("%-14s %s err %.3e bound %.3e" % (name, shape, err, bound))
            assert err <= bound, (name, shape)
    x = fr.block_input("avg_pool", fr.POOL_SHAPE, 256)
    up = fr.block_input("upsample_add", (fr.POOL_SHAPE[0], 2 * fr.POOL_SHAPE[1], 2 * fr.POOL_SHAPE[2]), 256)
    # one rounding to fp32 of an exactly computed value: half an ulp of the largest value
    for name, got, want in (("avg_pool", net.block("avg_pool", x.to(dev())), fr.pool(x.double())),
                            ("upsample_add", net.block("upsample_add", x.to(dev()), skip=up.to(dev())), fr.upadd(x.double(), up.double()))):
        err = float((got.double().cpu() - want).abs().max())
        print("%s err %.3e" % (name, err))
        assert err <= 2.0 ** -24 * float(want.abs().max()), name


@pytest.mark.parametrize("case", list(fr.CASES))
def test_forward_with_the_references_gates(case, fixture, nets, chains):
    data, m = fixture
    M, N, n = fr.CASES[case]
    gates = ref_gates(data, case)
    g = torch.stack(gates, 1).to(torch.uint8).to(dev()) if M > 1 else None
    out = nets[M].forward(fr.fixture_images(case).to(dev()), gates=g)
    assert len(out) == M and all(tuple(h.shape) == (n, N + 1, 64, 64) for h in out)
    if M > 1:
        assert torch.equal(nets[M].last_gates, g)
    for s in range(M):
        err, bound = float((out[s].double().cpu() - chains[case][0][s]).abs().max()), F * m["bounds"]["heat"][case][s]
        print("%s stack %d err %.3e bound %.3e" % (case, s, err, bound))
        assert err <= bound, (case, s)


@pytest.mark.parametrize("case", ["m2", "m4"])
def test_forward_with_its_own_gates(case, fixture, nets, chains):
    """last_gates equals the reference's on every stable cell, and the heat maps are within bound of the restatement run with the
    device's own gates"""
    data, m = fixture
    M, N, n = fr.CASES[case]
    x = fr.fixture_images(case)
    out = nets[M].forward(x.to(dev()))
    mine = nets[M].last_gates.cpu().bool()
    assert tuple(mine.shape) == (n, M - 1, 64, 64)
    for s, ref in enumerate(ref_gates(data, case)):
        unstable = fr.unstable_gate_cells(chains[case][0][s], F * m["bounds"]["heat"][case][s])
        differ = mine[:, s] != ref
        print("%s stack %d: %d gate cells differ, %d unstable" % (case, s, int(differ.sum()), int(unstable.sum())))
        assert not bool((differ & ~unstable).any()), (case, s)
    heats, _ = fr.forward(weights(M), x, M, N, gates=[mine[:, s] for s in range(M - 1)])
    for s in range(M):
        err, bound = float((out[s].double().cpu() - heats[s]).abs().max()), F * m["bounds"]["heat"][case][s]
        print("%s stack %d err %.3e bound %.3e" % (case, s, err, bound))
        assert err <= bound, (case, s)


def test_points_on_the_decode_cases_exactly(fixture, nets):
    data, m = fixture
    hs = np.stack([fr.decode_heatmaps(c) for c in fr.DECODE_CASES])
    pts, status = nets[1].points(torch.as_tensor(hs).to(dev()))
    pts, status = pts.cpu().numpy(), status.cpu().numpy()
    for i, case in enumerate(fr.DECODE_CASES):
        print(case, int(status[i]), pts[i, :2].tolist())
        if m["decode"][case]["raises_index_error"]:
            assert status[i] == 2 and (pts[i] == -1).all()
        else:
            assert status[i] == 0 and np.array_equal(pts[i], data["decode/" + case]), case
    # a [:, :N] view of a heat map with the boundary channel behind it is taken as it is
    full = torch.cat((torch.as_tensor(hs), torch.zeros(len(hs), 1, 64, 64)), 1).to(dev())
    again, _ = nets[1].points(full[:, :5])
    assert np.array_equal(again.cpu().numpy(), pts)


def _clip():
    frames = torch.rand(4, 3, 120, 100, generator=torch.Generator().manual_seed(3))
    boxes = torch.tensor([[10, 100, 5, 95], [0, 120, 0, 100], [-1, 50, 0, 40], [20, 84, 30, 94]], dtype=torch.int32)
    return frames, boxes


def test_landmarks_against_the_restated_chain(fixture, nets):
    from n3dt import fan as nf
    _, m = fixture
    M, N = 2, 98
    net = nets[M]
    frames, boxes = _clip()
    crops, used = net.crops(frames.to(dev()), boxes.to(dev()))
    want_crops = fr.crop(frames.numpy(), boxes.numpy())
    print("crop err %.3e" % float(np.abs(crops.cpu().numpy() - want_crops).max()))
    assert np.array_equal(crops.cpu().numpy(), want_crops) and torch.equal(used.cpu(), boxes)
    for convert, table in ((True, nf.MAP_98_TO_68), (False, None)):
        lm, status = net.landmarks(frames.to(dev()), boxes.to(dev()), convert=convert)
        heat = net.last_heatmaps.cpu()
        # exactly the restatement's decode and glue on the device's own heat maps
        want, wst = fr.glue([fr.decode(heat[f, :N].numpy()) for f in range(4)], boxes.numpy(), 120, 100, table=table)
        assert lm.dtype == torch.float64 and tuple(lm.shape) == (4, 68 if convert else N, 2)
        assert np.array_equal(status.cpu().numpy(), wst) and wst.tolist() == [0, 0, 4, 0]
        assert np.array_equal(lm.cpu().numpy(), want), convert
        assert np.array_equal(lm[2].cpu().numpy(), lm[1].cpu().numpy())  # the bad box takes the frame before it
    # the float64 chain (with the device's own gates): every stable landmark of a frame whose flags no unstable landmark can flip
    delta = F * m["bounds"]["heat"]["m2"][-1]
    ref, _ = fr.forward(weights(M), torch.as_tensor(want_crops), M, N, gates=[net.last_gates[:, 0].cpu().bool()])
    ref = ref[-1]
    print("heat err %.3e delta %.3e" % (float((heat.double() - ref).abs().max()), delta))
    unstable = fr.unstable_landmarks(ref, delta)
    flat = ref[:, :N].reshape(4, N, -1)
    top2 = flat.topk(2, dim=2).indices.numpy()
    flags = lambda i: (i + 64 >= 4096, i - 64 <= 0)  # noqa: E731
    lm98, _ = net.landmarks(frames.to(dev()), boxes.to(dev()), convert=False, carry=False)
    compared = 0
    for f in (0, 1, 3):
        if any(unstable[f, l] and flags(top2[f, l, 0]) != flags(top2[f, l, 1]) for l in range(N)):
            continue
        want = fr.glue([fr.decode(ref[f, :N].float().numpy())], boxes.numpy()[f:f + 1], 120, 100)[0][0]
        ok = ~unstable[f]
        compared += int(ok.sum())
        assert np.array_equal(lm98[f].cpu().numpy()[ok], want[ok]), f
    print("%d stable landmarks compared, %d unstable" % (compared, int(unstable[[0, 1, 3]].sum())))
    assert compared >= 98


def test_bitwise_properties(nets):
    from n3dt import ops
    net = nets[1]
    x = torch.rand(65, 3, 256, 256, generator=torch.Generator().manual_seed(11)).to(dev())
    whole = net.forward(x)[0]
    # batch position and batch size: 65 = 1 + 3 + 61
    parts = torch.cat([net.forward(x[a:b])[0] for a, b in ((0, 1), (1, 4), (4, 65))])
    assert torch.equal(parts, whole)
    assert torch.equal(net.forward(x, chunk=7)[0], whole)  # chunking
    for buf in ops.WORKSPACE.buf.values():                 # replay on a workspace filled with 0xFF: nothing is read before it is written
        buf.fill_(0xFF)
    assert torch.equal(net.forward(x)[0], whole)
    # two stacks: gates and bl / al, a frame alone against the frame inside a batch
    net2 = nets[2]
    a = net2.forward(x[:5])
    g = net2.last_gates.clone()
    b = net2.forward(x[3:4])
    assert torch.equal(b[1][0], a[1][3]) and torch.equal(net2.last_gates[0], g[3])
    assert torch.equal(net2.forward(x[:5], chunk=2)[1], a[1])
    # the carry-forward against hand-made -1 frames: the first stays -1, a later one takes the last good frame's points
    frames, boxes = _clip()
    boxes = boxes[[2, 0, 2, 2, 1]].contiguous()
    frames = frames[[2, 0, 2, 2, 1]].contiguous()
    lm, st = net.landmarks(frames.to(dev()), boxes.to(dev()), carry=True)
    raw, st2 = net.landmarks(frames.to(dev()), boxes.to(dev()), carry=False)
    assert st.tolist() == [4, 0, 4, 4, 0] == st2.tolist()
    assert bool((lm[0] == -1).all()) and torch.equal(lm[2], lm[1]) and torch.equal(lm[3], lm[1]) and torch.equal(lm[[1, 4]], raw[[1, 4]])
    assert bool((raw[[0, 2, 3]] == -1).all())


def test_landmarks_feed_face_recon(nets):
    from n3dt import FaceRecon, synthetic as syn
    recon = FaceRecon(syn.face_recon_state_dict(0), syn.face_recon_lm3d())
    frames, boxes = _clip()
    frames, boxes = frames.to(dev()), boxes.to(dev())
    lm, _ = nets[2].landmarks(frames, boxes)
    direct = recon.expressions(frames, lm)
    through_host = recon.expressions(frames, torch.as_tensor(lm.cpu().numpy().copy()).to(dev()))
    assert tuple(direct.shape) == (4, 64) and bool(torch.isfinite(direct).all()) and torch.equal(direct, through_host)
