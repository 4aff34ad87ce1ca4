"""n3dt.FlatAdam on the GPU against torch.optim.Adam.

Reference: torch.optim.Adam on float64 CPU copies fed the same gradients.  Bound: computed here from torch's own fp32 CPU
Adam(foreach=False) on the same inputs against that float64 run -- for each of p / exp_avg / exp_avg_sq the largest
deviation over the parameters, each relative to its tensor's max-abs -- times 4 (room for a different but equally valid
fp32 evaluation order: the kernel forms m as b1 m + (1 - b1) g where torch's CPU path uses lerp).  The bound comes from
torch, never from the code under test; every test prints the floor and FlatAdam's deviation before it asserts.

Measured on MI355X (7 steps of the parity case): floor p 3.2e-7, exp_avg 2.3e-7, exp_avg_sq 2.5e-7; FlatAdam 3.2e-7, 2.3e-7, 2.5e-7
(DESIGN 3.12).
"""
import ctypes

import pytest
import torch

from conftest import load_golden, synthetic_case

pytestmark = pytest.mark.gpu

STEPS = 7
# numels 1, 3, 63, 64, 65, 4097, 12x5; then a 133-element view one element into a larger buffer; then one whose grad stays None
SHAPES = [(1,), (3,), (63,), (64,), (65,), (4097,), (12, 5), (133,), (64,)]
VIEW, GRADLESS = 7, 8
GROUP1 = (1, 3, 5, 7)  # indices of the second group; the rest form the first
HYPER = [dict(lr=1e-4, betas=(0.9, 0.999), weight_decay=0), dict(lr=1e-7, betas=(0.5, 0.999), weight_decay=1e-2)]
SCALES = [1e-6, 1e-4, 1e-2, 1.0, 1e2, 1e-3, 10.0, 0.1, 1.0]


def dev():
    return torch.device("cuda:0")


def make_case(steps=STEPS, seed=0):
    gen = torch.Generator().manual_seed(seed)
    init = [torch.randn(s, generator=gen) for s in SHAPES]
    grads = []
    for _ in range(steps):
        row = []
        for i, s in enumerate(SHAPES):
            if i == GRADLESS:
                row.append(None)
                continue
            g = torch.randn(s, generator=gen) * SCALES[i]
            if i == 5:
                g[1000:1100] = 0.0  # a block of exact zeros
            row.append(g)
        grads.append(row)
    return init, grads


def make_params(init, dtype, device):
    """Leaf parameters holding `init`; parameter VIEW is a view at storage offset 1 of a larger buffer (returned too)."""
    params, buf = [], None
    for i, t in enumerate(init):
        if i == VIEW:
            buf = torch.full((t.numel() + 8,), 7.0, dtype=dtype, device=device)
            buf[1:1 + t.numel()] = t.to(device=device, dtype=dtype)
            params.append(torch.nn.Parameter(buf[1:1 + t.numel()]))
            assert params[-1].storage_offset() == 1
        else:
            params.append(torch.nn.Parameter(t.to(device=device, dtype=dtype).clone()))
    return params, buf


def groups_of(params, hyper=HYPER):
    g0 = [p for i, p in enumerate(params) if i not in GROUP1]
    g1 = [p for i, p in enumerate(params) if i in GROUP1]
    return [dict(params=g0, **hyper[0]), dict(params=g1, **hyper[1])]


def feed(params, row):
    for p, g in zip(params, row):
        p.grad = None if g is None else g.to(device=p.device, dtype=p.dtype).clone()


def run_torch(init, grads, dtype, device="cpu", lr_at=None, **kw):
    """torch.optim.Adam over `grads`; lr_at: {step index: lr of group 0 from that step on}."""
    params, _ = make_params(init, dtype, device)
    opt = torch.optim.Adam(groups_of(params), **kw)
    for k, row in enumerate(grads):
        if lr_at and k in lr_at:
            opt.param_groups[0]["lr"] = lr_at[k]
        feed(params, row)
        opt.step()
    return params, opt


def state_of(params, opt):
    out = {"p": [], "exp_avg": [], "exp_avg_sq": []}
    for i, p in enumerate(params):
        if i == GRADLESS:
            continue
        out["p"].append(p.detach().double().cpu())
        out["exp_avg"].append(opt.state[p]["exp_avg"].double().cpu())
        out["exp_avg_sq"].append(opt.state[p]["exp_avg_sq"].double().cpu())
    return out


def deviation(got, ref):
    """Per kind, the largest over the tensors of max|got - ref| / max|ref|."""
    return {k: max(float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300) for a, b in zip(got[k], ref[k])) for k in ref}


@pytest.fixture(scope="module")
def parity():
    """The shared case: inputs, the float64 reference and the fp32 floor.  Computed once; nothing writes to it."""
    init, grads = make_case()
    ref = state_of(*run_torch(init, grads, torch.float64))
    floor = deviation(state_of(*run_torch(init, grads, torch.float32, foreach=False)), ref)
    return {"init": init, "grads": grads, "ref": ref, "floor": floor}


def check(tag, got, ref, floor, kinds=("p", "exp_avg", "exp_avg_sq")):
    d = deviation({k: got[k] for k in kinds}, {k: ref[k] for k in kinds})
    print("%s: fp32 floor %s | FlatAdam deviation %s" % (tag, {k: "%.3e" % floor[k] for k in kinds}, {k: "%.3e" % d[k] for k in kinds}))
    for k in kinds:
        assert d[k] <= 4.0 * floor[k], "%s: %s deviates %.3e, bound %.3e" % (tag, k, d[k], 4.0 * floor[k])


def test_parity_with_float64_adam(parity):
    from n3dt import FlatAdam
    params, buf = make_params(parity["init"], torch.float32, dev())
    gradless0 = params[GRADLESS].detach().clone()
    opt = FlatAdam(groups_of(params))
    for row in parity["grads"]:
        feed(params, row)
        opt.step()
    check("parity", state_of(params, opt), parity["ref"], parity["floor"])
    assert int(opt.state[params[0]]["step"]) == STEPS
    # the parameter without a gradient, and its state, are bit-unchanged
    assert torch.equal(params[GRADLESS].detach(), gradless0)
    assert not bool(opt.state[params[GRADLESS]]["exp_avg"].any()) and not bool(opt.state[params[GRADLESS]]["exp_avg_sq"].any())
    # elements of the buffer outside the misaligned view are bit-unchanged
    n = params[VIEW].numel()
    assert torch.equal(buf[:1].cpu(), torch.full((1,), 7.0)) and torch.equal(buf[1 + n:].cpu(), torch.full((7,), 7.0))
    # the padding of the state arenas was never written (a vector access that overran a tail would land there)
    for ai, a in enumerate(opt._arenas):
        used = torch.zeros(a.flat.numel(), dtype=torch.bool, device=dev())
        for i, p in enumerate(a.params):
            used[a.offsets[i]:a.offsets[i] + p.numel()] = True
        assert not bool(opt._exp_avg[ai][~used].any()) and not bool(opt._exp_avg_sq[ai][~used].any())


def _adam_cpu64(p, g, m, v, t, lr, b1, b2, eps, wd):
    g = g + wd * p
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    p = p - lr / (1 - b1 ** t) * m / (v.sqrt() / (1 - b2 ** t) ** 0.5 + eps)
    return p, m, v


@pytest.mark.parametrize("offs", [(0, 0, 0, 0), (1, 1, 1, 1), (3, 3, 3, 3), (2, 0, 0, 0), (0, 1, 1, 1), (0, 0, 1, 2), (1, 2, 3, 0)])
def test_kernel_heads_tails_and_mixed_alignment(offs):
    """The C entry point on hand-built tables: p / g / m / v start `offs` elements past a 16-byte boundary (all congruent: head +
    vector body + tail; parameter alone off: its own 4-byte path; state off: the element-wise path), chunks of odd lengths.
    Results against Adam in float64 on the host (1e-5 of each tensor's max-abs: fp32 arithmetic, one step); guard elements around
    every buffer stay bit-unchanged."""
    from n3dt import _lib
    L = _lib.lib()
    n, pad = 4103, 8
    gen = torch.Generator().manual_seed(sum(offs) + 11)
    host = [torch.randn(n, generator=gen), torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 0.1,
            torch.rand(n, generator=gen) * 0.01]
    bufs = []
    for h, o in zip(host, offs):
        b = torch.full((pad + n + pad,), 5.0, device=dev())
        b[4 + o:4 + o + n] = h.to(dev())  # cudaMalloc'ed base is 256-byte aligned: element 4 sits on a 16-byte boundary
        bufs.append(b)
    ptr = [b.data_ptr() + 4 * (4 + o) for b, o in zip(bufs, offs)]
    assert all((q % 16) // 4 == o for q, o in zip(ptr, offs))
    bounds = [0, 1, 6, 70, 4099, n]  # chunk lengths 1, 5, 64, 4029, 4
    chunks = [_lib.AdamChunk(a, 0, b - a) for a, b in zip(bounds[:-1], bounds[1:])]
    tens = [_lib.AdamTensor(ptr[0], ptr[1], ptr[2], ptr[3], n, 0, 1)]
    lr, b1, b2, eps, wd, t0 = 1e-2, 0.9, 0.999, 1e-8, 1e-2, 4
    grp = [_lib.AdamGroup(lr, b1, b2, eps, wd, 0, 0)]

    def up(recs, kind):
        raw = bytes((kind * len(recs))(*recs))
        return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev())
    td, cd, gd = up(tens, _lib.AdamTensor), up(chunks, _lib.AdamChunk), up(grp, _lib.AdamGroup)
    counter = torch.tensor([t0, 0, 0, 0], dtype=torch.int32, device=dev())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(L.n3dt_flat_adam_step(td.data_ptr(), cd.data_ptr(), len(chunks), gd.data_ptr(), 1, counter.data_ptr(), stream), "step")
    torch.cuda.synchronize()
    assert counter.tolist() == [t0 + 1, 0, 0, 0]
    ref = _adam_cpu64(*(h.double() for h in host), t0 + 1, lr, b1, b2, eps, wd)
    for k, o, r in zip((0, 2, 3), (offs[0], offs[2], offs[3]), ref):
        got = bufs[k].cpu()
        assert bool((got[:4 + o] == 5.0).all()) and bool((got[4 + o + n:] == 5.0).all()), "a guard element was written"
        err = float((got[4 + o:4 + o + n].double() - r).abs().max())
        assert err <= 1e-5 * float(r.abs().max()), (k, err)
    assert torch.equal(bufs[1].cpu()[4 + offs[1]:4 + offs[1] + n], host[1])  # the gradient is read only


def test_first_step_moves_every_entry_by_lr():
    """|g| >> eps: step 1 is lr * sign(g) to 1e-6 relative.  Pins the double-precision bias correction (an fp32 1 - 0.999^1
    misses by ~6e-5).  Parameters start at zero so that the move itself is what fp32 holds."""
    from n3dt import FlatAdam
    gen = torch.Generator().manual_seed(3)
    lr = 1e-3
    params = [torch.nn.Parameter(torch.zeros(s, device=dev())) for s in ((4097,), (65,), (12, 5))]
    opt = FlatAdam(params, lr=lr)
    sign = []
    for p in params:
        g = (0.5 + torch.rand(p.shape, generator=gen)) * (torch.randint(0, 2, p.shape, generator=gen) * 2 - 1)
        p.grad = g.to(dev())
        sign.append(torch.sign(g))
    opt.step()
    worst = 0.0
    for p, s in zip(params, sign):
        rel = (p.detach().cpu().double() / (-lr * s.double()) - 1.0).abs().max()
        worst = max(worst, float(rel))
    print("first step: max relative distance from lr*sign(g) = %.3e" % worst)
    assert worst <= 1e-6


def test_gradients_living_outside_the_arena(parity):
    from n3dt import FlatAdam
    torch.manual_seed(5)
    init = parity["init"]
    pa, _ = make_params(init, torch.float32, dev())
    pb, _ = make_params(init, torch.float32, dev())
    flat = FlatAdam(groups_of(pa))
    ref = torch.optim.Adam(groups_of(pb), fused=True)
    for _ in range(2):
        for i, (a, b) in enumerate(zip(pa, pb)):
            if i == GRADLESS:
                a.grad = b.grad = None
                continue
            a.grad = torch.randn_like(a)
            b.grad = a.grad.clone()
        flat.step()
        ref.step()
    check("stray grads vs fused fp32", state_of(pa, flat), state_of(pb, ref), parity["floor"])
    arena = flat._arenas[0]
    for i, p in enumerate(arena.params):
        if p is pa[GRADLESS]:
            assert p.grad is None
        else:
            assert arena.is_view(i, p.grad)


@pytest.mark.parametrize("direction", ["torch_to_flat", "flat_to_torch"])
def test_state_dict_interchange_on_device(parity, direction):
    from n3dt import FlatAdam
    init, grads = parity["init"], parity["grads"]
    init = [t for i, t in enumerate(init) if i != GRADLESS]  # (torch keeps no state for a parameter that never had a gradient)
    grads = [[g for i, g in enumerate(row) if i != GRADLESS] for row in grads]

    def build(kind, params):
        gs = [dict(params=[p for i, p in enumerate(params) if i not in GROUP1], **HYPER[0]),
              dict(params=[p for i, p in enumerate(params) if i in GROUP1], **HYPER[1])]
        return FlatAdam(gs) if kind == "flat" else torch.optim.Adam(gs)
    first, second = ("torch", "flat") if direction == "torch_to_flat" else ("flat", "torch")
    pa = [torch.nn.Parameter(t.to(dev()).clone()) for t in init]
    oa = build(first, pa)
    for row in grads[:3]:
        feed(pa, row)
        oa.step()
    pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    ob = build(second, pb)
    ob.load_state_dict(oa.state_dict())
    for row in grads[3:6]:
        feed(pa, row)
        oa.step()
        feed(pb, row)
        ob.step()
    sa = {"p": [p.detach().double().cpu() for p in pa]}
    sb = {"p": [p.detach().double().cpu() for p in pb]}
    flat_side, torch_side = (sb, sa) if second == "flat" else (sa, sb)
    check(direction, flat_side, torch_side, parity["floor"], kinds=("p",))
    assert int(ob.state[pb[0]]["step"]) == 6 and int(oa.state[pa[0]]["step"]) == 6
    # the loaded optimizer owns its state: nothing aliases the other's buffers
    assert ob.state[pb[2]]["exp_avg"].data_ptr() != oa.state[pa[2]]["exp_avg"].data_ptr()


def test_scheduler_refreshes_the_device_lr(parity):
    from n3dt import FlatAdam
    init, grads = parity["init"], parity["grads"][:5]

    def run(make, dtype, device):
        params, _ = make_params(init, dtype, device)
        opt = make(groups_of(params))
        sched = torch.optim.lr_scheduler.StepLR(opt, step_size=2, gamma=0.1)
        for row in grads:
            feed(params, row)
            opt.step()
            sched.step()
        return params, opt
    ref = state_of(*run(torch.optim.Adam, torch.float64, "cpu"))
    params, opt = run(FlatAdam, torch.float32, dev())
    assert opt.param_groups[0]["lr"] == pytest.approx(1e-6) and opt.param_groups[1]["lr"] == pytest.approx(1e-9)
    check("StepLR", state_of(params, opt), ref, parity["floor"])


def test_capture_and_replay(parity):
    from n3dt import FlatAdam
    init, grads = parity["init"], parity["grads"][:6]
    lr_at = {4: 1e-2}  # after replay 3 (the fourth step overall), group 0's lr changes
    ref = state_of(*run_torch(init, grads, torch.float64, lr_at=lr_at))
    params, _ = make_params(init, torch.float32, dev())
    opt = FlatAdam(groups_of(params))
    feed(params, grads[0])
    opt.step()  # eager warm-up: tables, state and the arena slices exist from here on
    slices = [p.grad for p in params]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    for k in range(1, 6):
        for s, g in zip(slices, grads[k]):
            if g is not None:
                s.copy_(g.to(dev()))
        if k in lr_at:
            opt.param_groups[0]["lr"] = lr_at[k]
            opt.sync_hyperparameters()
        graph.replay()
    torch.cuda.synchronize()
    assert int(opt.state[params[0]]["step"]) == 6
    check("capture", state_of(params, opt), ref, parity["floor"])


def _render(net, d):
    with torch.no_grad():
        out = net("test", d["batch_xy"], d["batch_uv"], d["audiostyle"], bg_code=None, shape_code=d["shape_code"],
                  appea_code=d["appea_code"], batch_Rmats=d["batch_Rmats"], batch_Tvecs=d["batch_Tvecs"],
                  batch_inv_inmats=d["batch_inv_inmats"])
    return out["coarse_dict"]["merge_img"].clone()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_version_keyed_caches_follow_a_step(precision):
    """A step with hand-set gradients (no backward of ours in between): the next render must use the new weights."""
    from n3dt import HeadNeRFNet, FlatAdam
    _, m = load_golden("tiny_test")
    opt_, sd, inp = synthetic_case(m)
    d = {k: (v.to(dev()) if torch.is_tensor(v) else v) for k, v in inp.items()}
    net = HeadNeRFNet(opt_, include_vd=False, hier_sampling=False, precision=precision).to(dev())
    net.load_state_dict(sd, strict=True)
    optim = FlatAdam(net.parameters(), lr=1e-2, modules=[net])
    img0 = _render(net, d)
    versions = [p._version for p in net.parameters()]
    for p in net.parameters():
        p.grad = torch.ones_like(p)
    optim.step()
    assert all(p._version > v for p, v in zip(net.parameters(), versions))
    img1 = _render(net, d)
    fresh = HeadNeRFNet(opt_, include_vd=False, hier_sampling=False, precision=precision).to(dev())
    fresh.load_state_dict(net.state_dict(), strict=True)
    img2 = _render(fresh, d)
    assert float((img1 - img2).abs().max()) <= 1e-6
    assert float((img1 - img0).abs().max()) > 1e-4


def _train_setup():
    from n3dt import HeadNeRFNet, synthetic as syn
    from n3dt.train import disk_mask
    _, m = load_golden("tiny_train")
    opt, sd, inp = synthetic_case(m)
    net = HeadNeRFNet(opt, include_vd=False, hier_sampling=False).to(dev())
    net.load_state_dict(sd, strict=True)
    d = {k: (v.to(dev()) if torch.is_tensor(v) else v) for k, v in inp.items()}
    t_rand = syn.stratified_noise(m["batch"], opt.featmap_size ** 2, opt.num_sample_coarse, m["t_rand_seed"]).to(dev())
    gt = torch.full((m["batch"], 3, opt.pred_img_size, opt.pred_img_size), 0.5, device=dev())
    mask = disk_mask(m["batch"], opt.pred_img_size).to(dev())
    return net, d, gt, mask, t_rand


def _outside(a, b, band):
    n = sum(x.numel() for x in a)
    worst = max(float((x - y).abs().max()) for x, y in zip(a, b))
    return sum(int(((x - y).abs() > band).sum()) for x, y in zip(a, b)) / n, worst


def test_train_step_through_the_product():
    """train.train_step with make_flat_optimizer at the tiny_train geometry: the loss falls over 3 steps, and the parameters after
    step 1 match the same step with torch.optim.Adam(lr=1e-4) within 2 lr per entry (Adam's first step is lr * sign(g)), with at most
    0.5 % of the entries outside 1e-2 lr -- those whose gradient is summation-order noise around zero (the backward adds with fp32
    atomics).  That cap is checked first on two runs of the torch optimizer against each other.
    Observed on MI355X: 0 entries outside the band in both comparisons (largest difference 7.5e-9: the exact-fp32 backward at this
    geometry repeats to the last bit or two), losses 0.6000, 0.5329, 0.4874, 0.4557."""
    from n3dt.train import train_step, make_optimizer, make_flat_optimizer
    lr = 1e-4
    after = []
    for make in (make_optimizer, make_optimizer, make_flat_optimizer):
        net, d, gt, mask, t_rand = _train_setup()
        optim, _ = make(net, lr=lr)
        _, terms = train_step(net, optim, d, gt, mask, t_rand=t_rand)
        after.append(([p.detach().clone() for p in net.parameters()], net, optim, float(terms["total_loss"].detach())))
    share_tt, worst_tt = _outside(after[0][0], after[1][0], 1e-2 * lr)
    share_ft, worst_ft = _outside(after[2][0], after[0][0], 1e-2 * lr)
    print("entries outside 1e-2 lr: torch vs torch %.4f %% (max %.3e), FlatAdam vs torch %.4f %% (max %.3e)"
          % (100 * share_tt, worst_tt, 100 * share_ft, worst_ft))
    assert share_tt <= 0.005, "the condition of this test does not hold: two torch runs differ in %.3f %% of the entries" % (100 * share_tt)
    assert worst_ft <= 2 * lr
    assert share_ft <= 0.005
    _, net, optim, loss0 = after[2]
    _, d, gt, mask, t_rand = _train_setup()
    losses = [loss0]
    for _ in range(3):
        _, terms = train_step(net, optim, d, gt, mask, t_rand=t_rand)
        losses.append(float(terms["total_loss"].detach()))
    print("losses:", losses)
    assert losses[3] < losses[0]  # (each loss is taken before its step's update: losses[3] follows three updates)
