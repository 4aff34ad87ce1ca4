"""FlatAdam's guarded step on the GPU: device-side global-norm clipping and non-finite step skipping.

Reference everywhere: torch on float64 CPU copies fed the same gradients -- clip_grad_norm_(params, max_norm), then
torch.optim.Adam.step().  Bound, as in test_gpu_flat_adam.py: for each of p / exp_avg / exp_avg_sq, 4 x the deviation of torch's own
fp32 CPU run (clip_grad_norm_ + Adam(foreach=False)) from that float64 run, the largest over the parameters, each relative to its
tensor's max-abs.  It comes from torch, never from the code under test, and is printed next to FlatAdam's deviation before the
assertion.  grad_norm: within 2^-23 relative of the float64 norm (the accumulation is in double; only the sqrt and the one rounding
to fp32, 2^-24, are inexact).

Shapes: the parity case of test_gpu_flat_adam.py (numels 1, 3, 63, 64, 65, 4097, 12x5, a 133-element view at storage offset 1, one
parameter whose grad stays None) plus one tensor of 2*4096 + 5 elements, which spans three chunks; two groups, 7 steps.  The
gradient scale alternates between rows so that with MAX_NORM some steps clip and some do not.
"""
import ctypes
import math

import pytest
import torch
from torch.nn.utils import clip_grad_norm_

pytestmark = pytest.mark.gpu

STEPS = 7
SHAPES = [(1,), (3,), (63,), (64,), (65,), (4097,), (12, 5), (133,), (64,), (2 * 4096 + 5,)]
VIEW, GRADLESS, BIG = 7, 8, 9
GROUP1 = (1, 3, 5, 7)
HYPER = [dict(lr=1e-4, betas=(0.9, 0.999), weight_decay=0), dict(lr=1e-7, betas=(0.5, 0.999), weight_decay=1e-2)]
SCALES = [1e-6, 1e-4, 1e-2, 1.0, 1e2, 1e-3, 10.0, 0.1, 1.0, 0.5]
ROW_SCALE = [1.0, 0.01, 1.0, 0.01, 1.0, 0.01, 1.0]  # norms of about 810 and 8.1
MAX_NORM = 100.0
EPS_NORM = 2.0 ** -23


def dev():
    return torch.device("cuda:0")


def make_case(steps=STEPS, seed=0):
    gen = torch.Generator().manual_seed(seed)
    init = [torch.randn(s, generator=gen) for s in SHAPES]
    grads = []
    for k in range(steps):
        row = []
        for i, s in enumerate(SHAPES):
            if i == GRADLESS:
                row.append(None)
                continue
            g = torch.randn(s, generator=gen) * (SCALES[i] * ROW_SCALE[k])
            if i == 5:
                g[1000:1100] = 0.0
            row.append(g)
        grads.append(row)
    return init, grads


def make_params(init, dtype, device):
    params = []
    for i, t in enumerate(init):
        if i == VIEW:
            buf = torch.full((t.numel() + 8,), 7.0, dtype=dtype, device=device)
            buf[1:1 + t.numel()] = t.to(device=device, dtype=dtype)
            params.append(torch.nn.Parameter(buf[1:1 + t.numel()]))
            assert params[-1].storage_offset() == 1
        else:
            params.append(torch.nn.Parameter(t.to(device=device, dtype=dtype).clone()))
    return params


def groups_of(params):
    g0 = [p for i, p in enumerate(params) if i not in GROUP1]
    g1 = [p for i, p in enumerate(params) if i in GROUP1]
    return [dict(params=g0, **HYPER[0]), dict(params=g1, **HYPER[1])]


def feed(params, row):
    for p, g in zip(params, row):
        p.grad = None if g is None else g.to(device=p.device, dtype=p.dtype).clone()


def run_torch(init, grads, dtype, max_norm=MAX_NORM, **kw):
    """clip_grad_norm_ + torch.optim.Adam on the CPU.  max_norm: one value or one per row.  Returns params, optimizer and the
    norm of every row as clip_grad_norm_ returned it."""
    params = make_params(init, dtype, "cpu")
    opt = torch.optim.Adam(groups_of(params), **kw)
    norms = []
    for k, row in enumerate(grads):
        feed(params, row)
        mn = max_norm[k] if isinstance(max_norm, (list, tuple)) else max_norm
        norms.append(float(clip_grad_norm_([p for p in params if p.grad is not None], mn)))
        opt.step()
    return params, opt, norms


def state_of(params, opt):
    out = {"p": [], "exp_avg": [], "exp_avg_sq": []}
    for i, p in enumerate(params):
        if i == GRADLESS:
            continue
        out["p"].append(p.detach().double().cpu())
        out["exp_avg"].append(opt.state[p]["exp_avg"].double().cpu())
        out["exp_avg_sq"].append(opt.state[p]["exp_avg_sq"].double().cpu())
    return out


def raw_state(params, opt):
    """Bit-exact copies of everything a step may write."""
    return ([p.detach().clone() for p in params], [opt.state[p]["exp_avg"].clone() for p in params],
            [opt.state[p]["exp_avg_sq"].clone() for p in params], int(opt.state[params[0]]["step"]))


def same_bits(a, b):
    return a[3] == b[3] and all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for k in range(3) for x, y in zip(a[k], b[k]))


def deviation(got, ref):
    return {k: max(float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300) for a, b in zip(got[k], ref[k])) for k in ref}


def reference(init, grads, max_norm=MAX_NORM):
    """The float64 run, torch's fp32 floor against it, and the float64 norms."""
    p64, o64, norms = run_torch(init, grads, torch.float64, max_norm)
    ref = state_of(p64, o64)
    p32, o32, _ = run_torch(init, grads, torch.float32, max_norm, foreach=False)
    return {"ref": ref, "floor": deviation(state_of(p32, o32), ref), "norms": norms}


def check(tag, got, ref, floor):
    d = deviation(got, ref)
    print("%s: fp32 floor %s | FlatAdam deviation %s" % (tag, {k: "%.3e" % v for k, v in floor.items()}, {k: "%.3e" % v for k, v in d.items()}))
    for k in ref:
        assert d[k] <= 4.0 * floor[k], "%s: %s deviates %.3e, bound %.3e" % (tag, k, d[k], 4.0 * floor[k])


def check_norm(tag, got, want):
    rel = abs(got - want) / want
    print("%s: grad_norm %.9g, float64 %.17g, relative difference %.3e (bound %.3e)" % (tag, got, want, rel, EPS_NORM))
    assert math.isfinite(got) and rel <= EPS_NORM, (tag, got, want)


@pytest.fixture(scope="module")
def case():
    """Inputs, the float64 reference with clipping at MAX_NORM, and the fp32 floor.  Computed once; nothing writes to it."""
    init, grads = make_case()
    out = {"init": init, "grads": grads}
    out.update(reference(init, grads))
    return out


def flat_run(init, grads, after=None, **kw):
    from n3dt import FlatAdam
    params = make_params(init, torch.float32, dev())
    opt = FlatAdam(groups_of(params), **kw)
    for k, row in enumerate(grads):
        feed(params, row)
        opt.step()
        if after is not None:
            after(k, params, opt)
    return params, opt


# ---- 1. clipping parity ------------------------------------------------------------------------------------------------
def test_clipping_parity_with_float64_clip_grad_norm_and_adam(case):
    coefs64 = [min(1.0, MAX_NORM / (n + 1e-6)) for n in case["norms"]]
    assert any(c < 1.0 for c in coefs64) and any(c == 1.0 for c in coefs64), "the case must clip on some steps and not on others"
    norms, coefs = [], []

    def after(k, params, opt):
        norms.append(opt.grad_norm.clone())
        coefs.append(opt.clip_coef.clone())
    params, opt = flat_run(case["init"], case["grads"], after=after, max_grad_norm=MAX_NORM)
    for k in range(STEPS):
        check_norm("step %d" % k, float(norms[k]), case["norms"][k])
        c = float(coefs[k])
        # fp32: the rounded norm, + 1e-6, the reciprocal, x max_norm, and 1e-6 as an fp32 constant -- five roundings of 2^-24
        assert (c == 1.0) == (coefs64[k] == 1.0) and abs(c - coefs64[k]) <= 2.0 ** -21 * coefs64[k], (k, c, coefs64[k])
    check("clipping parity", state_of(params, opt), case["ref"], case["floor"])
    assert int(opt.state[params[0]]["step"]) == STEPS and int(opt.skipped_steps) == 0
    assert opt.grad_norm.dtype == torch.float32 and opt.grad_norm.dim() == 0 and opt.grad_norm.is_cuda
    assert opt.clip_coef.dtype == torch.float32 and opt.clip_coef.dim() == 0
    assert opt.skipped_steps.dtype == torch.int32 and opt.skipped_steps.dim() == 0
    # .grad is not rewritten (the documented difference from clip_grad_norm_)
    assert torch.equal(params[4].grad.cpu(), case["grads"][-1][4])


# ---- 2. an inactive clip is exact --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(max_grad_norm=1e9), dict(max_grad_norm=math.inf, skip_nonfinite=True), dict(skip_nonfinite=True)],
                         ids=["above_every_norm", "inf_and_skip", "skip_only"])
def test_inactive_clip_is_bit_identical_to_the_unguarded_step(case, kw):
    assert max(case["norms"]) < 1e9
    coefs = []
    plain = raw_state(*flat_run(case["init"], case["grads"]))
    params, opt = flat_run(case["init"], case["grads"], after=lambda k, p, o: coefs.append(o.clip_coef.clone()), **kw)
    assert opt.guarded
    assert all(float(c) == 1.0 for c in coefs)
    assert same_bits(raw_state(params, opt), plain)
    assert int(opt.skipped_steps) == 0


# ---- 3. inactive tensors are not counted -------------------------------------------------------------------------------
def test_a_gradless_parameters_arena_slice_is_not_counted(case):
    from n3dt import FlatAdam
    params = make_params(case["init"], torch.float32, dev())
    opt = FlatAdam(groups_of(params), max_grad_norm=MAX_NORM, skip_nonfinite=True)
    opt.sync_hyperparameters()  # lays the arenas out
    feed(params, case["grads"][0])
    for a in opt._arenas:
        a.adopt(assign_missing=False)  # every .grad is its arena slice from here on, so step() has nothing to copy or clear
    where = [(a, i) for a in opt._arenas for i, p in enumerate(a.params) if p is params[GRADLESS]]
    assert len(where) == 1
    arena, i = where[0]
    dead = arena.flat[arena.offsets[i]:arena.offsets[i] + params[GRADLESS].numel()]
    dead.fill_(float("nan"))
    for k, row in enumerate(case["grads"]):
        for p, g in zip(params, row):
            if g is not None:
                p.grad.copy_(g.to(dev()))
        opt.step()
        check_norm("step %d" % k, float(opt.grad_norm), case["norms"][k])
    assert params[GRADLESS].grad is None and bool(torch.isnan(dead).all())
    assert int(opt.skipped_steps) == 0 and int(opt.state[params[0]]["step"]) == STEPS
    check("NaN in an inactive slice", state_of(params, opt), case["ref"], case["floor"])


def test_grid_stride_with_an_inactive_tensor_between_active_ones():
    """More chunks than the grid has workgroups (1 024) and more than one pass of the final sum stages (2 048): tensors of
    1 024, 1 024 and 100 chunks + 5 elements, the middle one without a gradient and its arena slice full of NaN.  Workgroups
    0..100 then walk an active, an inactive and an active chunk in turn.  One step: grad_norm against the float64 norm of the two
    active gradients, nothing skipped, the gradless parameter untouched."""
    from n3dt import FlatAdam
    n = 1024 * 4096
    gen = torch.Generator().manual_seed(21)
    shapes = [(n,), (n,), (100 * 4096 + 5,)]
    params = [torch.nn.Parameter(torch.randn(s, generator=gen).to(dev())) for s in shapes]
    grads = [torch.randn(shapes[0], generator=gen) * 0.3, None, torch.randn(shapes[2], generator=gen) * 2.0]
    want = math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads if g is not None))
    opt = FlatAdam(params, lr=1e-3, max_grad_norm=1.0, skip_nonfinite=True)
    opt.sync_hyperparameters()
    assert opt._n_chunks == 2149 > 2048
    feed(params, grads)
    for a in opt._arenas:
        a.adopt(assign_missing=False)
    where = [(a, i) for a in opt._arenas for i, p in enumerate(a.params) if p is params[1]]
    assert len(where) == 1
    arena, i = where[0]
    dead = arena.flat[arena.offsets[i]:arena.offsets[i] + n]
    dead.fill_(float("nan"))
    before = [p.detach().clone() for p in params]
    opt.step()
    check_norm("2 149 chunks", float(opt.grad_norm), want)
    assert int(opt.skipped_steps) == 0 and int(opt.state[params[0]]["step"]) == 1
    assert params[1].grad is None and bool(torch.isnan(dead).all())
    assert torch.equal(params[1].detach(), before[1]) and not bool(opt.state[params[1]]["exp_avg_sq"].any())
    # every element of the active tensors moved by about lr (first Adam step), none is NaN
    for k in (0, 2):
        move = (params[k].detach() - before[k]).abs()
        assert bool(torch.isfinite(params[k]).all()) and float(move.max()) <= 1.01e-3 and float(move.mean()) > 0.9e-3
    # the same decision with the NaN made visible: activate the middle tensor and the step is skipped
    params[1].grad = dead.view(shapes[1])
    snap = [p.detach().clone() for p in params]
    opt.step()
    assert int(opt.skipped_steps) == 1 and int(opt.state[params[0]]["step"]) == 1
    assert all(torch.equal(p.detach().view(torch.int32), q.view(torch.int32)) for p, q in zip(params, snap))


# ---- 4. skip -----------------------------------------------------------------------------------------------------------
# {row: (tensor, flat index, value)}: the vector body of a chunk and the last element of the last chunk (a scalar tail);
# a scalar tail (numel 63 = 15 vectors + 3) and the body of the middle chunk of the three-chunk tensor
PLANTS = {"inf_body_nan_last": {2: (5, 100, math.inf), 5: (BIG, 2 * 4096 + 4, math.nan)},
          "nan_tail_inf_mid_chunk": {1: (2, 62, math.nan), 4: (BIG, 5000, math.inf)}}


def planted(grads, plants):
    out = [list(row) for row in grads]
    for k, (t, i, v) in plants.items():
        g = out[k][t].clone()
        g.view(-1)[i] = v
        out[k][t] = g
    return out


@pytest.mark.parametrize("name", sorted(PLANTS))
def test_poisoned_steps_change_nothing_and_are_counted(case, name):
    from n3dt import FlatAdam
    plants = PLANTS[name]
    grads = planted(case["grads"], plants)
    clean_rows = [row for k, row in enumerate(case["grads"]) if k not in plants]
    ref = reference(case["init"], clean_rows)  # the float64 run that leaves the two steps out on the host
    params = make_params(case["init"], torch.float32, dev())
    opt = FlatAdam(groups_of(params), max_grad_norm=MAX_NORM, skip_nonfinite=True)
    skipped = 0
    for k, row in enumerate(grads):
        feed(params, row)
        if k in plants:
            before = raw_state(params, opt)
            opt.step()
            assert same_bits(raw_state(params, opt), before), "step %d changed something" % k
            assert not math.isfinite(float(opt.grad_norm))
            skipped += 1
        else:
            opt.step()
        assert int(opt.skipped_steps) == skipped
    assert int(opt.state[params[0]]["step"]) == STEPS - 2 == 5
    check("skip " + name, state_of(params, opt), ref["ref"], ref["floor"])


@pytest.mark.parametrize("name", sorted(PLANTS))
def test_without_skipping_the_nan_mask_is_torchs(case, name):
    grads = planted(case["grads"], PLANTS[name])
    p32, _, _ = run_torch(case["init"], grads, torch.float32, MAX_NORM, foreach=False)
    params, opt = flat_run(case["init"], grads, max_grad_norm=MAX_NORM, skip_nonfinite=False)
    assert int(opt.skipped_steps) == 0 and int(opt.state[params[0]]["step"]) == STEPS
    n_nan = 0
    for i, (a, b) in enumerate(zip(params, p32)):
        mask = torch.isnan(a.detach().cpu())
        assert torch.equal(mask, torch.isnan(b.detach())), "parameter %d" % i
        n_nan += int(mask.sum())
    assert n_nan > 0 and not bool(torch.isnan(params[GRADLESS]).any())


def _upload(recs, kind):
    raw = bytes((kind * len(recs))(*recs))
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev())


@pytest.mark.parametrize("value", [math.inf, math.nan], ids=["inf", "nan"])
@pytest.mark.parametrize("where", ["head", "body", "tail", "last"])
def test_entry_point_finds_a_non_finite_value_wherever_it_sits(where, value):
    """The C entry point on hand-built tables whose pointers sit one element past a 16-byte boundary, so that chunks have a
    scalar head (the arenas never produce one): chunk [6, 70) is 1 head element + 15 vectors + 3 tail elements.  A clean launch
    gives the float64 norm and takes a step; with one non-finite gradient in the head / body / tail of that chunk, or in the
    last element of the last chunk, the next launch changes no buffer and no step count, and counts one skipped step."""
    from n3dt import _lib
    L = _lib.lib()
    n, pad, o = 4103, 8, 1
    gen = torch.Generator().manual_seed(17)
    host = [torch.randn(n, generator=gen), torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 0.1, torch.rand(n, generator=gen) * 0.01]
    bufs = []
    for h in host:
        b = torch.full((pad + n + pad,), 5.0, device=dev())
        b[4 + o:4 + o + n] = h.to(dev())
        bufs.append(b)
    ptr = [b.data_ptr() + 4 * (4 + o) for b in bufs]
    assert all((q % 16) // 4 == o for q in ptr)
    bounds = [0, 1, 6, 70, 4099, n]
    chunks = [_lib.AdamChunk(a, 0, b - a) for a, b in zip(bounds[:-1], bounds[1:])]
    td = _upload([_lib.AdamTensor(ptr[0], ptr[1], ptr[2], ptr[3], n, 0, 1)], _lib.AdamTensor)
    cd = _upload(chunks, _lib.AdamChunk)
    gd = _upload([_lib.AdamGroup(1e-2, 0.9, 0.999, 1e-8, 1e-2, 0, 0)], _lib.AdamGroup)
    guard = torch.zeros(ctypes.sizeof(_lib.AdamGuard) // 4, dtype=torch.int32, device=dev())
    guard[:2] = torch.frombuffer(bytearray(bytes(_lib.AdamGuard(0.5, 1))[:8]), dtype=torch.int32).to(dev())
    partials = torch.full((len(chunks),), float("nan"), dtype=torch.float64, device=dev())  # contents immaterial
    counter = torch.tensor([4, 0, 0, 0], dtype=torch.int32, device=dev())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def launch():
        _lib.check(L.n3dt_flat_adam_guarded_step(td.data_ptr(), cd.data_ptr(), len(chunks), gd.data_ptr(), 1, counter.data_ptr(),
                                                 partials.data_ptr(), guard.data_ptr(), stream), "guarded step")
        torch.cuda.synchronize()
        return _lib.AdamGuard.from_buffer_copy(guard.cpu().numpy().tobytes())
    rec = launch()
    want = float(host[1].double().norm())
    check_norm("clean", rec.grad_norm, want)
    assert rec.skip == 0 and rec.skipped_steps == 0 and rec.norm_done == 0 and counter.tolist() == [5, 0, 0, 0]
    assert abs(rec.clip_coef - 0.5 / (want + 1e-6)) <= 2.0 ** -21 * rec.clip_coef and rec.clip_coef < 1.0  # five fp32 roundings
    assert bool((bufs[0][4 + o:4 + o + n].cpu() != host[0]).any())  # the clean step moved the parameters
    index = {"head": 6, "body": 7 + 4 * 9 + 2, "tail": 69, "last": n - 1}[where]
    bufs[1][4 + o + index] = value
    before = [b.clone() for b in bufs]
    rec = launch()
    assert not math.isfinite(rec.grad_norm)
    assert rec.skip == 1 and rec.skipped_steps == 1 and rec.norm_done == 0 and counter.tolist() == [5, 0, 0, 0]
    for b, b0 in zip(bufs, before):
        assert torch.equal(b.view(torch.int32), b0.view(torch.int32))


# ---- 5. range ----------------------------------------------------------------------------------------------------------
def test_gradients_of_1e30_have_a_finite_norm_and_are_not_skipped(case):
    gen = torch.Generator().manual_seed(9)
    row = []
    for i, s in enumerate(SHAPES):
        row.append(None if i == GRADLESS else (torch.randint(0, 2, s, generator=gen) * 2.0 - 1.0) * 1e30)
    want = math.sqrt(sum(float((g.double() ** 2).sum()) for g in row if g is not None))
    assert math.isfinite(want) and want > 3.5e19  # (the square root of fp32's largest number: an fp32 sum of squares is inf)
    params, opt = flat_run(case["init"], [row], max_grad_norm=1.0, skip_nonfinite=True)
    check_norm("1e30", float(opt.grad_norm), want)
    assert int(opt.skipped_steps) == 0 and int(opt.state[params[0]]["step"]) == 1
    assert 0.0 < float(opt.clip_coef) < 1e-30
    assert all(bool(torch.isfinite(p).all()) for p in params)
    assert not torch.equal(params[BIG].detach().cpu(), case["init"][BIG])


# ---- 6. determinism, 7. graph ------------------------------------------------------------------------------------------
def replay_run(init, grads, events=None, **kw):
    """One eager step on row 0, capture of step() with the gradients bound to the arena, then one replay per remaining row with
    nothing between replays but .copy_() of the gradients -- and events[k](opt), when given, before the replay of row k."""
    from n3dt import FlatAdam
    params = make_params(init, torch.float32, dev())
    opt = FlatAdam(groups_of(params), **kw)
    feed(params, grads[0])
    opt.step()
    norms = [opt.grad_norm.clone()]
    slices = [p.grad for p in params]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
        norm_out = opt.grad_norm.clone()
    for k in range(1, len(grads)):
        for s, g in zip(slices, grads[k]):
            if g is not None:
                s.copy_(g.to(dev()))
        if events and k in events:
            events[k](opt)
        graph.replay()
        norms.append(norm_out.clone())
    torch.cuda.synchronize()
    return params, opt, norms


def test_two_runs_and_a_graph_replay_agree_to_the_bit(case):
    grads = case["grads"][:4]
    norms = [[], []]
    runs = [flat_run(case["init"], grads, after=lambda k, p, o, n=n: n.append(o.grad_norm.clone()), max_grad_norm=MAX_NORM, skip_nonfinite=True)
            for n in norms]
    assert same_bits(raw_state(*runs[0]), raw_state(*runs[1]))
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(*norms))
    # the same rows with steps 1.. replayed from a graph (capturing runs nothing): the same norms and the same state
    params, opt, replayed = replay_run(case["init"], grads, max_grad_norm=MAX_NORM, skip_nonfinite=True)
    assert len(replayed) == len(norms[0]) == 4
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(norms[0], replayed))
    assert same_bits(raw_state(params, opt), raw_state(*runs[0]))


def test_skip_and_a_new_max_grad_norm_inside_graph_replays(case):
    """Rows: 0 eager; capture (the capture itself runs nothing); replays of rows 1..6, row 3 poisoned, max_grad_norm raised above
    every norm before row 5.  Reference: float64 without row 3, with the per-row max_norm."""
    plants = {3: (BIG, 4096 + 7, math.nan)}
    grads = planted(case["grads"], plants)
    max_norms = [MAX_NORM] * 5 + [1e9] * 2
    keep = [k for k in range(STEPS) if k not in plants]
    ref = reference(case["init"], [case["grads"][k] for k in keep], [max_norms[k] for k in keep])
    seen = {}

    def raise_max(opt):
        seen["coef_row4"] = float(opt.clip_coef)
        seen["skipped_by_row4"] = int(opt.skipped_steps)
        opt.max_grad_norm = 1e9
        opt.sync_hyperparameters()
    params, opt, norms = replay_run(case["init"], grads, events={5: raise_max}, max_grad_norm=MAX_NORM, skip_nonfinite=True)
    assert seen["coef_row4"] < 1.0 and seen["skipped_by_row4"] == 1  # row 4 clips; row 3 was skipped inside its replay
    assert float(opt.clip_coef) == 1.0  # row 6 would clip at MAX_NORM (its norm is about 810)
    assert case["norms"][6] > MAX_NORM
    assert int(opt.skipped_steps) == 1 and int(opt.state[params[0]]["step"]) == STEPS - 1
    assert math.isnan(float(norms[3]))
    for k, j in zip(keep, range(len(keep))):
        check_norm("row %d" % k, float(norms[k]), ref["norms"][j])
    check("graph", state_of(params, opt), ref["ref"], ref["floor"])
