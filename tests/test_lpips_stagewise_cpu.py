"""CPU checks of the stage-wise pin of LPIPS (tests/lpips_stagewise.py): the restated layouts against the library's size queries, the
pack decode as a bijection, the float32 prologue against the restatement's, the conv floors the GPU bounds of
test_gpu_lpips_stagewise.py are derived from (4 x FLOOR, never a GPU figure), the emulated chain under every rule, and one deliberate
fault at a time -- each must be reported by the rule named for it, and the table says which of them the score and layer bounds of
test_gpu_lpips.py would have reported."""
import functools

import numpy as np
import pytest
import torch

import lpips_restatement as lr
import lpips_stagewise as ls


# ---- layouts -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(ls.CASES))
def test_workspace_layout_mirrors_the_library(case):
    from n3dt import _lib
    B, H, W = ls.CASES[case]
    reg, poff, total = ls.ws_layout(B, H, W)
    assert total == _lib.lib().n3dt_lpips_workspace_bytes(B, H, W)
    assert list(reg) == list(ls.NAMES) and all(o % 256 == 0 for o, _ in reg.values()) and poff % 256 == 0
    ends = [o + 4 * ls.rup(int(np.prod(s)), 64) for o, s in reg.values()]
    assert [o for o, _ in reg.values()][1:] + [poff] == ends          # back to back, each rounded up to 64 floats
    assert total - poff == ls.LAYERS * B * ls.PARTS * 8
    for name, (_, shp) in reg.items():                                 # the halos of lpips_core.h
        inner = ls.interior(name, np.zeros(shp, np.int8)).shape
        assert shp[1] - inner[1] == shp[2] - inner[2] == 2 * ls.PAD[name]
    x = torch.zeros(1, 3, H, W)                                        # the extents are torch's own
    convs = [(torch.zeros(c[2], c[1], c[3], c[3]), torch.zeros(c[2])) for c in lr.CONVS]
    feats = lr.features(x, convs, torch.float32)
    for name, f in zip(ls.RELU, feats):
        assert ls.interior(name, np.zeros(reg[name][1], np.int8)).shape[1:] == (f.shape[2], f.shape[3], f.shape[1])
    written = ls.ws_written(B, H, W)
    assert written.sum() == sum(4 * int(np.prod(s)) for _, s in reg.values()) + total - poff
    slack = 4 * (ls.rup(int(np.prod(reg["in0"][1])), 64) - int(np.prod(reg["in0"][1])))      # every other map is a multiple of 64 floats
    assert (~written).sum() == slack and (slack > 0) == (case != "cap")


def test_case_geometries_are_the_ones_the_cases_are_for():
    s = {c: ls.shapes(*ls.CASES[c]) for c in ls.CASES}
    assert [s["min"][n][1:3] for n in ("relu1", "relu2", "relu5")] == [(7, 7), (3, 3), (1, 1)]
    assert s["odd"]["relu1"][1:3] == (16, 14) and s["odd"]["relu2"][1:3] == (7, 6) and s["odd"]["relu5"][1:3] == (3, 2)
    assert 6 * 16 * 14 == 1344 == 5 * 256 + 64 and 6 * 7 * 6 == 252                         # five workgroups plus one wave; a 60-row tail
    assert 2 * 7 + 1 < 16 and 2 * 6 + 1 < 14 and 2 * 2 + 1 < 6 and 2 * 3 + 1 == 7           # pool1 drops a row and a column, pool2 a column
    assert s["wide"]["relu1"][1:3] == (31, 23) and 31 * 23 == 713 > 4 * ls.PARTS and s["wide"]["relu5"][1:3] == (7, 5) and 4 * 35 == 140
    assert ls.CASES["cap"][0] == ls.MAX_BATCH
    assert ls.part_of_pixel(713).max() == 127 and ls.part_of_pixel(713)[512] == 0 and ls.part_of_pixel(713)[515] == 0 and ls.part_of_pixel(713)[516] == 1


def test_pack_layout_mirrors_the_library_and_the_decode_is_a_bijection():
    from n3dt import _lib
    pw, elems, pb, pl, total = ls.pack_layout()
    assert total == _lib.lib().n3dt_lpips_packed_bytes()
    assert all(o % 256 == 0 for o in pw + pb + pl) and pw[0] == 0 and pb[0] == ls.rup(pw[4] + 4 * elems[4], 256) and pl[0] > pb[4]
    for l in range(ls.LAYERS):
        nt = ls.COUT[l] // 32
        k, n = ls.pack_decode(np.arange(elems[l]), nt)
        assert k.min() == 0 and k.max() == ls.KP[l] - 1 and n.min() == 0 and n.max() == ls.COUT[l] - 1
        assert len(np.unique(k * ls.COUT[l] + n)) == elems[l] == ls.KP[l] * ls.COUT[l]      # onto [0, kp) x [0, cout), each once
        # the inverse is the address the MFMA step reads: fragment (s, t), lane (r = n % 32, h), element j (conv_frag.h: cf_frag_elem)
        s, t, h, j = k // 16, n // 32, (k % 16) // 8, k % 8
        assert np.array_equal(((s * nt + t) * 64 + 32 * h + n % 32) * 8 + j, np.arange(elems[l]))
    assert ls.K == (363, 1600, 1728, 3456, 2304) and ls.KP[0] == 368


def test_expected_pack_splits_every_weight_and_zeroes_the_padded_rows():
    W = ls.weights()[0]
    buf = ls.expected_pack(W, ls.pack_layout()[4] + 256)
    assert ls.judge_pack(buf, W) is None and np.all(buf[-256:] == ls.PREFILL)
    dec = ls.decode_pack(buf)
    for l, (w, b, lin) in enumerate(W):
        hi, lo, bias, ln = dec[l]
        m = ls.weight_matrix(w)
        assert np.array_equal(hi, ls.vs.bf16_rne(m)) and np.array_equal(lo, ls.vs.bf16_rne(m - hi))
        assert np.abs((hi.astype(np.float64) + lo) - m).max() <= 2.0 ** -16 * np.abs(m).max()
        assert ls.same_bits(bias, b) and ls.same_bits(ln, lin)
        tap, ci = 7, ls.CIN[l] - 1
        assert m[tap * ls.CIN[l] + ci, 5] == w[5, ci, tap // ls.KSIZE[l], tap % ls.KSIZE[l]]
    assert not dec[0][0][363:].view(np.uint32).any() and not dec[0][1][363:].view(np.uint32).any()      # +0, not -0
    for fault in ("pack_swap", "pack_trunc"):
        assert ls.judge_pack(ls.expected_pack(W, fault=fault), W) is not None


# ---- the inputs and the prologue -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,mode", ls.RUNS)
def test_inputs_hold_what_the_prologue_rule_needs(case, mode):
    B, H, W = ls.CASES[case]
    pred, gt = ls.images(case, mode)
    assert pred.shape == gt.shape == (B, 3, H, W) and pred.dtype == gt.dtype == np.float32
    for x in (pred, gt):
        assert np.isnan(x).any() and (x < 0).any() and (x > 1).any() and (x == 1).any() and np.isinf(x).any()
        assert ((x == 0) & np.signbit(x)).any() and ((x == 0) & ~np.signbit(x)).any()
    same = ls.identical_pairs(pred, gt)
    assert same == {"min": [], "odd": [], "wide": [1], "cap": [7, 15, 23, 31, 39, 47, 55, 63]}[case] and 0 not in same
    # the float32 prologue is the restatement's own scaling of its own input forms, bit for bit
    want = torch.cat([lr.scaling(lr.INPUTS[mode](img)) for img in np.concatenate([pred, gt])]).permute(0, 2, 3, 1).numpy()
    got = ls.in0_expected(pred, gt, mode)
    assert ls.same_bits(ls.interior("in0", got), want) and ls.halo_is_plus_zero("in0", got) and np.isfinite(got).all()
    if mode == "reference":
        fed_a, _ = ls.fed_bytes(case, mode)
        x = (ls.interior("in0", got)[:B] * ls.SCALE + ls.SHIFT).round().astype(np.int64).transpose(0, 3, 1, 2)
        assert (x != fed_a).sum() <= len(ls.SPECIALS)       # through the quantiser and the reshape the network sees the fed bytes
    assert ls.CASES["odd"][1] != ls.CASES["odd"][2] and ls.CASES["wide"][1] != ls.CASES["wide"][2]


# ---- floors, and the emulated chain under every rule --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chain(case, mode):
    m = []
    ws, pack, out, layers = ls.emulate(case, mode, measure=m)
    return ws, pack, out, layers, tuple(m)


def test_floors_have_not_moved():
    """FLOOR re-measured over every run and the three accumulation forms (ascending and descending K steps of 16, torch's float32
    convolution of the same split products).  A GPU bound is MARGIN x FLOOR."""
    measured = [0.0] * ls.LAYERS
    for case, mode in ls.RUNS:
        for l, v in chain(case, mode)[4]:
            measured[l] = max(measured[l], v)
    for l in range(ls.LAYERS):
        print("conv%d: measured floor %.3e, constant %.3e, bound %.3e" % (l + 1, measured[l], ls.FLOOR[l], ls.bound(l)))
    for l in range(ls.LAYERS):
        assert measured[l] <= ls.FLOOR[l] <= 1.25 * measured[l], (l, measured[l], ls.FLOOR[l])
        assert ls.bound(l) == 4.0 * ls.FLOOR[l]
    assert ls.MARGIN == 4.0 and ls.PARTIAL_BOUND == 1e-13


@pytest.mark.parametrize("case,mode", ls.RUNS)
def test_emulated_chain_passes_every_rule(case, mode):
    B, H, W = ls.CASES[case]
    ws, pack, out, layers, _ = chain(case, mode)
    worst, fails = ls.judge(case, mode, ws, out, layers)
    print("%s %s: " % (case, mode) + "  ".join("%s %.3g" % kv for kv in worst.items()))
    assert not fails, "\n" + "\n".join(m for _, m in fails)
    assert ls.judge_pack(pack, ls.weights()[0]) is None
    for prefill in (0xFF, 0x00):        # nothing is read before it is written
        other = ls.emulate(case, mode, prefill)
        assert ls.same_results(ws, other[0], B, H, W) is None and ls.same_bits(out, other[2]) and ls.same_bits(layers, other[3])
    # the chain is the metric: within the end-to-end bounds of the free-running float64 restatement
    assert not ls.old_bounds_report(case, mode, out, layers)
    score, lay = ls.restated(case, mode)
    live = [b for b in range(B) if b not in ls.identical_pairs(*ls.images(case, mode))]
    assert (score[live] > 0.1).all() and (lay[:, live] > 0).all()


def test_partials_reference_owns_every_pixel_once():
    rng = np.random.default_rng(0)
    feat = np.maximum(rng.standard_normal((4, 31, 23, 64)), 0).astype(np.float32)
    lin = np.abs(rng.standard_normal(64)).astype(np.float32)
    ref, S, owns = ls.partials_reference(feat, 2, lin)
    assert owns.all() and (S >= ref).all() and (ref > 0).all()
    t = torch.from_numpy(feat).double().permute(0, 3, 1, 2)
    want = lr.distance(t[:2], t[2:], torch.from_numpy(lin)).numpy()
    assert np.abs(ref.sum(axis=1) / 713 / want - 1).max() <= 1e-13
    assert not ls.partials_reference(feat[:, :1, :2], 2, lin)[2][1:].any()          # two pixels: part 0 alone
    part = ls.part_of_pixel(713)
    assert np.array_equal(np.bincount(part), np.where(np.arange(128) < 51, 8, 4) - np.where(np.arange(128) == 50, 3, 0))


# ---- deliberate faults ------------------------------------------------------------------------------------------------------------------
# the faults test_gpu_lpips.py's bounds on the score and the layer values let through at these cases
OLD_BOUNDS_MISS = {"gather_363", "pool_halo", "relu3_halo_cell", "no_eps", "layer_order", "pack_trunc"}


def test_each_deliberate_fault_is_reported_by_the_rule_named_for_it():
    W = ls.weights()[0]
    table = []
    for fault, rule in ls.FAULTS.items():
        seen, old, silent, runs = set(), [], True, 0
        for case, mode in (ls.RUNS if fault == "layer_order" else ls.FAULT_RUNS):   # five terms re-ordered often give the same bits: all 67 live pairs
            ws, pack, out, layers = ls.emulate(case, mode, fault=fault)
            _, fails = ls.judge(case, mode, ws, out, layers)
            if ls.judge_pack(pack, W) is not None:
                fails = fails + [("pack", "")]
            good = chain(case, mode)
            silent = silent and not fails and ls.same_bits(out, good[2]) and ls.same_bits(layers, good[3])
            seen |= {"%s (%s %s)" % (r, case, mode) for r, _ in fails}
            runs += 1
            old += ["%s %s" % (case, mode)] if ls.old_bounds_report(case, mode, out, layers) else []
        table.append((fault, rule, sorted(seen), old, silent, runs))
    print("%-16s %-70s %s" % ("fault", "reported by (the first three)", "old score / layer bounds"))
    for fault, rule, seen, old, _, runs in table:
        what = ", ".join(seen[:3]) + (" ... %d in all" % len(seen) if len(seen) > 3 else "") if seen else "nothing"
        print("%-16s %-70s %s" % (fault, what, "report it in %d of %d runs: %s" % (len(old), runs, ", ".join(old)) if old else "pass in all %d runs" % runs))
    for fault, rule, seen, old, silent, _ in table:
        if rule is None:
            assert fault in ls.INDISTINGUISHABLE and silent and not old, (fault, seen)
        else:
            assert any(s.startswith(rule) for s in seen), (fault, rule, seen)
    assert set(ls.INDISTINGUISHABLE) == {f for f, r in ls.FAULTS.items() if r is None}
    # the justification of the pin, recorded in DESIGN section 4: what the end-to-end bounds let through
    assert {f for f, _, _, old, _, _ in table if not old} >= OLD_BOUNDS_MISS, [f for f, _, _, old, _, _ in table if not old]


def test_gpu_bounds_are_the_floors_times_four():
    import test_gpu_lpips as old
    import test_gpu_lpips_stagewise as g
    assert g.BOUND == tuple(4.0 * f for f in ls.FLOOR) and all(b > 0 for b in g.BOUND)
    assert (ls.OLD_SCORE_TOL, ls.OLD_LAYER_TOL) == (old.SCORE_TOL, old.LAYER_TOL)
