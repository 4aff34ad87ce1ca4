"""CPU side of the pin of the hierarchical pass (tests/hier_stagewise.py):
  * the float64 restatement of fine_sample_kernel reproduces the reference's own fine planes (tests/golden/hier_test, hier_train) from
    their coarse weights, coarse z values and u, to what fixtures written in float32 allow (measured and recorded below, not assumed), and
    the oracle's float32 fine_sample passes every rule against it;
  * every floor of hier_stagewise.FLOOR re-measured from the float32 emulations (four orders) against the restatement over all cases; a
    floor that moved, up or down by more than a quarter, fails;
  * every emulation passes every rule in every case; the restatement alone leaves at most 2 % of the draws of any random case undecided;
  * each deliberate fault of the emulation is reported by the rule named for it, or stands in INDISTINGUISHABLE with its reason and is
    then asserted to stay invisible;
  * the same for the given-plane branch of the point sampler.
No GPU.

Undecided shares of the restatement alone, seeds as committed (test_undecided_cap re-asserts the 2 % cap): none at the five smaller
shapes, 0.15 - 0.59 % at (1024, 1023)."""
import functools

import numpy as np
import pytest

import hier_stagewise as hh
from conftest import load_golden
from oracle import oracle as orc

ALL = hh.case_names()

# what the float32 fixtures allow: the largest |restated plane - fixture plane| over both fixtures, measured 2026-10 (printed by the test)
FIXTURE_AGREEMENT = {"hier_test": 7.0e-6, "hier_train": 4.0e-6}   # measured 6.91e-6 and 3.93e-6: seven float32 steps of a plane near 12


@functools.lru_cache(maxsize=None)
def reference(name):
    c = hh.case(name)
    zc = hh.coarse_planes32(c)
    return c, zc, hh.restate(c["weight"], zc, hh.draw_u(c))


@functools.lru_cache(maxsize=None)
def emulation(name, variant, fault=None):
    c, zc, ref = reference(name)
    em = hh.emulate(c["weight"], zc, hh.draw_u(c), variant, fault, c)
    return em, hh.judge(em["z_out"], zc, ref, c["Nc"])


@pytest.mark.parametrize("name", ["hier_test", "hier_train"])
def test_restatement_reproduces_the_reference_fixtures(name):
    g, m = load_golden(name)
    w, zc = g["coarse_weight"], g["coarse_zvals"]
    B, _, Nr, Nc = w.shape
    Nf = m["num_sample_fine"]
    R = B * Nr
    u = g["fine_u"].reshape(R, Nf + 1) if m["mode"] == "train" else np.broadcast_to(hh.linspace01(np.float32, Nf + 1), (R, Nf + 1))
    ref = hh.restate(w.reshape(R, Nc), zc.reshape(R, Nc), u)
    fix = g["fine_zvals"][:, 0].reshape(R, Nc + Nf).astype(np.float64)
    err = np.abs(ref["planes"][:, :-1] - fix)
    iv = hh.intervals(ref, Nc)
    print("%s: |restated - fixture| max %.3e, q99 %.3e; %.4f of the draws undecided; recorded %.1e" % (
        name, err.max(), np.quantile(err, 0.99), (~iv["decided"]).mean(), FIXTURE_AGREEMENT[name]))
    assert 0.8 * FIXTURE_AGREEMENT[name] <= err.max() <= FIXTURE_AGREEMENT[name], "the recorded agreement is the measured one"
    # the oracle (float32, sequential normaliser, qsort) against the restatement, by the rules
    planes = orc.fine_sample(w, zc, Nf, g["fine_u"] if m["mode"] == "train" else None).reshape(R, Nc + Nf + 1)
    f = hh.judge(planes, zc.reshape(R, Nc), ref, Nc)
    v = hh.show("oracle.fine_sample on " + name, f)
    print("    |oracle - restated| max %.3e (a flat figure: where it is largest the draw is ill-conditioned, and the rules say by how much)"
          % np.abs(planes - ref["planes"]).max())
    assert hh.failing(v) == []


def test_the_oracle_at_the_smallest_call():
    """n_fine = 0 with the default u: torch.linspace(0, 1, 1) is [0], not the NaN of a step 1 / 0 (the defect rule order found in the kernel)"""
    c, zc, ref = reference("rand_3_0_given_linspace")
    R = zc.shape[0]
    planes = orc.fine_sample(c["weight"].reshape(1, 1, R, 3), zc.reshape(1, 1, R, 3), 0, None).reshape(R, 4)
    v = hh.show("oracle.fine_sample (3, 0)", hh.judge(planes, zc, ref, 3))
    assert hh.failing(v) == []


@functools.lru_cache(maxsize=None)
def measured():
    out = {}
    for name in ALL:
        c, zc, ref = reference(name)
        for variant in hh.VARIANTS:
            fl = hh.floors_of(emulation(name, variant)[0], ref, c["Nc"])
            assert fl["wrongly_decided"] == 0, (name, variant, "a decided draw took another decision in float32")
            for family in ("cdf", "z"):
                if family not in out or fl[family] > out[family][0]:
                    out[family] = (fl[family], "%s %s" % (name, variant))
    for name in POINT_CASES:
        c = hh.point_case(name)
        e = hh.sample_given(np.float32, c)
        f = hh.judge_points(c, e["pts"], e["dist"], e["zval"])
        if "dist" not in out or f["dist"] > out["dist"][0]:
            out["dist"] = (f["dist"], name)
    return out


@pytest.mark.parametrize("family", hh.FAMILIES)
def test_floor_is_its_recorded_constant(family):
    r, where = measured()[family]
    rec = hh.FLOOR[family]
    print("%-5s measured floor %.3e (%s), recorded %.3e, unit %.3e" % (family, r, where, rec, hh.unit(family)))
    assert 0.0 < r <= rec
    assert rec <= 1.25 * r, "the recorded constant is the measured floor rounded up, not a wider number"


@pytest.mark.parametrize("name", ALL)
def test_every_emulation_passes_every_rule(name):
    for variant in hh.VARIANTS:
        v = hh.show("%s %s" % (name, variant), emulation(name, variant)[1])
        assert hh.failing(v) == [], (name, variant, hh.failing(v))


@pytest.mark.parametrize("name", [n for n in ALL if hh.is_random(n)])
def test_undecided_cap(name):
    """a condition, not a measurement: the float64 restatement alone decides at least 98 % of the draws of every random case"""
    c, zc, ref = reference(name)
    share = float((~hh.intervals(ref, c["Nc"])["decided"]).mean())
    print("%-40s %.4f of the draws undecided" % (name, share))
    assert share <= hh.UNDECIDED_MAX


def test_hand_made_patterns_are_what_they_claim():
    for nc, nf in hh.PATTERN_SHAPES:
        c, zc, ref = reference("zero_%d_%d" % (nc, nf))
        assert (ref["cdf"] == 0).all() and (ref["inds"] == nc - 1).all() and (ref["denom"] == 1).all()
        assert (ref["z"] == ref["bins"][:, nc - 2:nc - 1]).all(), "all Nu values equal bins[Nc - 2]"
        assert hh.intervals(ref, nc)["decided"].all()
        c, zc, ref = reference("onehot_%d_%d" % (nc, nf))
        flat = (np.diff(ref["cdf"], axis=1) == 0).sum(1)
        assert (flat == nc - 3).all(), "one step in the cdf, flat runs on both sides"
        assert (ref["inds"][:, 0] > 1).all(), "u = 0 steps over the whole run of zeros (right=True)"
        c, zc, ref = reference("switch_%d_%d" % (nc, nf))
        iv = hh.intervals(ref, nc)
        dc = hh.take(iv["delta"], ref["above"])
        assert (ref["raw"][:, 0] < hh.EPS32).all() and (ref["raw"][:, 1:3] > hh.EPS32).all(), "one denom under, one over the switch"
        assert iv["decided"][:, :3].all()
        assert (np.abs(ref["raw"][:, :3] - hh.EPS32) >= 10 * dc[:, :3]).all(), "at least 10 delta_c from the switch"
        c, zc, ref = reference("uedge_%d_%d" % (nc, nf))
        iv = hh.intervals(ref, nc)
        assert not iv["decided"][:, 2].any(), "u equal to a float32 cdf entry is a tie the float64 reference cannot decide"
        assert (c["u"][:, 0] == 0).all() and (c["u"][:, 1] == 1).all()
        c, zc, ref = reference("ends_%d_%d" % (nc, nf))
        assert (c["weight"][:, [0, -1]] > 1e4).all() and ref["cdf"].max() <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# deliberate faults
# ---------------------------------------------------------------------------------------------------------------------
FAULT_CASES = tuple(n for n in ALL if not hh.is_random(n)) + tuple(
    "rand_%d_%d_%s_%s" % (nc, nf, pm, um) for (nc, nf) in ((3, 0), (16, 24), (66, 64)) for pm in hh.PLANE_MODES for um in hh.U_MODES)
# fault -> the figures (hier_stagewise.RULES) that are to report it
NAMED = {
    "right_false": ("z",), "above_nc1": ("z", "order", "prefill"), "no_switch": ("z", "prefill", "order", "count"), "eps_numerator": ("z",),
    "cumsum_w0": ("z",), "bins_lower": ("z",), "u_over_nu": ("z",), "no_tie_break": ("prefill", "count", "coarse"),
    "draws_ge_64": ("prefill", "count", "order"), "T_frame0": ("coarse",), "u_stride_nc": ("z",), "linspace_nu1": ("prefill",),
}
INDISTINGUISHABLE = {
    "switch_le": "`<=` differs from `<` only where the float32 difference of two cdf entries equals float32(1e-5) bit for bit; no case holds "
                 "such a draw (asserted here), and one built by hand would be undecided for the float64 reference by rule",
}


@pytest.mark.parametrize("fault", hh.FAULTS)
def test_deliberate_fault(fault):
    worst, rule, where = 0.0, None, None
    for name in FAULT_CASES:
        v = hh.verdict(emulation(name, "lanes", fault)[1])
        k = max(v, key=lambda q: v[q])
        if v[k] > 1.0:
            print("%-14s %-32s reported by: %s" % (fault, name, "  ".join("%s (%.3g)" % (hh.RULES[q], v[q]) for q in v if v[q] > 1.0)))
        if v[k] > worst:
            worst, rule, where = v[k], k, name
    if fault in INDISTINGUISHABLE:
        print("    listed as indistinguishable: " + INDISTINGUISHABLE[fault])
        assert worst <= 1.0, "%s is visible (rule %s, case %s): take it out of the table" % (fault, rule, where)
        for name in FAULT_CASES:
            assert not (emulation(name, "lanes")[0]["raw"] == np.float32(1e-5)).any()
    else:
        assert worst > 1.0, "%s is reported by no rule (worst %.3f x, rule %s, case %s)" % (fault, worst, rule, where)
        seen = set()
        for name in FAULT_CASES:
            v = hh.verdict(emulation(name, "lanes", fault)[1])
            seen |= {k for k in v if v[k] > 1.0}
        assert seen & set(NAMED[fault]), (fault, "reported by %s, not by the rule named for it %s" % (sorted(seen), NAMED[fault]))


# ---------------------------------------------------------------------------------------------------------------------
# given planes through the point sampler
# ---------------------------------------------------------------------------------------------------------------------
POINT_CASES = ("p40", "p65", "p3")
POINT_NAMED = {"stride_ns": ("zval_bits",), "zhi_next_ray": ("dist",), "dist_prev_pair": ("dist", "dist_nonzero")}


@pytest.mark.parametrize("name", POINT_CASES)
def test_point_emulation_passes_every_rule(name):
    c = hh.point_case(name)
    p = c["planes"]
    assert (np.diff(p, axis=-1) >= 0).all() and (np.diff(p, axis=-1)[..., -1] > np.diff(p, axis=-1)[..., :-1].max(-1)).all(), "last interval widest"
    e = hh.sample_given(np.float32, c)
    f = hh.judge_points(c, e["pts"], e["dist"], e["zval"])
    v = hh.show_points(name + " float32 emulation", f)
    assert hh.failing(v) == []
    if c["Ns"] >= 40:
        assert f["equal_planes"] == 2


@pytest.mark.parametrize("fault", hh.POINT_FAULTS)
def test_point_fault(fault):
    seen = set()
    for name in POINT_CASES:
        c = hh.point_case(name)
        e = hh.sample_given(np.float32, c, fault)
        v = hh.show_points("%s %s" % (fault, name), hh.judge_points(c, e["pts"], e["dist"], e["zval"]))
        seen |= set(hh.failing(v))
    assert seen & set(POINT_NAMED[fault]), (fault, sorted(seen))
