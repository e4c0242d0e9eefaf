"""No GPU: what tests/test_gpu_psola_envelope.py takes for granted, asserted on the restatement (tests/helpers/psola_ref.py) and
the case table (tests/helpers/psola_envelope.py) alone.  The ring-stress case reaches the two maxima the ring induction of
csrc/psola.hip allows (a range starting 2048 samples after the last one, a voiced range 2559 samples into the half not yet
committed) and stays inside the live halves under the kernel's own rule; the long case wraps the period ring; every numeric
case's fp32 statement is within fp32_bound of its fp64 one, with next to no sample on the weight floor; the hostile-marks
restatement keeps every index in the clip; the ramps' closed forms are the restatement's marks."""
from fractions import Fraction

import numpy as np
import pytest

from tests.helpers import psola_envelope as E, psola_ref as R


def trace(x, f, geo):
    return R.marks_trace(x, len(x), f, geo.hop, geo.sr, geo.P_u, geo.P_min, geo.P_max, geo.alpha)


def test_the_ring_stress_case_reaches_both_maxima_of_the_induction():
    x, f = E.stress()
    g = E.STRESS
    assert len(x) == 60000 and len(f) == 3751 and set(np.unique(f)) == {np.float32(0), np.float32(22050 / 1024)}
    assert R.period(f.max(), g.sr, g.P_u, g.P_min, g.P_max) == 1024 and R.period(0.0, g.sr, g.P_u, g.P_min, g.P_max) == -1024
    marks, searches = trace(x, f, g)
    w = E.ring_walk(marks, searches, g.hop, len(f))
    print("ring stress:", w, len(marks), "marks")
    assert w["step"] == 2048 and w["reach"] == 2559              # the most the contract (P <= 1024, alpha <= 1/2) allows
    assert w["advances"] >= 14 and w["frame"] > 3 * E.PS_FR and w["inside"]
    assert all(lo >= 0 and hi - lo + 1 <= 1025 for lo, hi, _ in searches)


def test_the_seam_case_reads_the_frame_two_halves_share_after_a_commit():
    x, f = E.seam()
    g = E.STRESS
    marks, searches = trace(x, f, g)
    k = marks.index(E.PS_H)
    assert marks[:k + 2] == [0, 1024, 2048, 3072, 4096, 4096 + 256]
    assert searches[k - 1][0] == E.PS_H                          # the search that found 4096 starts in half 1: it commits half 2 ...
    t = R.frame(E.PS_H, g.hop, len(f))
    assert t == 256 and len(f) > 768 and (E.PS_H * 2 + E.PS_H - 1 + g.hop // 2) // g.hop == 768          # ... whose last frame is 768
    assert R.period(f[256], g.sr, g.P_u, g.P_min, g.P_max) == 512 and R.period(f[768], g.sr, g.P_u, g.P_min, g.P_max) == -1024
    f2 = f.copy()
    f2[256] = f[768]                                             # what a period ring of 512 slots would hold by then
    assert trace(x, f2, g)[0][k + 1] == E.PS_H + 1024
    assert E.ring_walk(marks, searches, g.hop, len(f))["inside"]


def test_the_long_case_wraps_the_period_ring():
    c = E.BY_NAME["long"]
    x, f, _ = E.build(c)
    marks, searches = trace(x, f, c.geo)
    w = E.ring_walk(marks, searches, c.geo.hop, len(f))
    print("long:", w, len(marks), "marks")
    assert w["frame"] >= E.PS_FR and w["advances"] >= 70 and w["inside"]


@pytest.mark.parametrize("name", [c.name for c in E.CASES])
def test_every_search_of_every_case_lies_in_the_live_halves(name):
    c = E.BY_NAME[name]
    x, f, _ = E.build(c)
    marks, searches = trace(x, f, c.geo)
    w = E.ring_walk(marks, searches, c.geo.hop, len(f))
    assert w["inside"] and w["step"] <= 2048 and w["reach"] <= 2559 and len(marks) == len(searches) + 1
    G, K_max, H_max, _, _ = R.sizes(c.n, c.geo.P_min, c.geo.P_max, c.geo.alpha)
    gaps = np.diff(marks)
    assert len(marks) <= K_max and gaps.min() >= G and gaps.max() <= H_max and marks[-1] <= c.n - 1


def test_the_cases_are_the_corners_they_are_named_for():
    g = E.BY_NAME["narrowest"].geo
    assert R.sizes(6000, g.P_min, g.P_max, g.alpha) == (1, 6000, 12, 1, 6000)           # G = 1: K_max = J_max = L
    assert R.clamp(g.P_u, g.P_min, g.P_max) == 2 and R.period(2000.0, g.sr, g.P_u, g.P_min, g.P_max) == 4
    g = E.BY_NAME["big denominator"].geo
    assert g.alpha[0] * g.P_max < 1 << 31 and g.alpha[0] * 2 <= g.alpha[1] == 1 << 20 and g.alpha[0] * g.P_max >= 1 << 26
    g = E.BY_NAME["P_u above"].geo
    assert R.clamp(g.P_u, g.P_min, g.P_max) == 339
    x, f, _ = E.build(E.BY_NAME["P_u above"])
    assert not f.any() and (np.diff(trace(x, f, g)[0]) == 339).all()
    x, f, _ = E.build(E.BY_NAME["widest"])
    P = {R.period(v, 22050, 700, 512, 1024) for v in f}
    assert P == {882, -700} and 0.05 < (f == 0).mean() < 0.3
    assert len(E.build(E.BY_NAME["T = 1"])[1]) == 1 and len(E.build(E.BY_NAME["one frame for all"])[1]) == 1
    assert len(E.build(E.BY_NAME["short track"])[1]) == 20 < 1 + 20000 // 256


@pytest.mark.parametrize("name", [c.name for c in E.CASES])
def test_fp32_statement_within_the_bound_of_the_fp64_one(name):
    c = E.BY_NAME[name]
    x, fi, fo = E.build(c)
    r32, r64 = E.reference(x, c.n, fi, fo, c.geo), E.reference(x, c.n, fi, fo, c.geo, dtype=np.float64)
    assert r32["marks"] == r64["marks"] and r32["syn"] == r64["syn"] and r32["map"] == r64["map"]
    _, K_max, H_max, _, J_max = R.sizes(c.n, c.geo.P_min, c.geo.P_max, c.geo.alpha)
    assert len(r32["syn"]) <= J_max and (np.diff(r32["syn"]) >= 1).all()
    again = E.reference(x, c.n, fi, fo, c.geo, J_max=J_max, H_max=H_max)                 # neither stop binds on well-formed marks
    assert again["syn"] == r32["syn"] and np.array_equal(again["out"].view(np.uint32), r32["out"].view(np.uint32))
    bound = R.fp32_bound(r64["den"], r64["grains"], float(np.abs(x).max()))
    safe = np.abs(r64["den"] - R.MIN_WEIGHT) > 1e-5
    assert (~safe).sum() <= 0.001 * c.n, (int((~safe).sum()), c.n)
    err = np.abs(r32["out"].astype(np.float64) - r64["out"])
    worst = float((err[safe] / np.maximum(bound[safe], 1e-300)).max())
    print(f"{name}: {len(r32['marks'])} marks, {len(r32['syn'])} synthesis marks, on the floor {int((~safe).sum())}, error / bound {worst:.4f}")
    assert (err[safe] <= bound[safe]).all()
    if c.ratio != 1.0 and c.unvoiced < 1.0:
        assert r32["syn"] != r32["marks"] and (err > 0).any()                            # the case does compute something


def test_hostile_marks_restatement_stays_inside_the_clip():
    c = E.SMALL
    x, fi, fo = E.build(c)
    g = c.geo
    _, K_max, H_max, _, J_max = R.sizes(c.n, g.P_min, g.P_max, g.alpha)
    true = R.marks_ref(x, c.n, fi, g.hop, g.sr, g.P_u, g.P_min, g.P_max, g.alpha)
    row = np.full(K_max, -1, dtype=np.int32)
    row[:len(true)] = true
    for name, (r, count) in E.hostile(row, len(true), K_max, c.n).items():
        marks = R.clamped_marks(r, count, K_max, c.n)
        assert len(marks) == min(max(count, 0), K_max) and all(0 <= m <= c.n - 1 for m in marks), name
        ref = E.reference(x, c.n, fi, fo, g, J_max=J_max, H_max=H_max, marks=r, clamps=(count, K_max))
        J = len(ref["syn"])
        assert J <= J_max and (J > 0) == (len(marks) > 0), name
        assert all(0 <= s <= c.n - 1 for s in ref["syn"]) and all(0 <= a < len(marks) for a in ref["map"]), name
        assert (np.diff(ref["syn"]) >= 1).all() and np.isfinite(ref["out"]).all(), name
        if name not in ("count -5", "count 0"):
            assert not np.array_equal(np.asarray(marks), np.asarray(true)), name           # the row is hostile
    tight = R.syn_ref(true, fi, fo, g.hop, g.P_u, g.P_min, g.P_max, J_max=5)               # the stop itself
    assert len(tight[0]) == 5 and tight[0] == R.syn_ref(true, fi, fo, g.hop, g.P_u, g.P_min, g.P_max)[0][:5]


@pytest.mark.parametrize("geo,P,n", [(E.DEFAULT, 339, 60000), (E.WIDE, 1024, 60000), (E.DEFAULT, 339, 200), (E.WIDE, 1024, 1025)])
def test_ramp_closed_forms_equal_the_restatement(geo, P, n):
    f = E.constant_track(n, geo, P)
    assert {R.period(v, geo.sr, geo.P_u, geo.P_min, geo.P_max) for v in f} == {P}
    up, _ = trace(E.ramp(n), f, geo)
    down, _ = trace(E.ramp(n, -1), f, geo)
    assert up == E.rising_marks(n, P, geo.alpha) and down == E.falling_marks(n, P, geo.alpha)
    if (P, n) == (339, 60000):
        assert (len(up), len(down)) == (142, 236)


def test_the_tie_of_the_ratio_edges_is_exact_in_fp64():
    r = np.float64(np.float32(100.0)) / np.float64(np.float32(150.0))
    assert 147.0 / r == 220.5 and Fraction(147) / Fraction(float(r)) > Fraction(441, 2)   # r is below 2 / 3; the fp64 quotient rounds onto the tie
    assert 147.0 / (np.float64(np.float32(300.0)) / np.float64(np.float32(150.0))) == 73.5
    x, f = E.pulses(E.EDGE_N, 147), E.constant_track(E.EDGE_N, E.DEFAULT, 147)
    marks, _ = trace(x, f, E.DEFAULT)
    assert marks[0] == 0 and (np.diff(marks) == 147).all() and len(marks) == 41
    assert E.RATIO_EDGES[0][1] / E.RATIO_EDGES[0][0] == 0.25 and E.RATIO_EDGES[1][1] / E.RATIO_EDGES[1][0] == 4.0
    for (vi, vo), want in zip(E.RATIO_EDGES[2:6], ("below", "above", "inside", "inside")):
        q = np.float64(vo) / np.float64(vi)
        assert {"below": q < 0.25, "above": q > 4.0, "inside": 0.25 < q < 4.0}[want], (vi, vo)
    fi, fo = E.edge_tracks(E.EDGE_N, E.DEFAULT)
    assert np.array_equal(fi, f)
    s = np.array(E.reference(x, E.EDGE_N, fi, fo, E.DEFAULT)["syn"])
    edge = (np.array([R.frame(int(v), E.DEFAULT.hop, len(fi)) for v in s[:-1]]) // 3) % len(E.RATIO_EDGES)
    for e, want in enumerate((588, 37, 588, 37, 588, 37, 221, 74)):       # every edge decides a step: 147 / r, the two ties rounded up
        assert (edge == e).any() and (np.diff(s)[edge == e] == want).all(), (e, want)
