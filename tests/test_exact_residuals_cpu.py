"""The CPU oracle (oracle/src/estimator.cpp evaluate_point, ScoreModel sums) and the engine's
host LO sweep (host/lo_sweep.cpp through mp_debug_lo_sweep) against exact rational
arithmetic on the same input doubles (tests/exact_residuals.py) -- no device.

Both are double-precision restatements of the reference written for this project, and
every device test compares with one of them; this file is what pins them to the
reference's formulas themselves.  n = 300, eight models per pair (near the truth and
far), every variant and score type, a standard K pair and one whose K0 has entries below
the diagonal (kstd = 0).  Per case:

* the inputs the exact reference takes are the engine's and the oracle's to the bit
  (normalization scale, thresholds, weights);
* sentinels agree with the exact decision wherever the exact gate quantity is farther
  than 1e-9 (relative) from zero;
* |min(e, thr) - min(e_exact, thr)| <= tau_t (mp_score.h score_margins, through the
  host-only hook mp_debug_score_margins) outside the gate windows;
* each ScoreModel sum lies within the model's margin of the exact sum;
* the worst relative errors below the sentinel are printed: the yardstick of
  tests/test_score_exact_gpu.py (DESIGN.md §5 records them).
"""
from fractions import Fraction as Fr

import numpy as np
import pytest

from madpose_amd import api
from tests import exact_cases as xc
from tests import exact_residuals as ex


def test_exact_reference_basics():
    """The pieces of the exact reference on inputs with known answers."""
    K = [[Fr(3), Fr(1, 2), Fr(7)], [Fr(1, 4), Fr(5), Fr(-2)], [Fr(0), Fr(1, 8), Fr(1)]]
    Ki = ex.inv3(K)
    P = [[sum(K[r][k] * Ki[k][c] for k in range(3)) for c in range(3)] for r in range(3)]
    assert P == [[Fr(int(r == c)) for c in range(3)] for r in range(3)]
    # sign of p - q sqrt(n2): 3 - 2 sqrt(2) > 0, 2 - 3 sqrt(1/2) < 0, exact zero, mixed signs
    assert ex.sign_p_minus_q_root(Fr(3), Fr(2), Fr(2)) == 1
    assert ex.sign_p_minus_q_root(Fr(2), Fr(3), Fr(1, 2)) == -1
    assert ex.sign_p_minus_q_root(Fr(6), Fr(3), Fr(4)) == 0
    assert ex.sign_p_minus_q_root(Fr(-1), Fr(-1), Fr(4)) == 1
    assert ex.sign_p_minus_q_root(Fr(-1), Fr(1), Fr(4)) == -1
    assert ex.sign_p_minus_q_root(Fr(0), Fr(-1), Fr(4)) == 1
    assert ex.sign_p_minus_q_root(Fr(5), Fr(0), Fr(4)) == 1
    # a pure translation along x with identity intrinsics: the reprojection of a point at
    # depth 2 moves by t_x / 2; a correspondence on its epipolar line has Sampson error 0
    I3 = [[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]]
    pair = ex.Pair(0, [(0.25, 0.5)], [(0.75, 0.5)], [2.0], [2.0], I3, I3)
    T = ex.evaluate(pair, ex.Model(I3, [1.0, 0.0, 0.0]))
    assert T.err[0][0] == 0 and T.err[1][0] == 0 and T.err[2][0] == 0
    assert T.z[0][0] == Fr(2) - ex.GATE and T.lsign[0][0] == 1 and T.lsign[1][0] == 1
    T = ex.evaluate(pair, ex.Model(I3, [0.5, 0.0, 0.0]))
    assert T.err[0][0] == Fr(1, 16) and T.err[1][0] == Fr(1, 16) and T.err[2][0] == 0
    # behind the second camera: z < 1e-2
    T = ex.evaluate(pair, ex.Model(I3, [0.0, 0.0, -3.0]))
    assert T.sent[0][0] and T.err[0][0] == ex.SENTINEL and T.z[0][0] == Fr(-1) - ex.GATE
    assert not T.sent[1][0] and T.z[1][0] == Fr(5) - ex.GATE
    assert ex.msac_sum(T, [1.0, 1.0, 4.0], [1.0, 1.0, 0.5]) == (
        Fr(1) + min(T.err[1][0], Fr(1)) + min(T.err[2][0], Fr(4)) / 2)
    assert ex.msac_sum(T, [1.0, 1.0, 4.0], [1.0, 1.0, 0.5], score_type=1) == Fr(2) + min(T.err[2][0], Fr(4)) / 2
    # the bearings point apart: the triangulated depths are negative, cheirality fails
    pair = ex.Pair(0, [(-1.0, 0.0)], [(1.0, 0.0)], [2.0], [2.0], I3, I3)
    T = ex.evaluate(pair, ex.Model(I3, [1.0, 0.0, 0.0]))  # (the rays meet at depth 1 / 2)
    assert not T.sent[2][0] and T.err[2][0] == 0 and T.lsign[0][0] == 1 and T.lsign[1][0] == 1
    T = ex.evaluate(pair, ex.Model(I3, [-1.0, 0.0, 0.0]))  # (at depth -1 / 2)
    assert T.sent[2][0] and T.lsign[0][0] == -1 and T.lsign[1][0] == -1


def test_margins_carry_the_documented_factors():
    """The constants DESIGN.md §5 and mp_score.h document, restated: the cheirality window
    wl = kSafe gamma_16 (8 |t|_1 + 0.1) with kSafe = 4, gamma_k = k u / (1 - k u), u =
    2^-53; the Sampson floor kg2 = 2^-26 g^2 max (alpha beta)^2 with g the largest |E_ij|
    (alpha = |a_0| + |a_1| + 1 over the pair's rays, beta likewise); the focal variants have
    no cheirality window.  (The measured errors sit far inside the margins, so a margin
    scaled by mistake shows here and nowhere else.)"""
    u = 2.0 ** -53
    g16 = 16 * u / (1 - 16 * u)
    cs = xc.case(0, "std")
    pm, _ = api.debug_score_margins(*cs.args(0), cs.models)
    P = cs.exact_pair()
    ab2 = max((abs(a[0]) + abs(a[1]) + 1) ** 2 * (abs(b[0]) + abs(b[1]) + 1) ** 2 for a, b in zip(P.a, P.b))
    for k, m in enumerate(cs.models):
        t1 = float(np.sum(np.abs(m.t())))
        assert abs(pm["wl"][k] / (4.0 * g16 * (8.0 * t1 + 0.1)) - 1) < 1e-12
        t = m.t()
        E = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]) @ m.R()
        assert abs(pm["kg2"][k] / (2.0 ** -26 * np.max(np.abs(E)) ** 2 * float(ab2)) - 1) < 1e-9
        # the depth windows are the same bound with gamma_12 / gamma_14 on the point's
        # magnitude: both scale with kSafe, so their ratio to wl is free of it; their
        # size is pinned from below by the rounding of the depth itself
        assert pm["wz0"][k] > 8 * u * max(abs(t[2]), 1e-2) and pm["wz1"][k] > 8 * u * 1e-2
    cs = xc.case(2, "std")
    pm, _ = api.debug_score_margins(*cs.args(0), cs.models)
    assert np.all(pm["wl"] == 0.0) and np.all(pm["kg2"] > 0)


@pytest.mark.parametrize("score_type", [0, 1, 2])
@pytest.mark.parametrize("variant,kpair", xc.CASES)
def test_oracle_and_host_sweep_against_exact(variant, kpair, score_type, capsys):
    cs = xc.case(variant, kpair)
    args = cs.args(score_type)
    pm, pp = api.debug_score_margins(*args, cs.models)
    assert pp["kstd"] == (1 if (cs.cal and kpair == "std") else 0)
    osc, oerr, oscale = xc.oracle_scores(cs, score_type)
    # the doubles the exact reference reads are the ones both restatements read
    assert pp["norm_scale"] == cs.scale and oscale == cs.scale, (pp["norm_scale"], oscale, cs.scale)
    o, _ = cs.options(score_type)
    thr_user = [o.squared_inlier_thresholds[0] / (cs.scale * cs.scale),
                o.squared_inlier_thresholds[1] / (cs.scale * cs.scale)]
    assert list(pp["thr"]) == [thr_user[0], thr_user[0], thr_user[1]]
    assert list(pp["w"]) == [1.0, 1.0, 1.75 * (2 * thr_user[0] / thr_user[1])]
    if cs.cal:
        assert Fr(pp["loss_scale"]) != 0 and abs(Fr(pp["loss_scale"]) / cs.exact_pair().loss_scale - 1) < Fr(1, 2 ** 50)
    hsc, herr = api.score_models(*args, cs.models, with_errors=True, host_lo=True)
    terms = cs.exact()
    assert any(any(T.sent[t]) for T in terms for t in range(3))  # the far models reach the sentinels
    assert sum(1 for T in terms for i in range(cs.n) if T.err[0][i] < Fr(float(pp["thr"][0]))) > cs.n  # inliers too
    sums = xc.exact_sums(cs, score_type, margins=(pm, pp))
    rep = {}
    for name, sc, err in (("oracle", osc, oerr), ("host sweep", hsc, herr)):
        r = xc.compare_errors(terms, err, score_type, gate=False, thr=pp["thr"], taus=pm["taus"], windows=pm)
        assert r["checked"] >= 0.9 * 3 * cs.n * len(cs.models) and r["windowed"] <= 8, r
        worst_tie = 0.0
        for m, s in enumerate(sums):
            assert np.isfinite(pm["tie"][m]) and pm["tie"][m] > 0
            d = abs(Fr(float(sc[m])) - s)
            assert d <= Fr(float(pm["tie"][m])), (name, m, float(d), pm["tie"][m])
            worst_tie = max(worst_tie, float(d) / pm["tie"][m])
        rep[name] = (r, worst_tie)
    with capsys.disabled():
        for name, (r, wt) in rep.items():
            print(f"\nexact[{name}] variant={variant} K={kpair} score_type={score_type}: rel "
                  + " ".join(f"{v:.2e}" for v in r["rel"]) + " | d/tau " + " ".join(f"{v:.2e}" for v in r["tau"])
                  + f" | d/tie {wt:.2e} | checked {r['checked']} windowed {r['windowed']}", end="")
