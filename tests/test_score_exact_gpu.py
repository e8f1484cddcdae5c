"""The scoring kernels against exact rational arithmetic (tests/exact_residuals.py), at the
trip edges of score_batch too.

mp_score.h states that the device's residuals lie within score_margins' bounds of *exact
arithmetic on the same input doubles*; the screen, the exact early exit and the record
skip are sound only if that holds.  The other margin tests compare with double-precision
restatements (the host sweep, the CPU oracle); tests/test_exact_residuals_cpu.py pins those
to exact arithmetic, this file the kernels:

* terms: debug_terms (both instances of every variant) and the sweep's errors -- the
  per-term claim for every unflagged correspondence, at the default thresholds and at
  1e-30, and, independently of the margins, a relative error of at most 16 x the oracle's
  worst on the same set (FMA contraction, the other operation order, the Newton
  reciprocal; never a number from the device run);
* flag completeness: ladders of ulps and of window multiples around the z gate, the
  cheirality threshold and the Sampson denominator floor -- wherever the device decides
  otherwise than exact arithmetic, the correspondence is flagged; ten windows away it is
  not, and the decision is the exact one;
* sums: score_batch, score_models and select_batch within each model's margin of the exact
  sum, and the iteration bounds lo <= min exact, exact(best) <= hi;
* trip edges: n from 8 to 2049 (no check at all; a partial last trip right after the first
  check; the 256 boundaries; the paired-trip loop, reached by the default schedule from n
  = 1793), plain and with the early exit -- survivors carry the plain kernel's bits, killed
  models cannot beat the bound in the reference order nor in exact arithmetic;
* schedules: the same under MADPOSE_SCORE_CHECK 1,1 / 2,2 / 3,2 and without pairing, in
  child processes one after another, survivors bit-identical across all four.
"""
import json
import os
import subprocess
import sys
from fractions import Fraction as Fr

import numpy as np
import pytest

import madpose
from madpose_amd import api
from tests import exact_cases as xc
from tests import exact_residuals as ex
from tests.exact_cases import BIG, SLOT, UNC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULPS = [0, 1, -1, 2, -2, 8, -8, 64, -64, 2 ** 10, -2 ** 10, 2 ** 20, -2 ** 20]
WINS = [0.5, -0.5, 2.0, -2.0, 10.0, -10.0]


@pytest.fixture(scope="module", autouse=True)
def require_gpu():
    if madpose.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on an MI355X")


def _fmt(v):
    return " ".join(f"{x:.2e}" for x in v)


# ---------------------------------------------------------------------------
# terms
@pytest.mark.parametrize("thr", [None, 1e-30])
@pytest.mark.parametrize("score_type", [0, 1, 2])
@pytest.mark.parametrize("variant,kpair", xc.CASES)
def test_terms_against_exact(variant, kpair, score_type, thr, capsys):
    cs = xc.case(variant, kpair)
    args = cs.args(score_type, thr)
    err, flags, taus, ties = api.debug_score_terms(*args, cs.models)
    pm, pp = api.debug_score_margins(*args, cs.models)
    assert np.array_equal(taus, pm["taus"]) and np.array_equal(ties, pm["tie"])
    assert np.all(np.isfinite(taus)) and np.all(taus > 0)
    skip = flags != 0
    assert skip.sum() <= 0.01 * skip.size, int(skip.sum())
    terms = cs.exact()
    # the claim as mp_score.h states it, for every unflagged (model, correspondence, type)
    dev = xc.compare_errors(terms, err, score_type, gate=True, thr=pp["thr"], taus=taus, skip=skip)
    gated_terms = 2 * cs.n * len(cs.models) if score_type == 1 else (cs.n * len(cs.models) if score_type == 2 else 0)
    assert dev["checked"] >= 0.9 * (3 * cs.n * len(cs.models) - gated_terms)
    if thr is not None:
        return
    # the sweep's errors (the gated eval_corr, is_for_inlier = true): the same claim
    _, serr = api.score_models(*args, cs.models, with_errors=True)
    swp = xc.compare_errors(terms, serr, score_type, gate=False, thr=pp["thr"], taus=taus, skip=skip, windows=pm)
    # independently of the margins: 16 x the oracle's own worst relative error on this set
    _, oerr, _ = xc.oracle_scores(cs, score_type)
    orc = xc.compare_errors(terms, oerr, score_type, gate=False, skip=skip)
    with capsys.disabled():
        print(f"\nexact[device] variant={variant} K={kpair} score_type={score_type}: rel debug_terms "
              f"{_fmt(dev['rel'])} sweep {_fmt(swp['rel'])} oracle {_fmt(orc['rel'])} | d/tau debug_terms "
              f"{_fmt(dev['tau'])} sweep {_fmt(swp['tau'])} | flagged {int(skip.sum())}", end="")
    for t in range(3):
        assert orc["rel"][t] > 0
        assert swp["rel"][t] <= 16 * orc["rel"][t], (t, swp["rel"][t], orc["rel"][t])
        if not ((score_type == 1 and t < 2) or (score_type == 2 and t == 2)):
            assert dev["rel"][t] <= 16 * orc["rel"][t], (t, dev["rel"][t], orc["rel"][t])


# ---------------------------------------------------------------------------
# flag completeness
def _step(x, k):
    """x moved by k units in its last place."""
    return float(x + k * np.spacing(abs(x)))


def _one(cs, i, x0=None, x1=None):
    """The exact pair holding correspondence i alone (x0, x1: replacements)."""
    p = cs.p
    return ex.Pair(0 if cs.cal else cs.variant, [cs.x0n[i] if x0 is None else x0], [cs.x1n[i] if x1 is None else x1],
                   [cs.d0[i]], [cs.d1[i]], p["K0"] if cs.cal else None, p["K1"] if cs.cal else None,
                   scale_only=cs.variant == 3)


def _with_t(m, t, variant):
    if variant == 0:
        return madpose.PoseScaleOffset(m.R(), t, m.scale, m.offset0, m.offset1)
    if variant == 1:
        return madpose.PoseScaleOffsetSharedFocal(m.R(), t, m.scale, m.offset0, m.offset1, m.focal)
    return madpose.PoseScaleOffsetTwoFocal(m.R(), t, m.scale, m.offset0, m.offset1, m.focal0, m.focal1)


def _clear(T, pm, k, which, factor=10):
    """The exact gate quantities of the single-correspondence terms T named in `which`
    ('z0', 'z1', 'l', 'den') lie more than `factor` windows from their gates."""
    ok = True
    if "z0" in which:
        ok = ok and abs(T.z[0][0]) > factor * Fr(float(pm["wz0"][k]))
    if "z1" in which:
        ok = ok and abs(T.z[1][0]) > factor * Fr(float(pm["wz1"][k]))
    if "l" in which and T.l[0][0] is not None:
        ok = ok and all(abs(T.l[j][0]) > factor * Fr(float(pm["wl"][k])) for j in range(2))
    if "den" in which:
        ok = ok and T.den[0] > factor * Fr(float(pm["kg2"][k]))
    return ok


def z_ladder(cs, i):
    """Models equal to the case's first but for t_z, which puts correspondence i's depth
    z of the 0 -> 1 reprojection at the gate 1e-2 exactly (to the nearest double of t_z),
    then ULPS away, then WINS windows away.  Returns (models, rung kinds)."""
    m = cs.models[0]
    T = ex.evaluate(_one(cs, i), xc.exact_model(m, cs.variant), which=(0,))
    zq = T.z[0][0] + ex.GATE - Fr(float(m.t()[2]))  # z = zq + t_z (the target K's last row is 0 0 1)
    tz0 = float(ex.GATE - zq)
    t = m.t()
    base = _with_t(m, np.r_[t[:2], tz0], cs.variant)
    pm, _ = api.debug_score_margins(*cs.args(0), [base])
    models, kinds = [], []
    for k in ULPS:
        models.append(_with_t(m, np.r_[t[:2], _step(tz0, k)], cs.variant))
        kinds.append(("ulp", k))
    for c in WINS:
        models.append(_with_t(m, np.r_[t[:2], tz0 + c * pm["wz0"][0]], cs.variant))
        kinds.append(("win", c))
    return models, kinds


@pytest.mark.parametrize("variant,kpair", [(0, "std"), (0, "low"), (1, "std"), (2, "std")])
def test_flag_completeness_z_gate(variant, kpair):
    cs = xc.case(variant, kpair)
    i = 5
    models, kinds = z_ladder(cs, i)
    args = cs.args(0)
    err, flags, _, _ = api.debug_score_terms(*args, models)
    pm, _ = api.debug_score_margins(*args, models)
    P1 = _one(cs, i)
    decisions = set()
    for k, (kind, c) in enumerate(kinds):
        T = ex.evaluate(P1, xc.exact_model(models[k], cs.variant))
        dev_sent = err[k, 0, i] == BIG
        decisions.add((dev_sent, T.sent[0][0]))
        if dev_sent != T.sent[0][0]:
            assert flags[k, i] == 1, (kind, c)
        if abs(T.z[0][0]) <= Fr(float(pm["wz0"][k])) / 2:  # well inside the window: flagged
            assert flags[k, i] == 1, (kind, c)
        if kind == "win" and abs(c) == 10.0:
            assert abs(T.z[0][0]) > 9 * Fr(float(pm["wz0"][k]))
            assert _clear(T, pm, k, ("z1", "l", "den"))  # (the ladder moves this gate alone)
            assert flags[k, i] == 0 and dev_sent == T.sent[0][0], (kind, c)
    assert (True, True) in decisions and (False, False) in decisions  # both sides of the gate


def l_ladder(cs, i):
    """Models equal to the case's second but for t, moved so that correspondence i's
    lambda1 equals min_depth (1 - a^2) (check_cheirality; lambda1 - min_depth is linear in
    t), then ULPS of one component away, then WINS windows.  (i: a correspondence whose
    lambda2 then passes, so that lambda1 alone decides.)"""
    m = cs.models[1]
    p = cs.p
    K0i, K1i = np.linalg.inv(p["K0"]), np.linalg.inv(p["K1"])
    a0, b0 = K0i @ np.r_[p["x0"][i], 1.0], K1i @ np.r_[p["x1"][i], 1.0]
    n0, n1 = a0 / np.linalg.norm(a0), b0 / np.linalg.norm(b0)
    rn = m.R() @ n0
    a = -rn @ n1
    g = -rn - a * n1  # lambda1 = g . t
    md = 1e-2 * (1 - a * a)
    t = m.t() + (md - g @ m.t()) / (g @ g) * g
    j = int(np.argmax(np.abs(g)))
    P1 = _one(cs, i)
    for _ in range(3):  # the remainder, measured exactly, taken out through component j
        T = ex.evaluate(P1, xc.exact_model(_with_t(m, t, 0), 0), which=(2,))
        t[j] -= float(T.l[0][0]) / g[j]
    pm, _ = api.debug_score_margins(*cs.args(0), [_with_t(m, t, 0)])
    models, kinds = [], []
    for k in ULPS:
        tt = t.copy()
        tt[j] = _step(t[j], k)
        models.append(_with_t(m, tt, 0))
        kinds.append(("ulp", k))
    for c in WINS:
        tt = t.copy()
        tt[j] = t[j] + c * pm["wl"][0] / g[j]
        models.append(_with_t(m, tt, 0))
        kinds.append(("win", c))
    return models, kinds


@pytest.mark.parametrize("kpair", ["std", "low"])
def test_flag_completeness_cheirality(kpair):
    cs = xc.case(0, kpair)
    for i in range(9, 40):
        models, kinds = l_ladder(cs, i)
        if ex.evaluate(_one(cs, i), xc.exact_model(models[0], 0), which=(2,)).lsign[1][0] > 0:
            break
    args = cs.args(0)
    err, flags, _, _ = api.debug_score_terms(*args, models)
    pm, _ = api.debug_score_margins(*args, models)
    P1 = _one(cs, i)
    decisions = set()
    for k, (kind, c) in enumerate(kinds):
        T = ex.evaluate(P1, xc.exact_model(models[k], 0))
        dev_sent = err[k, 2, i] == BIG
        decisions.add((dev_sent, T.sent[2][0]))
        if dev_sent != T.sent[2][0]:
            assert flags[k, i] == 1, (kind, c)
        if abs(T.l[0][0]) <= Fr(float(pm["wl"][k])) / 2:
            assert flags[k, i] == 1, (kind, c)
        if kind == "win" and abs(c) == 10.0:
            assert abs(T.l[0][0]) > 9 * Fr(float(pm["wl"][k])) and abs(T.l[1][0]) > 10 * Fr(float(pm["wl"][k]))
            assert _clear(T, pm, k, ("z0", "z1", "den"))
            assert flags[k, i] == 0 and dev_sent == T.sent[2][0], (kind, c)
    assert (True, True) in decisions and (False, False) in decisions


def den_ladder(cs):
    """Correspondences 20 .. become projections of points next to the baseline of a near
    model (beyond the camera that looks along it, so that cheirality passes): on the
    baseline both rays meet the epipoles and the Sampson denominator is ~0; a point eps
    off it has a denominator ~eps^2.  Rungs: the baseline itself; the first eps (to the
    double) where the exact denominator reaches the floor kg2, and x0_u ULPS from there;
    0.5, 2 and 10 floors.  Returns (model, x0, x1, rung correspondences, rung kinds)."""
    p = cs.p
    K0, K1 = p["K0"], p["K1"]
    for m in cs.models:
        R, t = m.R(), m.t()
        C1 = -R.T @ t  # the second camera's centre in the first one's frame
        if C1[2] > 0.05 and t[2] < -0.05:
            X0 = 2.0 * C1  # beyond the second camera, in front of both
            break
        if C1[2] < -0.05 and t[2] > 0.05:
            X0 = -C1  # behind the second camera's back, in front of both
            break
    else:
        raise AssertionError("no model moves along its viewing direction")
    perp = np.cross(C1, [0.0, 1.0, 0.0])
    perp /= np.linalg.norm(perp)

    def project(eps):
        X = X0 + eps * perp
        a, b = K0 @ X, K1 @ (R @ X + t)
        return (float(a[0] / a[2]), float(a[1] / a[2])), (float(b[0] / b[2]), float(b[1] / b[2]))

    kinds = [("epipole", 0)] + [("ulp", k) for k in ULPS] + [("floor", c) for c in (0.5, 2.0, 10.0)]
    idx = list(range(20, 20 + len(kinds)))
    x0, x1 = p["x0"].copy(), p["x1"].copy()
    for i in idx:
        x0[i], x1[i] = project(0.0)
    xm = xc.exact_model(m, 0)

    def den(eps):
        u0, u1 = project(eps)
        return ex.evaluate(_one(cs, idx[0], u0, u1), xm, which=(2,)).den[0]

    for _ in range(2):  # (the floor reads the pair's largest ray magnitudes: settle it)
        args = (0, x0, x1, cs.d0, cs.d1, cs.cam0, cs.cam1) + cs.options(0)
        kg2 = Fr(float(api.debug_score_margins(*args, [m])[0]["kg2"][0]))
        lo, hi = 0.0, 0.05
        assert den(lo) < kg2 <= den(hi)
        while True:  # den(lo) < kg2 <= den(hi)
            mid = 0.5 * (lo + hi)
            if mid == lo or mid == hi:
                break
            lo, hi = (lo, mid) if den(mid) >= kg2 else (mid, hi)
        for r, (kind, c) in enumerate(kinds):
            if kind == "ulp":
                x0[idx[r]], x1[idx[r]] = project(hi)
                x0[idx[r], 0] = _step(x0[idx[r], 0], c)
            elif kind == "floor":
                x0[idx[r]], x1[idx[r]] = project(hi * np.sqrt(c))
    return m, x0, x1, idx, kinds


@pytest.mark.parametrize("kpair", ["std", "low"])
def test_flag_completeness_sampson_floor(kpair):
    cs = xc.case(0, kpair)
    m, x0, x1, idx, kinds = den_ladder(cs)
    args = (0, x0, x1, cs.d0, cs.d1, cs.cam0, cs.cam1) + cs.options(0)
    err, flags, taus, _ = api.debug_score_terms(*args, [m])
    pm, pp = api.debug_score_margins(*args, [m])
    kg2, thr = Fr(float(pm["kg2"][0])), Fr(float(pp["thr"][2]))
    xm = xc.exact_model(m, 0)
    seen = set()
    for r, (kind, c) in enumerate(kinds):
        i = idx[r]
        T = ex.evaluate(_one(cs, i, tuple(x0[i]), tuple(x1[i])), xm)
        dev_sent = err[0, 2, i] == BIG
        if dev_sent != T.sent[2][0]:
            assert flags[0, i] == 1, (kind, c)
        if T.sent[2][0]:
            continue
        if T.den[0] < kg2 * (1 - Fr(1, 10 ** 9)):  # below the floor: outside the claim, flagged
            assert flags[0, i] == 1, (kind, c, float(T.den[0] / kg2))
        if kind == "floor" and c == 10.0:
            assert T.den[0] > 9 * kg2 and _clear(T, pm, 0, ("z0", "z1", "l"))
            assert flags[0, i] == 0, (kind, c)
        seen.add((kind, int(flags[0, i])))
        if flags[0, i] == 0:  # unflagged: the per-term claim holds
            assert T.err[2][0] is not None
            d = abs(min(Fr(float(err[0, 2, i])), thr) - min(T.err[2][0], thr))
            assert d <= Fr(float(taus[0, 2])), (kind, c, float(d), taus[0, 2])
    assert ("ulp", 0) in seen and ("ulp", 1) in seen and ("floor", 0) in seen  # both sides of the floor


# ---------------------------------------------------------------------------
# sums
@pytest.mark.parametrize("score_type", [0, 1, 2])
@pytest.mark.parametrize("variant,kpair", xc.CASES)
def test_sums_against_exact(variant, kpair, score_type, capsys):
    cs = xc.case(variant, kpair)
    args = cs.args(score_type)
    pm, pp = api.debug_score_margins(*args, cs.models)
    sums = xc.exact_sums(cs, score_type, margins=(pm, pp))
    nm = len(cs.models)
    M = 4 if variant == 2 else 8
    groups = [list(range(0, M)), list(range(nm - M, nm)), [1, 3, 6]]
    iters = [[m] for m in cs.models] + [[cs.models[k] for k in g] for g in groups]
    dev, slots, _, bounds = api.debug_score_batch(*args, iters, best=BIG, exit=False, record_skip=False)
    pair = dict(cs.p, depth0=cs.d0, depth1=cs.d1)
    o, c = cs.options(score_type)
    sel = api.select_batch(variant, [pair], [[xc.user_model(m, variant) for m in cs.models]], o, c, with_scores=True)[0]
    by = {"score_batch": dev[:nm], "score_models": api.score_models(*args, cs.models), "select_batch": sel.scores}
    worst = {}
    unc = 0
    for name, sc in by.items():
        worst[name] = 0.0
        for k in range(nm):
            if name == "score_batch":
                assert bounds["tie"][k][0] == pm["tie"][k]
                if slots[k] & UNC:  # a flagged correspondence: the sum is outside the claim
                    unc += 1
                    continue
            d = abs(Fr(float(sc[k])) - sums[k])
            assert d <= Fr(float(pm["tie"][k])), (name, k, float(d), pm["tie"][k])
            worst[name] = max(worst[name], float(d) / pm["tie"][k])
    assert unc <= 1
    assert sel.index == int(np.argmin([float(s) for s in sums]))
    for j, g in enumerate(groups):
        b = nm + j
        if slots[b] & UNC:
            continue
        assert Fr(float(bounds["lo"][b])) <= min(sums[k] for k in g), (b, bounds["lo"][b])
        assert sums[g[int(slots[b] & SLOT)]] <= Fr(float(bounds["hi"][b])), (b, bounds["hi"][b])
    with capsys.disabled():
        print(f"\nexact[sums] variant={variant} K={kpair} score_type={score_type}: d/tie "
              + " ".join(f"{k} {v:.2e}" for k, v in worst.items()), end="")


# ---------------------------------------------------------------------------
# trip edges
@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("n", xc.TRIP_NS)
def test_trip_edges(n, variant):
    """The default schedule.  n <= 256 is one trip: no check runs, so the run must kill
    nothing (a kill there would be a check after the last trip); from n = 257 on every run
    must both kill and keep models.  1793 and 2049 reach q = 2: paired steps, at 2049 with a
    partial last trip."""
    tc = xc.trip_case(n, variant)
    r = xc.run_trip_case(tc)
    # (exact sums of two killed and two kept models, one of each from n = 512 on: a second)
    xc.check_exit_relations(tc, r, xc.check_points(n), exact_models=(2 if n <= 300 else 1) if n <= 769 else 0)


# ---------------------------------------------------------------------------
# schedules
SCHEDULES = [("1,1", "1"), ("2,2", "1"), ("3,2", "1"), ("2,2", "0")]
SCHEDULE_NS = (300, 513, 769, 1793)


def _child(variant, check, pair):
    env = dict(os.environ, MADPOSE_SCORE_CHECK=check, MADPOSE_SCORE_PAIR=pair)
    return subprocess.run([sys.executable, os.path.join(ROOT, "tests", "score_exit_worker.py"), str(variant)]
                          + [str(n) for n in SCHEDULE_NS], env=env, capture_output=True, text=True, timeout=120,
                          cwd=ROOT)


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_exit_schedules(variant):
    """2,2 at n = 300: the paired step covers trips 0 and 1, the second partial, no check;
    at 513 and 769 a check follows a paired step and a single trip follows that.  The
    children run strictly one after another; the first that fails ends the test."""
    runs = []
    for check, pair in SCHEDULES:
        cp = _child(variant, check, pair)
        faulted = "illegal memory access" in (cp.stdout + cp.stderr)
        assert cp.returncode == 0 and not faulted, (check, pair, cp.returncode, cp.stderr[-2000:])
        runs.append(json.loads(cp.stdout.strip().splitlines()[-1]))
    for n in SCHEDULE_NS:
        tc = xc.trip_case(n, variant)
        rs = []
        for (check, pair), out in zip(SCHEDULES, runs):
            o = out[str(n)]
            r = {k: np.array([float.fromhex(v) for v in o[k]]) for k in ("plain", "exit", "tie")}
            r["plain_slot"], r["exit_slot"] = np.array(o["plain_slot"]), np.array(o["exit_slot"])
            r["best"] = float.fromhex(o["best"])
            first, every = (int(v) for v in check.split(","))
            xc.check_exit_relations(tc, r, xc.check_points(n, first, every),
                                    exact_models=1 if (n <= 769 and check == "2,2" and pair == "1") else 0)
            rs.append(r)
        for r in rs[1:]:
            # the plain launch does not depend on the schedule; a model that survives under
            # two schedules has the same bits under both (the plain kernel's)
            assert np.array_equal(r["plain"], rs[0]["plain"]) and r["best"] == rs[0]["best"]
            both = (r["exit"][:tc.nm] != BIG) & (rs[0]["exit"][:tc.nm] != BIG)
            assert np.array_equal(r["exit"][:tc.nm][both], rs[0]["exit"][:tc.nm][both])
