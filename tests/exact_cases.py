"""Shared inputs of tests/test_exact_residuals_cpu.py and tests/test_score_exact_gpu.py:
small pairs with models near the truth and far from it, the exact residuals of each
(tests/exact_residuals.py; computed once per process and left unchanged), and the
comparisons both files make."""
import functools
from fractions import Fraction as Fr

import numpy as np

import madpose
from madpose_amd import api, synthetic
from tests import exact_residuals as ex

BIG = np.finfo(np.float64).max
KINDS = ["calibrated", "shared_focal", "two_focal", "calibrated"]
# (variant, intrinsics): "std" upper-triangular K (the calibrated ray form applies, kstd =
# 1), "low" a K0 with a non-zero entry below the diagonal (kstd = 0: the matrix form)
CASES = [(0, "std"), (0, "low"), (1, "std"), (2, "std"), (3, "std"), (3, "low")]


def _rand_rot(rng):
    R = np.linalg.qr(rng.standard_normal((3, 3)))[0]
    return R * np.linalg.det(R)


def depth_transform(p, offsets=True):
    """The pair's true model in the estimators' parametrization, (t, scale, offset0,
    offset1): the depths along the true rays (triangulated with the true R, t) regressed on
    the priors over the inliers, z0 = a0 d0 + b0 and z1 = a1 d1 + b1, then the whole scene
    divided by a0 so that the first prior's factor is 1.  offsets=False: b0 = b1 = 0."""
    K0i, K1i = np.linalg.inv(p["K0"]), np.linalg.inv(p["K1"])
    ok = p["inlier_mask"]
    a = (K0i @ np.c_[p["x0"][ok], np.ones(ok.sum())].T).T
    b = (K1i @ np.c_[p["x1"][ok], np.ones(ok.sum())].T).T
    lam = np.array([np.linalg.lstsq(np.c_[p["R"] @ a[i], -b[i]], -p["t"], rcond=None)[0] for i in range(len(a))])
    d0, d1 = p["depth0"][ok], p["depth1"][ok]
    if offsets:
        a0, b0 = np.polyfit(d0, lam[:, 0], 1)
        a1, b1 = np.polyfit(d1, lam[:, 1], 1)
    else:
        a0, b0, a1, b1 = np.median(lam[:, 0] / d0), 0.0, np.median(lam[:, 1] / d1), 0.0
    return p["t"] / a0, a1 / a0, b0 / a0, b1 / a1


def make_models(p, rng, k, variant, scale=1.0, spread=1.0):
    """k models in problem units: three of four near the ground truth (small rotation,
    translation and depth-transform errors; most correspondences inliers), every fourth far
    (random rotation, translation and depth transform: z < 1e-2 and cheirality sentinels).
    scale: the pair's normalization scale -- a focal is drawn in pixels and divided by it,
    the one operation the entries that take user units apply (user_model).  spread: factor
    on the near models' errors."""
    out = []
    t_gt, s_gt, o0_gt, o1_gt = depth_transform(p, offsets=variant != 3)
    for j in range(k):
        far = j % 4 == 3
        ang = rng.normal(0, 0.01 * (1.0 if far else spread), 3)
        Kx = np.array([[0, -ang[2], ang[1]], [ang[2], 0, -ang[0]], [-ang[1], ang[0], 0]])
        U, _, Vt = np.linalg.svd((_rand_rot(rng) if far else np.eye(3)) @ (np.eye(3) + Kx) @ p["R"])
        R = U @ Vt
        if far:
            t = rng.standard_normal(3) * rng.uniform(0.1, 3)
            s, o0, o1 = rng.uniform(0.2, 5), rng.normal(0, 2), rng.normal(0, 2)
            fu = [rng.uniform(0.3, 3) * p["f0"], rng.uniform(0.3, 3) * p["f1"]]
        else:
            t = t_gt + rng.normal(0, 0.01 * spread, 3)
            s = s_gt * (1 + 0.02 * spread * rng.uniform(-1, 1))
            o0, o1 = o0_gt + rng.normal(0, 0.02 * spread), o1_gt + rng.normal(0, 0.02 * spread)
            fu = [(1 + 0.03 * spread * rng.uniform(-1, 1)) * p["f0"],
                  (1 + 0.03 * spread * rng.uniform(-1, 1)) * p["f1"]]
        f = [fu[0] / scale, fu[1] / scale]
        if variant == 0:
            out.append(madpose.PoseScaleOffset(R, t, s, o0, o1))
        elif variant == 3:
            out.append(api.PoseAndScale(R, t, s))
        elif variant == 1:
            out.append(madpose.PoseScaleOffsetSharedFocal(R, t, s, o0, o1, f[0]))
        else:
            out.append(madpose.PoseScaleOffsetTwoFocal(R, t, s, o0, o1, f[0], f[1]))
        out[-1].user_focals = fu
    return out


def user_model(m, variant):
    """The model in user units, as select_batch takes it: the focals in pixels (the entry
    divides them by the scale again, which gives the problem-unit doubles back)."""
    if variant == 1:
        return madpose.PoseScaleOffsetSharedFocal(m.R(), m.t(), m.scale, m.offset0, m.offset1, m.user_focals[0])
    if variant == 2:
        return madpose.PoseScaleOffsetTwoFocal(m.R(), m.t(), m.scale, m.offset0, m.offset1, *m.user_focals)
    return m


def exact_model(m, variant):
    f0 = m.focal if variant == 1 else getattr(m, "focal0", 1.0)
    f1 = m.focal if variant == 1 else getattr(m, "focal1", 1.0)
    return ex.Model(m.R(), m.t(), m.scale, getattr(m, "offset0", 0.0), getattr(m, "offset1", 0.0), f0, f1)


class Case:
    """One pair with its models.  args(score_type, thr): the argument tuple of
    api.score_models and the debug hooks.  exact(): the models' exact terms (ungated)."""

    def __init__(self, variant, kpair, n, nmodels, seed, spread=1.0, **pair_kw):
        self.variant, self.kpair, self.n = variant, kpair, n
        K0 = synthetic.SCANNET_K.copy()
        K1 = synthetic.SCANNET_K.copy()
        if kpair == "low":
            K0[1, 0] = 3.25
            K0[0, 1] = -1.5
            K1[0, 0] = 540.125
        self.p = p = synthetic.make_pair(seed, n=n, K0=K0, K1=K1, **pair_kw)
        self.cal = variant in (0, 3)
        self.cam0, self.cam1 = (p["K0"], p["K1"]) if self.cal else (p["pp0"], p["pp1"])
        self.d0, self.d1 = p["depth0"].copy(), p["depth1"].copy()
        if variant == 3:  # scale-only rejects priors below 1e-2 (src/hybrid_pose_estimator.cpp:386, 398)
            self.d0[::17] = 1e-3
            self.d1[::23] = 5e-3
        rng = np.random.default_rng(1000 + seed)
        if self.cal:
            self.x0n, self.x1n, self.scale = p["x0"], p["x1"], 1.0
        else:
            self.x0n, self.x1n, self.scale = ex.normalize_points(p["x0"], p["x1"], p["pp0"], p["pp1"])
        self.models = make_models(p, rng, nmodels, variant, self.scale, spread)
        self._exact = None

    def options(self, score_type=0, thr=None):
        o, c = synthetic.example_options(KINDS[self.variant])
        o.data_type_weights = [1.0, 1.75]
        if thr is not None:
            o.squared_inlier_thresholds = [thr, thr]
        c.score_type = score_type
        return o, c

    def args(self, score_type=0, thr=None):
        o, c = self.options(score_type, thr)
        return (self.variant, self.p["x0"], self.p["x1"], self.d0, self.d1, self.cam0, self.cam1, o, c)

    def exact_pair(self):
        if self.cal:
            return ex.Pair(0, self.x0n, self.x1n, self.d0, self.d1, self.p["K0"], self.p["K1"],
                           scale_only=self.variant == 3)
        return ex.Pair(self.variant, self.x0n, self.x1n, self.d0, self.d1)

    def exact(self):
        if self._exact is None:
            P = self.exact_pair()
            self._exact = [ex.evaluate(P, exact_model(m, self.variant)) for m in self.models]
        return self._exact


@functools.lru_cache(maxsize=None)
def case(variant, kpair, n=300, nmodels=8, seed=17):
    return Case(variant, kpair, n, nmodels, seed)


def oracle_scores(case_, score_type=0, thr=None):
    """The CPU oracle's ScoreModel sums and ungated errors of the case's models, and the
    normalization scale it formed."""
    import oracle
    from tests.helpers import oracle_cfg, oracle_opts

    o, c = case_.options(score_type, thr)
    oms = []
    for m in case_.models:
        om = oracle.OrModel()
        om.R[:] = m.R().ravel().tolist()
        om.t[:] = m.t().tolist()
        om.scale = m.scale
        om.offset0, om.offset1 = getattr(m, "offset0", 0.0), getattr(m, "offset1", 0.0)
        om.focal0 = m.focal if case_.variant == 1 else getattr(m, "focal0", 1.0)
        om.focal1 = m.focal if case_.variant == 1 else getattr(m, "focal1", 1.0)
        oms.append(om)
    p = case_.p
    return oracle.score_models(case_.variant, p["x0"], p["x1"], case_.d0, case_.d1, case_.cam0, case_.cam1,
                               oracle_opts(o), oracle_cfg(c), oms)


def rel_gate(q, ref):
    """|q| relative to the magnitudes it was formed from."""
    return abs(q) / ref if ref else abs(q)


def far_from_gates(T, t, i, rel=Fr(1, 10 ** 9)):
    """The exact gate quantities deciding the sentinel of term t at correspondence i are
    farther from zero than `rel`, relative to the quantities compared (z against 1e-2;
    l against min_depth <= 1e-2 and the translation-sized lambdas: against max(|l|, 1e-2))."""
    if t < 2:
        z = T.z[t][i]
        return rel_gate(z, max(abs(z + ex.GATE), ex.GATE)) > rel
    if T.l[0][i] is None:
        return True
    return all(rel_gate(T.l[k][i], max(abs(T.l[k][i]), ex.GATE)) > rel for k in range(2))


def compare_errors(terms, err, score_type, gate, thr=None, taus=None, skip=None, windows=None):
    """err [nm x 3 x n] doubles against the exact terms.  gate: err carries the
    score_type gating (is_for_inlier = false).  Checks, for every (m, t, i) not in skip
    [nm x n bool]: the sentinel decision equals the exact one wherever the gates are
    farther than 1e-9 (relative); and, with taus [nm x 3] and thr [3], |min(e, thr) -
    min(e_exact, thr)| <= tau outside the windows.  windows: dict of per-model arrays
    wz0, wz1, wl, kg2 -- a correspondence whose exact gate quantity lies inside one is
    outside the claim and is left out (counted).  Returns dict: worst relative error per
    term below the sentinel, worst d / tau per term, counts."""
    nm, n = len(terms), len(terms[0].den)
    worst_rel, worst_tau = [0.0] * 3, [0.0] * 3
    checked = windowed = 0
    for m in range(nm):
        T = terms[m]
        for t in range(3):
            gated = gate and ((score_type == 1 and t < 2) or (score_type == 2 and t == 2))
            for i in range(n):
                if skip is not None and skip[m][i]:
                    continue
                e = float(err[m][t][i])
                if gated:
                    assert e == BIG, (m, t, i, e)
                    continue
                xe = T.err[t][i]
                if xe is None:  # 0 / 0: outside every claim
                    continue
                if windows is not None:
                    inside = False
                    if t < 2:
                        inside = abs(T.z[t][i]) <= Fr(float(windows["wz0" if t == 0 else "wz1"][m]))
                    else:
                        if T.l[0][i] is not None:
                            wl = Fr(float(windows["wl"][m]))
                            inside = abs(T.l[0][i]) <= wl or abs(T.l[1][i]) <= wl
                        inside = inside or T.den[i] < Fr(float(windows["kg2"][m]))
                    if inside:
                        windowed += 1
                        continue
                sent = T.sent[t][i]
                if far_from_gates(T, t, i):
                    assert (e == BIG) == sent, (m, t, i, e, sent)
                elif (e == BIG) != sent:
                    continue
                checked += 1
                if sent:
                    continue
                assert e == e and e >= 0.0, (m, t, i, e)
                d = abs(Fr(e) - xe)
                if xe > 0:
                    worst_rel[t] = max(worst_rel[t], float(d / xe))
                if taus is not None:
                    th = Fr(float(thr[t]))
                    dc = abs(min(Fr(e), th) - min(xe, th))
                    tau = float(taus[m][t])
                    assert dc <= Fr(tau), (m, t, i, float(dc), tau)
                    if tau > 0 and np.isfinite(tau):
                        worst_tau[t] = max(worst_tau[t], float(dc) / tau)
    return {"rel": worst_rel, "tau": worst_tau, "checked": checked, "windowed": windowed}


def exact_sums(case_, score_type=0, thr=None, margins=None):
    """The exact ScoreModel sums of the case's models (Fractions) at the engine's
    thresholds and weights (per pair, from mp_debug_score_margins)."""
    if margins is None:
        margins = api.debug_score_margins(*case_.args(score_type, thr), case_.models)
    _, pp = margins
    return [ex.msac_sum(T, pp["thr"], pp["w"], score_type) for T in case_.exact()]


# ---------------------------------------------------------------------------
# score_batch's trip loop (one trip = 256 correspondences)
MAXM = {0: 10, 1: 16, 2: 4}
TRIP_NS = (8, 255, 256, 257, 300, 512, 513, 769, 1793, 2049)
UNC, AMB, SLOT = 1 << 17, 1 << 16, 0xFFFF


class TripCase:
    """A pair of n correspondences and a batch: every model as a single-model iteration
    (these give each model's own score), then iterations of MAXM models and of a count in
    between."""

    def __init__(self, n, variant):
        M = MAXM[variant]
        mid = max(2, M // 2 + 1)
        self.singles = 12
        # few outliers and near models close to the truth: their scores are a small part of
        # a far model's, so that a far model's partial sum passes them after half the trips
        self.case = cs = Case(variant, "std", n, self.singles + 2 * M + 2 * mid, 500 + n, spread=0.2,
                              outlier_ratio=0.1, noise_px=0.5, depth_noise=0.02)
        ms = cs.models
        self.groups = [list(range(self.singles, self.singles + M)),
                       list(range(self.singles + M, self.singles + 2 * M)),
                       list(range(self.singles + 2 * M, self.singles + 2 * M + mid)),
                       list(range(self.singles + 2 * M + mid, self.singles + 2 * M + 2 * mid))]
        self.iterations = [[m] for m in ms] + [[ms[k] for k in g] for g in self.groups]
        self.nm = len(ms)


@functools.lru_cache(maxsize=None)
def trip_case(n, variant):
    return TripCase(n, variant)


def check_points(n, first=0, every=1):
    """The trips after which score_batch checks its partial sums (kernels.hip score_bound:
    first > 0 overrides the default schedule): `done` trips in [first, ntrip) at steps of
    `every` -- never after the last trip."""
    ntrip = (n + 255) // 256
    if first <= 0:
        first = every = min(2, max(1, ntrip // 4))
    return [d for d in range(first, ntrip) if (d - first) % every == 0]


def run_trip_case(tc):
    """The plain launch, then the launch with the exact early exit against the 20 %
    quantile of the models' plain scores.  Returns dict of float arrays / ints."""
    args = tc.case.args(0) + (tc.iterations,)
    pb, ps, _, bounds = api.debug_score_batch(*args, best=BIG, exit=False, record_skip=False)
    best = float(np.quantile(pb[:tc.nm], 0.2))
    eb, es, _, _ = api.debug_score_batch(*args, best=best, exit=True, record_skip=False)
    return {"plain": pb, "plain_slot": ps, "exit": eb, "exit_slot": es, "best": best,
            "tie": np.array([t[0] for t in bounds["tie"][:tc.nm]])}


def check_exit_relations(tc, r, checks, exact_models=0):
    """The relations between a plain and an early-exit launch of tc's batch (r: the arrays
    of run_trip_case; checks: the schedule's check points).  exact_models: this many killed
    and this many kept single-model iterations are also held against exact sums."""
    cs, nm = tc.case, tc.nm
    pb, eb, best = r["plain"], r["exit"], r["best"]
    pm, pp = api.debug_score_margins(*cs.args(0), cs.models)
    assert np.array_equal(pm["tie"], r["tie"])
    assert not np.any(r["plain_slot"] & UNC) and not np.any(r["exit_slot"] & UNC)
    assert np.all(pb < BIG) and np.all(pb == pb)
    ref = api.score_models(*cs.args(0), cs.models, host_lo=True)
    killed = [k for k in range(nm) if eb[k] == BIG]
    kept = [k for k in range(nm) if eb[k] != BIG]
    for k in kept:  # not killed: the plain kernel's bits
        assert eb[k] == pb[k] and (r["exit_slot"][k] & SLOT) == 0, (k, eb[k], pb[k])
    for k in killed:  # killed: the reference-order sum cannot beat best
        assert ref[k] >= best, (k, ref[k], best)
    for k in range(nm):  # a model whose whole sum stays below best + its margin is never killed
        if pb[k] - pm["tie"][k] < best:
            assert k in kept, (k, pb[k], best)
    if checks:
        assert killed and kept, (len(killed), len(kept))
    else:  # no check falls before the last trip: nothing can be killed
        assert not killed
    for j, g in enumerate(tc.groups):
        b = nm + j
        alive = [k for k in g if pb[k] - pm["tie"][k] < best]
        if eb[b] == BIG:
            assert not alive and checks
            assert all(ref[k] >= best for k in g)
            continue
        slot = int(r["exit_slot"][b] & SLOT)
        assert eb[b] == pb[g[slot]], (b, slot)  # a survivor's own bits
        # every model ahead of it in the walk (lower score, or equal and earlier) was killed
        for q, k in enumerate(g):
            if pb[k] < eb[b] or (pb[k] == eb[b] and q < slot):
                assert k not in alive and ref[k] >= best, (b, k)
        if g[int(r["plain_slot"][b] & SLOT)] in alive:  # the plain winner cannot be killed: it wins again
            assert eb[b] == pb[b] and slot == int(r["plain_slot"][b] & SLOT)
    if exact_models:
        pick = killed[:exact_models] + kept[:exact_models]
        P = cs.exact_pair()
        for k in pick:
            s = ex.msac_sum(ex.evaluate(P, exact_model(cs.models[k], cs.variant)), pp["thr"], pp["w"], 0)
            tie = Fr(float(pm["tie"][k]))
            if k in killed:
                assert s >= Fr(best) - tie, (k, float(s), best)
            else:
                assert abs(Fr(float(eb[k])) - s) <= tie, (k, float(s), eb[k])
    return len(killed), len(kept)
