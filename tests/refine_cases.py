"""Pairs, start models and the single-pair composition behind the refine_batch tests
(tests/test_refine_batch_gpu.py) and tools/refine_batch_bench.py.

A start model is the pair's ground truth -- the rotation and translation of
synthetic.make_pair and the affine depth relation recovered from its inliers by
triangulation -- perturbed by a degree or so and a few percent in translation, scale,
offsets and focal.  refine_single() restates mp_refine_batch's semantics for one pair
from the entries that existed before it: score_models(with_errors=True), the thresholds,
lm_refine_batch (kind 0) and the acceptance rule."""
import numpy as np

import madpose
from madpose_amd import api, synthetic
from tests.lm_cases import small_rot

KIND = {0: "calibrated", 1: "shared_focal", 2: "two_focal", 3: "calibrated"}
K_TF1 = np.array([[374.91, 0, 319.5], [0, 374.91, 239.5], [0, 0, 1.0]])


def make_pair(variant, seed, n):
    if n == 0:
        p = synthetic.make_pair(seed, n=8)
        for k in ("x0", "x1"):
            p[k] = np.zeros((0, 2))
        for k in ("depth0", "depth1"):
            p[k] = np.zeros(0)
        p["inlier_mask"] = np.zeros(0, dtype=bool)
        return p
    return synthetic.make_pair(seed, n=n, K1=K_TF1 if variant == 2 else None)


def cams(variant, p):
    return (p["K0"], p["K1"]) if variant in (0, 3) else (p["pp0"], p["pp1"])


def pair_args(variant, p):
    """(x0, x1, depth0, depth1, min_depth, cam0, cam1) of the single-pair entries"""
    return (p["x0"], p["x1"], p["depth0"], p["depth1"], p["min_depth"], *cams(variant, p))


def make_model(variant, R, t, scale, o0, o1, f0, f1):
    if variant == 0:
        return madpose.PoseScaleOffset(R, t, scale, o0, o1)
    if variant == 1:
        return madpose.PoseScaleOffsetSharedFocal(R, t, scale, o0, o1, f0)
    if variant == 2:
        return madpose.PoseScaleOffsetTwoFocal(R, t, scale, o0, o1, f0, f1)
    return madpose.PoseAndScale(R, t, scale)


def ground_truth(variant, p):
    """(R, t, scale, offset0, offset1, f0, f1) in the estimators' user units: depths of the
    inliers by triangulation with the true pose, then z0 ~ A0 d0 + B0, z1 ~ A1 d1 + B1."""
    inl = np.flatnonzero(p["inlier_mask"])
    R, t = p["R"], p["t"]
    if len(inl) < 2:
        return R, t, 1.0, 0.0, 0.0, p["f0"], p["f1"]
    h = lambda x: np.c_[x, np.ones(len(x))]
    a = h(p["x0"][inl]) @ np.linalg.inv(p["K0"]).T @ R.T
    b = h(p["x1"][inl]) @ np.linalg.inv(p["K1"]).T
    # z0 R a + t = z1 b per inlier, by its 2 x 2 normal equations
    A = np.stack([a, -b], axis=2)
    z = np.linalg.solve(np.einsum("mij,mik->mjk", A, A), np.einsum("mij,i->mj", A, -t)[..., None])[..., 0]
    z0, z1 = z[:, 0], z[:, 1]
    d0, d1 = p["depth0"][inl], p["depth1"][inl]
    if variant == 3:  # no offsets: z0 ~ A0 d0, z1 ~ A1 d1
        A0, B0 = float(d0 @ z0 / (d0 @ d0)), 0.0
        A1, B1 = float(d1 @ z1 / (d1 @ d1)), 0.0
    else:
        A0, B0 = np.polyfit(d0, z0, 1)
        A1, B1 = np.polyfit(d1, z1, 1)
    return R, t / A0, A1 / A0, B0 / A0, B1 / A1, p["f0"], p["f1"]


def start_model(variant, p, rng, rot_deg=1.0, rel=0.03):
    R, t, s, o0, o1, f0, f1 = ground_truth(variant, p)
    j = lambda: 1.0 + rel * rng.standard_normal()
    return make_model(variant, R @ small_rot(rng, rot_deg), t * (1 + rel * rng.standard_normal(3)), s * j(), o0 * j(),
                      o1 * j(), f0 * j(), f1 * j())


def to_problem_units(variant, m, norm_scale):
    if variant == 1:
        return make_model(1, m.R(), m.t(), m.scale, m.offset0, m.offset1, m.focal / norm_scale, None)
    if variant == 2:
        return make_model(2, m.R(), m.t(), m.scale, m.offset0, m.offset1, m.focal0 / norm_scale,
                          m.focal1 / norm_scale)
    return m


def to_user_units(variant, m, norm_scale):
    if variant == 1:
        return make_model(1, m.R(), m.t(), m.scale, m.offset0, m.offset1, m.focal * norm_scale, None)
    if variant == 2:
        return make_model(2, m.R(), m.t(), m.scale, m.offset0, m.offset1, m.focal0 * norm_scale,
                          m.focal1 * norm_scale)
    return m


def thresholds(variant, o, norm_scale):
    """PairConst::thr: the squared thresholds after make_problem's option transform"""
    t0, t1 = (float(v) for v in o.squared_inlier_thresholds[:2])
    if variant in (1, 2):
        t0, t1 = t0 / (norm_scale * norm_scale), t1 / (norm_scale * norm_scale)
    return [t0, t0, t1]


def model_bytes(variant, m):
    return bytes(api._model_to_c(m, variant))


class Expected:
    pass


def refine_single(variant, p, m_user, o, c, rounds, norm_scale, on_host=False):
    """mp_refine_batch's result for one pair from the single-pair entries."""
    e = Expected()
    e.rounds_run = e.rounds_accepted = 0
    e.status = -1
    e.model = m_user
    n = len(p["depth0"])
    if n == 0:  # legal: score 0, empty lists, the size rule stops the first round
        e.score_initial = e.score_final = 0.0
        e.lists = [np.zeros(0, dtype=np.int32)] * 3
        e.rounds_run, e.status = 1, 3
        return e
    args = pair_args(variant, p)
    thr = thresholds(variant, o, norm_scale)

    def sweep(m):
        s, err = madpose.score_models(variant, *args[:4], *args[5:], o, c, [m], with_errors=True)
        return float(s[0]), [np.flatnonzero(err[0, t] < thr[t]).astype(np.int32) for t in range(3)]

    cur = to_problem_units(variant, m_user, norm_scale)
    score, lists = sweep(cur)
    e.score_initial = score
    for _ in range(rounds):
        e.rounds_run += 1
        (cand, st), = madpose.lm_refine_batch(variant, *args, o, c, [(0, lists, cur)], on_host=on_host)
        e.status = st
        if st != 1:
            break
        s2, l2 = sweep(cand)
        if not s2 < score:
            break
        cur, score, lists = cand, s2, l2
        e.rounds_accepted += 1
    e.score_final = score
    e.lists = lists
    if e.rounds_accepted:
        e.model = to_user_units(variant, cur, norm_scale)
    return e


def result_key(variant, r):
    """everything a RefineResult holds, as comparable bytes / numbers"""
    return (model_bytes(variant, r.model), r.score_initial, r.score_final, r.rounds_run, r.rounds_accepted, r.status,
            tuple(a.tobytes() for a in r.inlier_indices), r.norm_scale)
