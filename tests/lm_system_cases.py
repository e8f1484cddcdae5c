"""Cases and comparisons shared by tests/test_lm_system_cpu.py and test_lm_system_gpu.py:
one LM evaluation and one LM step of the engine (mp_debug_lm_system) against
tests/lm_reference.py.

Inputs as tests/lm_cases.py: the inliers of a synthetic pair, start models perturbed from
the oracle's estimate.  Every case counts; the reference asserts its guard bands on every
block, and the seeds below were chosen on the CPU so that they hold.

The bound of an entry X (cost, g[a] or H[a, b]) with magnitude sum S_X over `rows` residual
rows is (k + rows) 2^-53 S_X: rows 2^-53 S_X is the bound of a fixed-order sum, k the
per-term allowance.  K_REF is the measured worst per-entry scaled error of the
reference's own float64 mode against its 50-digit mode over the 50-digit cases
(test_lm_system_cpu.py::test_reference_float64_yardstick measures it on every run and
holds it below this constant); the engine gets 16 K_REF: another operation order, FMA
contraction, K^-1 applied as a matrix.  Where S_X is exactly zero -- a structural zero, or a
parameter the variant does not have -- the engine's entry must be exactly 0.0.
"""
import collections
import copy
import functools
import math

import numpy as np

import madpose
import oracle
from madpose_amd import synthetic
from tests import lm_cases as LC
from tests import lm_reference as LR
from tests.helpers import oracle_cfg, oracle_opts

U = 2.0 ** -53
# measured (CPU, this suite's 50-digit cases): worst |f64 - mp| / (2^-53 S) per entry
K_REF = 821.0  # per variant 795.6 / 173.0 / 820.3
K_ENGINE = 16 * K_REF

Spec = collections.namedtuple("Spec", "variant kind lo_type use_shift mdc lists model")
Ctx = collections.namedtuple("Ctx", "variant p o args norm_scale est data inl")


def _context(variant, p):
    o, c = synthetic.example_options(LC.KIND[variant], iterations=100)
    cam0, cam1 = (p["K0"], p["K1"]) if variant == 0 else (p["pp0"], p["pp1"])
    args = (p["x0"], p["x1"], p["depth0"], p["depth1"], p["min_depth"], cam0, cam1)
    _, _, norm_scale = oracle.score_models(variant, *args[:4], cam0, cam1, oracle_opts(o), oracle_cfg(c), [])
    m, _, _ = oracle.estimate(variant, *args, oracle_opts(o), oracle_cfg(c))
    est = LC.model_of(m, variant)
    return Ctx(variant, p, o, args, norm_scale, est, engine_doubles(variant, args, o, norm_scale),
               np.flatnonzero(p["inlier_mask"]))


@functools.lru_cache(maxsize=None)
def small(variant):
    """the pair of lm_cases.setup"""
    return _context(variant, synthetic.make_pair(40 + variant, n=800) if variant < 2
                    else synthetic.config_pair(4, seed=40))


@functools.lru_cache(maxsize=None)
def big(variant):
    """about 6000 correspondences, nearly all inliers: lists of up to 5547 strictly
    increasing indices each"""
    return _context(variant, synthetic.make_pair(90 + variant, n=6000, outlier_ratio=0.05))


def engine_doubles(variant, args, o, norm_scale):
    """The doubles the LM reads: pixels and K (calibrated), or the principal-point-centred
    coordinates over the normalisation scale; the Sampson weight as the optimizers form it
    (src/optimizer.h:69-70 after the option transform of src/hybrid_pose_estimator.cpp:13-23)."""
    x0, x1, d0, d1, _md, cam0, cam1 = args
    x0, x1 = np.asarray(x0, np.float64), np.asarray(x1, np.float64)
    thr0, thr1 = [np.float64(v) for v in o.squared_inlier_thresholds[:2]]
    d = dict(d0=np.asarray(d0, np.float64), d1=np.asarray(d1, np.float64))
    if variant == 0:
        K0, K1 = np.asarray(cam0, np.float64).reshape(3, 3), np.asarray(cam1, np.float64).reshape(3, 3)
        ssw = np.float64(o.data_type_weights[1]) * (2 * thr0 / thr1)
        d.update(x0=x0, x1=x1, K0=K0, K1=K1,
                 weight=float(np.sqrt(ssw) / (1.0 / (K0[0, 0] + K0[1, 1]) + 1.0 / (K1[0, 0] + K1[1, 1]))))
    else:
        s = np.float64(norm_scale)
        thr0, thr1 = thr0 / (s * s), thr1 / (s * s)
        ssw = np.float64(o.data_type_weights[1]) * (2 * thr0 / thr1)
        d.update(x0=(x0 - np.asarray(cam0, np.float64).reshape(2)) / s,
                 x1=(x1 - np.asarray(cam1, np.float64).reshape(2)) / s, weight=float(np.sqrt(ssw)))
    return d


def rot_to_quat(R):
    """Eigen::Quaternion(Matrix3), the conversion of the optimizers' constructor, in doubles"""
    R = np.asarray(R, np.float64).reshape(9)
    tr = R[0] + R[4] + R[8]
    if tr > 0:
        s = np.sqrt(tr + 1.0)
        w = 0.5 * s
        s = 0.5 / s
        return np.array([w, (R[7] - R[5]) * s, (R[2] - R[6]) * s, (R[3] - R[1]) * s])
    i = 0
    if R[4] > R[0]:
        i = 1
    if R[8] > R[4 * i]:
        i = 2
    j, k = (i + 1) % 3, (i + 2) % 3
    s = np.sqrt(R[4 * i] - R[4 * j] - R[4 * k] + 1.0)
    v = np.zeros(3)
    v[i] = 0.5 * s
    s = 0.5 / s
    w = (R[3 * k + j] - R[3 * j + k]) * s
    v[j] = (R[3 * j + i] + R[3 * i + j]) * s
    v[k] = (R[3 * k + i] + R[3 * i + k]) * s
    return np.array([w, v[0], v[1], v[2]])


def params_of(model, variant):
    f0 = f1 = 1.0
    if variant == 1:
        f0 = f1 = float(model.focal)
    elif variant == 2:
        f0, f1 = float(model.focal0), float(model.focal1)
    return (rot_to_quat(model.R()), np.asarray(model.t(), np.float64), float(model.scale), float(model.offset0),
            float(model.offset1), f0, f1)


def start_model(rng, cx):
    """a start near the estimate, perturbed as lm_cases.problems perturbs it"""
    est, variant = cx.est, cx.variant
    R = est.R() @ LC.small_rot(rng, 0.5)
    t = est.t() * (1 + 0.02 * rng.standard_normal(3))
    sc, o0, o1 = est.scale * (1 + 0.01 * rng.standard_normal()), est.offset0, est.offset1
    if variant == 0:
        return madpose.PoseScaleOffset(R, t, sc, o0, o1)
    if variant == 1:
        return madpose.PoseScaleOffsetSharedFocal(R, t, sc, o0, o1, est.focal / cx.norm_scale * 1.02)
    return madpose.PoseScaleOffsetTwoFocal(R, t, sc, o0, o1, est.focal0 / cx.norm_scale * 1.02,
                                           est.focal1 / cx.norm_scale * 0.98)


def with_offsets(m, variant, o0, o1):
    if variant == 0:
        return madpose.PoseScaleOffset(m.R(), m.t(), m.scale, o0, o1)
    if variant == 1:
        return madpose.PoseScaleOffsetSharedFocal(m.R(), m.t(), m.scale, o0, o1, m.focal)
    return madpose.PoseScaleOffsetTwoFocal(m.R(), m.t(), m.scale, o0, o1, m.focal0, m.focal1)


def draw(rng, cx, sizes, sort=True, replace=False):
    ls = [rng.choice(cx.inl, s, replace=replace).astype(np.int32) for s in sizes]
    return [np.sort(l) for l in ls] if sort else ls


def spec(rng, cx, sizes, kind=0, lo_type=0, use_shift=True, mdc=False, **kw):
    return Spec(cx.variant, kind, lo_type, use_shift, mdc, draw(rng, cx, sizes, **kw), start_model(rng, cx))


# sizes of the mixed 50-digit problems: every list empty alone and in pairs, up to 40 blocks
MIXED = [(5, 4, 6), (12, 0, 9), (0, 7, 8), (9, 8, 0), (0, 0, 10), (6, 0, 0), (0, 5, 0), (14, 13, 13)]


def formula_specs(variant):
    """The 50-digit problems of one variant (195 blocks): one block of each type alone,
    mixed problems, both solver kinds, the three LO types, use_shift off, the depth bound on."""
    cx = small(variant)
    rng = np.random.default_rng(500 + variant)
    out = [spec(rng, cx, s) for s in ((1, 0, 0), (0, 1, 0), (0, 0, 1))]
    out += [spec(rng, cx, s) for s in MIXED]
    out.append(spec(rng, cx, (4, 3, 5), kind=1))
    out.append(spec(rng, cx, (5, 5, 7), lo_type=1))
    out.append(spec(rng, cx, (5, 6, 7), lo_type=2))
    out.append(spec(rng, cx, (4, 4, 4), kind=1, use_shift=False))
    out.append(spec(rng, cx, (4, 4, 4), mdc=True))
    out.append(spec(rng, cx, (3, 3, 3), use_shift=False, mdc=True))
    return out


def effective_lists(s):
    """the lists the optimizer is given: no reprojection blocks for LO type 1 (EPI_ONLY), no
    Sampson blocks for LO type 2 (MD_ONLY)"""
    e = np.zeros(0, np.int32)
    return [e if s.lo_type == 1 else s.lists[0], e if s.lo_type == 1 else s.lists[1],
            e if s.lo_type == 2 else s.lists[2]]


def job_use_shift(s):
    """config.use_shift reaches the calibrated optimizers and the shared-focal
    NonMinimalSolver (src/hybrid_pose_estimator.cpp:206, 281, ..shared_focal..cpp:149); the
    others run with the optimizers' default, true"""
    return s.use_shift if (s.variant == 0 or (s.variant == 1 and s.kind == 1)) else True


def reference(cx, s, mode):
    lists = effective_lists(s)
    r = LR.system(s.variant, cx.data, lists, params_of(s.model, s.variant), mode)
    r["col"] = LR.active_set(s.variant, len(lists[0]), len(lists[1]), len(lists[2]), job_use_shift(s))
    return r


def config_of(s):
    c = synthetic.example_options(LC.KIND[s.variant], iterations=100)[1]
    c.LO_type = s.lo_type
    c.use_shift = s.use_shift
    c.min_depth_constraint = s.mdc
    return c


def engine(cx, specs, where, radius=1e4, ranges=None, device=None):
    """mp_debug_lm_system of the problems, one call per run of equal configs; a list of
    per-problem dicts (cost, g, H, col, d, pd, status)"""
    out = [None] * len(specs)
    radius = np.broadcast_to(np.asarray(radius, np.float64), (len(specs),))
    key = lambda s: (s.lo_type, s.use_shift, s.mdc)
    for k in sorted({key(s) for s in specs}):
        js = [j for j, s in enumerate(specs) if key(s) == k]
        probs = [(specs[j].kind, specs[j].lists, specs[j].model) for j in js]
        r = madpose.lm_system(cx.variant, *cx.args, cx.o, config_of(specs[js[0]]), probs, radius[js], where=where,
                              block_ranges=None if ranges is None else [ranges[j] for j in js], device=device)
        for i, j in enumerate(js):
            out[j] = {name: v[i] for name, v in r.items()}
    return out


def scaled_errors(got, ref, inactive_zero=False):
    """Per entry |X - X_ref| / (2^-53 S_X) of cost, g and H (nan where S_X = 0), after
    asserting the exact zeros: where S_X is exactly zero the engine's entry is 0.0; with
    inactive_zero (the compacted system) also every entry of an inactive parameter."""
    X = np.r_[got["cost"], got["g"], got["H"]]
    Xr = np.r_[ref["cost"], ref["g"], ref["H"]]
    Sx = np.r_[ref["S_cost"], ref["S_g"], ref["S_H"]]
    zero = Sx == 0.0
    if inactive_zero:
        col = np.asarray(ref["col"], bool)
        pair = np.array([col[a] and col[b] for a in range(11) for b in range(a, 11)])
        zero = zero | np.r_[False, ~col, ~pair]
    assert np.all(X[zero] == 0.0), ("an entry that must be exactly zero is not", np.flatnonzero(zero & (X != 0.0)),
                                    X[zero])
    err = np.full(len(X), np.nan)
    err[~zero] = np.abs(X[~zero] - Xr[~zero]) / (U * Sx[~zero])
    return err


def check_system(got, ref, where, tag):
    """col, the exact zeros and the bound (K_ENGINE + rows) 2^-53 S_X on every other entry;
    returns the worst per-term part max(err - rows, 0) for the printed figure"""
    assert list(got["col"]) == [int(c) for c in ref["col"]], (tag, list(got["col"]), ref["col"])
    err = scaled_errors(got, ref, inactive_zero=where == 3)
    worst = float(np.nanmax(err)) if np.any(~np.isnan(err)) else 0.0
    bound = K_ENGINE + ref["rows"]
    assert bound * U < 1e-9, (tag, bound)  # a wrong factor, sign or term cannot fit inside
    assert worst <= bound, (tag, "worst scaled error", worst, "bound", bound, "entry", int(np.nanargmax(err)))
    return max(worst - ref["rows"], 0.0)


def check_step(got, radius, tag):
    """The step on the engine's own H and g: with A, b of lm_reference.damped_system at 50
    digits from those doubles and y = d / D, |A y - b|_inf <= c n 2^-53 (|A|_inf |y|_inf +
    |b|_inf), c = 3 n + 4; d = 0 on inactive parameters.

    c: Cholesky with the two triangular solves gives (A + dA) y = b, |dA| <= gamma_{3n+1}
    |L||L^T| (Higham, Accuracy and Stability of Numerical Algorithms, Theorem 10.4), and
    (|L||L^T|)_ij <= sqrt(a_ii a_jj), so |dA y|_inf <= (3 n + 1) n u |A|_inf |y|_inf to first
    order.  The engine forms A, b and d in doubles as well: two roundings per entry of D H D,
    three in D, two in the damping, one each in b and in d = y D -- below 3 n u (|A| |y| +
    |b|) for n >= 6, the smallest system.  Hence 3 n + 4, not tuned."""
    col = np.asarray(got["col"], bool)
    assert np.all(got["d"][~col] == 0.0), (tag, got["d"])
    assert got["pd"] == 1, (tag, got["pd"])
    A, b, D, act = LR.damped_system(got["H"], got["g"], col, radius)
    n = len(act)
    y = [LR.MP.mpf(float(got["d"][a])) / D[i] for i, a in enumerate(act)]
    res = max(abs(sum((A[i][j] * y[j] for j in range(n)), LR.MP.mpf(0)) - b[i]) for i in range(n))
    nA = max(sum(abs(v) for v in row) for row in A)
    scale = nA * max(abs(v) for v in y) + max(abs(v) for v in b)
    c = 3 * n + 4
    ratio = float(res / (n * U * scale))
    assert ratio <= c, (tag, "backward error over n u (|A||y| + |b|)", ratio, "c", c)
    return ratio


def clamp_case(variant):
    """a Sampson-only problem with a tiny Sampson weight: every H_aa is below 1e-6, so the
    damping is the clamp's 1e-6 / radius"""
    cx = small(variant)
    o2 = copy.deepcopy(cx.o)
    w = list(o2.data_type_weights)
    w[1] = 1e-16
    o2.data_type_weights = w
    cx2 = cx._replace(o=o2, data=engine_doubles(variant, cx.args, o2, cx.norm_scale))
    return cx2, spec(np.random.default_rng(40 + variant), cx2, (0, 0, 12), lo_type=1)


def nan_case(variant):
    """a NaN offset0 in a problem that reads it: a system that is not finite"""
    cx = small(variant)
    s = spec(np.random.default_rng(60 + variant), cx, (5, 5, 7))
    return cx, s._replace(model=with_offsets(s.model, variant, float("nan"), s.model.offset1))


# ---- Plus(x, d) as the LM forms the candidate, in doubles ----

def _fma(a, b, c):
    """a b + c rounded once (fractions are exact; float() rounds to nearest even)"""
    from fractions import Fraction as Fr
    if not all(map(math.isfinite, (a, b, c))):
        return a * b + c
    return float(Fr(a) * Fr(b) + Fr(c))


def plus_model(s, d, min_depth, form):
    """The candidate of the first step from model s.model: the quaternion of the model
    (Eigen's conversion), Plus with the step quaternion on the left, the remaining
    parameters added and projected onto their lower bounds (scale >= 1e-2; with the depth
    bound, offsets >= -min_depth + 1e-2; two-focal focals >= 1e-6), then the rotation matrix
    of the normalised quaternion.  Returns (R 9, t 3, scale, o0, o1, f0, f1) in doubles.

    form: how the build contracts the sums of products into fused multiply-adds.  "host":
    clang's rule within one expression, left to right -- a b +- c d +- e f = fma(+-e, f,
    fma(a, b, +-(c d))) -- as the host LM is built.  "device": the same, except that the two
    rows of the quaternion product that begin with a sum round their first product and
    fuse the second (fma(c, d, a b)); this is what lm_batch_kernel's code object does,
    found by comparing with its results, so a compiler that contracts these rows otherwise
    moves the last bit of the rotation and needs this restated."""
    variant = s.variant
    q, t, sc, o0, o1, f0, f1 = params_of(s.model, variant)
    q = [float(v) for v in q]
    d = [float(v) for v in d]

    def dot(*terms, swap=False):  # terms: (sign, a, b), the first with sign +
        (_, a0, b0), (s1, a1, b1) = terms[0], terms[1]
        acc = _fma(s1 * a1, b1, a0 * b0) if swap else _fma(a0, b0, s1 * (a1 * b1))
        for sg, a, b in terms[2:]:
            acc = _fma(sg * a, b, acc)
        return acc

    dev = form == "device"
    nd = math.sqrt(dot((1, d[0], d[0]), (1, d[1], d[1]), (1, d[2], d[2])))
    cq = list(q)
    if nd > 0:
        sn = math.sin(nd) / nd
        qd = [math.cos(nd), sn * d[0], sn * d[1], sn * d[2]]
        cq = [dot((1, qd[0], q[0]), (-1, qd[1], q[1]), (-1, qd[2], q[2]), (-1, qd[3], q[3])),
              dot((1, qd[0], q[1]), (1, qd[1], q[0]), (1, qd[2], q[3]), (-1, qd[3], q[2]), swap=dev),
              dot((1, qd[0], q[2]), (-1, qd[1], q[3]), (1, qd[2], q[0]), (1, qd[3], q[1])),
              dot((1, qd[0], q[3]), (1, qd[1], q[2]), (-1, qd[2], q[1]), (1, qd[3], q[0]), swap=dev)]
    col = LR.active_set(variant, *[len(l) for l in effective_lists(s)], job_use_shift(s))

    def upd(slot, v, lo):
        if not col[slot]:
            return v
        v = v + d[slot]
        return lo if (lo is not None and v < lo) else v

    tt = [float(t[k]) + d[3 + k] for k in range(3)]
    sc = upd(LR.S, sc, 1e-2)
    o0 = upd(LR.O0, o0, -float(min_depth[0]) + 1e-2 if s.mdc else None)
    o1 = upd(LR.O1, o1, -float(min_depth[1]) + 1e-2 if s.mdc else None)
    f0 = upd(LR.F0, f0, 1e-6 if variant == 2 else None)
    f1 = upd(LR.F1, f1, 1e-6 if variant == 2 else None)
    if variant == 1:
        f1 = f0
    n = math.sqrt(dot((1, cq[0], cq[0]), (1, cq[1], cq[1]), (1, cq[2], cq[2]), (1, cq[3], cq[3])))
    w, x, y, z = [c / n for c in cq]
    one_minus_2 = lambda a, b: _fma(-2.0, _fma(a, a, b * b), 1.0)  # 1 - 2 * (a*a + b*b)
    two = lambda a, b, sg, c, e: 2.0 * _fma(a, b, sg * (c * e))   # 2 * (a*b +- c*e)
    R = [one_minus_2(y, z), two(x, y, -1, w, z), two(x, z, 1, w, y),
         two(x, y, 1, w, z), one_minus_2(x, z), two(y, z, -1, w, x),
         two(x, z, -1, w, y), two(y, z, 1, w, x), one_minus_2(x, y)]
    return R, tt, sc, o0, o1, f0, f1


def model_doubles(m, variant):
    f0 = f1 = None
    if variant == 1:
        f0 = f1 = float(m.focal)
    elif variant == 2:
        f0, f1 = float(m.focal0), float(m.focal1)
    return (list(np.asarray(m.R(), np.float64).reshape(9)), list(np.asarray(m.t(), np.float64)), float(m.scale),
            float(m.offset0), float(m.offset1), f0, f1)


# the kernel's sums of products, as its compiler contracts them (plus_model)
DEVICE_FORM = "device"

TIE_CASES = [((8, 8, 8), 0, False), ((12, 0, 9), 1, True), ((0, 7, 8), 0, False), ((30, 30, 30), 1, False),
             ((20, 25, 30), 0, True), ((9, 9, 7), 0, False), ((40, 0, 40), 1, False), ((0, 33, 17), 0, False)]


def first_step_ties(on_host, where, form, device=None):
    """Iteration cap 1 on problems whose first step is accepted: the LM's result is, bit for
    bit, Plus(start, d) of the hook's d (lm_system_cases.plus_model).  Returns how many
    problems were compared and how many matched, per variant."""
    out = {}
    for v in (0, 1, 2):
        cx = small(v)
        rng = np.random.default_rng(300 + v)
        same = total = 0
        for sizes, kind, mdc in TIE_CASES:
            s = spec(rng, cx, sizes, kind=kind, mdc=mdc)
            c = config_of(s)
            c.ceres_max_num_iterations = 1
            (m1, st), = madpose.lm_refine_batch(v, *cx.args, cx.o, c, [(s.kind, s.lists, s.model)], on_host=on_host)
            assert st == 1
            start = model_doubles(s.model, v)
            got = model_doubles(m1, v)
            if got[1:] == start[1:]:
                continue  # the step was rejected (or a tolerance stopped the run): the start comes back
            g = engine(cx, [s], where, radius=1e4, device=device)[0]
            assert g["pd"] == 1
            want = plus_model(s, g["d"], cx.args[4], form)
            total += 1
            ok = all(np.asarray(a, np.float64).tobytes() == np.asarray(b, np.float64).tobytes()
                     for a, b in zip(got, want) if a is not None)
            if not ok:
                print("variant", v, sizes, "differs:", [(a, b) for a, b in zip(got, want) if a is not None and
                                                          np.asarray(a).tobytes() != np.asarray(b).tobytes()])
            same += ok
        out[v] = (total, same)
    return out
