"""Python surface of the reference's pybind11 module (src/bindings.cpp), backed by the
MI355X engine through the C ABI.  Names, defaults, argument meaning and return types
follow src/bindings.cpp:34-175 so user code written for `import madpose` runs unchanged.
"""
import ctypes
import math

import numpy as np

from . import _lib as L


# ---------------------------------------------------------------------------
# option / config containers (src/bindings.cpp:78-109, src/hybrid_ransac.h:17-25,
# src/estimator_config.h:7-33; RansacLib defaults as restated in DESIGN.md)
class HybridLORansacOptions:
    def __init__(self):
        self.min_num_iterations = 100
        self.max_num_iterations = 10000
        self.max_num_iterations_per_solver = 10000
        self.success_probability = 0.99
        self.squared_inlier_thresholds = []
        self.data_type_weights = []
        self.random_seed = 0
        self.num_lo_steps = 10
        self.threshold_multiplier = math.sqrt(2.0)
        self.num_lsq_iterations = 4
        self.min_sample_multiplicator = 7
        self.non_min_sample_multiplier = 3
        self.lo_starting_iterations = 50
        self.final_least_squares = False
        self.use_ours = False
        self.use_4p4d = False

    def _to_c(self):
        o = L.mp_ransac_options()
        thr = list(self.squared_inlier_thresholds)
        w = list(self.data_type_weights)
        if len(thr) < 2:
            raise ValueError("squared_inlier_thresholds must hold [reprojection^2, epipolar^2]")
        if len(w) < 2:
            raise ValueError("data_type_weights must hold [reprojection, epipolar]")
        o.success_probability = float(self.success_probability)
        o.squared_inlier_thresholds[0] = float(thr[0])
        o.squared_inlier_thresholds[1] = float(thr[1])
        o.data_type_weights[0] = float(w[0])
        o.data_type_weights[1] = float(w[1])
        o.threshold_multiplier = float(self.threshold_multiplier)
        o.min_num_iterations = int(self.min_num_iterations)
        o.max_num_iterations = int(self.max_num_iterations)
        o.max_num_iterations_per_solver = int(self.max_num_iterations_per_solver)
        o.random_seed = int(self.random_seed)
        o.num_lo_steps = int(self.num_lo_steps)
        o.num_lsq_iterations = int(self.num_lsq_iterations)
        o.min_sample_multiplicator = int(self.min_sample_multiplicator)
        o.non_min_sample_multiplier = int(self.non_min_sample_multiplier)
        o.lo_starting_iterations = int(self.lo_starting_iterations)
        o.final_least_squares = int(bool(self.final_least_squares))
        o.use_ours = int(bool(self.use_ours))
        o.use_4p4d = int(bool(self.use_4p4d))
        return o


class EstimatorConfig:
    HYBRID, EPI_ONLY, MD_ONLY = 0, 1, 2

    def __init__(self, solver=0, score=0, LO=0):
        self.solver_type = int(solver)
        self.score_type = int(score)
        self.LO_type = int(LO)
        self.min_depth_constraint = True
        self.use_shift = True
        self.ceres_function_tolerance = 1e-6
        self.ceres_gradient_tolerance = 1e-8
        self.ceres_parameter_tolerance = 1e-6
        self.ceres_max_num_iterations = 25.0
        self.ceres_use_nonmonotonic_steps = True
        self.ceres_num_threads = 1

    def _to_c(self):
        c = L.mp_estimator_config()
        c.ceres_function_tolerance = float(self.ceres_function_tolerance)
        c.ceres_gradient_tolerance = float(self.ceres_gradient_tolerance)
        c.ceres_parameter_tolerance = float(self.ceres_parameter_tolerance)
        c.ceres_max_num_iterations = float(self.ceres_max_num_iterations)
        c.solver_type = int(self.solver_type)
        c.score_type = int(self.score_type)
        c.lo_type = int(self.LO_type)
        c.min_depth_constraint = int(bool(self.min_depth_constraint))
        c.use_shift = int(bool(self.use_shift))
        c.ceres_use_nonmonotonic_steps = int(bool(self.ceres_use_nonmonotonic_steps))
        c.ceres_num_threads = int(self.ceres_num_threads)
        return c


class RansacOptions:
    def __init__(self):
        self.min_num_iterations_ = 100
        self.max_num_iterations_ = 10000
        self.success_probability_ = 0.99
        self.squared_inlier_threshold_ = 1.0
        self.random_seed_ = 0


class LORansacOptions:
    def __init__(self):
        self.min_num_iterations = 100
        self.max_num_iterations = 10000
        self.success_probability = 0.99
        self.squared_inlier_threshold = 1.0
        self.random_seed = 0
        self.num_lo_steps = 10
        self.threshold_multiplier = math.sqrt(2.0)
        self.num_lsq_iterations = 4
        self.min_sample_multiplicator = 7
        self.non_min_sample_multiplier = 3
        self.lo_starting_iterations = 50
        self.final_least_squares = False


class RansacStats:
    def __init__(self):
        self.num_iterations = 0
        self.best_num_inliers = 0
        self.best_model_score = float("inf")
        self.inlier_ratio = 0.0
        self.inlier_indices = []
        self.number_lo_iterations = 0


class HybridRansacStatistics:
    def __init__(self):
        self.num_iterations_total = 0
        self.num_iterations_per_solver = [0, 0]
        self.best_num_inliers = 0
        self.best_solver_type = -1
        self.best_model_score = float("inf")
        self.inlier_ratios = [0.0, 0.0, 0.0]
        self.inlier_indices = [[], [], []]
        self.number_lo_iterations = 0
        # engine counters (not in the reference)
        self.num_hypotheses = 0
        self.num_lo_sweeps = 0
        self.num_batches = 0
        self.seconds_total = 0.0
        self.seconds_lo = 0.0
        self.seconds_gpu_wait = 0.0

    def __repr__(self):
        return (f"HybridRansacStatistics(iterations={self.num_iterations_total}, per_solver={self.num_iterations_per_solver}, "
                f"inliers={self.best_num_inliers}, score={self.best_model_score:.6g}, lo={self.number_lo_iterations})")


# ---------------------------------------------------------------------------
# model types (src/pose.h:7-56, src/bindings.cpp:111-154)
class PoseAndScale:
    def __init__(self, *args):
        self.pose = np.zeros((3, 4))
        self.scale = 1.0
        if len(args) == 2:
            self.pose = np.array(args[0], dtype=np.float64).reshape(3, 4)
            self.scale = float(args[1])
        elif len(args) == 3:
            self.pose[:, :3] = np.asarray(args[0], dtype=np.float64).reshape(3, 3)
            self.pose[:, 3] = np.asarray(args[1], dtype=np.float64).reshape(3)
            self.scale = float(args[2])
        elif args:
            raise TypeError("PoseAndScale(pose, scale) or PoseAndScale(R, t, scale)")

    def R(self):
        return self.pose[:, :3].copy()

    def t(self):
        return self.pose[:, 3].copy()


class PoseScaleOffset(PoseAndScale):
    _n_extra = 0

    def __init__(self, *args):
        self.pose = np.zeros((3, 4))
        self.scale, self.offset0, self.offset1 = 1.0, 0.0, 0.0
        self._init_extra()
        k = self._n_extra
        if len(args) == 4 + k:  # pose, scale, b0, b1, [focals]
            self.pose = np.array(args[0], dtype=np.float64).reshape(3, 4)
            vals = args[1:]
        elif len(args) == 5 + k:  # R, t, scale, b0, b1, [focals]
            self.pose[:, :3] = np.asarray(args[0], dtype=np.float64).reshape(3, 3)
            self.pose[:, 3] = np.asarray(args[1], dtype=np.float64).reshape(3)
            vals = args[2:]
        elif not args:
            return
        else:
            raise TypeError(f"{type(self).__name__}: unexpected constructor arguments")
        self.scale, self.offset0, self.offset1 = float(vals[0]), float(vals[1]), float(vals[2])
        self._set_extra([float(v) for v in vals[3:]])

    def _init_extra(self):
        pass

    def _set_extra(self, vals):
        pass

    def __repr__(self):
        return f"{type(self).__name__}(scale={self.scale:.6g}, offset0={self.offset0:.6g}, offset1={self.offset1:.6g})"


class PoseScaleOffsetSharedFocal(PoseScaleOffset):
    _n_extra = 1

    def _init_extra(self):
        self.focal = 1.0

    def _set_extra(self, vals):
        self.focal = vals[0]


class PoseScaleOffsetTwoFocal(PoseScaleOffset):
    _n_extra = 2

    def _init_extra(self):
        self.focal0 = 1.0
        self.focal1 = 1.0

    def _set_extra(self, vals):
        self.focal0, self.focal1 = vals[0], vals[1]


def _model_from_c(m, variant):
    R = np.array(m.R[:]).reshape(3, 3)
    t = np.array(m.t[:])
    if variant == L.CALIBRATED:
        return PoseScaleOffset(R, t, m.scale, m.offset0, m.offset1)
    if variant == L.SHARED_FOCAL:
        return PoseScaleOffsetSharedFocal(R, t, m.scale, m.offset0, m.offset1, m.focal0)
    if variant == L.SCALE_ONLY:
        return PoseAndScale(R, t, m.scale)
    return PoseScaleOffsetTwoFocal(R, t, m.scale, m.offset0, m.offset1, m.focal0, m.focal1)


def _model_to_c(p, variant):
    m = L.mp_model()
    pose = np.asarray(p.pose, dtype=np.float64).reshape(3, 4)
    m.R[:] = pose[:, :3].ravel().tolist()
    m.t[:] = pose[:, 3].tolist()
    m.scale, m.offset0, m.offset1 = float(p.scale), float(getattr(p, "offset0", 0.0)), float(getattr(p, "offset1", 0.0))
    if variant == L.SHARED_FOCAL:
        m.focal0 = m.focal1 = float(p.focal)
    elif variant == L.TWO_FOCAL:
        m.focal0, m.focal1 = float(p.focal0), float(p.focal1)
    else:
        m.focal0 = m.focal1 = 1.0
    return m


def _stats_from_c(s, idx, n):
    out = HybridRansacStatistics()
    out.num_iterations_total = int(s.num_iterations_total)
    out.num_iterations_per_solver = [int(s.num_iterations_per_solver[0]), int(s.num_iterations_per_solver[1])]
    out.best_num_inliers = int(s.best_num_inliers)
    out.best_solver_type = int(s.best_solver_type)
    out.best_model_score = float(s.best_model_score)
    out.inlier_ratios = [float(v) for v in s.inlier_ratios]
    out.inlier_indices = [idx[t * n: t * n + s.num_inliers[t]].tolist() for t in range(3)]
    out.number_lo_iterations = int(s.number_lo_iterations)
    out.num_hypotheses = int(s.num_hypotheses)
    out.num_lo_sweeps = int(s.num_lo_sweeps)
    out.num_batches = int(s.num_batches)
    out.seconds_total = float(s.seconds_total)
    out.seconds_lo = float(s.seconds_lo)
    out.seconds_gpu_wait = float(s.seconds_gpu_wait)
    return out


# ---------------------------------------------------------------------------
def _pts(a, name):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError(f"{name} must be an N x 2 array of pixel coordinates")
    return a


def _vec(a, n, name):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1))
    if a.shape[0] != n:
        raise ValueError(f"{name} must hold one value per correspondence ({n}), got {a.shape[0]}")
    return a


def _dp(a):
    return a.ctypes.data_as(L.c_double_p)


_DEFAULT_DEVICE = 0


def set_device(device):
    """Select the HIP device used by subsequent calls (one process per GPU)."""
    global _DEFAULT_DEVICE
    _DEFAULT_DEVICE = int(device)


def _estimate(variant, x0, x1, depth0, depth1, min_depth, cam0, cam1, options, est_config, device):
    x0 = _pts(x0, "x0")
    x1 = _pts(x1, "x1")
    n = x0.shape[0]
    if x1.shape[0] != n:
        raise ValueError("x0 and x1 must have the same number of rows")
    d0 = _vec(depth0, n, "depth0")
    d1 = _vec(depth1, n, "depth1")
    md = np.ascontiguousarray(np.asarray(min_depth, dtype=np.float64).reshape(-1))
    if md.shape[0] != 2:
        raise ValueError("min_depth must hold two values")
    ncam = 9 if variant in (L.CALIBRATED, L.SCALE_ONLY) else 2
    c0 = np.ascontiguousarray(np.asarray(cam0, dtype=np.float64).reshape(-1))
    c1 = np.ascontiguousarray(np.asarray(cam1, dtype=np.float64).reshape(-1))
    if c0.shape[0] != ncam or c1.shape[0] != ncam:
        raise ValueError("K0/K1 must be 3x3" if ncam == 9 else "pp0/pp1 must hold two values")
    if est_config is None:
        est_config = EstimatorConfig()
    o = options._to_c()
    c = est_config._to_c()
    model = L.mp_model()
    stats = L.mp_stats()
    idx = np.zeros(3 * max(n, 1), dtype=np.int32)
    code = L.lib().mp_estimate(variant, n, _dp(x0), _dp(x1), _dp(d0), _dp(d1), _dp(md), _dp(c0), _dp(c1),
                               ctypes.byref(o), ctypes.byref(c), ctypes.byref(model), ctypes.byref(stats),
                               idx.ctypes.data_as(L.c_int32_p), _DEFAULT_DEVICE if device is None else int(device))
    L.check(code)
    return _model_from_c(model, variant), _stats_from_c(stats, idx, n)


def HybridEstimatePoseScaleOffset(x0, x1, depth0, depth1, min_depth, K0, K1, options, est_config=None, device=None):
    """src/hybrid_pose_estimator.cpp:8-35 (bindings.cpp:169-170)."""
    return _estimate(L.CALIBRATED, x0, x1, depth0, depth1, min_depth, K0, K1, options, est_config, device)


def HybridEstimatePoseScaleOffsetSharedFocal(x0, x1, depth0, depth1, min_depth, pp0, pp1, options, est_config=None,
                                             device=None):
    """src/hybrid_pose_shared_focal_estimator.cpp:8-51 (bindings.cpp:171-172)."""
    return _estimate(L.SHARED_FOCAL, x0, x1, depth0, depth1, min_depth, pp0, pp1, options, est_config, device)


def HybridEstimatePoseScaleOffsetTwoFocal(x0, x1, depth0, depth1, min_depth, pp0, pp1, options, est_config=None,
                                          device=None):
    """src/hybrid_pose_two_focal_estimator.cpp:34-75 (bindings.cpp:173-174)."""
    return _estimate(L.TWO_FOCAL, x0, x1, depth0, depth1, min_depth, pp0, pp1, options, est_config, device)


def HybridEstimatePoseAndScale(x0, x1, depth0, depth1, K0, K1, options, est_config=None, device=None):
    """src/hybrid_pose_estimator.cpp:37-63, 297-442 (bindings.cpp:167-168): scale-only
    estimator (no depth offsets); returns (PoseAndScale, HybridRansacStatistics)."""
    return _estimate(L.SCALE_ONLY, x0, x1, depth0, depth1, [0.0, 0.0], K0, K1, options, est_config, device)


def estimate_scale_and_pose(X, Y, W):
    """src/solver.cpp:5-33 (bindings.cpp:156): weighted Procrustes with scale on the
    device; X, Y are 3 x N point matrices (columns), W the N weights."""
    X = np.asarray(X, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    if X.ndim != 2 or X.shape[0] != 3 or X.shape != Y.shape:
        raise ValueError("X and Y must be 3 x N matrices of the same shape")
    n = X.shape[1]
    W = _vec(W, n, "W")
    Xp = np.ascontiguousarray(X.T)
    Yp = np.ascontiguousarray(Y.T)
    out = L.mp_model()
    L.check(L.lib().mp_estimate_scale_and_pose(_dp(Xp), _dp(Yp), _dp(W), n, ctypes.byref(out), _DEFAULT_DEVICE))
    return _model_from_c(out, L.SCALE_ONLY)


def estimate_batch(variant, pairs, options, est_config=None, device=None, num_streams=4):
    """Many independent pairs on one device (host threads x HIP streams).

    pairs: list of dicts with x0, x1, depth0, depth1, min_depth, and K0/K1 (calibrated)
    or pp0/pp1.  Returns a list of (model, stats)."""
    if est_config is None:
        est_config = EstimatorConfig()
    x0s, x1s, d0s, d1s, mds, c0s, c1s, offs = [], [], [], [], [], [], [], [0]
    for p in pairs:
        x0 = _pts(p["x0"], "x0")
        n = x0.shape[0]
        x0s.append(x0)
        x1s.append(_pts(p["x1"], "x1"))
        d0s.append(_vec(p["depth0"], n, "depth0"))
        d1s.append(_vec(p["depth1"], n, "depth1"))
        mds.append(np.asarray(p["min_depth"], dtype=np.float64).reshape(2))
        if variant == L.CALIBRATED:
            c0s.append(np.asarray(p["K0"], dtype=np.float64).reshape(9))
            c1s.append(np.asarray(p["K1"], dtype=np.float64).reshape(9))
        else:
            c0s.append(np.asarray(p["pp0"], dtype=np.float64).reshape(2))
            c1s.append(np.asarray(p["pp1"], dtype=np.float64).reshape(2))
        offs.append(offs[-1] + n)
    P = len(pairs)
    cat = lambda xs, w: np.ascontiguousarray(np.concatenate(xs).reshape(-1)) if xs else np.zeros(w)
    X0, X1, D0, D1 = cat(x0s, 2), cat(x1s, 2), cat(d0s, 1), cat(d1s, 1)
    MD, C0, C1 = cat(mds, 2), cat(c0s, 9), cat(c1s, 9)
    offsets = np.asarray(offs, dtype=np.int64)
    models = (L.mp_model * max(P, 1))()
    stats = (L.mp_stats * max(P, 1))()
    idx = np.zeros(3 * max(offs[-1], 1), dtype=np.int32)
    o = options._to_c()
    c = est_config._to_c()
    code = L.lib().mp_estimate_batch(variant, P, offsets.ctypes.data_as(L.c_int64_p), _dp(X0), _dp(X1), _dp(D0),
                                     _dp(D1), _dp(MD), _dp(C0), _dp(C1), ctypes.byref(o), ctypes.byref(c), models,
                                     stats, idx.ctypes.data_as(L.c_int32_p),
                                     _DEFAULT_DEVICE if device is None else int(device), int(num_streams))
    L.check(code)
    out = []
    for p in range(P):
        n = offs[p + 1] - offs[p]
        out.append((_model_from_c(models[p], variant), _stats_from_c(stats[p], idx[3 * offs[p]:], n)))
    return out


def _concat_pairs(variant, pairs, with_min_depth=True):
    """The pairs of a batch call or a PairSet as the C ABI takes them: (offs, X0, X1, D0, D1,
    MD, C0, C1) -- offs a list of len(pairs) + 1 offsets, the rest contiguous float64 arrays
    (MD None without min_depth).  pairs must not be empty."""
    ncam = 9 if variant in (L.CALIBRATED, L.SCALE_ONLY) else 2
    k0, k1 = ("K0", "K1") if ncam == 9 else ("pp0", "pp1")
    x0s, x1s, d0s, d1s, mds, c0s, c1s, offs = [], [], [], [], [], [], [], [0]
    for p in pairs:
        x0 = _pts(p["x0"], "x0")
        n = x0.shape[0]
        x1 = _pts(p["x1"], "x1")
        if x1.shape[0] != n:
            raise ValueError("x0 and x1 must have the same number of rows")
        x0s.append(x0.reshape(-1))
        x1s.append(x1.reshape(-1))
        d0s.append(_vec(p["depth0"], n, "depth0"))
        d1s.append(_vec(p["depth1"], n, "depth1"))
        if with_min_depth:
            mds.append(np.asarray(p.get("min_depth", (0.0, 0.0)), dtype=np.float64).reshape(2))
        c0s.append(np.asarray(p[k0], dtype=np.float64).reshape(ncam))
        c1s.append(np.asarray(p[k1], dtype=np.float64).reshape(ncam))
        offs.append(offs[-1] + n)
    cat = lambda xs: np.ascontiguousarray(np.concatenate(xs), dtype=np.float64)
    X0, X1, D0, D1, C0, C1 = (cat(v) for v in (x0s, x1s, d0s, d1s, c0s, c1s))
    MD = cat(mds) if with_min_depth else None
    if offs[-1] == 0:  # (no correspondence at all: the arrays still need an address)
        X0, X1, D0, D1 = np.zeros(2), np.zeros(2), np.zeros(1), np.zeros(1)
    return offs, X0, X1, D0, D1, MD, C0, C1


def _refine_results(variant, arr, res, idx, offs):
    """mp_refine_batch's / mp_refine_set's outputs as RefineResults (offs: the entries'
    offsets in idx)."""
    out = []
    for p in range(len(offs) - 1):
        n = offs[p + 1] - offs[p]
        r = RefineResult()
        r.model = _model_from_c(arr[p], variant)
        r.score_initial, r.score_final = float(res[p].score_initial), float(res[p].score_final)
        r.rounds_run, r.rounds_accepted = int(res[p].rounds_run), int(res[p].rounds_accepted)
        r.status = int(res[p].lm_status)
        base = 3 * offs[p]
        r.inlier_indices = [idx[base + t * n: base + t * n + res[p].num_inliers[t]].copy() for t in range(3)]
        r.norm_scale = float(res[p].norm_scale)
        out.append(r)
    return out


def _concat_candidates(variant, candidates):
    """select's candidates as the C ABI takes them: (moffs, arr, keep) -- moffs a list of
    len(candidates) + 1 offsets, arr the mp_model pointer or array, keep what must stay
    alive while arr is used."""
    moffs = [0]
    for cands in candidates:
        if isinstance(cands, np.ndarray):
            if cands.dtype != np.float64 or cands.ndim != 2 or cands.shape[1] != 17:
                raise ValueError(f"array candidates must be float64 of shape (K, 17), got {cands.dtype} {cands.shape}")
        moffs.append(moffs[-1] + len(cands))
    M = moffs[-1]
    if any(isinstance(cands, np.ndarray) for cands in candidates):
        # (rows copied as they are; objects through _model_to_c, the same bytes as below)
        rows = np.zeros((max(M, 1), 17))
        for p, cands in enumerate(candidates):
            if isinstance(cands, np.ndarray):
                rows[moffs[p]:moffs[p + 1]] = cands
            else:
                for j, m in enumerate(cands):
                    c_m = _model_to_c(m, variant)
                    ctypes.memmove(rows[moffs[p] + j].ctypes.data, ctypes.byref(c_m), ctypes.sizeof(c_m))
        return moffs, rows.ctypes.data_as(ctypes.POINTER(L.mp_model)), rows
    arr = (L.mp_model * max(M, 1))(*[_model_to_c(m, variant) for cands in candidates for m in cands])
    return moffs, arr, arr


def _select_results(variant, candidates, res, idx, offs, moffs, scores, counts):
    """mp_select_batch's / mp_select_set's outputs as SelectResults (scores, counts: the
    arrays or None)."""
    out = []
    for p in range(len(offs) - 1):
        n = offs[p + 1] - offs[p]
        r = SelectResult()
        r.index = int(res[p].best_index)
        if r.index >= 0 and isinstance(candidates[p], np.ndarray):
            r.model = _pose_from_row(candidates[p][r.index], variant)
        else:
            r.model = candidates[p][r.index] if r.index >= 0 else None
        r.score = float(res[p].best_score)
        base = 3 * offs[p]
        r.inlier_indices = [idx[base + t * n: base + t * n + res[p].num_inliers[t]].copy() for t in range(3)]
        r.norm_scale = float(res[p].norm_scale)
        if scores is not None:
            r.scores = scores[moffs[p]:moffs[p + 1]].copy()
        if counts is not None:
            r.counts = counts[3 * moffs[p]:3 * moffs[p + 1]].reshape(-1, 3).copy()
        out.append(r)
    return out


def _concat_samples(variant, sizes, samples):
    """hypothesize's samples as the C ABI takes them, checked: (soffs, T, I) -- sizes: the
    correspondences of each entry's pair."""
    stride = L.HYPOTHESIZE_SAMPLE_STRIDE
    ksz = (3 if variant == L.CALIBRATED else 4, (5, 6, 7)[variant])
    soffs, tys, ids = [0], [], []
    for p, (n, smp) in enumerate(zip(sizes, samples)):
        try:
            types, idx = smp
        except (TypeError, ValueError):
            raise ValueError(f"pair {p}: samples must hold one (types, idx) per pair") from None
        types, idx = np.asarray(types), np.asarray(idx)
        if types.dtype != np.int32 or idx.dtype != np.int32:
            raise ValueError(f"pair {p}: types and idx must be int32 arrays")
        K = types.shape[0] if types.ndim == 1 else -1
        if K < 0 or idx.shape != (K, stride):
            raise ValueError(f"pair {p}: types must have shape (K,) and idx (K, {stride}), got {types.shape} "
                             f"and {idx.shape}")
        if K:
            if ((types != 0) & (types != 1)).any():
                raise ValueError(f"pair {p}: a sample's type must be 0 (MD solver) or 1 (point solver)")
            for t in (0, 1):
                rows = idx[types == t][:, :ksz[t]]
                if rows.shape[0] == 0:
                    continue
                if n < ksz[t]:
                    raise ValueError(f"pair {p}: {n} correspondences are too few for a type-{t} sample")
                if (rows < 0).any() or (rows >= n).any():
                    raise ValueError(f"pair {p}: a sample index lies outside [0, {n})")
                srt = np.sort(rows, axis=1)
                if (srt[:, 1:] == srt[:, :-1]).any():
                    raise ValueError(f"pair {p}: a sample repeats an index")
        tys.append(types)
        ids.append(idx.reshape(-1))
        soffs.append(soffs[-1] + K)
    S = soffs[-1]
    if S > L.HYPOTHESIZE_MAX_SAMPLES:
        raise ValueError(f"at most 2^22 samples per call, got {S}")
    T = np.ascontiguousarray(np.concatenate(tys), dtype=np.int32) if S else np.zeros(1, dtype=np.int32)
    I = np.ascontiguousarray(np.concatenate(ids), dtype=np.int32) if S else np.zeros(stride, dtype=np.int32)
    return soffs, T, I


class RefineResult:
    """One pair's outcome of refine_batch."""

    def __init__(self):
        self.model = None
        self.score_initial = 0.0
        self.score_final = 0.0
        self.rounds_run = 0
        self.rounds_accepted = 0
        self.status = -1
        self.inlier_indices = [np.zeros(0, dtype=np.int32) for _ in range(3)]
        self.norm_scale = 1.0

    def __repr__(self):
        return (f"RefineResult(score {self.score_initial:.6g} -> {self.score_final:.6g}, rounds "
                f"{self.rounds_accepted}/{self.rounds_run}, status={self.status}, "
                f"inliers={[len(a) for a in self.inlier_indices]})")


def refine_batch(variant, pairs, models, options, est_config=None, rounds=1, chunk=0, device=None):
    """Refine given poses over many pairs on the device (mp_refine_batch).

    pairs: estimate_batch's dicts; models: one pose object per pair, as the estimators
    return them (user units).  Per pair and round: the inliers of the model under the
    estimator's thresholds, the LeastSquares fit over all of them (device LM), and the
    result kept when it scores strictly lower; a pair stops at its first round that is
    not accepted (LeastSquaresFit with all inliers and the final least squares' rule,
    src/hybrid_ransac.h:406, 484-510, 186-203).  All pairs of a run of `chunk` pairs (0:
    a default bound on the run's correspondences) are resident at once, one sweep launch
    and one LM launch per round.  Returns one RefineResult per pair: model, score_initial,
    score_final, rounds_run, rounds_accepted, status (of the last LM: 1 refined, 0 no
    residuals, 2 infeasible constant block, 3 too few inliers), inlier_indices (three
    int32 arrays, the returned model's) and norm_scale."""
    if len(models) != len(pairs):
        raise ValueError(f"one model per pair: {len(models)} models for {len(pairs)} pairs")
    if variant not in (L.CALIBRATED, L.SHARED_FOCAL, L.TWO_FOCAL, L.SCALE_ONLY):
        raise ValueError("variant must be 0 (calibrated), 1 (shared focal), 2 (two focal) or 3 (scale only)")
    if int(rounds) != rounds or not 1 <= rounds <= 64:
        raise ValueError("rounds must be an integer in 1..64")
    if int(chunk) != chunk or chunk < 0:
        raise ValueError("chunk must be a non-negative integer (0: the default)")
    if est_config is None:
        est_config = EstimatorConfig()
    o = options._to_c()
    c = est_config._to_c()
    P = len(pairs)
    if P == 0:
        return []
    offs, X0, X1, D0, D1, MD, C0, C1 = _concat_pairs(variant, pairs)
    offsets = np.asarray(offs, dtype=np.int64)
    arr = (L.mp_model * P)(*[_model_to_c(m, variant) for m in models])
    res = (L.mp_refine_result * P)()
    idx = np.zeros(3 * max(offs[-1], 1), dtype=np.int32)
    L.check(L.lib().mp_refine_batch(variant, P, offsets.ctypes.data_as(L.c_int64_p), _dp(X0), _dp(X1), _dp(D0),
                                    _dp(D1), _dp(MD), _dp(C0), _dp(C1), ctypes.byref(o), ctypes.byref(c),
                                    int(rounds), arr, res, idx.ctypes.data_as(L.c_int32_p), int(chunk),
                                    _DEFAULT_DEVICE if device is None else int(device)))
    return _refine_results(variant, arr, res, idx, offs)


class SelectResult:
    """One pair's outcome of select_batch."""

    def __init__(self):
        self.index = -1
        self.model = None
        self.score = float(np.finfo(np.float64).max)
        self.inlier_indices = [np.zeros(0, dtype=np.int32) for _ in range(3)]
        self.norm_scale = 1.0
        self.scores = None
        self.counts = None

    def __repr__(self):
        return (f"SelectResult(index={self.index}, score={self.score:.6g}, "
                f"inliers={[len(a) for a in self.inlier_indices]})")


def select_batch(variant, pairs, candidates, options, est_config=None, with_scores=False, with_counts=False,
                 chunk=0, model_chunk=0, device=None):
    """Rank candidate poses over many pairs on the device (mp_select_batch).

    pairs: estimate_batch's dicts; candidates: per pair one sequence of pose objects, as
    the estimators return them (user units), or one float64 array of shape (K, 17), a model
    per row in mp_model field order as hypothesize_batch and solve_scale_shift_pose_batch
    return them; either may be empty.  Every candidate gets
    the estimators' MSAC score (score_models' value for it, bit for bit) and the three
    counts of errors below the thresholds; per pair the first candidate with the lowest
    score wins (the reference's GetBestEstimatedModelId: strict <, a NaN or infinite score
    never wins).  All pairs of a run of `chunk` pairs (0: refine_batch's default bound) are
    resident at once; the score records of `model_chunk` candidates (0: the default) are on
    the device at a time; results depend on neither.  Returns one SelectResult per pair:
    index (-1: no winner), model (the chosen candidate object itself -- for an array entry
    the winning row as a pose object, poses_from_models' -- or None), score
    (DBL_MAX without a winner), inlier_indices (three int32 arrays, the winner's, as
    refine_batch would form them), norm_scale, scores (float64, one per candidate, with
    with_scores, else None) and counts (int32 K x 3, with with_counts, else None)."""
    if len(candidates) != len(pairs):
        raise ValueError(f"one candidate list per pair: {len(candidates)} lists for {len(pairs)} pairs")
    if variant not in (L.CALIBRATED, L.SHARED_FOCAL, L.TWO_FOCAL, L.SCALE_ONLY):
        raise ValueError("variant must be 0 (calibrated), 1 (shared focal), 2 (two focal) or 3 (scale only)")
    for name, val in (("chunk", chunk), ("model_chunk", model_chunk)):
        if isinstance(val, bool) or not isinstance(val, (int, np.integer, float)) or int(val) != val or val < 0:
            raise ValueError(f"{name} must be a non-negative integer (0: the default)")
    if est_config is None:
        est_config = EstimatorConfig()
    o = options._to_c()
    c = est_config._to_c()
    P = len(pairs)
    if P == 0:
        return []
    offs, X0, X1, D0, D1, _, C0, C1 = _concat_pairs(variant, pairs, with_min_depth=False)
    moffs, arr, _keep = _concat_candidates(variant, candidates)
    offsets = np.asarray(offs, dtype=np.int64)
    model_offsets = np.asarray(moffs, dtype=np.int64)
    M = moffs[-1]
    res = (L.mp_select_result * P)()
    idx = np.zeros(3 * max(offs[-1], 1), dtype=np.int32)
    scores = np.zeros(max(M, 1), dtype=np.float64) if with_scores else None
    counts = np.zeros(3 * max(M, 1), dtype=np.int32) if with_counts else None
    L.check(L.lib().mp_select_batch(variant, P, offsets.ctypes.data_as(L.c_int64_p), _dp(X0), _dp(X1), _dp(D0),
                                    _dp(D1), _dp(C0), _dp(C1), ctypes.byref(o), ctypes.byref(c),
                                    model_offsets.ctypes.data_as(L.c_int64_p), arr,
                                    None if scores is None else _dp(scores),
                                    None if counts is None else counts.ctypes.data_as(L.c_int32_p), res,
                                    idx.ctypes.data_as(L.c_int32_p), int(chunk), int(model_chunk),
                                    _DEFAULT_DEVICE if device is None else int(device)))
    return _select_results(variant, candidates, res, idx, offs, moffs, scores, counts)


def lm_refine_batch(variant, x0, x1, depth0, depth1, min_depth, cam0, cam1, options, est_config, problems,
                    device=None, on_host=False):
    """Batched device LM (the LO's Ceres solves, src/optimizer.h:48-125 over
    src/cost_functions.h): problems is a list of (kind, (idx0, idx1, idx2), model) with
    kind 0 = LeastSquares, 1 = NonMinimalSolver, idx* the residual blocks of the three
    data types and model a PoseScaleOffset* in problem units (SF/TF focals divided by
    the pair's normalize_points scale).  One device workgroup per problem.  Returns a
    list of (model, status): 1 refined, 0 no residuals, 2 infeasible constant block,
    3 too few data (unchanged)."""
    if est_config is None:
        est_config = EstimatorConfig()
    x0 = _pts(x0, "x0")
    n = x0.shape[0]
    x1 = _pts(x1, "x1")
    d0, d1 = _vec(depth0, n, "depth0"), _vec(depth1, n, "depth1")
    md = np.asarray(min_depth, dtype=np.float64).reshape(2)
    k = 9 if variant in (L.CALIBRATED, L.SCALE_ONLY) else 2
    c0 = np.ascontiguousarray(np.asarray(cam0, dtype=np.float64).reshape(k))
    c1 = np.ascontiguousarray(np.asarray(cam1, dtype=np.float64).reshape(k))
    P = len(problems)
    kinds = np.array([int(p[0]) for p in problems] or [0], dtype=np.int32)
    offs, idx = [0], []
    for _, lists, _m in problems:
        for t in range(3):
            a = np.asarray(lists[t], dtype=np.int32).reshape(-1)
            idx.append(a)
            offs.append(offs[-1] + len(a))
    offs = np.asarray(offs, dtype=np.int64)
    idx = np.ascontiguousarray(np.concatenate(idx) if idx and offs[-1] > 0 else np.zeros(1, dtype=np.int32))
    models = (L.mp_model * max(P, 1))()
    for j, (_, _, m) in enumerate(problems):
        models[j] = _model_to_c(m, variant)
    status = np.zeros(max(P, 1), dtype=np.int32)
    o = options._to_c()
    c = est_config._to_c()
    common = (variant, n, _dp(x0), _dp(x1), _dp(d0), _dp(d1), _dp(md), _dp(c0), _dp(c1), ctypes.byref(o),
              ctypes.byref(c), P, kinds.ctypes.data_as(L.c_int32_p), offs.ctypes.data_as(L.c_int64_p),
              idx.ctypes.data_as(L.c_int32_p), models, status.ctypes.data_as(L.c_int32_p))
    if on_host:  # test hook: the engine's host LM (the default LO path) on the same problems
        L.check(L.lib().mp_debug_lm_refine_host(*common))
    else:
        L.check(L.lib().mp_lm_refine_batch(*common, _DEFAULT_DEVICE if device is None else int(device)))
    return [(_model_from_c(models[j], variant), int(status[j])) for j in range(P)]


def lm_system(variant, x0, x1, depth0, depth1, min_depth, cam0, cam1, options, est_config, problems, radius,
              where=0, block_ranges=None, device=None):
    """One evaluation and one step of lm_refine_batch's problems at their start models -- test
    hook (mp_debug_lm_system).  radius: one trust-region radius, or one per problem; where: 0
    the device, 1 / 2 the host's 4- / 8-wide residual evaluation (block_ranges: optional
    (b0, b1) per problem over the concatenated block list), 3 the host LM's evaluate().
    Returns a dict of arrays over the problems in the full 11-parameter layout: cost (P), g
    (P, 11), H (P, 66: packed upper triangle), col (P, 11), d (P, 11), pd (P: 1 positive
    definite, 0 not, -1 nothing evaluated) and status (P)."""
    if est_config is None:
        est_config = EstimatorConfig()
    x0 = _pts(x0, "x0")
    n = x0.shape[0]
    x1 = _pts(x1, "x1")
    d0, d1 = _vec(depth0, n, "depth0"), _vec(depth1, n, "depth1")
    md = np.asarray(min_depth, dtype=np.float64).reshape(2)
    k = 9 if variant in (L.CALIBRATED, L.SCALE_ONLY) else 2
    c0 = np.ascontiguousarray(np.asarray(cam0, dtype=np.float64).reshape(k))
    c1 = np.ascontiguousarray(np.asarray(cam1, dtype=np.float64).reshape(k))
    P = len(problems)
    kinds = np.array([int(p[0]) for p in problems] or [0], dtype=np.int32)
    offs, idx = [0], []
    for _, lists, _m in problems:
        for t in range(3):
            a = np.asarray(lists[t], dtype=np.int32).reshape(-1)
            idx.append(a)
            offs.append(offs[-1] + len(a))
    offs = np.asarray(offs, dtype=np.int64)
    idx = np.ascontiguousarray(np.concatenate(idx) if idx and offs[-1] > 0 else np.zeros(1, dtype=np.int32))
    models = (L.mp_model * max(P, 1))()
    for j, (_, _, m) in enumerate(problems):
        models[j] = _model_to_c(m, variant)
    rad = np.ascontiguousarray(np.broadcast_to(np.asarray(radius, dtype=np.float64), (max(P, 1),)))
    rng = None
    if block_ranges is not None:
        rng = np.ascontiguousarray(np.asarray(block_ranges, dtype=np.int64).reshape(max(P, 1), 2))
    out = dict(cost=np.zeros(max(P, 1)), g=np.zeros((max(P, 1), 11)), H=np.zeros((max(P, 1), 66)),
               col=np.zeros((max(P, 1), 11), dtype=np.int32), d=np.zeros((max(P, 1), 11)),
               pd=np.zeros(max(P, 1), dtype=np.int32), status=np.zeros(max(P, 1), dtype=np.int32))
    o = options._to_c()
    c = est_config._to_c()
    i32 = lambda a: a.ctypes.data_as(L.c_int32_p)
    L.check(L.lib().mp_debug_lm_system(
        variant, n, _dp(x0), _dp(x1), _dp(d0), _dp(d1), _dp(md), _dp(c0), _dp(c1), ctypes.byref(o), ctypes.byref(c), P,
        i32(kinds), offs.ctypes.data_as(L.c_int64_p), i32(idx), models, _dp(rad), int(where),
        None if rng is None else rng.ctypes.data_as(L.c_int64_p), _dp(out["cost"]), _dp(out["g"]), _dp(out["H"]),
        i32(out["col"]), _dp(out["d"]), i32(out["pd"]), i32(out["status"]),
        _DEFAULT_DEVICE if device is None else int(device)))
    return {k: v[:P] for k, v in out.items()}


def bougnoux_focals_batch(F, device=None):
    """Squared Bougnoux focal lengths (f0^2, f1^2) of fundamental matrices F (k x 3 x 3,
    principal points at the origin) on the device: the two-focal 7-point tail's own
    code (src/hybrid_pose_two_focal_estimator.cpp:11-32; madpose/utils.py:25-56)."""
    F = np.ascontiguousarray(np.asarray(F, dtype=np.float64).reshape(-1, 9))
    out = np.zeros((len(F), 2))
    L.check(L.lib().mp_bougnoux_focals(len(F), _dp(F), _dp(out), _DEFAULT_DEVICE if device is None else int(device)))
    return out


def pose_eval_batch(T_0to1, R, t, thresholds=(5, 10, 20), t_thres=None, device=None):
    """compute_pose_error (madpose/utils.py:59-78) of k estimated poses and the pose
    AUC of max(err_R, err_t) at each threshold (degrees), in two device launches
    (SURVEY.md §8(f)4).  T_0to1: k x 4 x 4 ground truths; R: k x 3 x 3; t: k x 3.
    Returns (err_t, err_R, aucs): the per-pair errors as madpose.utils computes them
    and the AUCs of madpose_amd.utils.pose_auc (NaN errors count as misses)."""
    T = np.ascontiguousarray(np.asarray(T_0to1, dtype=np.float64).reshape(-1, 16))
    Rm = np.ascontiguousarray(np.asarray(R, dtype=np.float64).reshape(-1, 9))
    tv = np.ascontiguousarray(np.asarray(t, dtype=np.float64).reshape(-1, 3))
    if not (len(T) == len(Rm) == len(tv)):
        raise ValueError("T_0to1, R and t must hold the same number of poses")
    thr = np.ascontiguousarray(np.asarray(thresholds, dtype=np.float64).reshape(-1))
    if np.any(~(thr > 0)):
        raise ValueError("AUC thresholds must be positive")
    k = len(T)
    et, eR, aucs = np.zeros(max(k, 1)), np.zeros(max(k, 1)), np.zeros(max(len(thr), 1))
    L.check(L.lib().mp_pose_eval(k, _dp(Rm), _dp(tv), _dp(T), -1.0 if t_thres is None else float(t_thres), _dp(et),
                                 _dp(eR), len(thr), _dp(thr), _dp(aucs),
                                 _DEFAULT_DEVICE if device is None else int(device)))
    return et[:k].copy(), eR[:k].copy(), [float(a) for a in aucs[:len(thr)]]


def pose_auc_batch(errors, thresholds=(5, 10, 20), device=None):
    """Pose AUC of given per-pair errors (degrees) at each threshold on the device: the
    evaluator of pose_eval_batch for errors gathered elsewhere (e.g. from all ranks)."""
    e = np.ascontiguousarray(np.asarray(errors, dtype=np.float64).reshape(-1))
    thr = np.ascontiguousarray(np.asarray(thresholds, dtype=np.float64).reshape(-1))
    if np.any(~(thr > 0)):
        raise ValueError("AUC thresholds must be positive")
    aucs = np.zeros(max(len(thr), 1))
    L.check(L.lib().mp_pose_auc(len(e), _dp(e if len(e) else np.zeros(1)), len(thr), _dp(thr), _dp(aucs),
                                _DEFAULT_DEVICE if device is None else int(device)))
    return [float(a) for a in aucs[:len(thr)]]


def get_depths_batch(images, depth_maps, mkpts, device=None):
    """madpose.utils.get_depths (madpose/utils.py:4-22) for many pairs in one device
    launch.  images: the images (only their shapes are used) or (h, w) tuples;
    depth_maps: 2-D float32 or float64 arrays (one dtype for the batch); mkpts: n_p x 2
    keypoints per map.  Returns one array of depths per map (the maps' dtype),
    bit-identical to the numpy reference."""
    if not (len(images) == len(depth_maps) == len(mkpts)):
        raise ValueError("images, depth_maps and mkpts must have the same length")
    P = len(depth_maps)
    if P == 0:
        return []
    dt = np.result_type(*[np.asarray(d).dtype for d in depth_maps])
    if dt not in (np.float32, np.float64):
        dt = np.dtype(np.float64)
    maps, dims, pts, offs = [], [], [], [0]
    for img, dm, kp in zip(images, depth_maps, mkpts):
        dm = np.asarray(dm)
        if dm.ndim != 2:
            raise ValueError("depth maps must be 2-D")
        ih, iw = (img if isinstance(img, tuple) else np.shape(img))[:2]
        kp = np.ascontiguousarray(kp, dtype=np.float64).reshape(-1, 2)
        maps.append(np.ascontiguousarray(dm, dtype=dt).reshape(-1))
        dims.append([dm.shape[0], dm.shape[1], ih, iw])
        pts.append(kp)
        offs.append(offs[-1] + len(kp))
    M = np.ascontiguousarray(np.concatenate(maps))
    D = np.ascontiguousarray(np.asarray(dims, dtype=np.int64).reshape(-1))
    O = np.asarray(offs, dtype=np.int64)
    X = np.ascontiguousarray(np.concatenate(pts).reshape(-1)) if offs[-1] else np.zeros(2)
    out = np.zeros(max(offs[-1], 1), dtype=dt)
    L.check(L.lib().mp_get_depths(0 if dt == np.float32 else 1, P, M.ctypes.data_as(ctypes.c_void_p),
                                  D.ctypes.data_as(L.c_int64_p), O.ctypes.data_as(L.c_int64_p), _dp(X),
                                  out.ctypes.data_as(ctypes.c_void_p),
                                  _DEFAULT_DEVICE if device is None else int(device)))
    return [out[offs[p]:offs[p + 1]].copy() for p in range(P)]


# ---------------------------------------------------------------------------
# standalone solver bindings (src/bindings.cpp:156-166)
def _homog_pm(a, k, name):
    a = np.asarray(a, dtype=np.float64)
    if a.shape == (3, k):
        return np.ascontiguousarray(a.T)
    raise ValueError(f"{name} must be a 3 x {k} matrix of homogeneous points (columns)")


def _solve_ss(variant, x_homo, y_homo, depth_x, depth_y):
    k = 3 if variant == L.CALIBRATED else 4
    x = _homog_pm(x_homo, k, "x_homo")
    y = _homog_pm(y_homo, k, "y_homo")
    dx = _vec(depth_x, k, "depth_x")
    dy = _vec(depth_y, k, "depth_y")
    w = [4, 5, 6][variant]
    out = np.zeros(8 * w)
    n = L.lib().mp_solve_scale_and_shift(variant, _dp(x), _dp(y), _dp(dx), _dp(dy), _dp(out), 8, _DEFAULT_DEVICE)
    if n < 0:
        L.check(-n)
    return [out[i * w:(i + 1) * w].copy() for i in range(n)]


def _solve_pose(variant, x_homo, y_homo, depth_x, depth_y, alt=0):
    k = 3 if variant == L.CALIBRATED else 4
    x = _homog_pm(x_homo, k, "x_homo")
    y = _homog_pm(y_homo, k, "y_homo")
    dx = _vec(depth_x, k, "depth_x")
    dy = _vec(depth_y, k, "depth_y")
    out = (L.mp_model * 8)()
    if alt:
        n = L.lib().mp_solve_scale_shift_pose_alt(variant, alt, _dp(x), _dp(y), _dp(dx), _dp(dy), out, 8,
                                                  _DEFAULT_DEVICE)
    else:
        n = L.lib().mp_solve_scale_shift_pose(variant, _dp(x), _dp(y), _dp(dx), _dp(dy), out, 8, _DEFAULT_DEVICE)
    if n < 0:
        L.check(-n)
    return [_model_from_c(out[i], variant) for i in range(n)]


def solve_scale_and_shift(x_homo, y_homo, depth_x, depth_y):
    """src/solver.cpp:35-125: list of (1, b1, a2, b2*a2)."""
    return _solve_ss(L.CALIBRATED, x_homo, y_homo, depth_x, depth_y)


def solve_scale_and_shift_shared_focal(x_homo, y_homo, depth_x, depth_y):
    """src/solver.cpp:127-293: list of (1, b1, a2, b2*a2, f)."""
    return _solve_ss(L.SHARED_FOCAL, x_homo, y_homo, depth_x, depth_y)


def solve_scale_and_shift_two_focal(x_homo, y_homo, depth_x, depth_y):
    """src/solver.cpp:295-480: list of (1, b1, a2, b2*a2, f1, f2)."""
    return _solve_ss(L.TWO_FOCAL, x_homo, y_homo, depth_x, depth_y)


def solve_scale_shift_pose(x_homo, y_homo, depth_x, depth_y):
    """src/solver.cpp:482-534 (wrapper :1408-1415)."""
    return _solve_pose(L.CALIBRATED, x_homo, y_homo, depth_x, depth_y)


def solve_scale_shift_pose_shared_focal(x_homo, y_homo, depth_x, depth_y):
    """src/solver.cpp:682-739 (wrapper :1417-1424)."""
    return _solve_pose(L.SHARED_FOCAL, x_homo, y_homo, depth_x, depth_y)


def solve_scale_shift_pose_two_focal(x_homo, y_homo, depth_x, depth_y):
    """src/solver.cpp:986-1043 (wrapper :1426-1433)."""
    return _solve_pose(L.TWO_FOCAL, x_homo, y_homo, depth_x, depth_y)


def relpose_5pt(x1, x2):
    """Device 5-point solver on unit bearings (5 x 3 each): list of PoseScaleOffset (scale 1)."""
    b1 = np.ascontiguousarray(np.asarray(x1, dtype=np.float64).reshape(5, 3))
    b2 = np.ascontiguousarray(np.asarray(x2, dtype=np.float64).reshape(5, 3))
    out = (L.mp_model * 16)()
    n = L.lib().mp_relpose_5pt(_dp(b1), _dp(b2), out, 16, _DEFAULT_DEVICE)
    if n < 0:
        L.check(-n)
    return [_model_from_c(out[i], L.CALIBRATED) for i in range(min(n, 16))]


def _point_direct(fn, k, variant, x0, x1):
    a = np.ascontiguousarray(np.asarray(x0, dtype=np.float64).reshape(k, 2))
    b = np.ascontiguousarray(np.asarray(x1, dtype=np.float64).reshape(k, 2))
    out = (L.mp_model * 16)()
    n = fn(_dp(a), _dp(b), out, 16, _DEFAULT_DEVICE)
    if n < 0:
        L.check(-n)
    return [_model_from_c(out[i], variant) for i in range(min(n, 16))]


def relpose_6pt_shared_focal(x0, x1):
    """Device shared-focal 6-point solver on normalized 2-D points (6 x 2 each):
    PoseScaleOffsetSharedFocal candidates before the depth fit."""
    return _point_direct(L.lib().mp_relpose_6pt_shared_focal, 6, L.SHARED_FOCAL, x0, x1)


def relpose_7pt_two_focal(x0, x1):
    """Device 7-point + Bougnoux + recoverPose on normalized 2-D points (7 x 2 each):
    PoseScaleOffsetTwoFocal candidates before the depth fit."""
    return _point_direct(L.lib().mp_relpose_7pt_two_focal, 7, L.TWO_FOCAL, x0, x1)


def solve_scale_shift_pose_ours(x_homo, y_homo, depth_x, depth_y):
    """src/solver.cpp:623-680 (the use_ours calibrated MD solver)."""
    return _solve_pose(L.CALIBRATED, x_homo, y_homo, depth_x, depth_y, alt=1)


def solve_scale_shift_pose_shared_focal_ours(x_homo, y_homo, depth_x, depth_y):
    """src/solver.cpp:818-984 (the use_ours shared-focal MD solver)."""
    return _solve_pose(L.SHARED_FOCAL, x_homo, y_homo, depth_x, depth_y, alt=1)


def solve_scale_shift_pose_two_focal_ours(x_homo, y_homo, depth_x, depth_y):
    """src/solver.cpp:1045-1148 (the use_ours two-focal MD solver)."""
    return _solve_pose(L.TWO_FOCAL, x_homo, y_homo, depth_x, depth_y, alt=1)


def solve_scale_shift_pose_two_focal_4p4d(x_homo, y_homo, depth_x, depth_y):
    """src/solver.cpp:1287-1406 (the use_4p4d two-focal solver)."""
    return _solve_pose(L.TWO_FOCAL, x_homo, y_homo, depth_x, depth_y, alt=2)


# ---------------------------------------------------------------------------
# the standalone solvers over many samples per call (mp_*_batch)
def _batch_array(a, tail, name):
    """a as a float64 array of shape (B,) + tail (no copy yet: B is checked first)"""
    a = np.asarray(a, dtype=np.float64)
    if a.ndim != 1 + len(tail) or tuple(a.shape[1:]) != tuple(tail):
        raise ValueError(f"{name} must have shape (B, {', '.join(str(t) for t in tail)}), got {a.shape}")
    return a


def _batch_common(arrays, chunk):
    B = arrays[0].shape[0]
    if any(a.shape[0] != B for a in arrays):
        raise ValueError("the arrays must hold the same number of samples")
    if B > L.SOLVE_BATCH_MAX:
        raise ValueError(f"at most 2^22 samples per call, got {B}")
    if int(chunk) != chunk or chunk < 0:
        raise ValueError("chunk must be a non-negative integer (0: the default)")
    return B


def _md_batch_inputs(variant, x_homo, y_homo, depth_x, depth_y, chunk):
    if variant not in (L.CALIBRATED, L.SHARED_FOCAL, L.TWO_FOCAL):
        raise ValueError("variant must be 0 (calibrated), 1 (shared focal) or 2 (two focal)")
    k = 3 if variant == L.CALIBRATED else 4
    arrs = [_batch_array(x_homo, (k, 3), "x_homo"), _batch_array(y_homo, (k, 3), "y_homo"),
            _batch_array(depth_x, (k,), "depth_x"), _batch_array(depth_y, (k,), "depth_y")]
    B = _batch_common(arrs, chunk)
    return B, [np.ascontiguousarray(a) for a in arrs] if B else arrs


def solve_scale_and_shift_batch(variant, x_homo, y_homo, depth_x, depth_y, chunk=0, device=None):
    """solve_scale_and_shift{,_shared_focal,_two_focal} (variant 0 / 1 / 2) over B samples
    in device launches that fill the GPU.  x_homo, y_homo: (B, K, 3) homogeneous points, one
    per row (K = 3 calibrated, 4 otherwise); depth_x, depth_y: (B, K).  Returns (sols, counts):
    sols (B, 8, w) with w = 4 / 5 / 6, rows in the single-sample function's order, rows from
    counts[b] on zero.  Every row equals the single-sample result bit for bit.  chunk:
    samples per launch round (bounds device memory; 0 = the default)."""
    B, (x, y, dx, dy) = _md_batch_inputs(variant, x_homo, y_homo, depth_x, depth_y, chunk)
    w = [4, 5, 6][variant]
    sols = np.zeros((B, 8, w))
    counts = np.zeros(B, dtype=np.int32)
    if B:
        L.check(L.lib().mp_solve_scale_and_shift_batch(variant, B, _dp(x), _dp(y), _dp(dx), _dp(dy), _dp(sols),
                                                       counts.ctypes.data_as(L.c_int32_p), int(chunk),
                                                       _DEFAULT_DEVICE if device is None else int(device)))
    return sols, counts


def solve_scale_shift_pose_batch(variant, x_homo, y_homo, depth_x, depth_y, alt=0, chunk=0, device=None):
    """solve_scale_shift_pose{,_shared_focal,_two_focal} over B samples (inputs as
    solve_scale_and_shift_batch); alt 1: the _ours solvers, alt 2: _two_focal_4p4d (variant
    2 only).  Returns (models, counts): models (B, 8, 17) float64 in mp_model field order
    (R 9, t 3, scale, offset0, offset1, focal0, focal1; poses_from_models converts a
    sample's rows), slots from counts[b] on zero; bit-identical to the single-sample calls."""
    if alt not in (0, 1, 2) or (alt == 2 and variant != L.TWO_FOCAL):
        raise ValueError("alt must be 0, 1 (use_ours) or 2 (use_4p4d, two-focal only)")
    B, (x, y, dx, dy) = _md_batch_inputs(variant, x_homo, y_homo, depth_x, depth_y, chunk)
    models = np.zeros((B, 8, 17))
    counts = np.zeros(B, dtype=np.int32)
    if B:
        L.check(L.lib().mp_solve_scale_shift_pose_batch(variant, int(alt), B, _dp(x), _dp(y), _dp(dx), _dp(dy),
                                                        models.ctypes.data_as(ctypes.POINTER(L.mp_model)),
                                                        counts.ctypes.data_as(L.c_int32_p), int(chunk),
                                                        _DEFAULT_DEVICE if device is None else int(device)))
    return models, counts


def relpose_batch(kind, x0, x1, chunk=0, device=None):
    """relpose_5pt (kind 0; x0, x1: (B, 5, 3) unit bearings), relpose_6pt_shared_focal (1;
    (B, 6, 2) normalized points) or relpose_7pt_two_focal (2; (B, 7, 2)) over B samples.
    Returns (models, counts): models (B, 16, 17) as solve_scale_shift_pose_batch returns
    them, bit-identical to the single-sample calls."""
    if kind not in (0, 1, 2):
        raise ValueError("kind must be 0 (5pt), 1 (6pt shared focal) or 2 (7pt two focal)")
    tail = [(5, 3), (6, 2), (7, 2)][kind]
    arrs = [_batch_array(x0, tail, "x0"), _batch_array(x1, tail, "x1")]
    B = _batch_common(arrs, chunk)
    models = np.zeros((B, 16, 17))
    counts = np.zeros(B, dtype=np.int32)
    if B:
        a, b = (np.ascontiguousarray(v) for v in arrs)
        L.check(L.lib().mp_relpose_batch(kind, B, _dp(a), _dp(b), models.ctypes.data_as(ctypes.POINTER(L.mp_model)),
                                         counts.ctypes.data_as(L.c_int32_p), int(chunk),
                                         _DEFAULT_DEVICE if device is None else int(device)))
    return models, counts


def _pose_from_row(row, variant):
    m = L.mp_model()
    row = np.ascontiguousarray(row, dtype=np.float64)
    ctypes.memmove(ctypes.byref(m), row.ctypes.data, ctypes.sizeof(m))
    return _model_from_c(m, variant)


def poses_from_models(models_rows, variant):
    """The rows of one sample's models (n x 17, e.g. models[b, :counts[b]]) as the pose
    objects the single-sample functions return (variant 0 / 1 / 2: PoseScaleOffset /
    ...SharedFocal / ...TwoFocal)."""
    if variant not in (L.CALIBRATED, L.SHARED_FOCAL, L.TWO_FOCAL):
        raise ValueError("variant must be 0 (calibrated), 1 (shared focal) or 2 (two focal)")
    rows = np.ascontiguousarray(np.asarray(models_rows, dtype=np.float64))
    if rows.ndim != 2 or rows.shape[1] != 17:
        raise ValueError(f"models_rows must have shape (n, 17), got {rows.shape}")
    return [_pose_from_row(row, variant) for row in rows]


def hypothesize_batch(variant, pairs, samples, options, est_config=None, chunk=0, sample_chunk=0, device=None):
    """The estimators' sample models over many pairs (mp_hypothesize_batch).

    pairs: estimate_batch's dicts; samples: one (types, idx) per pair -- types int32 of
    shape (K_p,), 0 the MD solver, 1 the point solver; idx int32 of shape (K_p, 8), indices
    into the pair's correspondences, of which a type-0 sample reads the first 3
    (calibrated) or 4 and a type-1 sample the first 5 / 6 / 7 (the other slots are
    ignored); K_p may be 0.  For every sample: exactly the models the estimator's
    MinimalSolver stage forms for that pair, options, config, solver type and sample, in
    its order and bit for bit, in user units.  Supported: variants 0 / 1 / 2 with
    use_shift on and without use_ours / use_4p4d.  All pairs of a run of `chunk` pairs (0:
    refine_batch's default bound) are resident at once, `sample_chunk` samples (0: the
    default) are on the device at a time; results depend on neither.  Returns (results,
    norm_scale): results holds one (models, counts) per pair, models float64 of shape
    (K_p, slots, 17) in mp_model field order (slots 10 / 16 / 4; rows from counts[k] on are
    zero; models[k, :counts[k]] are select_batch's array candidates once flattened),
    counts int32 of shape (K_p,); norm_scale float64, one per pair."""
    if variant not in (L.CALIBRATED, L.SHARED_FOCAL, L.TWO_FOCAL):
        raise ValueError("variant must be 0 (calibrated), 1 (shared focal) or 2 (two focal); "
                         "scale only is not supported")
    if len(samples) != len(pairs):
        raise ValueError(f"one (types, idx) per pair: {len(samples)} entries for {len(pairs)} pairs")
    for name, val in (("chunk", chunk), ("sample_chunk", sample_chunk)):
        if isinstance(val, bool) or not isinstance(val, (int, np.integer, float)) or int(val) != val or val < 0:
            raise ValueError(f"{name} must be a non-negative integer (0: the default)")
    if est_config is None:
        est_config = EstimatorConfig()
    if not est_config.use_shift:
        raise ValueError("hypothesize_batch does not support use_shift = False")
    if getattr(options, "use_ours", False) or getattr(options, "use_4p4d", False):
        raise ValueError("hypothesize_batch does not support the alternate MD solvers (use_ours / use_4p4d)")
    o = options._to_c()
    c = est_config._to_c()
    P = len(pairs)
    if P == 0:
        return [], np.zeros(0)
    slots = L.HYPOTHESIZE_SLOTS[variant]
    offs, X0, X1, D0, D1, MD, C0, C1 = _concat_pairs(variant, pairs)
    soffs, T, I = _concat_samples(variant, [offs[p + 1] - offs[p] for p in range(P)], samples)
    S = soffs[-1]
    offsets = np.asarray(offs, dtype=np.int64)
    sample_offsets = np.asarray(soffs, dtype=np.int64)
    models = np.zeros((max(S, 1), slots, 17))
    counts = np.zeros(max(S, 1), dtype=np.int32)
    norm = np.ones(P)
    L.check(L.lib().mp_hypothesize_batch(variant, P, offsets.ctypes.data_as(L.c_int64_p), _dp(X0), _dp(X1), _dp(D0),
                                         _dp(D1), _dp(MD), _dp(C0), _dp(C1), ctypes.byref(o), ctypes.byref(c),
                                         sample_offsets.ctypes.data_as(L.c_int64_p), T.ctypes.data_as(L.c_int32_p),
                                         I.ctypes.data_as(L.c_int32_p),
                                         models.ctypes.data_as(ctypes.POINTER(L.mp_model)),
                                         counts.ctypes.data_as(L.c_int32_p), _dp(norm), int(chunk), int(sample_chunk),
                                         _DEFAULT_DEVICE if device is None else int(device)))
    out = [(models[soffs[p]:soffs[p + 1]].copy(), counts[soffs[p]:soffs[p + 1]].copy()) for p in range(P)]
    return out, norm


def _device_array(a, name, shape):
    """(address, element-type code 0 float32 / 1 float64, shape) of a device array given through
    __cuda_array_interface__, checked: C-contiguous, of the given shape (None: any 2-D shape
    with positive sides).  ValueError otherwise; the object is only inspected."""
    try:
        cai = a.__cuda_array_interface__
    except Exception as e:
        raise ValueError(f"{name} must be a device array (an object with __cuda_array_interface__): {e}") from None
    typestr = cai.get("typestr")
    code = {"<f4": 0, "=f4": 0, "<f8": 1, "=f8": 1}.get(typestr)
    if code is None:
        raise ValueError(f"{name} must be float32 or float64, got {typestr!r}")
    shp = tuple(int(s) for s in cai.get("shape", ()))
    if shape is None:
        if len(shp) != 2 or shp[0] <= 0 or shp[1] <= 0:
            raise ValueError(f"{name} must be a 2-D (h, w) map with positive sides, got shape {shp}")
    elif shp != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)} (offsets[-1] correspondences), got {shp}")
    strides = cai.get("strides")
    if strides is not None:
        item, want = 4 if code == 0 else 8, []
        for s in reversed(shp):
            want.append(item)
            item *= s
        if any(s > 1 and st != w for s, st, w in zip(shp, strides, reversed(want))):
            raise ValueError(f"{name} must be C-contiguous")
    ptr = cai.get("data", (0, False))[0]
    size = 1
    for s in shp:
        size *= s
    if size > 0 and not ptr:
        raise ValueError(f"{name} has no device address")
    return (int(ptr) or None), code, shp


def _output_array(a, name, typestrs, dtype, shape, note):
    """(kind, address) of a caller's output array, checked: a numpy array ("host") or an object
    with __cuda_array_interface__ ("device") of the given dtype and shape, C-contiguous and
    writable.  note: what the shape stands for, for the message.  ValueError otherwise; the
    object is only inspected."""
    if isinstance(a, np.ndarray):
        if a.dtype != dtype or a.shape != shape:
            raise ValueError(f"{name} must be {np.dtype(dtype).name} of shape {shape}, got {a.dtype} {a.shape}")
        if not a.flags.c_contiguous:
            raise ValueError(f"{name} must be C-contiguous")
        if not a.flags.writeable:
            raise ValueError(f"{name} is read-only")
        return "host", a.ctypes.data
    try:
        cai = a.__cuda_array_interface__
    except Exception as e:
        raise ValueError(f"{name} must be a numpy array or a device array (an object with "
                         f"__cuda_array_interface__): {e}") from None
    if cai.get("typestr") not in typestrs:
        raise ValueError(f"{name} must be {np.dtype(dtype).name}, got typestr {cai.get('typestr')!r}")
    shp = tuple(int(s) for s in cai.get("shape", ()))
    if shp != shape:
        raise ValueError(f"{name} must have shape {shape} ({note}), got {shp}")
    strides = cai.get("strides")
    if strides is not None:
        item, want = np.dtype(dtype).itemsize, []
        for s in reversed(shp):
            want.append(item)
            item *= s
        if any(s > 1 and st != w for s, st, w in zip(shp, strides, reversed(want))):
            raise ValueError(f"{name} must be C-contiguous")
    data = cai.get("data", (0, False))
    if len(data) > 1 and data[1]:
        raise ValueError(f"{name} is read-only")
    size = 1
    for s in shp:
        size *= s
    if size > 0 and not data[0]:
        raise ValueError(f"{name} has no device address")
    return "device", int(data[0])


class PairSet:
    """Pairs set up once and resident on the device (mp_pair_set_*): hypothesize, select
    and refine as methods on them.

    hypothesize_batch, select_batch and refine_batch each set their pairs up per call (the
    problem of every pair, the packed upload, the pair records, the calibrated preparation);
    a PairSet does it once.  pairs: estimate_batch's dicts; options and est_config are bound
    at creation (the thresholds, weights, score type and min depths live in the pairs'
    device records).  Every method takes pair_ids (None: all pairs in order; else distinct
    indices into the set in any order) and takes and returns one entry per selected pair, in
    selection order, with exactly the values the batch function returns for [pairs[i] for i
    in pair_ids] under the set's options and config.  A call leaves nothing in the set that
    a later call can see.  Use as a context manager, or close(); any method after close()
    raises ValueError."""

    def __init__(self, variant, pairs, options, est_config=None, device=None):
        self._h = None
        est_config = self._bind(variant, options, est_config, device)
        o = options._to_c()
        c = est_config._to_c()
        P = len(pairs)
        if P:
            offs, X0, X1, D0, D1, MD, C0, C1 = _concat_pairs(variant, pairs)
        else:
            offs, X0, X1, D0, D1, MD, C0, C1 = [0], None, None, None, None, None, None, None
        self._sizes = [offs[p + 1] - offs[p] for p in range(P)]
        offsets = np.asarray(offs, dtype=np.int64)
        h = ctypes.c_void_p()
        dp = lambda a: None if a is None else _dp(a)
        L.check(L.lib().mp_pair_set_create(variant, P, offsets.ctypes.data_as(L.c_int64_p), dp(X0), dp(X1), dp(D0),
                                           dp(D1), dp(MD), dp(C0), dp(C1), ctypes.byref(o), ctypes.byref(c),
                                           self.device, ctypes.byref(h)))
        self._opened(h, P)

    def _bind(self, variant, options, est_config, device):
        """what both ways of creating a set do first: the variant check, the device, and why
        hypothesize may not be available on the set; returns the config to use"""
        if variant not in (L.CALIBRATED, L.SHARED_FOCAL, L.TWO_FOCAL, L.SCALE_ONLY):
            raise ValueError("variant must be 0 (calibrated), 1 (shared focal), 2 (two focal) or 3 (scale only)")
        if est_config is None:
            est_config = EstimatorConfig()
        self.variant = variant
        self.device = _DEFAULT_DEVICE if device is None else int(device)
        self._hyp_error = None  # why hypothesize is not available on this set
        if variant == L.SCALE_ONLY:
            self._hyp_error = "hypothesize does not support scale only (variant 3)"
        elif not est_config.use_shift:
            self._hyp_error = "hypothesize does not support use_shift = False"
        elif getattr(options, "use_ours", False) or getattr(options, "use_4p4d", False):
            self._hyp_error = "hypothesize does not support the alternate MD solvers (use_ours / use_4p4d)"
        return est_config

    def _opened(self, h, P):
        """... and last: keep the handle and fetch the normalization scales"""
        self._h = h
        norm = np.ones(max(P, 1))
        L.check(L.lib().mp_pair_set_norm_scales(self._h, _dp(norm)))
        self._norm = norm[:P]

    @classmethod
    def from_device(cls, variant, x0, x1, offsets, cam0, cam1, options, est_config=None, depth0=None, depth1=None,
                    depth_maps=None, map_ids=None, image_sizes=None, min_depth=None, stream=None, device=None):
        """A PairSet from arrays that are already on the device (mp_pair_set_create_device): the
        set PairSet(...) builds from the same numbers, bit for bit, without the trip through the
        host.

        Device inputs -- any object with __cuda_array_interface__ (torch tensors on a ROCm device
        have it), float32 or float64, C-contiguous: x0, x1 of shape (T, 2), the pixel coordinates
        of all pairs; and the depth priors, either depth0, depth1 of shape (T,), or depth_maps, a
        sequence of (h, w) maps of one dtype, looked up at the keypoints as get_depths does, with
        map_ids (P, 2): the map of side 0 / side 1 of each pair, and image_sizes (M, 2) = the
        (height, width) of the image each map belongs to (default: the map's own shape).  Host
        inputs: offsets (P + 1 ints, pair p = rows offsets[p] .. offsets[p + 1] - 1; T =
        offsets[-1]), cam0 / cam1 ((P, 3, 3) intrinsics, or (P, 2) principal points for the focal
        variants), min_depth ((P, 2), default zeros).  stream: the stream the inputs are produced
        on -- None (the null stream), an integer handle or an object with .cuda_stream; the
        library's stream waits for it on the device, the host does not.  The inputs are only read
        and are not referenced after the call returns.  ValueError, before any library call, for a
        wrong dtype, shape, contiguity or length, and for both depth sources or none."""
        self = cls.__new__(cls)
        self._h = None
        est_config = self._bind(variant, options, est_config, device)
        offs = np.asarray(offsets)
        if offs.ndim != 1 or offs.shape[0] < 1 or offs.dtype.kind not in "iu":
            raise ValueError("offsets must be a 1-D integer array of P + 1 values")
        offs = np.ascontiguousarray(offs, dtype=np.int64)
        P = offs.shape[0] - 1
        if offs[0] != 0 or np.any(np.diff(offs) < 0):
            raise ValueError("offsets must start at 0 and must not decrease")
        T = int(offs[-1])
        ncam = 9 if variant in (L.CALIBRATED, L.SCALE_ONLY) else 2

        def host(a, shape, name):
            a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
            if a.size != P * shape or (a.ndim and a.shape[0] != P and P > 0):
                raise ValueError(f"{name} must hold {shape} values for each of the {P} pairs")
            return a.reshape(-1)
        C0, C1 = host(cam0, ncam, "cam0"), host(cam1, ncam, "cam1")
        MD = np.zeros(2 * P) if min_depth is None else host(min_depth, 2, "min_depth")
        X0, xt, _ = _device_array(x0, "x0", (T, 2))
        X1, xt1, _ = _device_array(x1, "x1", (T, 2))
        if xt != xt1:
            raise ValueError("x0 and x1 must have the same dtype")
        arrays = depth0 is not None or depth1 is not None
        maps = depth_maps is not None or map_ids is not None or image_sizes is not None
        if arrays and maps:
            raise ValueError("both depth sources given: pass depth0 / depth1 or depth_maps / map_ids, not both")
        if not arrays and not maps:
            raise ValueError("no depth source given: pass depth0 / depth1 or depth_maps / map_ids")
        inp = L.mp_device_pairs()
        inp.x0, inp.x1, inp.xy_type = X0, X1, xt
        keep = []
        if arrays:
            if depth0 is None or depth1 is None:
                raise ValueError("depth0 and depth1 must both be given")
            D0, dt, _ = _device_array(depth0, "depth0", (T,))
            D1, dt1, _ = _device_array(depth1, "depth1", (T,))
            if dt != dt1:
                raise ValueError("depth0 and depth1 must have the same dtype")
            inp.d0, inp.d1, inp.depth_type = D0, D1, dt
        else:
            if depth_maps is None or map_ids is None:
                raise ValueError("the map source needs depth_maps and map_ids")
            M = len(depth_maps)
            if M == 0:
                raise ValueError("depth_maps is empty")
            ptrs, shapes, mts = [], [], set()
            for m, dm in enumerate(depth_maps):
                ptr, mt, shp = _device_array(dm, f"depth_maps[{m}]", None)
                ptrs.append(ptr)
                shapes.append(shp)
                mts.add(mt)
            if len(mts) != 1:
                raise ValueError("all depth maps must have one dtype")
            ids = np.asarray(map_ids)
            if ids.dtype.kind not in "iu" or ids.shape != (P, 2):
                raise ValueError(f"map_ids must be an integer array of shape ({P}, 2)")
            if ids.size and (ids.min() < 0 or ids.max() >= M):
                raise ValueError(f"map_ids must lie in 0..{M - 1}")
            ids = np.ascontiguousarray(ids, dtype=np.int32)
            if image_sizes is None:
                sizes = np.asarray(shapes, dtype=np.int64).reshape(M, 2)
            else:
                sizes = np.asarray(image_sizes)
                if sizes.dtype.kind not in "iu" or sizes.shape != (M, 2):
                    raise ValueError(f"image_sizes must be an integer array of shape ({M}, 2)")
                if np.any(sizes <= 0):
                    raise ValueError("image_sizes must be positive")
            dims = np.ascontiguousarray(np.concatenate([np.asarray(shapes, dtype=np.int64).reshape(M, 2),
                                                        sizes.astype(np.int64)], axis=1))
            table = (ctypes.c_void_p * M)(*ptrs)
            keep += [table, dims, ids]
            inp.depth_maps = ctypes.cast(table, ctypes.POINTER(ctypes.c_void_p))
            inp.map_dims = dims.ctypes.data_as(L.c_int64_p)
            inp.map_ids = ids.ctypes.data_as(L.c_int32_p)
            inp.num_maps, inp.map_type = M, mts.pop()
        if stream is not None:
            handle = getattr(stream, "cuda_stream", stream)
            if isinstance(handle, bool) or not isinstance(handle, int) or handle < 0:
                raise ValueError("stream must be None, an integer stream handle or an object with .cuda_stream")
            inp.producer_stream = handle or None
        o = options._to_c()
        c = est_config._to_c()
        self._sizes = [int(offs[p + 1] - offs[p]) for p in range(P)]
        h = ctypes.c_void_p()
        L.check(L.lib().mp_pair_set_create_device(variant, P, offs.ctypes.data_as(L.c_int64_p), ctypes.byref(inp),
                                                  _dp(MD), _dp(C0), _dp(C1), ctypes.byref(o), ctypes.byref(c),
                                                  self.device, ctypes.byref(h)))
        self._opened(h, P)
        return self

    # ---- lifetime ----
    def close(self):
        """Release the set's device memory; idempotent."""
        h, self._h = getattr(self, "_h", None), None
        if h is not None:
            L.check(L.lib().mp_pair_set_destroy(h))

    def __enter__(self):
        self._live()
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:  # (interpreter teardown: the library releases live sets itself)
            pass

    def _live(self):
        if getattr(self, "_h", None) is None:
            raise ValueError("the PairSet is closed")
        return self._h

    def __len__(self):
        self._live()
        return len(self._sizes)

    @property
    def norm_scale(self):
        """The pairs' normalization scales (float64, one per pair; 1 for calibrated)."""
        self._live()
        return self._norm.copy()

    def _info(self):
        h = self._live()
        nc, nb = ctypes.c_int64(), ctypes.c_int64()
        L.check(L.lib().mp_pair_set_info(h, None, None, ctypes.byref(nc), ctypes.byref(nb), None))
        return int(nc.value), int(nb.value)

    @property
    def num_correspondences(self):
        return self._info()[0]

    @property
    def resident_bytes(self):
        """Device bytes of the rows (96 per correspondence) and of the list buffers allocated
        so far (12 per correspondence each: one after select, two after refine)."""
        return self._info()[1]

    # ---- the selection ----
    def _selection(self, pair_ids, count, what):
        """(ids int32 array or None, its ctypes pointer or None, the selected pairs' sizes, their
        offsets), checked: `count` entries of `what` must match the selection."""
        P = len(self._sizes)
        if pair_ids is None:
            ids, sizes = None, self._sizes
        else:
            ids = np.ascontiguousarray(np.asarray(pair_ids, dtype=np.int64).reshape(-1))
            seen = set()
            for j, k in enumerate(ids.tolist()):
                if not 0 <= k < P:
                    raise ValueError(f"pair_ids[{j}] = {k} is outside the set of {P} pairs")
                if k in seen:
                    raise ValueError(f"pair_ids[{j}] = {k} occurs twice")
                seen.add(k)
            ids = ids.astype(np.int32)
            sizes = [self._sizes[k] for k in ids.tolist()]
        if count != len(sizes):
            raise ValueError(f"one {what} per selected pair: {count} for {len(sizes)} pairs")
        # (an empty selection is answered here, without the library: NULL would mean all pairs)
        ptr = None if ids is None else ids.ctypes.data_as(L.c_int32_p)
        offs = [0]
        for n in sizes:
            offs.append(offs[-1] + n)
        return ids, ptr, sizes, offs

    # ---- the stages ----
    def hypothesize(self, samples, pair_ids=None, sample_chunk=0):
        """hypothesize_batch on the selected pairs: (results, norm_scale) as it returns them."""
        h = self._live()
        if self._hyp_error:
            raise ValueError(self._hyp_error)
        if isinstance(sample_chunk, bool) or int(sample_chunk) != sample_chunk or sample_chunk < 0:
            raise ValueError("sample_chunk must be a non-negative integer (0: the default)")
        ids, ptr, sizes, _ = self._selection(pair_ids, len(samples), "(types, idx)")
        ns = len(sizes)
        norm = self._norm.copy() if ids is None else self._norm[ids].copy()
        if ns == 0:
            return [], norm
        slots = L.HYPOTHESIZE_SLOTS[self.variant]
        soffs, T, I = _concat_samples(self.variant, sizes, samples)
        S = soffs[-1]
        sample_offsets = np.asarray(soffs, dtype=np.int64)
        models = np.zeros((max(S, 1), slots, 17))
        counts = np.zeros(max(S, 1), dtype=np.int32)
        L.check(L.lib().mp_hypothesize_set(h, ns, ptr, sample_offsets.ctypes.data_as(L.c_int64_p),
                                           T.ctypes.data_as(L.c_int32_p), I.ctypes.data_as(L.c_int32_p),
                                           models.ctypes.data_as(ctypes.POINTER(L.mp_model)),
                                           counts.ctypes.data_as(L.c_int32_p), int(sample_chunk)))
        out = [(models[soffs[p]:soffs[p + 1]].copy(), counts[soffs[p]:soffs[p + 1]].copy()) for p in range(ns)]
        return out, norm

    def select(self, candidates, with_scores=False, with_counts=False, pair_ids=None, model_chunk=0):
        """select_batch on the selected pairs: one SelectResult per selected pair."""
        h = self._live()
        if isinstance(model_chunk, bool) or int(model_chunk) != model_chunk or model_chunk < 0:
            raise ValueError("model_chunk must be a non-negative integer (0: the default)")
        ids, ptr, sizes, offs = self._selection(pair_ids, len(candidates), "candidate list")
        ns = len(sizes)
        if ns == 0:
            return []
        moffs, arr, _keep = _concat_candidates(self.variant, candidates)
        model_offsets = np.asarray(moffs, dtype=np.int64)
        M = moffs[-1]
        res = (L.mp_select_result * ns)()
        idx = np.zeros(3 * max(offs[-1], 1), dtype=np.int32)
        scores = np.zeros(max(M, 1), dtype=np.float64) if with_scores else None
        counts = np.zeros(3 * max(M, 1), dtype=np.int32) if with_counts else None
        L.check(L.lib().mp_select_set(h, ns, ptr, model_offsets.ctypes.data_as(L.c_int64_p), arr,
                                      None if scores is None else _dp(scores),
                                      None if counts is None else counts.ctypes.data_as(L.c_int32_p), res,
                                      idx.ctypes.data_as(L.c_int32_p), int(model_chunk)))
        return _select_results(self.variant, candidates, res, idx, offs, moffs, scores, counts)

    def refine(self, models, rounds=1, pair_ids=None, relax=False):
        """refine_batch on the selected pairs: one RefineResult per selected pair.

        relax=True (mp_refine_relaxed_set): round 0 is the estimators' first local-optimisation
        fit -- its least squares runs over the inliers under the thresholds times the options'
        threshold_multiplier, formed in the same first sweep as the tight lists; rounds 1 onward
        and every returned score, count and list are the tight ones."""
        h = self._live()
        if not isinstance(relax, (bool, np.bool_)):
            raise ValueError("relax must be True or False")
        if int(rounds) != rounds or not 1 <= rounds <= 64:
            raise ValueError("rounds must be an integer in 1..64")
        ids, ptr, sizes, offs = self._selection(pair_ids, len(models), "model")
        ns = len(sizes)
        if ns == 0:
            return []
        arr = (L.mp_model * ns)(*[_model_to_c(m, self.variant) for m in models])
        res = (L.mp_refine_result * ns)()
        idx = np.zeros(3 * max(offs[-1], 1), dtype=np.int32)
        entry = L.lib().mp_refine_relaxed_set if relax else L.lib().mp_refine_set
        L.check(entry(h, ns, ptr, int(rounds), arr, res, idx.ctypes.data_as(L.c_int32_p)))
        return _refine_results(self.variant, arr, res, idx, offs)

    def lsq_fit(self, models, solver_types, factor=1.0, rule="lsq", seed=0, streams=None, substreams=None,
                pair_ids=None, with_subsets=False, entry_chunk=0):
        """One least-squares fit per entry on a random subset of the entry's inliers
        (mp_lsq_fit_set): the estimators' LeastSquaresFit (rule "lsq") or the non-minimal fit
        of a local-optimisation step (rule "nonmin").  One entry per model; pair_ids (None: all
        pairs in order) MAY repeat a pair.  solver_types: 0 (MD) or 1 (point) per entry, or one
        value for all; factor: the thresholds' factor, a scalar or one value per entry; streams,
        substreams: the subset's streams per entry (None: zeros; a scalar: for all).  Per
        entry, a LsqFitResult: score and num_inliers of the given model (select's values),
        num_wide (the inliers under the thresholds times factor), subset_sizes (the subset the
        rule draws from those; sizes and rule: include/madpose_mi355x.h), status (3: the rule
        or the solver's size test skipped the entry; else the LM's) and the model -- the LM's on
        status 1, else the given one.  with_subsets: also the subset's three index lists."""
        h = self._live()
        if rule not in L.LSQ_RULES:
            raise ValueError('rule must be "lsq" or "nonmin"')
        if isinstance(entry_chunk, bool) or int(entry_chunk) != entry_chunk or entry_chunk < 0:
            raise ValueError("entry_chunk must be a non-negative integer (0: the default)")
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= seed < 1 << 64:
            raise ValueError("seed must be an integer in 0 .. 2^64 - 1")
        P = len(self._sizes)
        ne = len(models)
        if pair_ids is None:
            if ne != P:
                raise ValueError(f"one model per pair: {ne} for {P} pairs")
            ids, ptr = None, None
            sizes = list(self._sizes)
        else:
            ids = np.ascontiguousarray(np.asarray(pair_ids, dtype=np.int64).reshape(-1))
            if len(ids) != ne:
                raise ValueError(f"one model per entry: {ne} for {len(ids)} pair_ids")
            for j, k in enumerate(ids.tolist()):
                if not 0 <= k < P:
                    raise ValueError(f"pair_ids[{j}] = {k} is outside the set of {P} pairs")
            ids = ids.astype(np.int32)
            ptr = ids.ctypes.data_as(L.c_int32_p)
            sizes = [self._sizes[k] for k in ids.tolist()]
        if ne == 0:
            return []

        def per_entry(val, name, dtype, lo, hi):
            a = np.asarray(0 if val is None else val)
            if a.dtype == np.bool_ or (dtype is np.int32 and not np.issubdtype(a.dtype, np.integer)):
                raise ValueError(f"{name} must be integers")
            a = np.ascontiguousarray(np.broadcast_to(a, (ne,)) if a.ndim == 0 else a.reshape(-1))
            if len(a) != ne:
                raise ValueError(f"one {name} value per entry: {len(a)} for {ne}")
            if not (np.all(a >= lo) and np.all(a < hi)):
                raise ValueError(f"{name} out of range")
            return np.ascontiguousarray(a.astype(dtype))
        st = per_entry(solver_types, "solver_types", np.int32, 0, 2)
        sr = per_entry(streams, "streams", np.int32, 0, 1 << 31)
        sb = per_entry(substreams, "substreams", np.int32, 0, 1 << 30)
        fa = per_entry(factor, "factor", np.float64, np.nextafter(0.0, 1.0), np.inf)
        offs = [0]
        for n in sizes:
            offs.append(offs[-1] + n)
        arr = (L.mp_model * ne)(*[_model_to_c(m, self.variant) for m in models])
        res = (L.mp_lsq_fit_result * ne)()
        idx = np.zeros(3 * max(offs[-1], 1), dtype=np.int32) if with_subsets else None
        L.check(L.lib().mp_lsq_fit_set(h, ne, ptr, st.ctypes.data_as(L.c_int32_p), _dp(fa), L.LSQ_RULES[rule],
                                       int(seed), sr.ctypes.data_as(L.c_int32_p), sb.ctypes.data_as(L.c_int32_p),
                                       arr, res, None if idx is None else idx.ctypes.data_as(L.c_int32_p),
                                       int(entry_chunk)))
        out = []
        for e in range(ne):
            q, n = res[e], sizes[e]
            r = LsqFitResult()
            r.score, r.status = float(q.score), int(q.status)
            r.num_inliers, r.num_wide, r.subset_sizes = list(q.num_inliers), list(q.num_wide), list(q.subset_sizes)
            r.model_row = np.frombuffer(bytes(arr[e]), dtype=np.float64).copy()
            r.model = _model_from_c(arr[e], self.variant)
            if idx is not None:
                base = 3 * offs[e]
                r.subsets = [idx[base + t * n: base + t * n + q.subset_sizes[t]].copy() for t in range(3)]
            out.append(r)
        return out

    def inlier_mass(self, models, weights, pair_ids=None):
        """The weight mass of models' inlier lists (mp_inlier_mass_set): one InlierMass per
        entry.  One entry per model; pair_ids (None: all pairs in order) MAY repeat a pair.
        weights: draw_weights' object.  For entry (pair p, model m), with L_t the three lists
        select([[m]], pair_ids=[p]) returns: count = their lengths; for a weighted pair mass[t] =
        the sum over L_t of the quantised weights q_i and total = weights.total[p]; for a pair
        that is not weighted mass = count and total = the pair's size.  weighted: which of the
        two.  These are the numbers ransac(weighted_stop=True) divides.  One launch; integer
        sums, so the values do not depend on the device's reduction order."""
        h = self._live()
        wh = self._weights_handle(weights)
        P = len(self._sizes)
        ne = len(models)
        if pair_ids is None:
            if ne != P:
                raise ValueError(f"one model per pair: {ne} for {P} pairs")
            ptr = None
        else:
            ids = np.ascontiguousarray(np.asarray(pair_ids, dtype=np.int64).reshape(-1))
            if len(ids) != ne:
                raise ValueError(f"one model per entry: {ne} for {len(ids)} pair_ids")
            for j, k in enumerate(ids.tolist()):
                if not 0 <= k < P:
                    raise ValueError(f"pair_ids[{j}] = {k} is outside the set of {P} pairs")
            ids = ids.astype(np.int32)
            ptr = ids.ctypes.data_as(L.c_int32_p)
        if ne > L.INLIER_MASS_MAX_ENTRIES:
            raise ValueError("at most 2^24 entries per call")
        if ne == 0:
            return []
        arr = (L.mp_model * ne)(*[_model_to_c(m, self.variant) for m in models])
        res = (L.mp_inlier_mass * ne)()
        L.check(L.lib().mp_inlier_mass_set(h, wh, ne, ptr, arr, res))
        return [InlierMass(tuple(int(v) for v in q.mass), int(q.total), tuple(int(v) for v in q.count),
                           bool(q.weighted)) for q in res]

    def residuals(self, models, pair_ids=None, factor=1.0, errors=False, out_mask=None, out_errors=None, stream=None):
        """What models do to every correspondence (mp_residuals_set): a ResidualsResult with the
        three-bit inlier mask and, with errors=True, the three squared errors of every row.

        One entry per model; models is a sequence of pose objects or an (ne, 17) float64 array
        in mp_model order (RansacResult.model_row, what select accepts); pair_ids (None: all
        pairs in order) MAY repeat a pair; factor: the thresholds' factor, a scalar or one value
        per entry.  Entry e owns rows res.rows(e) of the outputs.  mask[i]: bit t set iff
        errors[t, i] < thr_t * factor (t = 0, 1: the depth-aware reprojection errors 0 -> 1 and
        1 -> 0, t = 2: Sampson; ungated by the score type); with factor 1 bit t marks exactly
        inlier_indices[t] of select([[m]], pair_ids=[p]), and counts are those lists' lengths.
        A model with a NaN entry has an all-zero mask.  The errors are in problem units: for the
        focal variants multiply by norm_scale[p] ** 2 for squared pixels.

        Without out_mask / out_errors the results are host numpy arrays.  out_mask (uint8, shape
        (R,)) and out_errors (float64, shape (3, R); implies errors=True), R the rows of the
        call, are C-contiguous writable arrays of one kind: numpy arrays, or device arrays
        (objects with __cuda_array_interface__, e.g. torch tensors on the set's device), which
        the kernel writes directly; stream is then the stream they were last used on, as in
        from_device.  ValueError, before any library call, for a wrong model count, shape or
        dtype, a bad output shape, dtype, contiguity or read-only flag, a factor that is not
        finite and positive, and outputs of different kinds."""
        h = self._live()
        P = len(self._sizes)
        if isinstance(models, np.ndarray):
            if models.dtype != np.float64 or models.ndim != 2 or models.shape[1] != 17:
                raise ValueError(f"array models must be float64 of shape (ne, 17), got {models.dtype} {models.shape}")
            ne = models.shape[0]
        else:
            try:
                ne = len(models)
            except TypeError:
                raise ValueError("models must be a sequence of poses or an (ne, 17) float64 array") from None
        if pair_ids is None:
            if ne != P:
                raise ValueError(f"one model per pair: {ne} for {P} pairs")
            ids, ptr = None, None
            sizes = list(self._sizes)
        else:
            ids = np.ascontiguousarray(np.asarray(pair_ids, dtype=np.int64).reshape(-1))
            if len(ids) != ne:
                raise ValueError(f"one model per entry: {ne} for {len(ids)} pair_ids")
            for j, k in enumerate(ids.tolist()):
                if not 0 <= k < P:
                    raise ValueError(f"pair_ids[{j}] = {k} is outside the set of {P} pairs")
            ids = ids.astype(np.int32)
            ptr = ids.ctypes.data_as(L.c_int32_p)
            sizes = [self._sizes[k] for k in ids.tolist()]
        if ne > L.RESIDUALS_MAX_ENTRIES:
            raise ValueError("at most 2^24 entries per call")
        fa = np.asarray(factor)
        if fa.dtype == np.bool_ or fa.dtype.kind not in "fiu":
            raise ValueError("factor must be a number or one number per entry")
        fa = np.ascontiguousarray(np.broadcast_to(fa, (ne,)) if fa.ndim == 0 else fa.reshape(-1), dtype=np.float64)
        if len(fa) != ne:
            raise ValueError(f"one factor value per entry: {len(fa)} for {ne}")
        if not np.all(np.isfinite(fa) & (fa > 0)):
            raise ValueError("factor must be finite and positive")
        if not isinstance(errors, (bool, np.bool_)):
            raise ValueError("errors must be True or False")
        offs = np.zeros(ne + 1, dtype=np.int64)
        np.cumsum(np.asarray(sizes, dtype=np.int64), out=offs[1:])
        R = int(offs[-1])
        want_err = bool(errors) or out_errors is not None

        kinds = set()
        mask_ptr = err_ptr = None
        if out_mask is not None:
            kind, mask_ptr = _output_array(out_mask, "out_mask", ("|u1", "<u1", "=u1"), np.uint8, (R,), f"R = {R} rows")
            kinds.add(kind)
        if out_errors is not None:
            kind, err_ptr = _output_array(out_errors, "out_errors", ("<f8", "=f8"), np.float64, (3, R),
                                          f"R = {R} rows")
            kinds.add(kind)
        if len(kinds) > 1:
            raise ValueError("out_mask and out_errors must be of one kind: both numpy arrays or both device arrays")
        on_device = "device" in kinds
        if on_device and (out_mask is None or (want_err and out_errors is None)):
            raise ValueError("device outputs: out_mask is needed, and out_errors when errors are asked for")
        producer = None
        if stream is not None:
            if not on_device:
                raise ValueError("stream goes with device outputs")
            handle = getattr(stream, "cuda_stream", stream)
            if isinstance(handle, bool) or not isinstance(handle, int) or handle < 0:
                raise ValueError("stream must be None, an integer stream handle or an object with .cuda_stream")
            producer = handle or None
        if isinstance(models, np.ndarray):
            keep = np.ascontiguousarray(models)
            arr = keep.ctypes.data_as(ctypes.POINTER(L.mp_model))
        else:
            keep = arr = (L.mp_model * max(ne, 1))(*[_model_to_c(m, self.variant) for m in models])

        res = ResidualsResult()
        res.mask = out_mask if out_mask is not None else np.zeros(R, dtype=np.uint8)
        res.errors = out_errors if out_errors is not None else (np.zeros((3, R)) if want_err else None)
        res.offsets = offs
        res.counts = np.zeros((ne, 3), dtype=np.int32)
        if R == 0:  # (no row: answered here, nothing to launch or write)
            return res
        out = L.mp_residuals_out()
        out.mask = mask_ptr if out_mask is not None else res.mask.ctypes.data
        out.errors = err_ptr if out_errors is not None else (res.errors.ctypes.data if want_err else None)
        out.on_device = 1 if on_device else 0
        out.producer_stream = producer
        row_offsets = np.zeros(ne + 1, dtype=np.int64)
        L.check(L.lib().mp_residuals_set(h, ne, ptr, arr, _dp(fa), ctypes.byref(out),
                                         row_offsets.ctypes.data_as(L.c_int64_p),
                                         res.counts.ctypes.data_as(L.c_int32_p)))
        del keep
        res.offsets = row_offsets
        return res

    def information(self, models, pair_ids=None, factor=1.0, covariance=True, out_H=None, out_g=None, out_cost=None,
                    out_cov=None, stream=None):
        """How well each pair's correspondences determine a model (mp_information_set): an
        InformationResult with, per entry, the Gauss-Newton system of the estimators' cost over
        the model's inliers and its inverse.

        Entries as in residuals: models is a sequence of pose objects or an (ne, 17) float64
        array in user units, pair_ids (None: all pairs in order) MAY repeat a pair, factor is a
        scalar or one value per entry.  For entry e (model m on pair p), row i is a residual
        block of type t iff bit t of residuals(m, factor) is set for it; LO_type 1 drops the
        reprojection blocks and 2 the Sampson blocks, and use_shift, the scale-only rule and the
        Sampson weight are those of the job refine would run on these lists.  In the layout
        rotation tangent 3, t 3, scale, offset0, offset1, focal0, focal1: H[e] (66) is the
        packed upper triangle of J^T J, g[e] (11) is J^T r, cost[e] = sum r^2 / 2, cov[e] (11,
        11) the inverse of H on the active parameters col[e] (zero elsewhere), rows[e] = 2 (n0 +
        n1) + n2 over the gated block counts and counts[e] residuals' counts.  status 1: at
        least one block; pd 1: the Cholesky factorisation completed, 0: an active H_aa or a
        pivot was not positive and finite (cov zero), -1: status 0, everything zero (a model
        with a NaN entry, a pair without correspondences, no row inside the thresholds).  pd = 1
        does not detect an ill-conditioned system: with Sampson blocks alone |t| is a gauge and
        its variance is rounding noise; gauges are not handled.

        Units: everything is in problem units, like residuals' errors -- residuals in pixels for
        the calibrated variants and pixels / norm_scale[p] for the focal variants, whose focal
        parameters are focal / norm_scale[p].  cov is the inverse of H under unit-variance
        residuals: for a focal's row and column multiply by norm_scale[p] per index, and the
        a-posteriori variance factor is 2 cost / (rows - n), n the number of active parameters.
        InformationResult.covariance(e, scaled=True) does both on the host.

        The results are host numpy arrays, or any subset of out_H (ne, 66), out_g (ne, 11),
        out_cost (ne,) and out_cov (ne, 11, 11): float64, C-contiguous, writable, pairwise
        disjoint and of one kind -- numpy arrays, or device arrays (__cuda_array_interface__,
        e.g. torch tensors on the set's device) that the finishing kernel writes directly;
        stream is then the stream they were last used on.  With host outputs, what is not given
        as out_* is a new numpy array of the result; with device outputs only the given arrays
        are computed and the others are None.  covariance=False without out_cov skips the
        inverse's stores (cov is None; pd is still reported).  col, pd, status, rows and counts
        always come back to the host.  ValueError, before any library call, for every malformed
        argument."""
        h = self._live()
        P = len(self._sizes)
        if isinstance(models, np.ndarray):
            if models.dtype != np.float64 or models.ndim != 2 or models.shape[1] != 17:
                raise ValueError(f"array models must be float64 of shape (ne, 17), got {models.dtype} {models.shape}")
            ne = models.shape[0]
        else:
            try:
                ne = len(models)
            except TypeError:
                raise ValueError("models must be a sequence of poses or an (ne, 17) float64 array") from None
        if pair_ids is None:
            if ne != P:
                raise ValueError(f"one model per pair: {ne} for {P} pairs")
            ptr = None
            sizes = list(self._sizes)
        else:
            ids = np.ascontiguousarray(np.asarray(pair_ids, dtype=np.int64).reshape(-1))
            if len(ids) != ne:
                raise ValueError(f"one model per entry: {ne} for {len(ids)} pair_ids")
            for j, k in enumerate(ids.tolist()):
                if not 0 <= k < P:
                    raise ValueError(f"pair_ids[{j}] = {k} is outside the set of {P} pairs")
            ids = ids.astype(np.int32)
            ptr = ids.ctypes.data_as(L.c_int32_p)
            sizes = [self._sizes[k] for k in ids.tolist()]
        if ne > L.INFORMATION_MAX_ENTRIES:
            raise ValueError("at most 2^24 entries per call")
        fa = np.asarray(factor)
        if fa.dtype == np.bool_ or fa.dtype.kind not in "fiu":
            raise ValueError("factor must be a number or one number per entry")
        fa = np.ascontiguousarray(np.broadcast_to(fa, (ne,)) if fa.ndim == 0 else fa.reshape(-1), dtype=np.float64)
        if len(fa) != ne:
            raise ValueError(f"one factor value per entry: {len(fa)} for {ne}")
        if not np.all(np.isfinite(fa) & (fa > 0)):
            raise ValueError("factor must be finite and positive")
        if not isinstance(covariance, (bool, np.bool_)):
            raise ValueError("covariance must be True or False")
        want_cov = bool(covariance) or out_cov is not None

        shapes = (("out_H", out_H, (ne, 66)), ("out_g", out_g, (ne, 11)), ("out_cost", out_cost, (ne,)),
                  ("out_cov", out_cov, (ne, 11, 11)))
        kinds, given = set(), {}
        for name, a, shape in shapes:
            if a is None:
                continue
            kind, addr = _output_array(a, name, ("<f8", "=f8"), np.float64, shape, f"ne = {ne} entries")
            kinds.add(kind)
            given[name] = (addr, 8 * int(np.prod(shape, dtype=np.int64)))
        if len(kinds) > 1:
            raise ValueError("out_H, out_g, out_cost and out_cov must be of one kind: all numpy arrays or all device "
                             "arrays")
        names = sorted(given)
        for i, a in enumerate(names):
            for b in names[i + 1:]:
                (pa, la), (pb, lb) = given[a], given[b]
                if la > 0 and lb > 0 and pa < pb + lb and pb < pa + la:
                    raise ValueError(f"{a} and {b} overlap")
        on_device = "device" in kinds
        producer = None
        if stream is not None:
            if not on_device:
                raise ValueError("stream goes with device outputs")
            handle = getattr(stream, "cuda_stream", stream)
            if isinstance(handle, bool) or not isinstance(handle, int) or handle < 0:
                raise ValueError("stream must be None, an integer stream handle or an object with .cuda_stream")
            producer = handle or None
        if isinstance(models, np.ndarray):
            keep = np.ascontiguousarray(models)
            arr = keep.ctypes.data_as(ctypes.POINTER(L.mp_model))
        else:
            keep = arr = (L.mp_model * max(ne, 1))(*[_model_to_c(m, self.variant) for m in models])

        res = InformationResult()
        res.H, res.g, res.cost = np.zeros((ne, 66)), np.zeros((ne, 11)), np.zeros(ne)
        res.cov = np.zeros((ne, 11, 11)) if want_cov else None
        res.col = np.zeros((ne, 11), dtype=np.int32)
        res.pd = np.full(ne, -1, dtype=np.int32)
        res.status = np.zeros(ne, dtype=np.int32)
        res.rows = np.zeros(ne, dtype=np.int32)
        res.counts = np.zeros((ne, 3), dtype=np.int32)
        res.norm_scale = np.array([self._norm[k] for k in (range(P) if pair_ids is None else ids.tolist())],
                                  dtype=np.float64).reshape(ne)
        res.focal_columns = (9,) if self.variant == L.SHARED_FOCAL else ((9, 10) if self.variant == L.TWO_FOCAL else ())
        for name, a, _ in shapes:  # (the caller's arrays are the result's; device outputs: no others)
            if a is not None or on_device:
                setattr(res, name[4:], a)
        if ne == 0 or (sum(sizes) == 0 and not on_device):  # (answered here: nothing to launch)
            for a in (res.H, res.g, res.cost, res.cov):
                if a is not None:
                    a[...] = 0.0
            return res
        ent = (L.mp_information_entry * ne)()
        out = L.mp_information_out()
        for name, _, _ in shapes:
            a = getattr(res, name[4:])
            setattr(out, name[4:], None if a is None else (given[name][0] if on_device else a.ctypes.data))
        out.on_device = 1 if on_device else 0
        out.producer_stream = producer
        L.check(L.lib().mp_information_set(h, ne, ptr, arr, _dp(fa), ctypes.byref(out), ent))
        del keep
        rec = np.frombuffer(ent, dtype=np.int32).reshape(ne, 17)
        res.col[...] = rec[:, 0:11]
        res.pd[...], res.status[...], res.rows[...] = rec[:, 11], rec[:, 12], rec[:, 13]
        res.counts[...] = rec[:, 14:17]
        return res

    def _check_draw(self, budget, seed, point_share, ns):
        if isinstance(budget, bool) or not isinstance(budget, (int, np.integer)) or budget < 0:
            raise ValueError("budget must be a non-negative integer")
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= seed < 1 << 64:
            raise ValueError("seed must be an integer in 0 .. 2^64 - 1")
        if point_share is not None and (isinstance(point_share, bool) or int(point_share) != point_share
                                        or not 0 <= point_share <= L.DRAW_POINT_SHARE_MAX):
            raise ValueError("point_share must be None (the solver type's default) or an integer in 0..256")
        if ns * int(budget) > L.HYPOTHESIZE_MAX_SAMPLES:
            raise ValueError(f"at most 2^22 samples per call, got {ns} pairs x {budget}")
        return int(budget), int(seed), -1 if point_share is None else int(point_share)

    def draw_weights(self, weights, stream=None, given=None):
        """Confidence weights for draw and ransac (mp_draw_weights_create): a DrawWeights, to be
        passed as weights= to any number of calls on this set, and closed (or used as a context
        manager) when done.

        weights: a sequence with one entry per pair of the set -- a 1-D C-contiguous float32 or
        float64 array of that pair's length, or None for a pair that draws uniformly -- or one
        device array (an object with __cuda_array_interface__) of shape (T,) over the whole set,
        float32 or float64; stream is then the stream it is produced on, as in from_device, and
        given (optional, one bool per pair) marks the pairs whose rows count.  A weight is a
        finite value in 0 .. 1 and is quantised to q = min(65535, floor(w * 65536)); q = 0 masks
        the correspondence.  A sample's indices are then proposed with probability q_i / sum q
        instead of uniformly; the sample types, the counter and the key are draw's, and equal
        weights give draw's bytes.  A pair with fewer positive weights than its largest sample
        draws uniformly (.weighted is False for it); a pair given weights may have at most
        65535 correspondences.  The adaptive modes' termination rule reads inlier count ratios
        unless ransac is given weighted_stop=True, which makes it read the weights' mass over the
        inlier lists (inlier_mass) divided by .total.  ValueError, before any
        library call, for a wrong length, dtype or contiguity and for a bad value in a host
        array."""
        h = self._live()
        if self._hyp_error:
            raise ValueError(self._hyp_error.replace("hypothesize", "draw_weights"))
        P, T = len(self._sizes), int(sum(self._sizes))
        producer = None
        if hasattr(weights, "__cuda_array_interface__"):
            ptr, code, _ = _device_array(weights, "weights", (T,))
            if given is None:
                mask = np.ones(P, dtype=np.uint8)
            else:
                mask = np.asarray(given)
                if mask.shape != (P,) or mask.dtype.kind not in "biu":
                    raise ValueError(f"given must hold one bool for each of the {P} pairs")
                mask = np.ascontiguousarray(mask != 0, dtype=np.uint8)
            if stream is not None:
                handle = getattr(stream, "cuda_stream", stream)
                if isinstance(handle, bool) or not isinstance(handle, int) or handle < 0:
                    raise ValueError("stream must be None, an integer stream handle or an object with .cuda_stream")
                producer = handle or None
            on_device, keep = 1, weights
        else:
            if given is not None or stream is not None:
                raise ValueError("given and stream go with a device array; a host sequence says None per pair")
            try:
                count = len(weights)
            except TypeError:
                raise ValueError("weights must be a sequence with one entry per pair, or a device array") from None
            if count != P:
                raise ValueError(f"one weights entry per pair of the set: {count} for {P} pairs")
            arrays = []
            for p, w in enumerate(weights):
                if w is None:
                    arrays.append(None)
                    continue
                a = np.asarray(w)
                if a.dtype not in (np.float32, np.float64):
                    raise ValueError(f"weights[{p}] must be float32 or float64, got {a.dtype}")
                if a.ndim != 1 or a.shape[0] != self._sizes[p]:
                    raise ValueError(f"weights[{p}] must be 1-D with the pair's {self._sizes[p]} values, "
                                     f"got shape {a.shape}")
                if not a.flags.c_contiguous:
                    raise ValueError(f"weights[{p}] must be C-contiguous")
                bad = np.flatnonzero(~((a >= 0) & (a <= 1)))
                if bad.size:
                    raise ValueError(f"weights[{p}][{int(bad[0])}] = {a[bad[0]]!r} is not a finite value in 0..1")
                arrays.append(a)
            all32 = all(a is None or a.dtype == np.float32 for a in arrays)
            code = 0 if all32 else 1
            keep = np.zeros(max(T, 1), dtype=np.float32 if all32 else np.float64)  # (float32 widens exactly)
            mask = np.zeros(P, dtype=np.uint8)
            at = 0
            for p, a in enumerate(arrays):
                if a is not None:
                    keep[at:at + self._sizes[p]] = a
                    mask[p] = 1
                at += self._sizes[p]
            ptr, on_device = keep.ctypes.data, 0
        for p in range(P):
            if mask[p] and self._sizes[p] > L.DRAW_WEIGHT_MAX_N:
                raise ValueError(f"pair {p} has {self._sizes[p]} correspondences: a pair given weights may have "
                                 f"at most {L.DRAW_WEIGHT_MAX_N} (pass None for it)")
        wh = ctypes.c_void_p()
        L.check(L.lib().mp_draw_weights_create(h, ptr, code, on_device,
                                               mask.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)) if P else None,
                                               producer, ctypes.byref(wh)))
        del keep
        return DrawWeights(self, wh, P)

    def _weights_handle(self, weights):
        if not isinstance(weights, DrawWeights):
            raise ValueError("weights must be None or the object draw_weights returned")
        return weights._live(self)

    def draw(self, budget, seed, point_share=None, pair_ids=None, weights=None):
        """`budget` minimal samples per selected pair, drawn on the device (mp_draw_set): one
        (types, idx) per pair, the list hypothesize takes.  A pair too small for the MD solver
        gets none, one too small for the point solver only type 0.  The draw of a pair depends
        on seed, point_share (of 256: the share of point-solver samples; None: 128 hybrid, 256
        point solver only, 0 MD solver only, by the set's solver type) and the pair's index in
        the set, not on the selection.  weights (None, or draw_weights' object): the indices of
        its weighted pairs are proposed by confidence (mp_draw_weighted_set)."""
        h = self._live()
        if self._hyp_error:
            raise ValueError(self._hyp_error.replace("hypothesize", "draw"))
        wh = None if weights is None else self._weights_handle(weights)
        ids, ptr, sizes, _ = self._selection(pair_ids, len(self._sizes) if pair_ids is None else len(pair_ids), "entry")
        ns = len(sizes)
        budget, seed, share = self._check_draw(budget, seed, point_share, ns)
        if ns == 0:
            return []
        T = np.zeros(max(ns * budget, 1), dtype=np.int32)
        I = np.zeros(max(ns * budget, 1) * L.HYPOTHESIZE_SAMPLE_STRIDE, dtype=np.int32)
        C = np.zeros(ns, dtype=np.int32)
        if wh is not None:
            L.check(L.lib().mp_draw_weighted_set(h, wh, ns, ptr, budget, seed, share, T.ctypes.data_as(L.c_int32_p),
                                                 I.ctypes.data_as(L.c_int32_p), C.ctypes.data_as(L.c_int32_p)))
        else:
            L.check(L.lib().mp_draw_set(h, ns, ptr, budget, seed, share, T.ctypes.data_as(L.c_int32_p),
                                        I.ctypes.data_as(L.c_int32_p), C.ctypes.data_as(L.c_int32_p)))
        offs = np.concatenate([[0], np.cumsum(C)])
        I = I.reshape(-1, L.HYPOTHESIZE_SAMPLE_STRIDE)
        return [(T[offs[j]:offs[j + 1]].copy(), I[offs[j]:offs[j + 1]].copy()) for j in range(ns)]

    def candidates(self, samples, pair_ids=None, sample_chunk=0):
        """hypothesize on the selected pairs with only the models that exist returned
        (mp_candidates_set): one (models, sample, slot) per pair -- models float64 of shape
        (K, 17), select's array candidates: the pair's models in sample order and slot order
        with hypothesize's bytes; sample and slot int32 of shape (K,), each model's origin."""
        h = self._live()
        if self._hyp_error:
            raise ValueError(self._hyp_error.replace("hypothesize", "candidates"))
        if isinstance(sample_chunk, bool) or int(sample_chunk) != sample_chunk or sample_chunk < 0:
            raise ValueError("sample_chunk must be a non-negative integer (0: the default)")
        ids, ptr, sizes, _ = self._selection(pair_ids, len(samples), "(types, idx)")
        ns = len(sizes)
        if ns == 0:
            return []
        soffs, T, I = _concat_samples(self.variant, sizes, samples)
        sample_offsets = np.asarray(soffs, dtype=np.int64)
        M = ctypes.c_int64(0)
        L.check(L.lib().mp_candidates_set(h, ns, ptr, sample_offsets.ctypes.data_as(L.c_int64_p),
                                          T.ctypes.data_as(L.c_int32_p), I.ctypes.data_as(L.c_int32_p),
                                          int(sample_chunk), ctypes.byref(M)))
        M = int(M.value)
        models = np.zeros((max(M, 1), 17))
        moffs = np.zeros(ns + 1, dtype=np.int64)
        smp, slot = np.zeros(max(M, 1), dtype=np.int32), np.zeros(max(M, 1), dtype=np.int32)
        L.check(L.lib().mp_candidates_fetch(h, models.ctypes.data_as(ctypes.POINTER(L.mp_model)),
                                            moffs.ctypes.data_as(L.c_int64_p), smp.ctypes.data_as(L.c_int32_p),
                                            slot.ctypes.data_as(L.c_int32_p)))
        return [(models[moffs[j]:moffs[j + 1]].copy(), smp[moffs[j]:moffs[j + 1]].copy(),
                 slot[moffs[j]:moffs[j + 1]].copy()) for j in range(ns)]

    def ransac(self, budget=None, seed=0, point_share=None, samples=None, rounds=3, pair_ids=None, sample_chunk=0,
               model_chunk=0, step=None, lo=None, lo_steps=None, weights=None, weighted_stop=False, out_mask=None,
               out_errors=None, out_models=None, out_index=None, out_counts=None, stream=None, lists=True):
        """Fixed-budget RANSAC on the selected pairs in one call (mp_ransac_set): draw ->
        hypothesize -> select -> refine on the device-resident pairs.  Exactly one of budget
        (samples drawn on the device as draw(budget, seed, point_share) draws them) and samples
        (hypothesize's list).  rounds 0 .. 64; 0 stops after the selection.  Returns one
        RansacResult per pair, equal byte for byte to candidates(S) -> select ->
        refine(winners, rounds, pair_ids=the pairs with a winner) on this set.

        step (None, or an integer >= 1; needs budget, refuses samples): the adaptive mode
        (mp_ransac_adaptive_set).  The drawn samples go through the device in rounds of `step`
        per pair, and a pair stops at the first checkpoint min(k step, budget) at which the
        estimators' termination rule holds on its best candidate so far (the options'
        success_probability, min_num_iterations and max_num_iterations_per_solver), or at
        budget.  Each result then equals, byte for byte, ransac(budget=r.num_samples,
        pair_ids=[that pair]) with the same seed, point_share and rounds; r.stopped tells
        whether the rule ended the pair.

        lo (None, or an integer in 1..64; needs step, refuses samples): local optimisation
        inside the adaptive rounds (mp_ransac_lo_set).  At every checkpoint at which a pair's
        best minimal model was replaced, that model is first offered to the pair's overall best
        (strictly lower score wins) and then refined by refine(relax=True, rounds=lo), whose
        result becomes the overall best if a round was accepted and it scores strictly lower.
        The termination rule reads the overall best's inlier counts, and the final `rounds`
        refine the overall best.  index, sample, slot, solver_type, score_selected,
        num_samples and num_candidates describe the minimal models' walk, as without lo; the
        model, score_initial, score_final, rounds_*, status and inlier_indices the refined
        overall best.  lo_runs, lo_accepted: the pair's local optimisations and how many of
        them became the overall best; lo_index: the candidate whose local optimisation gave
        the overall best (-1: it is a minimal model).

        lo_steps (None, or an integer in 1..64; needs lo): the estimators' LO steps after each
        local optimisation (mp_ransac_lo_steps_set).  From the model a that refine(relax=True,
        rounds=lo) returned for candidate c of solver type s, step r = 0 .. lo_steps - 1 runs
        lsq_fit(a, s, rule="nonmin") -> m1 (a status other than 1 ends the step), lsq_fit(m1, s,
        rule="lsq") -> m2, then num_lsq_iterations fits lsq_fit(m, s, factor=f_i, rule="lsq") with
        f_i = t - i (t - 1) / (Q - 1) falling from t = threshold_multiplier to 1, each with
        streams=c and substreams=256 r + stage; the steps' last models are ranked by one select.
        Every model a stage scored (each lsq_fit scores its input) and the select's winner are
        offered to the overall best, strictly lower score wins.  All steps of all pairs of a
        checkpoint go through a stage in one launch sequence.  lo_step, lo_stage: the step and
        the stage that produced the overall best (-1: no step did; lo_stage is 2 +
        num_lsq_iterations for a step's last model); lo_step_offers, lo_step_accepted: the
        offers made and those that became the overall best.

        weights (None, or draw_weights' object; needs budget, refuses samples): the drawn samples
        are draw(..., weights=weights)'s in every mode (mp_ransac_weighted_set), and each mode's
        identity above holds with weights passed to both sides.  Without weighted_stop the
        termination rule still reads inlier count ratios c[t] / n.

        weighted_stop (a bool; True needs weights and step): the adaptive modes stop a weighted
        pair on the weight mass of its rule model's inlier lists (mp_ransac_weighted_stop_set):
        the rule's ratios are mass[t] / total, mass[t] the sum of the quantised weights q_i over
        list t and total their sum over the pair (inlier_mass gives both for any model).  The
        rule model is the best minimal model with step alone and the overall best at a
        checkpoint's end with lo / lo_steps; its masses are computed by one launch per
        checkpoint over the pairs whose rule model was replaced.  A pair that is not weighted
        (w.weighted False) keeps the count rule, and equal weights give the count rule's stop
        points bit for bit, so the bytes of the call with weighted_stop=False.  The mass rule is
        NOT "never later" than the count rule: a list made mostly of low-confidence rows has a
        mass ratio below its count ratio and stops later; informative weights, where inliers
        carry the confidence, stop much earlier.  Each mode's identity above still holds at
        r.num_samples.  r.rule_mass (a tuple of 3) and r.rule_total: what the rule last read
        for the pair (zeros and the pair's total when it never had a winner); None and 0 with
        weighted_stop off.

        out_mask, out_errors, out_models, out_index, out_counts (any subset; every mode above):
        the results written into the caller's device arrays by the call itself
        (mp_ransac_out_set).  With ns selected pairs in selection order and R the sum of their
        sizes, pair j owns rows r.rows of out_mask (uint8, (R,)) and of the second axis of
        out_errors (float64, (3, R); needs out_mask), and row j of out_models (float64, (ns, 17)),
        out_index (int32, (ns,)) and out_counts (int32, (ns, 3)).  All are device arrays (objects
        with __cuda_array_interface__, e.g. torch tensors) on the set's device, C-contiguous,
        writable and disjoint; stream is the stream they were last used on, as in residuals.  For a
        pair with a winner out_models[j] holds r.model_row's bytes, out_index[j] = r.index,
        out_counts[j] the three list lengths, bit t of out_mask[row] is set iff the row is in
        r.inlier_indices[t] (bits 3 .. 7 zero), and out_errors[t, row] is the squared error in
        problem units under the model the lists were formed from -- so (out_errors[t] < thr_t)
        equals bit t on every row, in every variant and after any number of rounds, where
        residuals(r.model_row) can differ on a refined focal model.  For a pair without a winner,
        or of size 0: mask rows 0, error rows NaN, model row zeros, index -1, counts 0.  Every
        element belonging to the selection is written once; nothing else is touched.  Device
        outputs together with lo and rounds=0 are refused: the overall best's lists may then be a
        local optimisation's, whose model in problem units is not kept.

        lists (a bool): False copies no index list back from the device -- r.inlier_indices is
        None, r.num_inliers still holds the three lengths -- with or without device outputs.
        r.rows: the pair's slice of out_mask and of out_errors' second axis (None when neither
        was given).  Every other field, and the list itself, is what the call returns without
        these arguments."""
        if not isinstance(lists, (bool, np.bool_)):
            raise ValueError("lists must be a bool")
        outs = (("out_mask", out_mask), ("out_errors", out_errors), ("out_models", out_models),
                ("out_index", out_index), ("out_counts", out_counts))
        on_device = any(a is not None for _, a in outs)
        for name, a in outs:
            if isinstance(a, np.ndarray):
                raise ValueError(f"{name} must be a device array (an object with __cuda_array_interface__): on the "
                                 "host, r.inlier_indices holds the lists and PairSet.residuals fills numpy arrays")
        if out_errors is not None and out_mask is None:
            raise ValueError("out_errors needs out_mask")
        if on_device and lo is not None and not isinstance(rounds, bool) and rounds == 0:
            raise ValueError("device outputs with lo need rounds >= 1: without final rounds the overall best's lists "
                             "may be a local optimisation's, whose model in problem units is not kept")
        producer = None
        if stream is not None:
            if not on_device:
                raise ValueError("stream goes with device outputs")
            handle = getattr(stream, "cuda_stream", stream)
            if isinstance(handle, bool) or not isinstance(handle, int) or handle < 0:
                raise ValueError("stream must be None, an integer stream handle or an object with .cuda_stream")
            producer = handle or None
        if not isinstance(weighted_stop, (bool, np.bool_)):
            raise ValueError("weighted_stop must be a bool")
        if weighted_stop and weights is None:
            raise ValueError("weighted_stop needs weights: the rule reads their mass over the inlier lists")
        if weighted_stop and step is None:
            raise ValueError("weighted_stop needs step: the rule is read at the adaptive mode's checkpoints")
        h = self._live()
        if self._hyp_error:
            raise ValueError(self._hyp_error.replace("hypothesize", "ransac"))
        wh = None
        if weights is not None:
            if samples is not None:
                raise ValueError("weights go with a budget: given samples are not drawn")
            wh = self._weights_handle(weights)
        if lo_steps is not None:
            if (isinstance(lo_steps, bool) or not isinstance(lo_steps, (int, np.integer))
                    or not 1 <= lo_steps <= L.LO_STEPS_MAX):
                raise ValueError("lo_steps must be None (no LO steps) or an integer in 1..64")
            if lo is None:
                raise ValueError("lo_steps needs lo: the steps start from a local optimisation's model")
        if lo is not None:
            if isinstance(lo, bool) or not isinstance(lo, (int, np.integer)) or not 1 <= lo <= 64:
                raise ValueError("lo must be None (no local optimisation) or an integer in 1..64")
            if samples is not None or step is None:
                raise ValueError("lo needs step and takes no samples: it runs inside the adaptive mode's rounds")
        if step is not None:
            if isinstance(step, bool) or not isinstance(step, (int, np.integer)) or step < 1:
                raise ValueError("step must be None (a fixed budget) or an integer >= 1")
            if samples is not None or budget is None:
                raise ValueError("step needs a budget and takes no samples: the adaptive mode draws its own")
        if (budget is None) == (samples is None):
            raise ValueError("exactly one of budget and samples must be given")
        if isinstance(rounds, bool) or int(rounds) != rounds or not 0 <= rounds <= 64:
            raise ValueError("rounds must be an integer in 0..64")
        for name, val in (("sample_chunk", sample_chunk), ("model_chunk", model_chunk)):
            if isinstance(val, bool) or int(val) != val or val < 0:
                raise ValueError(f"{name} must be a non-negative integer (0: the default)")
        count = len(samples) if samples is not None else (len(self._sizes) if pair_ids is None else len(pair_ids))
        ids, ptr, sizes, offs = self._selection(pair_ids, count, "(types, idx)")
        ns = len(sizes)
        if step is not None:
            budget, seed, share = self._check_draw(budget, seed, point_share, 0)
            if budget > L.RANSAC_ADAPTIVE_MAX_BUDGET:
                raise ValueError("budget must be at most 2^20 in the adaptive mode")
            # (a round obeys the bound a fixed-budget call obeys)
            if ns * min(budget, int(step)) > L.HYPOTHESIZE_MAX_SAMPLES:
                raise ValueError(f"at most 2^22 samples per round, got {ns} pairs x {min(budget, int(step))}")
        elif samples is None:
            budget, seed, share = self._check_draw(budget, seed, point_share, ns)
        R = offs[-1]
        ptrs = {}
        if on_device:
            spans = []
            for name, a, typestrs, dtype, shape, note in (
                    ("out_mask", out_mask, ("|u1", "<u1", "=u1"), np.uint8, (R,), f"R = {R} rows"),
                    ("out_errors", out_errors, ("<f8", "=f8"), np.float64, (3, R), f"R = {R} rows"),
                    ("out_models", out_models, ("<f8", "=f8"), np.float64, (ns, 17), f"{ns} selected pairs"),
                    ("out_index", out_index, ("<i4", "=i4"), np.int32, (ns,), f"{ns} selected pairs"),
                    ("out_counts", out_counts, ("<i4", "=i4"), np.int32, (ns, 3), f"{ns} selected pairs")):
                if a is None:
                    continue
                _, ptr_a = _output_array(a, name, typestrs, dtype, shape, note)
                nbytes = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
                if nbytes > 0:
                    ptrs[name] = ptr_a
                    spans.append((ptr_a, nbytes, name))
            spans.sort()
            for (a0, n0, name0), (a1, _, name1) in zip(spans, spans[1:]):
                if a1 - a0 < n0:
                    raise ValueError(f"{name0} and {name1} overlap")
        if ns == 0:
            return []
        if samples is None:
            so = ty = ix = None
        else:
            soffs, T, I = _concat_samples(self.variant, sizes, samples)
            sample_offsets = np.asarray(soffs, dtype=np.int64)
            so, ty, ix = (sample_offsets.ctypes.data_as(L.c_int64_p), T.ctypes.data_as(L.c_int32_p),
                          I.ctypes.data_as(L.c_int32_p))
            budget, seed, share = -1, 0, -1
        arr = (L.mp_model * ns)()
        res = (L.mp_ransac_result * ns)()
        idx = np.zeros(3 * max(offs[-1], 1), dtype=np.int32)
        stopped = np.zeros(ns, dtype=np.int32)
        info = sinfo = rmass = None
        if on_device or not lists:
            if lo is not None:
                info = (L.mp_ransac_lo_info * ns)()
            if lo_steps is not None:
                sinfo = (L.mp_ransac_lo_steps_info * ns)()
            if weighted_stop:
                rmass = (L.mp_inlier_mass * ns)()
            dev = L.mp_ransac_out()
            dev.mask, dev.errors = ptrs.get("out_mask"), ptrs.get("out_errors")
            dev.models, dev.index, dev.counts = ptrs.get("out_models"), ptrs.get("out_index"), ptrs.get("out_counts")
            dev.producer_stream = producer
            L.check(L.lib().mp_ransac_out_set(h, wh, ns, ptr, budget, 0 if step is None else int(step), seed, share, so,
                                              ty, ix, int(rounds), 0 if lo is None else int(lo),
                                              0 if lo_steps is None else int(lo_steps), 1 if weighted_stop else 0,
                                              arr, res, idx.ctypes.data_as(L.c_int32_p) if lists else None,
                                              stopped.ctypes.data_as(L.c_int32_p), info, sinfo, int(sample_chunk),
                                              int(model_chunk), rmass, ctypes.byref(dev) if on_device else None))
        elif wh is not None and weighted_stop:
            if lo is not None:
                info = (L.mp_ransac_lo_info * ns)()
            if lo_steps is not None:
                sinfo = (L.mp_ransac_lo_steps_info * ns)()
            rmass = (L.mp_inlier_mass * ns)()
            L.check(L.lib().mp_ransac_weighted_stop_set(h, wh, ns, ptr, budget, int(step), seed, share, int(rounds),
                                                        0 if lo is None else int(lo),
                                                        0 if lo_steps is None else int(lo_steps), arr, res,
                                                        idx.ctypes.data_as(L.c_int32_p),
                                                        stopped.ctypes.data_as(L.c_int32_p), info, sinfo,
                                                        int(sample_chunk), int(model_chunk), rmass))
        elif wh is not None:
            if lo is not None:
                info = (L.mp_ransac_lo_info * ns)()
            if lo_steps is not None:
                sinfo = (L.mp_ransac_lo_steps_info * ns)()
            L.check(L.lib().mp_ransac_weighted_set(h, wh, ns, ptr, budget, 0 if step is None else int(step), seed,
                                                   share, int(rounds), 0 if lo is None else int(lo),
                                                   0 if lo_steps is None else int(lo_steps), arr, res,
                                                   idx.ctypes.data_as(L.c_int32_p),
                                                   stopped.ctypes.data_as(L.c_int32_p), info, sinfo,
                                                   int(sample_chunk), int(model_chunk)))
        elif lo is not None and lo_steps is not None:
            info = (L.mp_ransac_lo_info * ns)()
            sinfo = (L.mp_ransac_lo_steps_info * ns)()
            L.check(L.lib().mp_ransac_lo_steps_set(h, ns, ptr, budget, int(step), seed, share, int(rounds), int(lo),
                                                   int(lo_steps), arr, res, idx.ctypes.data_as(L.c_int32_p),
                                                   stopped.ctypes.data_as(L.c_int32_p), info, sinfo,
                                                   int(sample_chunk), int(model_chunk)))
        elif lo is not None:
            info = (L.mp_ransac_lo_info * ns)()
            L.check(L.lib().mp_ransac_lo_set(h, ns, ptr, budget, int(step), seed, share, int(rounds), int(lo), arr,
                                             res, idx.ctypes.data_as(L.c_int32_p),
                                             stopped.ctypes.data_as(L.c_int32_p), info, int(sample_chunk),
                                             int(model_chunk)))
        elif step is not None:
            L.check(L.lib().mp_ransac_adaptive_set(h, ns, ptr, budget, int(step), seed, share, int(rounds), arr, res,
                                                   idx.ctypes.data_as(L.c_int32_p),
                                                   stopped.ctypes.data_as(L.c_int32_p), int(sample_chunk),
                                                   int(model_chunk)))
        else:
            L.check(L.lib().mp_ransac_set(h, ns, ptr, budget, seed, share, so, ty, ix, int(rounds), arr, res,
                                          idx.ctypes.data_as(L.c_int32_p), int(sample_chunk), int(model_chunk)))
        out = []
        for j in range(ns):
            n, q = sizes[j], res[j]
            r = RansacResult()
            r.num_samples, r.num_candidates = int(q.num_samples), int(q.num_candidates)
            r.stopped = bool(stopped[j])
            if rmass is not None:
                r.rule_mass, r.rule_total = tuple(int(v) for v in rmass[j].mass), int(rmass[j].total)
            if info is not None:
                r.lo_runs, r.lo_accepted, r.lo_index = (int(info[j].lo_runs), int(info[j].lo_accepted),
                                                        int(info[j].lo_index))
            if sinfo is not None:
                r.lo_step, r.lo_stage = int(sinfo[j].lo_step), int(sinfo[j].lo_stage)
                r.lo_step_offers, r.lo_step_accepted = (int(sinfo[j].lo_step_offers),
                                                        int(sinfo[j].lo_step_accepted))
            r.index, r.sample, r.slot, r.solver_type = (int(q.best_candidate), int(q.best_sample), int(q.best_slot),
                                                        int(q.best_type))
            r.score_selected = float(q.score_selected)
            r.score_initial, r.score_final = float(q.score_initial), float(q.score_final)
            r.rounds_run, r.rounds_accepted, r.status = int(q.rounds_run), int(q.rounds_accepted), int(q.lm_status)
            r.norm_scale = float(q.norm_scale)
            r.model_row = np.frombuffer(bytes(arr[j]), dtype=np.float64).copy()
            r.model = _model_from_c(arr[j], self.variant) if r.index >= 0 else None
            base = 3 * offs[j]
            r.num_inliers = tuple(int(q.num_inliers[t]) for t in range(3))
            r.inlier_indices = ([idx[base + t * n: base + t * n + q.num_inliers[t]].copy() for t in range(3)]
                                if lists else None)
            r.rows = slice(offs[j], offs[j + 1]) if out_mask is not None else None
            out.append(r)
        return out


class DrawWeights:
    """The confidence weights of one PairSet (PairSet.draw_weights; mp_draw_weights_*): the
    pairs' integer tables on the device, immutable, shared by any number of draw / ransac calls
    on that set.  weighted (bool), positive (the number of correspondences with q > 0) and total
    (the sum of the q) hold one entry per pair.  Use as a context manager, or close() (idempotent);
    closing the PairSet first is fine.  A call with closed weights, or with the weights of another
    set, raises ValueError."""

    def __init__(self, pair_set, handle, num_pairs):
        self._set, self._h = pair_set, handle
        wt, pos = np.zeros(max(num_pairs, 1), dtype=np.int32), np.zeros(max(num_pairs, 1), dtype=np.int32)
        tot = np.zeros(max(num_pairs, 1), dtype=np.uint32)
        L.check(L.lib().mp_draw_weights_info(handle, wt.ctypes.data_as(L.c_int32_p), pos.ctypes.data_as(L.c_int32_p),
                                             tot.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))))
        self.weighted = wt[:num_pairs] != 0
        self.positive = pos[:num_pairs].copy()
        self.total = tot[:num_pairs].astype(np.int64)

    def close(self):
        """Release the tables; idempotent."""
        h, self._h = getattr(self, "_h", None), None
        if h is not None:
            L.check(L.lib().mp_draw_weights_destroy(h))

    def __enter__(self):
        if self._h is None:
            raise ValueError("the DrawWeights is closed")
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:  # (interpreter teardown)
            pass

    def _live(self, pair_set):
        if getattr(self, "_h", None) is None:
            raise ValueError("the DrawWeights is closed")
        if pair_set is not self._set:
            raise ValueError("the weights belong to another PairSet")
        return self._h


class InlierMass:
    """One entry's outcome of PairSet.inlier_mass: mass (three ints, the weight mass of the
    model's three inlier lists), total (the pair's weight total, or its size when the pair is
    not weighted), count (the lists' lengths) and weighted."""

    def __init__(self, mass=(0, 0, 0), total=0, count=(0, 0, 0), weighted=False):
        self.mass, self.total, self.count, self.weighted = mass, total, count, weighted

    def __repr__(self):
        return f"InlierMass(mass={self.mass} of {self.total}, count={self.count}, weighted={self.weighted})"


class ResidualsResult:
    """PairSet.residuals' outcome: offsets ((ne + 1,) int64: entry e owns rows offsets[e] ..
    offsets[e + 1] - 1), counts ((ne, 3) int32: the entry's rows with bit t set), mask ((R,)
    uint8, bits 0 .. 2: the row is an inlier of term t; a numpy array or the object passed as
    out_mask) and errors ((3, R) float64 in problem units, the object passed as out_errors, or
    None when not asked for)."""

    def __init__(self):
        self.offsets = None
        self.counts = None
        self.mask = None
        self.errors = None

    def rows(self, e):
        """The rows of entry e, as a slice of mask and of errors' second axis."""
        return slice(int(self.offsets[e]), int(self.offsets[e + 1]))

    def __repr__(self):
        return f"ResidualsResult(entries={len(self.counts)}, rows={int(self.offsets[-1])})"


INFORMATION_PARAMETERS = ("rot0", "rot1", "rot2", "t0", "t1", "t2", "scale", "offset0", "offset1", "focal0", "focal1")


class InformationResult:
    """PairSet.information's outcome, one row per entry, in problem units and in the layout of
    INFORMATION_PARAMETERS: H ((ne, 66) packed upper triangle of J^T J), g ((ne, 11) J^T r), cost
    ((ne,) sum r^2 / 2), cov ((ne, 11, 11) the inverse of H on the active parameters, or None when
    not asked for) -- numpy arrays, or the objects passed as out_* -- and, always numpy: col ((ne,
    11) the active mask), pd (1 inverted, 0 not positive definite, -1 nothing evaluated), status
    (1: at least one block), rows (2 (n0 + n1) + n2 after gating), counts ((ne, 3) residuals'
    counts), norm_scale (the entry's pair's) and focal_columns (the variant's focal parameters)."""

    def __init__(self):
        self.H = self.g = self.cost = self.cov = None
        self.col = self.pd = self.status = self.rows = self.counts = None
        self.norm_scale = None
        self.focal_columns = ()

    @staticmethod
    def _host(a, name):
        if not isinstance(a, np.ndarray):
            raise ValueError(f"{name} is not a host array of this result"
                             + ("" if a is None else ": copy the device array to the host first"))
        return a

    def active(self, e):
        """The indices of entry e's active parameters."""
        return np.flatnonzero(self.col[e])

    def matrix(self, e):
        """The full symmetric 11 x 11 H of entry e."""
        Hp = self._host(self.H, "H")[e]
        M = np.zeros((11, 11))
        M[np.triu_indices(11)] = Hp
        return M + np.triu(M, 1).T

    def covariance(self, e, scaled=True):
        """The covariance of entry e's active parameters (in active(e)'s order), symmetrised
        (C + C^T) / 2.  scaled: in user units and with the a-posteriori variance factor -- a
        focal's row and column times norm_scale per index, everything times 2 cost / (rows -
        n); scaled=False: the inverse of H in problem units.  ValueError when the inverse was
        not formed (pd != 1) or, with scaled, rows <= n."""
        C = self._host(self.cov, "cov")[e]
        if self.pd[e] != 1:
            raise ValueError(f"entry {e} has no covariance: pd = {int(self.pd[e])}")
        act = self.active(e)
        n = len(act)
        C = C[np.ix_(act, act)]
        C = (C + C.T) / 2
        if scaled:
            if self.rows[e] <= n:
                raise ValueError(f"entry {e} has {int(self.rows[e])} rows for {n} parameters: no variance factor")
            s = np.array([self.norm_scale[e] if a in self.focal_columns else 1.0 for a in act])
            C = C * np.outer(s, s) * (2.0 * float(self._host(self.cost, "cost")[e]) / (int(self.rows[e]) - n))
        return C

    def __repr__(self):
        return f"InformationResult(entries={len(self.pd)})"


def information_finish(H, g, col):
    """The finishing arithmetic of PairSet.information on the host -- test hook
    (mp_debug_information_finish; no device): (H, g, cov, pd) with H (66) and g (11) masked by
    col (11) and cov (11, 11) the inverse on the active set, pd 1 or 0."""
    H = np.array(H, dtype=np.float64).reshape(66)
    g = np.array(g, dtype=np.float64).reshape(11)
    c = np.ascontiguousarray(np.asarray(col).reshape(11) != 0, dtype=np.int32)
    cov = np.zeros((11, 11))
    pd = ctypes.c_int32(-2)
    L.check(L.lib().mp_debug_information_finish(_dp(H), _dp(g), c.ctypes.data_as(L.c_int32_p), _dp(cov),
                                                ctypes.byref(pd)))
    return H, g, cov, int(pd.value)


class LsqFitResult:
    """One entry's outcome of PairSet.lsq_fit: score and num_inliers (of the given model),
    num_wide, subset_sizes, status (3: skipped; else the LM's: 1 refined), model and model_row
    (user units: the LM's on status 1, else the given model's bytes), subsets (with_subsets
    only: the subset's three int32 index arrays; None otherwise)."""

    def __init__(self):
        self.score = 0.0
        self.num_inliers = [0, 0, 0]
        self.num_wide = [0, 0, 0]
        self.subset_sizes = [0, 0, 0]
        self.status = -1
        self.model = None
        self.model_row = np.zeros(17)
        self.subsets = None

    def __repr__(self):
        return (f"LsqFitResult(score {self.score:.6g}, inliers={self.num_inliers}, wide={self.num_wide}, "
                f"subset={self.subset_sizes}, status={self.status})")


class RansacResult:
    """One pair's outcome of PairSet.ransac: num_samples, num_candidates; index (the winner
    among the pair's candidates; -1: none), sample and slot (its origin), solver_type (0 the
    MD solver, 1 the point solver); score_selected (select's score; DBL_MAX without a winner);
    score_initial, score_final, rounds_run, rounds_accepted, status (refine's; without a
    winner or with rounds = 0: status -1, no round, score_final = score_selected); model (a
    pose object in user units, None without a winner) and model_row (its 17 doubles in mp_model
    order, zeros without a winner); inlier_indices (three int32 arrays, the returned
    model's); norm_scale; stopped (the adaptive mode only: the termination rule ended the
    pair before its budget; False otherwise); lo_runs, lo_accepted, lo_index (ransac(lo=...)
    only: local optimisations run, those that became the overall best, and the candidate
    whose local optimisation gave the returned start model; 0, 0 and -1 otherwise); lo_step,
    lo_stage, lo_step_offers, lo_step_accepted (ransac(lo_steps=...) only: the LO step and stage
    that produced the returned start model, -1 when no step did, and the steps' offers to the
    overall best and those accepted; -1, -1, 0 and 0 otherwise); rule_mass, rule_total
    (ransac(weighted_stop=True) only: the three weight masses and the total the termination rule
    last read for the pair; None and 0 otherwise); num_inliers (a tuple of 3: the lengths of the
    returned model's three lists, also with ransac(lists=False), where inlier_indices is None);
    rows (ransac(out_mask=...) only: the pair's slice of out_mask and of out_errors' second axis;
    None otherwise)."""

    def __init__(self):
        self.num_samples = self.num_candidates = 0
        self.stopped = False
        self.lo_runs = self.lo_accepted = 0
        self.lo_index = -1
        self.lo_step = self.lo_stage = -1
        self.lo_step_offers = self.lo_step_accepted = 0
        self.rule_mass, self.rule_total = None, 0
        self.index = self.sample = self.slot = self.solver_type = -1
        self.score_selected = self.score_initial = self.score_final = float(np.finfo(np.float64).max)
        self.rounds_run = self.rounds_accepted = 0
        self.status = -1
        self.model = None
        self.model_row = np.zeros(17)
        self.inlier_indices = [np.zeros(0, dtype=np.int32) for _ in range(3)]
        self.num_inliers = (0, 0, 0)
        self.rows = None
        self.norm_scale = 1.0

    def __repr__(self):
        return (f"RansacResult(index={self.index} of {self.num_candidates}, score {self.score_selected:.6g} -> "
                f"{self.score_final:.6g}, rounds {self.rounds_accepted}/{self.rounds_run}, status={self.status}, "
                f"inliers={list(self.num_inliers)})")


def score_models(variant, x0, x1, depth0, depth1, cam0, cam1, options, est_config, models, with_errors=False,
                 host_lo=False, fast_bounds=None):
    """Device ScoreModel over explicit models given in problem units (tests / diagnostics).
    host_lo=True: the engine's host LO sweep instead (mp_debug_lo_sweep; no device);
    fast_bounds (host_lo only): an (nm, 2) float64 array filled with the LO's fast sums
    and their bounds (lo_sweep.h lo_sweep_fast)."""
    x0 = _pts(x0, "x0")
    x1 = _pts(x1, "x1")
    n = x0.shape[0]
    d0 = _vec(depth0, n, "depth0")
    d1 = _vec(depth1, n, "depth1")
    c0 = np.ascontiguousarray(np.asarray(cam0, dtype=np.float64).reshape(-1))
    c1 = np.ascontiguousarray(np.asarray(cam1, dtype=np.float64).reshape(-1))
    nm = len(models)
    arr = (L.mp_model * max(nm, 1))(*[_model_to_c(m, variant) for m in models])
    scores = np.zeros(max(nm, 1))
    errors = np.zeros((max(nm, 1), 3, n)) if with_errors else None
    o = options._to_c()
    c = (est_config or EstimatorConfig())._to_c()
    if host_lo:
        code = L.lib().mp_debug_lo_sweep(variant, n, _dp(x0), _dp(x1), _dp(d0), _dp(d1), _dp(c0), _dp(c1),
                                         ctypes.byref(o), ctypes.byref(c), arr, nm, _dp(scores),
                                         _dp(errors) if with_errors else None,
                                         _dp(fast_bounds) if fast_bounds is not None else None)
    else:
        code = L.lib().mp_score_models(variant, n, _dp(x0), _dp(x1), _dp(d0), _dp(d1), _dp(c0), _dp(c1),
                                       ctypes.byref(o), ctypes.byref(c), arr, nm, _dp(scores),
                                       _dp(errors) if with_errors else None, _DEFAULT_DEVICE)
    L.check(code)
    return (scores[:nm], errors[:nm]) if with_errors else scores[:nm]


def debug_score_batch(variant, x0, x1, depth0, depth1, cam0, cam1, options, est_config, iterations, best,
                      exit=True, record_skip=True):
    """The estimator's scoring kernel on explicit per-iteration model lists (test hook,
    mp_debug_score_batch).  iterations: list of model lists (problem units).  Returns
    (best scores, slots with the ambiguity / uncertainty bits, record models, bounds):
    bounds["hi"], bounds["lo"] per iteration and bounds["tie"][b][m], each model's
    screening margin (mp_score.h score_margins)."""
    x0 = _pts(x0, "x0")
    x1 = _pts(x1, "x1")
    n = x0.shape[0]
    d0 = _vec(depth0, n, "depth0")
    d1 = _vec(depth1, n, "depth1")
    c0 = np.ascontiguousarray(np.asarray(cam0, dtype=np.float64).reshape(-1))
    c1 = np.ascontiguousarray(np.asarray(cam1, dtype=np.float64).reshape(-1))
    M = {0: 10, 1: 16, 2: 4, 3: 10}[variant]
    B = len(iterations)
    arr = (L.mp_model * (B * M))()
    counts = np.zeros(B, dtype=np.int32)
    for b, ms in enumerate(iterations):
        counts[b] = len(ms)
        for m, mod in enumerate(ms):
            arr[b * M + m] = _model_to_c(mod, variant)
    rb = np.zeros(B)
    rs = np.zeros(B, dtype=np.int32)
    rec = (L.mp_model * B)()
    hilo = np.zeros(2 * B)
    ties = np.zeros(B * M)
    o = options._to_c()
    c = (est_config or EstimatorConfig())._to_c()
    flags = (1 if exit else 0) | (2 if record_skip else 0)
    L.check(L.lib().mp_debug_score_batch(variant, n, _dp(x0), _dp(x1), _dp(d0), _dp(d1), _dp(c0), _dp(c1),
                                         ctypes.byref(o), ctypes.byref(c), B, counts.ctypes.data_as(L.c_int32_p),
                                         arr, float(best), flags, _dp(rb), rs.ctypes.data_as(L.c_int32_p), rec,
                                         _dp(hilo), _dp(ties), _DEFAULT_DEVICE))
    bounds = {"hi": hilo[0::2].copy(), "lo": hilo[1::2].copy(),
              "tie": [ties[b * M:b * M + counts[b]].copy() for b in range(B)]}
    return rb, rs, [_model_from_c(rec[b], variant) for b in range(B)], bounds


def debug_score_terms(variant, x0, x1, depth0, depth1, cam0, cam1, options, est_config, models):
    """score_batch's per-correspondence errors of explicit models (test hook,
    mp_debug_score_terms).  Returns (errors [nm x 3 x n], flags [nm x n], taus [nm x 3],
    ties [nm])."""
    x0 = _pts(x0, "x0")
    x1 = _pts(x1, "x1")
    n = x0.shape[0]
    d0 = _vec(depth0, n, "depth0")
    d1 = _vec(depth1, n, "depth1")
    c0 = np.ascontiguousarray(np.asarray(cam0, dtype=np.float64).reshape(-1))
    c1 = np.ascontiguousarray(np.asarray(cam1, dtype=np.float64).reshape(-1))
    nm = len(models)
    arr = (L.mp_model * max(nm, 1))()
    for m, mod in enumerate(models):
        arr[m] = _model_to_c(mod, variant)
    err = np.zeros(max(nm, 1) * 3 * n)
    flags = np.zeros(max(nm, 1) * n, dtype=np.int32)
    taus = np.zeros(max(nm, 1) * 3)
    ties = np.zeros(max(nm, 1))
    o = options._to_c()
    c = (est_config or EstimatorConfig())._to_c()
    L.check(L.lib().mp_debug_score_terms(variant, n, _dp(x0), _dp(x1), _dp(d0), _dp(d1), _dp(c0), _dp(c1),
                                         ctypes.byref(o), ctypes.byref(c), arr, nm, _dp(err),
                                         flags.ctypes.data_as(L.c_int32_p), _dp(taus), _dp(ties), _DEFAULT_DEVICE))
    return (err[:nm * 3 * n].reshape(nm, 3, n), flags[:nm * n].reshape(nm, n), taus[:3 * nm].reshape(nm, 3),
            ties[:nm])


def debug_score_margins(variant, x0, x1, depth0, depth1, cam0, cam1, options, est_config, models):
    """The screening margins of explicit models, formed on the host (test hook,
    mp_debug_score_margins; no device).  Returns (per model: dict of taus [nm x 3], wz0,
    wz1, wl, kg2, tie [nm each]; per pair: dict of thr [3], w [3], norm_scale, loss_scale,
    kstd)."""
    x0 = _pts(x0, "x0")
    x1 = _pts(x1, "x1")
    n = x0.shape[0]
    d0 = _vec(depth0, n, "depth0")
    d1 = _vec(depth1, n, "depth1")
    c0 = np.ascontiguousarray(np.asarray(cam0, dtype=np.float64).reshape(-1))
    c1 = np.ascontiguousarray(np.asarray(cam1, dtype=np.float64).reshape(-1))
    nm = len(models)
    arr = (L.mp_model * max(nm, 1))(*[_model_to_c(m, variant) for m in models])
    pm = np.zeros((max(nm, 1), 8))
    pp = np.zeros(9)
    o = options._to_c()
    c = (est_config or EstimatorConfig())._to_c()
    L.check(L.lib().mp_debug_score_margins(variant, n, _dp(x0), _dp(x1), _dp(d0), _dp(d1), _dp(c0), _dp(c1),
                                           ctypes.byref(o), ctypes.byref(c), arr, nm, _dp(pm), _dp(pp)))
    pm = pm[:nm]
    per_model = {"taus": pm[:, 0:3].copy(), "wz0": pm[:, 3].copy(), "wz1": pm[:, 4].copy(), "wl": pm[:, 5].copy(),
                 "kg2": pm[:, 6].copy(), "tie": pm[:, 7].copy()}
    per_pair = {"thr": pp[0:3].copy(), "w": pp[3:6].copy(), "norm_scale": float(pp[6]), "loss_scale": float(pp[7]),
                "kstd": int(pp[8])}
    return per_model, per_pair


def device_count():
    return int(L.lib().mp_device_count())


def version():
    return L.lib().mp_version().decode()


def profile_enable(on=True):
    """Turn on HIP-event timing of the estimator's batch kernels (process-wide)."""
    L.check(L.lib().mp_profile_enable(1 if on else 0))


def profile_reset():
    L.check(L.lib().mp_profile_reset())


def profile_read():
    """Totals since the last reset: batches, iterations, hypotheses, correspondences,
    sweeps, solve_ms, score_ms (device time from HIP events on the engine stream)."""
    p = L.mp_kernel_profile()
    L.check(L.lib().mp_profile_read(ctypes.byref(p)))
    return {name: getattr(p, name) for name, _ in p._fields_}
