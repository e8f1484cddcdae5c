"""Restatements behind the weighted stopping rule's tests (tests/test_weighted_stop_cpu.py,
tests/test_weighted_stop_gpu.py), from entries that exist without the feature wherever they can:

* required_mass: the rule on (total, mass) in the style of tests/ransac_stop_restatement.py --
  the same function with r[t] = mass[t] / total (math.pow / log / ceil are the C library's).
* model_mass: the mass of a model as the sum of the restated q (weighted_draw_restatement.quantise)
  over the lists ps.select([[m]], pair_ids=[p]) returns, or the lists' lengths over n for a pair
  that is not weighted.
* step_walk, lo_walk, lo_steps_walk: PairSet.ransac(step=, [lo=, [lo_steps=]], weighted_stop=True)
  for one pair as walks over public entries: tests/ransac_lo_walk.py lo_walk and
  tests/lsq_subset_restatement.py lo_steps_walk restated with the one line that calls the rule
  replaced -- the rule reads the restated mass of the overall best's model."""
import copy
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ransac_stop_restatement as S  # noqa: E402
import weighted_draw_restatement as WD  # noqa: E402
from tests.lsq_subset_restatement import StepTrack, step_factor, step_substream, subset_size  # noqa: E402
from tests.ransac_lo_walk import Track, Walked  # noqa: E402


def required_mass(variant, total, mass, sp, mn, mx):
    """req[0] (the MD solver) and req[1] (the point solver) for a pair whose weights sum to
    total and whose rule model's lists have the masses mass (None: no winner)."""
    out = []
    for ss in ((S.K_MD[variant], S.K_MD[variant], 0), (0, 0, S.K_PT[variant])):
        p_all = 1.0
        for t in range(3):
            r = float(mass[t]) / float(total) if total > 0 and mass is not None else 0.0
            p_all *= math.pow(r, float(ss[t]))
        if p_all <= 0.0:
            out.append(mx)
            continue
        if p_all >= 1.0:
            out.append(mn)
            continue
        p_bad = 1.0 - p_all
        if p_bad >= 0.99999999999999:
            out.append(mx)
            continue
        num = math.log(1.0 - sp) if sp < 1.0 else -math.inf  # (C: log(0) = -inf)
        it = num / math.log(p_bad) + 0.5
        it = float(math.ceil(it)) if math.isfinite(it) else it
        val = int(it) if it < mx else mx  # the clamp, in double
        out.append(max(mn, val))
    return out


class PairWeights:
    """What the rule knows of one pair: q (int64 per row; None: the pair is not weighted -- it
    was given no weights or it fell back) and total (W, or n)."""

    def __init__(self, variant, n, weights):
        self.n, self.q, self.total = n, None, n
        if weights is not None:
            assert n <= WD.MAX_N
            q = WD.quantise(weights)
            if WD.is_weighted(variant, n, int((q > 0).sum())):
                self.q, self.total = q, int(q.sum())

    @property
    def weighted(self):
        return self.q is not None

    def mass_of(self, lists):
        """(mass, count) of three index lists"""
        count = tuple(len(a) for a in lists)
        if self.q is None:
            return count, count
        return tuple(int(self.q[np.asarray(a, dtype=np.int64)].sum()) for a in lists), count


def model_mass(ps, p, model, pw):
    """(mass, count) of model m of pair p: over the lists select returns for the single candidate
    (a model that select refuses as a winner -- a NaN score -- has empty lists)"""
    sr, = ps.select([[model]], pair_ids=[p])
    lists = sr.inlier_indices if sr.index == 0 else [np.zeros(0, dtype=np.int32)] * 3
    return pw.mass_of(lists)


class Rule:
    """the weighted rule of one pair for the walks: read(model) -> (req0, req1), keeping what it
    last read in .mass (zeros before a winner)"""

    def __init__(self, ps, p, pw, variant, o):
        self.ps, self.p, self.pw, self.variant = ps, p, pw, variant
        self.opts = (o.success_probability, o.min_num_iterations, o.max_num_iterations_per_solver)
        self.mass, self.count = (0, 0, 0), (0, 0, 0)
        self._model = None

    def read(self, model):
        if model is None:
            return required_mass(self.variant, self.pw.total, None, *self.opts)
        if model is not self._model:
            self.mass, self.count = model_mass(self.ps, self.p, model, self.pw)
            self._model = model
        return required_mass(self.variant, self.pw.total, self.mass, *self.opts)


def step_walk(ps, p, types, marks, seed, rule, cache, weights):
    """ransac(budget, step, rounds=0, pair_ids=[p], weights=w, weighted_stop=True): the stop point.
    Returns (num_samples, stopped, the minimal result at the stop)."""
    r, stopped = None, False
    if len(types) == 0:
        marks = []
    for m in marks:
        if (p, m) not in cache:
            cache[(p, m)], = ps.ransac(budget=m, seed=seed, rounds=0, pair_ids=[p], weights=weights)
        r = cache[(p, m)]
        assert r.num_samples == m
        d1 = int(types[:m].sum())
        if S.stop_reached(rule.read(r.model if r.index >= 0 else None), (m - d1, d1)):
            stopped = True
            break
    return (r.num_samples if r is not None else 0), stopped, r


def lo_walk(ps, p, types, marks, seed, lo, rounds, rule, cache, weights):
    """tests/ransac_lo_walk.py lo_walk with the weighted rule on the overall best's model"""
    w = Walked()
    T = Track()
    w.trace = []
    w.stopped, w.minimal = False, None
    best_model, best_lists = None, [np.zeros(0, dtype=np.int32)] * 3
    last_index = -1
    if len(types) == 0:
        marks = []
    for m in marks:
        if (p, m) not in cache:
            cache[(p, m)], = ps.ransac(budget=m, seed=seed, rounds=0, pair_ids=[p], weights=weights)
        r = cache[(p, m)]
        assert r.num_samples == m
        w.minimal = r
        replaced = r.index != last_index
        took_min = took_lo = False
        if replaced:
            last_index = r.index
            counts = [len(a) for a in r.inlier_indices]
            took_min = T.take_minimal(r.score_selected, counts)
            if took_min:
                best_model, best_lists = r.model, r.inlier_indices
            f, = ps.refine([r.model], rounds=lo, relax=True, pair_ids=[p])
            took_lo = T.take_refined(r.index, f.rounds_accepted, f.score_final, [len(a) for a in f.inlier_indices])
            if took_lo:
                best_model, best_lists = f.model, f.inlier_indices
        w.trace.append((m, replaced, took_min, took_lo))
        d1 = int(types[:m].sum())
        if S.stop_reached(rule.read(best_model if T.source else None), (m - d1, d1)):  # <- the rule
            w.stopped = True
            break
    w.track = T
    w.num_samples = w.minimal.num_samples if w.minimal is not None else 0
    w.model, w.lists = best_model, best_lists
    w.score_initial = w.score_final = T.score
    w.rounds_run = w.rounds_accepted = 0
    w.status = -1
    w.rule_mass, w.rule_count = rule.mass, rule.count
    if best_model is not None and rounds >= 1:
        f, = ps.refine([best_model], rounds=rounds, pair_ids=[p])
        w.model, w.lists = f.model, f.inlier_indices
        w.score_initial, w.score_final = f.score_initial, f.score_final
        w.rounds_run, w.rounds_accepted, w.status = f.rounds_run, f.rounds_accepted, f.status
    return w


def lo_steps_walk(ps, p, types, marks, seed, lo, lo_steps, rounds, rule, cache, weights, Q, lam, nu):
    """tests/lsq_subset_restatement.py lo_steps_walk with the weighted rule on the overall best's
    model"""
    w = Walked()
    T, ST = Track(), StepTrack()
    w.trace, w.stage0 = [], []
    w.stopped, w.minimal = False, None
    best_model, best_lists = None, [np.zeros(0, dtype=np.int32)] * 3
    best_from_step = False
    last_index = -1
    if len(types) == 0:
        marks = []
    for m in marks:
        if (p, m) not in cache:
            cache[(p, m)], = ps.ransac(budget=m, seed=seed, rounds=0, pair_ids=[p], weights=weights)
        r = cache[(p, m)]
        assert r.num_samples == m
        w.minimal = r
        replaced = r.index != last_index
        if replaced:
            last_index = r.index
            counts = [len(a) for a in r.inlier_indices]
            if T.take_minimal(r.score_selected, counts):
                ST.clear()
                best_model, best_lists, best_from_step = r.model, r.inlier_indices, False
            f, = ps.refine([r.model], rounds=lo, relax=True, pair_ids=[p])
            if T.take_refined(r.index, f.rounds_accepted, f.score_final, [len(a) for a in f.inlier_indices]):
                ST.clear()
                best_model, best_lists, best_from_step = f.model, f.inlier_indices, False
            a, c, s = f.model, r.index, r.solver_type
            live = list(range(lo_steps))
            cur = [a] * lo_steps
            for q in range(0, 2 + Q):
                if not live:
                    break
                fac = 1.0 if q < 2 else step_factor(q - 2, Q, lam)
                out = ps.lsq_fit(cur, [s] * len(live), factor=fac, rule="nonmin" if q == 0 else "lsq", seed=seed,
                                 streams=[c] * len(live), substreams=[step_substream(rr, q) for rr in live],
                                 pair_ids=[p] * len(live))
                if q == 0:
                    w.stage0 += [(sum(g.num_wide), subset_size("nonmin", s, ps.variant, 1, nu, g.num_wide)[1])
                                 for g in out]
                    keep = [i for i, g in enumerate(out) if g.status == 1]
                    live = [live[i] for i in keep]
                    cur = [out[i].model for i in keep]
                    continue
                for i, g in enumerate(out):
                    if ST.offer(T, c, live[i], q - 1, g.score, g.num_inliers):
                        best_model, best_from_step = cur[i], True
                cur = [g.model for g in out]
            if live:
                sr, = ps.select([cur], pair_ids=[p])
                if sr.index >= 0 and ST.offer(T, c, live[sr.index], 2 + Q, sr.score,
                                              [len(x) for x in sr.inlier_indices]):
                    best_model, best_from_step = cur[sr.index], True
        w.trace.append((m, replaced))
        d1 = int(types[:m].sum())
        if S.stop_reached(rule.read(best_model if T.source else None), (m - d1, d1)):  # <- the rule
            w.stopped = True
            break
    w.track, w.steps = T, ST
    w.num_samples = w.minimal.num_samples if w.minimal is not None else 0
    if best_from_step:
        sr, = ps.select([[best_model]], pair_ids=[p])
        assert sr.index == 0 and np.float64(sr.score).tobytes() == np.float64(T.score).tobytes()
        best_lists = sr.inlier_indices
    w.model, w.lists = best_model, best_lists
    w.score_initial = w.score_final = T.score
    w.rounds_run = w.rounds_accepted = 0
    w.status = -1
    w.rule_mass, w.rule_count = rule.mass, rule.count
    if best_model is not None and rounds >= 1:
        f, = ps.refine([best_model], rounds=rounds, pair_ids=[p])
        w.model, w.lists = f.model, f.inlier_indices
        w.score_initial, w.score_final = f.score_initial, f.score_final
        w.rounds_run, w.rounds_accepted, w.status = f.rounds_run, f.rounds_accepted, f.status
    return w


def finish(ps, p, w0, rounds):
    """a walk made with rounds = 0, with the final `rounds` applied to its overall best (the walks'
    own last step): the loop does not depend on rounds, so one walk serves every value"""
    w = copy.copy(w0)
    if w.model is not None and rounds >= 1:
        f, = ps.refine([w.model], rounds=rounds, pair_ids=[p])
        w.model, w.lists = f.model, f.inlier_indices
        w.score_initial, w.score_final = f.score_initial, f.score_final
        w.rounds_run, w.rounds_accepted, w.status = f.rounds_run, f.rounds_accepted, f.status
    return w
