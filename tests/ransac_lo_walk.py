"""Restatements behind the local-optimisation tests (tests/test_ransac_lo_cpu.py,
tests/test_ransac_lo_gpu.py), from entries that exist without the feature wherever they can:

* Track: the two-track bookkeeping of mp_ransac_lo_set (host/ransac_lo_track.h) on plain
  numbers.
* refine_relaxed_single: tests/refine_cases.py refine_single with round 0 on the relaxed lists
  err[t] < thr[t] * threshold_multiplier, from score_models(with_errors=True) and
  lm_refine_batch (kind 0).
* lo_walk: PairSet.ransac(step=, lo=) for one pair as a walk over public entries."""
import numpy as np

import madpose
from tests import refine_cases as RC

DBL_MAX = float(np.finfo(np.float64).max)


class Track:
    """The overall best of a pair: score, counts, lo_index, the counters, and source (0 none,
    1 a minimal model, 2 a local optimisation's result).  Every test is a strict `<`, so equal
    and NaN scores replace nothing."""

    def __init__(self):
        self.score, self.counts = DBL_MAX, (0, 0, 0)
        self.lo_index, self.lo_runs, self.lo_accepted, self.source = -1, 0, 0, 0

    def take_minimal(self, score, counts):
        if not score < self.score:
            return False
        self.score, self.counts, self.lo_index, self.source = score, tuple(counts), -1, 1
        return True

    def take_refined(self, candidate, rounds_accepted, score_final, counts):
        self.lo_runs += 1
        if rounds_accepted < 1 or not score_final < self.score:
            return False
        self.score, self.counts, self.lo_index, self.source = score_final, tuple(counts), candidate, 2
        self.lo_accepted += 1
        return True


def refine_relaxed_single(variant, p, m_user, o, c, rounds, norm_scale, on_host=False):
    """PairSet.refine(relax=True) for one pair from the single-pair entries.  on_host: the
    host's sweep and LM instead of the device's (no GPU; for choosing cases, not for bytes).
    Beside refine_single's fields: tight0 / wide0 (the start model's tight and relaxed list
    lengths) and accepted (the rounds that were accepted)."""
    e = RC.Expected()
    e.rounds_run = e.rounds_accepted = 0
    e.status = -1
    e.model = m_user
    e.accepted = []
    n = len(p["depth0"])
    if n == 0:
        e.score_initial = e.score_final = 0.0
        e.lists = [np.zeros(0, dtype=np.int32)] * 3
        e.tight0 = e.wide0 = (0, 0, 0)
        e.rounds_run, e.status = 1, 3
        return e
    args = RC.pair_args(variant, p)
    thr = RC.thresholds(variant, o, norm_scale)
    wide_thr = [t * float(o.threshold_multiplier) for t in thr]  # one product, rounded once

    def sweep(m):
        s, err = madpose.score_models(variant, *args[:4], *args[5:], o, c, [m], with_errors=True, host_lo=on_host)
        return (float(s[0]), [np.flatnonzero(err[0, t] < thr[t]).astype(np.int32) for t in range(3)],
                [np.flatnonzero(err[0, t] < wide_thr[t]).astype(np.int32) for t in range(3)])

    cur = RC.to_problem_units(variant, m_user, norm_scale)
    score, lists, wide = sweep(cur)
    e.score_initial = score
    e.tight0, e.wide0 = tuple(len(a) for a in lists), tuple(len(a) for a in wide)
    for r in range(rounds):
        e.rounds_run += 1
        (cand, st), = madpose.lm_refine_batch(variant, *args, o, c, [(0, wide if r == 0 else lists, cur)],
                                              on_host=on_host)
        e.status = st
        if st != 1:
            break
        s2, l2, _ = sweep(cand)
        if not s2 < score:
            break
        cur, score, lists = cand, s2, l2
        e.rounds_accepted += 1
        e.accepted.append(r)
    e.score_final = score
    e.lists = lists
    if e.rounds_accepted:
        e.model = RC.to_user_units(variant, cur, norm_scale)
    return e


class Walked:
    pass


def lo_walk(ps, p, n, types, marks, seed, lo, rounds, required, stop_reached, cache):
    """ransac(budget, step, lo, rounds, pair_ids=[p]) as a walk over the checkpoints `marks`.
    lo None: the walk without local optimisation (the rule on the minimal best).  required(n,
    counts) -> (req0, req1) and stop_reached(req, drawn) are the rule's restatement; cache: a
    dict that keeps ransac(budget=m, rounds=0, pair_ids=[p]) between walks.  Returns the
    expected fields; w.trace lists (checkpoint, replaced, took_minimal, took_refined)."""
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
            cache[(p, m)], = ps.ransac(budget=m, seed=seed, rounds=0, pair_ids=[p])
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
            if lo is not None:
                f, = ps.refine([r.model], rounds=lo, relax=True, pair_ids=[p])
                took_lo = T.take_refined(r.index, f.rounds_accepted, f.score_final,
                                         [len(a) for a in f.inlier_indices])
                if took_lo:
                    best_model, best_lists = f.model, f.inlier_indices
        w.trace.append((m, replaced, took_min, took_lo))
        d1 = int(types[:m].sum())
        if stop_reached(required(n, list(T.counts) if T.source else None), (m - d1, d1)):
            w.stopped = True
            break
    w.track = T
    w.num_samples = w.minimal.num_samples if w.minimal is not None else 0
    w.model, w.lists = best_model, best_lists
    w.score_initial = w.score_final = T.score
    w.rounds_run = w.rounds_accepted = 0
    w.status = -1
    if best_model is not None and rounds >= 1:
        f, = ps.refine([best_model], rounds=rounds, pair_ids=[p])
        w.model, w.lists = f.model, f.inlier_indices
        w.score_initial, w.score_final = f.score_initial, f.score_final
        w.rounds_run, w.rounds_accepted, w.status = f.rounds_run, f.rounds_accepted, f.status
    return w
