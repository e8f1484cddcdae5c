"""Restatements behind the LO-step tests (tests/test_ransac_lo_steps_cpu.py,
tests/test_ransac_lo_steps_gpu.py), from entries that exist without the feature wherever they
can:

* subset_keys / subset_select / subset_size: the subset rule of
  madpose_amd/csrc/include/mp_subset.h in plain numpy and Python integers (Philox from
  tests/draw_restatement.py).  Nothing here calls the library.
* step_factor / step_substream: the thresholds' schedule and the stream packing of
  madpose_amd/csrc/host/ransac_lo_steps.h.
* lsq_fit_single: PairSet.lsq_fit for one entry from score_models(with_errors=True), the
  thresholds, the Python subset and lm_refine_batch (kind 0 / 1) on the subset.
* lo_steps_walk: PairSet.ransac(step=, lo=, lo_steps=) for one pair as a walk over public
  entries: tests/ransac_lo_walk.py lo_walk with the stages of the steps."""
import numpy as np

import madpose
from tests import refine_cases as RC
from tests.draw_restatement import philox4x32_10
from tests.ransac_lo_walk import Track, Walked

MASK_ALL = (1 << 64) - 1
MASK_TOP_BYTE = 0xFF << 56
RULES = {"lsq": 0, "nonmin": 1}


# ---- the subset rule ----

def subset_keys(seed, pair, stream, substream, t, idx):
    """the 64-bit keys of the elements (t, i), i in idx: a uint64 array"""
    idx = np.asarray(idx, dtype=np.uint64)
    w = philox4x32_10(idx, np.uint64((substream << 2) | t), np.uint64(pair), np.uint64(0x80000000 | stream),
                      np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32))
    return (w[0] << np.uint64(32)) | w[1]


def subset_select(lists, k, seed, pair, stream, substream, key_mask=MASK_ALL):
    """the subset of three ascending lists: everything when M <= k, else the k smallest elements
    in the order (key & key_mask, t, i); three ascending int32 arrays"""
    lists = [np.asarray(a, dtype=np.int32) for a in lists]
    M = sum(len(a) for a in lists)
    k = max(int(k), 0)
    if M <= k:
        return [a.copy() for a in lists]
    elems = []
    for t in range(3):
        keys = subset_keys(seed, pair, stream, substream, t, lists[t])
        elems += [(int(key) & key_mask, t, int(i)) for key, i in zip(keys.tolist(), lists[t].tolist())]
    elems.sort()
    out = [[], [], []]
    for _, t, i in elems[:k]:
        out[t].append(i)
    return [np.array(sorted(a), dtype=np.int32) for a in out]


def solver_sizes(variant):
    """k_md, k_pt (scale only runs on the calibrated geometry)"""
    v = 0 if variant == 3 else variant
    return (3 if v == 0 else 4), (5, 6, 7)[v]


def subset_size(rule, s, variant, mu, nu, M):
    """(run, k): run False when the rule skips the entry (k = 0 then)"""
    k_md, k_pt = solver_sizes(variant)
    total = sum(M)
    if rule == "nonmin":
        k = max(35 if variant in (0, 3) else 36, min(k_pt * nu, total // 2))
    else:
        ss = (k_md, k_md, 0) if s == 0 else (0, 0, k_pt)
        if any(M[t] < ss[t] for t in range(3)):
            return False, 0
        k = mu * sum(min(ss[t] * mu, M[t]) for t in range(3))
    return True, min(k, total)


def lm_size_test(variant, z):
    """mp_lm_refine_batch's own size rule: True when the problem is too small"""
    k_md, k_pt = solver_sizes(variant)
    return (z[0] < k_md and z[1] < k_md) or z[2] < k_pt


# the list lengths per type of the subset cases: empty types, all three full, either side of a
# wave and of the 256-lane block
LENGTHS = [(0, 0, 0), (1, 0, 0), (0, 0, 63), (64, 65, 0), (63, 64, 65), (255, 0, 257), (256, 256, 256),
           (257, 1, 255), (700, 0, 0), (0, 700, 64), (700, 257, 65), (700, 700, 700), (1, 1, 1)]
MASKS = (MASK_ALL, MASK_TOP_BYTE, 0)


def case_lists(lengths, rng):
    """three strictly ascending int32 lists of the given lengths out of 0 .. 2 max(len) + 2"""
    n = 2 * max(max(lengths), 1) + 3
    return [np.sort(rng.choice(n, size=m, replace=False)).astype(np.int32) for m in lengths]


def case_sizes(M):
    """k in {0, 1, M - 1, M, M + 1, 24, 294}, without the negative one"""
    return sorted({k for k in (0, 1, M - 1, M, M + 1, 24, 294) if k >= 0})


# ---- the steps' schedule ----

def step_factor(i, Q, lam):
    """f_i = lam - i (lam - 1) / (Q - 1) for Q >= 2, f_0 = lam for Q = 1: by exactly this expression"""
    if Q < 2:
        return float(lam)
    return float(lam) - (float(i) * (float(lam) - 1.0)) / float(Q - 1)


def step_substream(r, q):
    return 256 * r + q


# ---- lsq_fit for one entry ----

def lsq_fit_single(variant, p, m_user, s, factor, rule, o, c, norm_scale, seed, pair, stream, substream,
                   on_host=False):
    """PairSet.lsq_fit's result for one entry from the single-pair entries.  on_host: the
    host's sweep and LM instead of the device's (no GPU; for choosing cases, not for bytes)."""
    e = RC.Expected()
    args = RC.pair_args(variant, p)
    thr = RC.thresholds(variant, o, norm_scale)
    wide_thr = [t * float(factor) for t in thr]  # one product, rounded once
    cur = RC.to_problem_units(variant, m_user, norm_scale)
    sc, err = madpose.score_models(variant, *args[:4], *args[5:], o, c, [cur], with_errors=True, host_lo=on_host)
    e.score = float(sc[0])
    e.num_inliers = [int(np.count_nonzero(err[0, t] < thr[t])) for t in range(3)]
    wide = [np.flatnonzero(err[0, t] < wide_thr[t]).astype(np.int32) for t in range(3)]
    e.num_wide = [len(a) for a in wide]
    e.model, e.status = m_user, 3
    run, k = subset_size(rule, s, variant, int(o.min_sample_multiplicator), int(o.non_min_sample_multiplier),
                         e.num_wide)
    e.k, e.select_path = k, run and sum(e.num_wide) > k
    e.subsets = [np.zeros(0, dtype=np.int32)] * 3
    e.subset_sizes = [0, 0, 0]
    if not run:
        return e
    e.subsets = subset_select(wide, k, seed, pair, stream, substream)
    e.subset_sizes = [len(a) for a in e.subsets]
    if lm_size_test(variant, e.subset_sizes):
        return e
    (cand, st), = madpose.lm_refine_batch(variant, *args, o, c, [(RULES[rule], e.subsets, cur)], on_host=on_host)
    e.status = st
    if st == 1:
        e.model = RC.to_user_units(variant, cand, norm_scale)
    return e


def lsq_key(variant, r):
    """everything a LsqFitResult (or lsq_fit_single's expectation) holds, as comparable bytes"""
    return (np.float64(r.score).tobytes(), tuple(r.num_inliers), tuple(r.num_wide), tuple(r.subset_sizes),
            None if r.subsets is None else tuple(np.asarray(a, dtype=np.int32).tobytes() for a in r.subsets),
            r.status, RC.model_bytes(variant, r.model))


# ---- the loop with steps as a walk ----

class StepTrack:
    """what a pair's steps did: lo_step / lo_stage of the overall best (-1: not a step's), the
    offers and those accepted"""

    def __init__(self):
        self.lo_step = self.lo_stage = -1
        self.offers = self.accepted = 0

    def clear(self):
        self.lo_step = self.lo_stage = -1

    def offer(self, T, c, r, stage, score, counts):
        self.offers += 1
        if not score < T.score:
            return False
        T.score, T.counts, T.lo_index, T.source = score, tuple(counts), c, 3
        self.lo_step, self.lo_stage = r, stage
        self.accepted += 1
        return True


def lo_steps_walk(ps, p, n, types, marks, seed, lo, lo_steps, rounds, required, stop_reached, cache, Q, lam, nu):
    """ransac(budget, step, lo, lo_steps, rounds, pair_ids=[p]) as a walk over the checkpoints
    `marks`: lo_walk's two steps, then the stages of the LO steps as public calls --
    ps.lsq_fit(..., pair_ids=[p] * live) per stage and ps.select over the finals.  w.steps: the
    StepTrack; w.stage0: (M, k) of every stage-0 entry; Q, lam, nu: the set's num_lsq_iterations,
    threshold_multiplier and non_min_sample_multiplier."""
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
            cache[(p, m)], = ps.ransac(budget=m, seed=seed, rounds=0, pair_ids=[p])
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
            # ---- the steps, from the model the relaxed refinement returned ----
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
                for i, g in enumerate(out):  # the stage scored its input: the model stage q - 1 produced
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
        if stop_reached(required(n, list(T.counts) if T.source else None), (m - d1, d1)):
            w.stopped = True
            break
    w.track, w.steps = T, ST
    w.num_samples = w.minimal.num_samples if w.minimal is not None else 0
    if best_from_step:  # the lists select returns for that single model
        sr, = ps.select([[best_model]], pair_ids=[p])
        assert sr.index == 0 and np.float64(sr.score).tobytes() == np.float64(T.score).tobytes()
        best_lists = sr.inlier_indices
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

