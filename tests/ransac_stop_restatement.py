"""The termination rule of PairSet.ransac(step=...) (mp_ransac_adaptive_set) restated in
Python as the issue states it: math.pow / log / ceil are the C library's, so the values are
the library's.  Used by tests/test_ransac_adaptive_cpu.py (against mp_debug_ransac_required)
and tests/test_ransac_adaptive_gpu.py (the expected stop point of every pair)."""
import math

K_MD, K_PT = (3, 4, 4), (5, 6, 7)


def required(variant, n, counts, sp, mn, mx):
    """req[0] (the MD solver) and req[1] (the point solver) for a pair of n correspondences
    whose best has the list lengths counts (None: no winner)."""
    out = []
    for ss in ((K_MD[variant], K_MD[variant], 0), (0, 0, K_PT[variant])):
        p_all = 1.0
        for t in range(3):
            r = counts[t] / n if n > 0 and counts is not None else 0.0
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


def stop_reached(req, drawn):
    return any(drawn[s] > 0 and drawn[s] >= req[s] for s in range(2))


def checkpoints(step, budget):
    """m_k = min(k step, budget) up to the budget"""
    out, m = [], 0
    while m < budget:
        m = min(m + step, budget)
        out.append(m)
    return out
