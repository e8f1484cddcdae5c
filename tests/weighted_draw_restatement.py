"""A Python restatement of the confidence-weighted draw (madpose_amd/csrc/include/mp_draw.h
draw_sample_weighted, include/mp_draw_weights.h draw_quantise), on top of the uniform
restatement in tests/draw_restatement.py.  Nothing here calls the library."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import draw_restatement as D  # noqa: E402

MAX_N = 65535
Q_MAX = 65535


def quantise(weights):
    """q (int64) of float32 / float64 weights: min(65535, floor(w * 65536)), the weight widened
    to float64 first (exact); ValueError naming the lowest bad row."""
    w = np.asarray(weights)
    assert w.dtype in (np.float32, np.float64) and w.ndim == 1
    w = w.astype(np.float64)
    bad = np.flatnonzero(~((w >= 0) & (w <= 1)))
    if bad.size:
        raise ValueError(f"row {int(bad[0])}")
    return np.minimum(Q_MAX, np.floor(w * 65536.0)).astype(np.int64)


def table(weights):
    """(cum int64 (n + 1,), n_pos) of one pair's weights; cum[-1] = W < 2^32 for n <= 65535."""
    q = quantise(weights)
    assert q.shape[0] <= MAX_N
    cum = np.concatenate([[0], np.cumsum(q)]).astype(np.int64)
    return cum, int((q > 0).sum())


def is_weighted(variant, n, n_pos):
    k_md, k_pt = D.sizes(variant)
    return n_pos >= (k_pt if n >= k_pt else k_md)


def draw_pair(variant, cum, seed, point_share, pair, budget, first=0):
    """(types, idx, fill) of samples first .. first + budget - 1 of a weighted pair with the table
    cum: draw_restatement.draw_pair with the proposal t = (w * W) >> 32 -> the i with cum[i] <= t <
    cum[i + 1], and the fill over the indices with q > 0."""
    cum = np.asarray(cum, dtype=np.int64)
    n = cum.shape[0] - 1
    k_md, k_pt = D.sizes(variant)
    W = int(cum[-1])
    assert is_weighted(variant, n, int((np.diff(cum) > 0).sum())) and W < 1 << 32
    words = D.words(seed, pair, np.arange(first, first + budget))
    types = np.zeros(budget, dtype=np.int32)
    idx = np.zeros((budget, 8), dtype=np.int32)
    fill = np.zeros(budget, dtype=bool)
    t = ((words * np.uint64(W)) >> D.SH).astype(np.int64)  # (w < 2^32, W < 2^32: no overflow in 64)
    prop = np.searchsorted(cum, t, side="right") - 1  # the last i with cum[i] <= t: cum[i + 1] > t
    positive = np.flatnonzero(np.diff(cum) > 0).tolist()
    for s in range(budget):
        ty = 1 if (n >= k_pt and (int(words[s, 0]) >> 24) < point_share) else 0
        k = k_pt if ty else k_md
        got = []
        for p in prop[s, 1:].tolist():
            if p not in got:
                got.append(p)
                if len(got) == k:
                    break
        if len(got) < k:
            fill[s] = True
            for c in positive:
                if c not in got:
                    got.append(c)
                    if len(got) == k:
                        break
        types[s] = ty
        idx[s, :k] = got
    return types, idx, fill


def draw_any(variant, n, weights, seed, point_share, pair, budget, first=0):
    """What a pair of the set draws: weights None, or too few positive ones -> the uniform rule."""
    if weights is not None:
        cum, n_pos = table(weights)
        if is_weighted(variant, n, n_pos):
            return draw_pair(variant, cum, seed, point_share, pair, budget, first)
    T, I, F = D.draw_pair(variant, n, seed, point_share, pair, first + budget)
    return T[first:], I[first:], F[first:]
