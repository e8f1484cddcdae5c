"""A Python restatement of the sampler of mp_draw_set (madpose_amd/csrc/include/mp_draw.h):
Philox4x32-10 in plain numpy uint64 arithmetic and the index rule, for the CPU and GPU tests
of the draw.  Nothing here calls the library."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
MASK = np.uint64(0xFFFFFFFF)
SH = np.uint64(32)
BLOCKS = 16


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """The four output words of Philox4x32-10; every argument a uint64 array (or scalar) of
    32-bit values, broadcast together."""
    c0, c1, c2, c3, k0, k1 = (np.asarray(v, dtype=np.uint64) for v in (c0, c1, c2, c3, k0, k1))
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2  # (32 x 32 bits: no overflow in 64)
        c0, c1, c2, c3 = (p1 >> SH) ^ c1 ^ k0, p1 & MASK, (p0 >> SH) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def words(seed, pair, s):
    """The 64-word streams of the samples s (an int array) of pair `pair`: shape (len(s), 64)."""
    s = np.asarray(s, dtype=np.uint64)
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    out = np.zeros((s.shape[0], 4 * BLOCKS), dtype=np.uint64)
    for b in range(BLOCKS):
        w = philox4x32_10(s, np.uint64(b), np.uint64(pair), np.uint64(0), k0, k1)
        for i in range(4):
            out[:, 4 * b + i] = w[i]
    return out


def sizes(variant):
    return (3 if variant == 0 else 4), (5, 6, 7)[variant]


def draw_pair(variant, n, seed, point_share, pair, budget):
    """(types int32 (K,), idx int32 (K, 8), fill bool (K,)) of the `budget` samples of a pair
    of n correspondences; K = 0 when the pair is too small for the MD solver."""
    k_md, k_pt = sizes(variant)
    if n < k_md or budget == 0:
        return np.zeros(0, dtype=np.int32), np.zeros((0, 8), dtype=np.int32), np.zeros(0, dtype=bool)
    W = words(seed, pair, np.arange(budget))
    types = np.zeros(budget, dtype=np.int32)
    idx = np.zeros((budget, 8), dtype=np.int32)
    fill = np.zeros(budget, dtype=bool)
    prop = ((W * np.uint64(n)) >> SH).astype(np.int64)  # (w < 2^32, n <= 2^28: no overflow)
    for s in range(budget):
        t = 1 if (n >= k_pt and (int(W[s, 0]) >> 24) < point_share) else 0
        k = k_pt if t else k_md
        got = []
        for p in prop[s, 1:].tolist():
            if p not in got:
                got.append(p)
                if len(got) == k:
                    break
        if len(got) < k:
            fill[s] = True
            c = 0
            while len(got) < k:
                if c not in got:
                    got.append(c)
                c += 1
        types[s] = t
        idx[s, :k] = got
    return types, idx, fill


def default_share(solver_type):
    return {0: 128, 1: 256, 2: 0}[solver_type]
