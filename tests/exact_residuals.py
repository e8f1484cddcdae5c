"""The estimators' per-correspondence residuals in exact rational arithmetic.

A plain restatement, from the reference's own formulas, of

* EvaluateModelOnPoint of the calibrated, shared-focal, two-focal and scale-only
  estimators (src/hybrid_pose_estimator.cpp:216-261, :371-418,
  src/hybrid_pose_shared_focal_estimator.cpp:160-202,
  src/hybrid_pose_two_focal_estimator.cpp:213-257),
* compute_sampson_error and to_essential_matrix (src/utils.h:56-83),
* check_cheirality (src/solver.cpp:1188-1206),
* the MSAC term min(e, thr) w and the running sum of ScoreModel
  (src/hybrid_ransac.h:265-287), and the score_type gating,

on the input doubles converted exactly (fractions.Fraction(float)): K is inverted
exactly, 1 / focal is exact, nothing is rounded anywhere, and a sum is rounded once at the
end.  The literals 1e-2 of the z test and of the cheirality test are the doubles the
reference compares with.  The only irrational quantities are the two bearing norms of the
cheirality test: both inequalities are decided by exact sign reasoning, and their
distances from the gate are evaluated with decimal at 80 digits.

Only the standard library is used.  It knows nothing of the engine: the tests hand it the
doubles the engine and the oracle evaluate (for the focal variants the normalized
coordinates, see normalize_points).
"""
import decimal
import math
import sys
from fractions import Fraction as Fr

DBL_MAX = sys.float_info.max
SENTINEL = Fr(DBL_MAX)
GATE = Fr(1e-2)  # the double the reference's `z < 1e-2` and check_cheirality(.., 1e-2) read
_CTX = decimal.Context(prec=80)


def fr(x):
    return Fr(float(x))


def _vec(a):
    return [fr(v) for v in a]


def _mat(a):
    return [[fr(a[r][c]) for c in range(3)] for r in range(3)]


def inv3(K):
    """Exact inverse of a 3 x 3 matrix of Fractions (adjugate over determinant)."""
    (a, b, c), (d, e, f), (g, h, i) = K
    det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g)
    adj = [[e * i - f * h, c * h - b * i, b * f - c * e],
           [f * g - d * i, a * i - c * g, c * d - a * f],
           [d * h - e * g, b * g - a * h, a * e - b * d]]
    return [[v / det for v in row] for row in adj]


def _mv(M, v):
    return [M[r][0] * v[0] + M[r][1] * v[1] + M[r][2] * v[2] for r in range(3)]


def _mtv(M, v):  # M^T v
    return [M[0][r] * v[0] + M[1][r] * v[1] + M[2][r] * v[2] for r in range(3)]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _mm(A, B):
    return [[sum(A[r][k] * B[k][c] for k in range(3)) for c in range(3)] for r in range(3)]


def _dec(q):
    return _CTX.divide(decimal.Decimal(q.numerator), decimal.Decimal(q.denominator))


def _sign(q):
    return (q > 0) - (q < 0)


def sign_p_minus_q_root(p, q, n2):
    """Exact sign of p - q sqrt(n2) for rationals p, q and n2 > 0."""
    sp, sq = _sign(p), _sign(q)
    if sq == 0:
        return sp
    if sp != sq:  # p <= 0 < q sqrt, or p >= 0 > q sqrt
        return sp if sp != 0 else -sq
    return sp * _sign(p * p - q * q * n2)  # same sign: compare the squares


def _value_p_over_root_minus_q(p, n2, q):
    """p / sqrt(n2) - q to 80 digits, as a Fraction."""
    root = _CTX.sqrt(_dec(n2))
    v = _CTX.subtract(_CTX.divide(_dec(p), root), _dec(q))
    return Fr(v)


def normalize_points(x0, x1, pp0, pp1):
    """The focal estimators' input transform in doubles, as the reference does it before
    EvaluateModelOnPoint sees a coordinate: principal point subtracted, then both images
    divided by one scale, the mean distance from the origin over sqrt(2)
    (src/hybrid_pose_shared_focal_estimator.cpp:15-25, PoseLib's normalize_points).  Plain
    float operations; the tests check the scale against the engine's and the oracle's to
    the bit.  Returns (x0n, x1n, scale) as lists of float pairs."""
    a = [(float(p[0]) - float(pp0[0]), float(p[1]) - float(pp0[1])) for p in x0]
    b = [(float(p[0]) - float(pp1[0]), float(p[1]) - float(pp1[1])) for p in x1]
    s = 0.0
    for (a0, a1), (b0, b1) in zip(a, b):
        s += math.sqrt(a0 * a0 + a1 * a1)
        s += math.sqrt(b0 * b0 + b1 * b1)
    s = s / (math.sqrt(2.0) * len(a)) if a else 1.0
    return [(u / s, v / s) for u, v in a], [(u / s, v / s) for u, v in b], s


class Model:
    """A model's doubles, exactly.  focal0 / focal1 are read by the focal variants only."""

    def __init__(self, R, t, scale=1.0, offset0=0.0, offset1=0.0, focal0=1.0, focal1=1.0):
        self.R, self.t = _mat(R), _vec(t)
        self.scale, self.o0, self.o1 = fr(scale), fr(offset0), fr(offset1)
        self.f0, self.f1 = fr(focal0), fr(focal1)


class Terms:
    """Exact results of one model over a pair, before the score_type gating:
    err[t][i]   the squared error as a Fraction, SENTINEL where the reference returns
                DBL_MAX, None where it is 0 / 0 (a zero Sampson denominator);
    sent[t][i]  True where the reference returns its sentinel;
    z[t][i]     z - 1e-2 of the two reprojections (exact);
    l[k][i]     l1 - md, l2 - md of check_cheirality (80 digits; None for the focal
                variants, which have no such test), with their exact signs in lsign;
    den[i]      the Sampson denominator (exact)."""

    def __init__(self, n):
        self.err = [[None] * n for _ in range(3)]
        self.sent = [[False] * n for _ in range(3)]
        self.z = [[None] * n for _ in range(2)]
        self.l = [[None] * n for _ in range(2)]
        self.lsign = [[None] * n for _ in range(2)]
        self.den = [None] * n


class Pair:
    """The pair's doubles, exactly, with the model-independent rays K^-1 x.  variant 0:
    K0, K1 given (3 x 3); variants 1, 2: K0 = K1 = None and x0, x1 are the normalized
    coordinates.  scale_only: the rules of HybridPoseEstimatorScaleOnly (no offsets, small
    depth priors rejected) on the calibrated geometry."""

    def __init__(self, variant, x0, x1, d0, d1, K0=None, K1=None, scale_only=False):
        self.variant, self.scale_only = variant, scale_only
        self.n = len(d0)
        self.x0 = [(fr(p[0]), fr(p[1])) for p in x0]
        self.x1 = [(fr(p[0]), fr(p[1])) for p in x1]
        self.d0, self.d1 = _vec(d0), _vec(d1)
        if variant == 0:
            self.K0, self.K1 = _mat(K0), _mat(K1)
            self.K0i, self.K1i = inv3(self.K0), inv3(self.K1)
            one = Fr(1)
            self.a = [_mv(self.K0i, (u, v, one)) for u, v in self.x0]
            self.b = [_mv(self.K1i, (u, v, one)) for u, v in self.x1]
            # sampson_loss_scale_ (src/hybrid_pose_estimator.h:35-36)
            s = 1 / (self.K0[0][0] + self.K0[1][1]) + 1 / (self.K1[0][0] + self.K1[1][1])
            self.loss_scale = 1 / (s * s)
        else:
            self.loss_scale = Fr(1)


def _essential(R, t):
    tx = [[Fr(0), -t[2], t[1]], [t[2], Fr(0), -t[0]], [-t[1], t[0], Fr(0)]]
    return _mm(tx, R)


def _sampson(G, x1, x2):
    """compute_sampson_error (src/utils.h:64-83); returns (C^2, Cx + Cy)."""
    e0 = G[0][0] * x1[0] + G[0][1] * x1[1] + G[0][2]
    e1 = G[1][0] * x1[0] + G[1][1] * x1[1] + G[1][2]
    e2 = G[2][0] * x1[0] + G[2][1] * x1[1] + G[2][2]
    f0 = G[0][0] * x2[0] + G[1][0] * x2[1] + G[2][0]
    f1 = G[0][1] * x2[0] + G[1][1] * x2[1] + G[2][1]
    c = x2[0] * e0 + x2[1] * e1 + e2
    return c * c, e0 * e0 + e1 * e1 + f0 * f0 + f1 * f1


def _reproj(K, q, target, out, t, i):
    """p2d_project = K q, the z test, then |p2d_project.xy / z - target|^2."""
    P = _mv(K, q)
    out.z[t][i] = P[2] - GATE
    if P[2] < GATE:
        out.err[t][i] = SENTINEL
        out.sent[t][i] = True
        return
    ex, ey = P[0] / P[2] - target[0], P[1] / P[2] - target[1]
    out.err[t][i] = ex * ex + ey * ey


def evaluate(pair, model, which=(0, 1, 2)):
    """EvaluateModelOnPoint(model, t, i, is_for_inlier = true) for t in `which`, all i."""
    P, m = pair, model
    out = Terms(P.n)
    one, zero = Fr(1), Fr(0)
    if P.variant == 0:
        K0, K1 = P.K0, P.K1
        o0, o1 = (zero, zero) if P.scale_only else (m.o0, m.o1)
    else:
        f0 = m.f0
        f1 = m.f0 if P.variant == 1 else m.f1
        K0 = [[f0, zero, zero], [zero, f0, zero], [zero, zero, one]]
        K1 = [[f1, zero, zero], [zero, f1, zero], [zero, zero, one]]
        K0i = [[1 / f0, zero, zero], [zero, 1 / f0, zero], [zero, zero, one]]
        K1i = [[1 / f1, zero, zero], [zero, 1 / f1, zero], [zero, zero, one]]
        o0, o1 = m.o0, m.o1
    R, t = m.R, m.t
    rtt = _mtv(R, t)
    E = _essential(R, t)
    if P.variant == 0:
        G = E
    else:  # F = K1^-T E K0^-1
        G = [[E[r][c] * K1i[r][r] * K0i[c][c] for c in range(3)] for r in range(3)]
    for i in range(P.n):
        if P.variant == 0:
            a, b = P.a[i], P.b[i]
        else:
            a = (P.x0[i][0] / f0, P.x0[i][1] / f0, one)
            b = (P.x1[i][0] / f1, P.x1[i][1] / f1, one)
        if 0 in which:
            s0 = P.d0[i] + o0
            q = _mv(R, [a[0] * s0, a[1] * s0, a[2] * s0])
            q = [q[0] + t[0], q[1] + t[1], q[2] + t[2]]
            _reproj(K1, q, P.x1[i], out, 0, i)
            if P.scale_only and P.d0[i] < GATE:
                out.err[0][i], out.sent[0][i] = SENTINEL, True
        if 1 in which:
            s1 = (P.d1[i] + o1) * m.scale
            q = _mtv(R, [b[0] * s1, b[1] * s1, b[2] * s1])
            q = [q[0] - rtt[0], q[1] - rtt[1], q[2] - rtt[2]]
            _reproj(K0, q, P.x0[i], out, 1, i)
            if P.scale_only and P.d1[i] < GATE:
                out.err[1][i], out.sent[1][i] = SENTINEL, True
        if 2 in which:
            if P.variant == 0:
                # check_cheirality(pose, a / |a|, b / |b|, 1e-2): with A = |a|, B = |b|,
                # u = R a . b, v = R a . t, w = b . t:
                #   a_ = -u / (A B), b1 = -v / A, b2 = w / B,
                #   lambda1 = b1 - a_ b2 = (u w / B^2 - v) / A,
                #   lambda2 = -a_ b1 + b2 = (w - u v / A^2) / B,
                #   min_depth = 1e-2 (1 - u^2 / (A^2 B^2))   (rational)
                ra = _mv(R, a)
                u, v, w = _dot(ra, b), _dot(ra, t), _dot(b, t)
                A2, B2 = _dot(a, a), _dot(b, b)
                md = GATE * (1 - u * u / (A2 * B2))
                p1, p2 = u * w / B2 - v, w - u * v / A2
                # sign(p / A - md) = sign(p - md A)
                s1_, s2_ = sign_p_minus_q_root(p1, md, A2), sign_p_minus_q_root(p2, md, B2)
                out.lsign[0][i], out.lsign[1][i] = s1_, s2_
                out.l[0][i] = _value_p_over_root_minus_q(p1, A2, md)
                out.l[1][i] = _value_p_over_root_minus_q(p2, B2, md)
                c2, den = _sampson(G, a, b)
                out.den[i] = den
                if not (s1_ > 0 and s2_ > 0):
                    out.err[2][i], out.sent[2][i] = SENTINEL, True
                else:
                    out.err[2][i] = None if den == 0 else c2 / den * P.loss_scale
            else:
                c2, den = _sampson(G, P.x0[i], P.x1[i])
                out.den[i] = den
                out.err[2][i] = None if den == 0 else c2 / den
    return out


def gated(terms, score_type):
    """The errors as ScoreModel reads them (is_for_inlier = false): EPI_ONLY (1) gates the
    two reprojections, MD_ONLY (2) the Sampson error.  Returns err[t][i] (same objects)."""
    n = len(terms.den)
    err = [list(terms.err[t]) for t in range(3)]
    if score_type == 1:
        err[0] = [SENTINEL] * n
        err[1] = [SENTINEL] * n
    elif score_type == 2:
        err[2] = [SENTINEL] * n
    return err


def msac_sum(terms, thr, w, score_type=0):
    """ScoreModel: sum over t, i of min(e, thr_t) w_t, exactly; thr, w: the three doubles
    the estimator uses.  Returns a Fraction (float() rounds it once); None if a term is
    undefined."""
    err = gated(terms, score_type)
    total = Fr(0)
    for t in range(3):
        th, wt = fr(thr[t]), fr(w[t])
        for e in err[t]:
            if e is None:
                return None
            total += (e if e < th else th) * wt
    return total
