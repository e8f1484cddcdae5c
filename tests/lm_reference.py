"""One evaluation of the LO least-squares problems at 50 digits: cost, gradient and
Gauss-Newton matrix from the reference's cost functors, with their Jacobians by forward-mode
jets.

A plain restatement, from the reference's own formulas, of

* LiftProjectionFunctor0 / 1 and SampsonErrorFunctor with their shared-focal and two-focal
  forms (src/cost_functions.h:16-387), as the optimizers add them (src/optimizer.h:48-111,
  :265-369, :383-499: x_calib = K^-1 x for the calibrated variant, the Sampson weight a
  double formed once per problem),
* the parameterisation of src/optimizer.h: the quaternion manifold
  Plus(q, delta) = (cos |delta|, sin |delta| delta / |delta|) (x) q, then t, the scale, the
  two offsets and the focals (one shared focal: one parameter), and which of them a
  problem holds (a block that no residual uses does not exist; use_shift off makes the
  offsets constant),
* the trust-region system of Ceres' LM on it: Jacobi scaling D = 1 / (1 + sqrt(H_aa)) and
  the diagonal clamp(diag(D H D), 1e-6, 1e32) / radius.

It knows nothing of the engine.  The tests hand it the doubles the engine reads (pixels
and K for the calibrated variant; normalised coordinates and problem-unit focals
otherwise), converted exactly.  Two modes share every function: `mp` (mpmath at 50 digits,
one block at a time, sums at 50 digits rounded once) and `f64` (numpy doubles over all
blocks of a type at once, sums by math.fsum: the yardstick of rounding and the reference of
the large reduction cases).

Parameter layout (11): rotation tangent 3, t 3, scale, offset0, offset1, focal0, focal1.
A jet is a value with its 11 partial derivatives at delta = 0.  There the first-order part
of Plus is exact: cos |delta| = 1 + O(delta^2), sin |delta| delta / |delta| = delta +
O(delta^3), so the quaternion of the step is the jet (1, delta); central_jacobian() checks
this against Plus itself with cos and sin at 60 digits.

Every block asserts the guard bands of the cases: projected |h_z| > 0.1 and Sampson
denominator > 1e-6 |F|^2.
"""
import math

import mpmath
import numpy as np

NP = 11
D0, T0, S, O0, O1, F0, F1 = 0, 3, 6, 7, 8, 9, 10
MP = mpmath.mp.clone()
MP.dps = 50


class Jet:
    """value + 11 partials; the scalars are mpf, floats or numpy arrays (one entry per block)"""
    __slots__ = ("v", "d")

    def __init__(self, v, d=None):
        self.v = v
        self.d = [0] * NP if d is None else d

    @staticmethod
    def lift(x):
        return x if isinstance(x, Jet) else Jet(x)

    def __add__(self, o):
        o = Jet.lift(o)
        return Jet(self.v + o.v, [a + b for a, b in zip(self.d, o.d)])

    __radd__ = __add__

    def __neg__(self):
        return Jet(-self.v, [-a for a in self.d])

    def __sub__(self, o):
        o = Jet.lift(o)
        return Jet(self.v - o.v, [a - b for a, b in zip(self.d, o.d)])

    def __rsub__(self, o):
        return Jet.lift(o) - self

    def __mul__(self, o):
        o = Jet.lift(o)
        return Jet(self.v * o.v, [a * o.v + self.v * b for a, b in zip(self.d, o.d)])

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Jet.lift(o)
        q = self.v / o.v
        return Jet(q, [(a - q * b) / o.v for a, b in zip(self.d, o.d)])

    def __rtruediv__(self, o):
        return Jet.lift(o) / self


def _is_mp(x):
    return hasattr(x, "context")


def _sqrt(x):
    return x.context.sqrt(x) if _is_mp(x) else np.sqrt(x)


def jsqrt(a):
    r = _sqrt(a.v)
    return Jet(r, [b / (2 * r) for b in a.d])


def _var(v, k):
    d = [0] * NP
    d[k] = 1
    return Jet(v, d)


def _quat_mul(a, b):
    return [a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
            a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
            a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1],
            a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]]


def _normalize(q):
    n = jsqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return [c / n for c in q]


def _rotate(q, p):
    """ceres::UnitQuaternionRotatePoint: p + 2 w (u x p) + 2 u x (u x p), u = (q1, q2, q3)"""
    w, u = q[0], q[1:]
    c1 = [u[1] * p[2] - u[2] * p[1], u[2] * p[0] - u[0] * p[2], u[0] * p[1] - u[1] * p[0]]
    c1 = [2 * c for c in c1]
    c2 = [u[1] * c1[2] - u[2] * c1[1], u[2] * c1[0] - u[0] * c1[2], u[0] * c1[1] - u[1] * c1[0]]
    return [p[k] + w * c1[k] + c2[k] for k in range(3)]


def _rotation_matrix(q):
    """Eigen's toRotationMatrix of the normalised quaternion"""
    w, x, y, z = _normalize(q)
    return [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
            [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
            [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]


def _mv(M, v):
    """M v with plain M; the jets stand on the left of every product"""
    v = [Jet.lift(c) for c in v]
    return [v[0] * M[r][0] + v[1] * M[r][1] + v[2] * M[r][2] for r in range(3)]


def _inv3(K):
    (a, b, c), (d, e, f), (g, h, i) = K
    det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g)
    adj = [[e * i - f * h, c * h - b * i, b * f - c * e],
           [f * g - d * i, a * i - c * g, c * d - a * f],
           [d * h - e * g, b * g - a * h, a * e - b * d]]
    return [[v / det for v in row] for row in adj]


class Params:
    """The parameters of one problem as jets.  vals: q (4), t (3), scale, o0, o1, f0, f1 in
    the mode's scalars.  variables: the jets carry unit partials at delta = 0 (the rotation
    through the step quaternion (1, delta) (x) q); otherwise they are constants at `vals`."""

    def __init__(self, variant, vals, variables=True):
        q, t, sc, o0, o1, f0, f1 = vals
        var = _var if variables else (lambda v, k: Jet(v))
        one, zero = q[0] * 0 + 1, q[0] * 0
        self.q = [Jet(c) for c in q]
        if variables:
            self.q = _quat_mul([Jet(one), _var(zero, D0), _var(zero, D0 + 1), _var(zero, D0 + 2)], self.q)
        self.t = [var(t[k], T0 + k) for k in range(3)]
        self.s = var(sc, S)
        self.o0 = var(o0, O0)
        self.o1 = var(o1, O1)
        self.f0 = var(f0, F0)
        self.f1 = self.f0 if variant == 1 else var(f1, F1)  # one focal parameter when shared


def _all(c):
    return bool(np.all(c))


def _project(h, target, rows):
    assert _all(abs(h[2].v) > 0.1), "guard band: |h_z| <= 0.1"
    rows.append(h[0] / h[2] - target[0])
    rows.append(h[1] / h[2] - target[1])


def lift0(variant, P, x0, x1, d0, K0inv, K1, rows):
    """LiftProjection*Functor0: x1_hat = K1 (R (K0^-1 x0 (d0 + o0)) + t)"""
    one = x0[0] * 0 + 1
    if variant == 0:
        c = _mv(K0inv, [x0[0], x0[1], one])
    else:
        c = [Jet(x0[0]) / P.f0, Jet(x0[1]) / P.f0, Jet(one)]
    a = P.o0 + d0
    x3d = [ck * a for ck in c]
    y = _rotate(_normalize(P.q), x3d)
    y = [y[k] + P.t[k] for k in range(3)]
    h = _mv(K1, y) if variant == 0 else [P.f1 * y[0], P.f1 * y[1], y[2]]
    _project(h, x1, rows)


def lift1(variant, P, x1, x0, d1, K1inv, K0, rows):
    """LiftProjection*Functor1: x0_hat = K0 R^T (K1^-1 x1 (d1 + o1) s - t)"""
    one = x1[0] * 0 + 1
    if variant == 0:
        c = _mv(K1inv, [x1[0], x1[1], one])
    else:
        c = [Jet(x1[0]) / P.f1, Jet(x1[1]) / P.f1, Jet(one)]
    a = (P.o1 + d1) * P.s
    u = [c[k] * a - P.t[k] for k in range(3)]
    qn = _normalize(P.q)
    y = _rotate([qn[0], -qn[1], -qn[2], -qn[3]], u)
    h = _mv(K0, y) if variant == 0 else [P.f0 * y[0], P.f0 * y[1], y[2]]
    _project(h, x0, rows)


def sampson(variant, P, x0, x1, weight, K0inv, K1inv, rows):
    """SampsonError*Functor: weight C / |(Ex1_0, Ex1_1, Ex2_0, Ex2_1)|, E = [t]x R (K^-T E K^-1)"""
    one = x0[0] * 0 + 1
    R = _rotation_matrix(P.q)
    t = P.t
    zero = Jet(one * 0)
    Tx = [[zero, -t[2], t[1]], [t[2], zero, -t[0]], [-t[1], t[0], zero]]
    E = [[Tx[r][0] * R[0][c] + Tx[r][1] * R[1][c] + Tx[r][2] * R[2][c] for c in range(3)] for r in range(3)]
    if variant == 0:
        a = _mv(K0inv, [x0[0], x0[1], one])
        b = _mv(K1inv, [x1[0], x1[1], one])
    else:
        k0 = [1 / P.f0, 1 / P.f0, Jet(one)]
        k1 = [1 / P.f1, 1 / P.f1, Jet(one)]
        E = [[k1[r] * E[r][c] * k0[c] for c in range(3)] for r in range(3)]
        a, b = [Jet(x0[0]), Jet(x0[1])], [Jet(x1[0]), Jet(x1[1])]
    e0 = E[0][0] * a[0] + E[0][1] * a[1] + E[0][2]
    e1 = E[1][0] * a[0] + E[1][1] * a[1] + E[1][2]
    e2 = E[2][0] * a[0] + E[2][1] * a[1] + E[2][2]
    g0 = E[0][0] * b[0] + E[1][0] * b[1] + E[2][0]
    g1 = E[0][1] * b[0] + E[1][1] * b[1] + E[2][1]
    C = b[0] * e0 + b[1] * e1 + e2
    den = e0 * e0 + e1 * e1 + g0 * g0 + g1 * g1
    F2 = sum(E[r][c].v * E[r][c].v for r in range(3) for c in range(3))
    assert _all(den.v > F2 * 1e-6), "guard band: Sampson denominator <= 1e-6 |F|^2"
    rows.append(C / jsqrt(den) * weight)


def active_set(variant, n0, n1, n2, use_shift):
    """Which of the 11 parameters the problem holds and varies (src/optimizer.h SetUp: a
    block that no residual uses is not in the problem; use_shift off: constant offsets)"""
    col = [False] * NP
    if n0 + n1 + n2 == 0:
        return col
    for k in range(6):
        col[k] = True
    col[S] = n1 > 0
    col[O0] = n0 > 0 and bool(use_shift)
    col[O1] = n1 > 0 and bool(use_shift)
    col[F0] = variant >= 1
    col[F1] = variant == 2
    return col


def _rows(variant, data, lists, P, conv, blockwise):
    """The residual rows (jets) of a problem at the parameter jets P.  data: x0, x1 (n x 2),
    d0, d1 (n), K0, K1 (3 x 3, calibrated), weight; lists: the three block lists (empty
    where the LO type leaves a residual type out).  blockwise: one block at a time through
    conv (the exact conversion of a double); otherwise all blocks of a type at once as
    numpy arrays."""
    K0 = K1 = K0i = K1i = None
    if variant == 0:
        K0 = [[conv(v) for v in row] for row in np.asarray(data["K0"], float).reshape(3, 3)]
        K1 = [[conv(v) for v in row] for row in np.asarray(data["K1"], float).reshape(3, 3)]
        if blockwise:
            K0i, K1i = _inv3(K0), _inv3(K1)
        else:  # the reference's K.inverse() in doubles
            K0i = np.linalg.inv(np.asarray(data["K0"], float).reshape(3, 3)).tolist()
            K1i = np.linalg.inv(np.asarray(data["K1"], float).reshape(3, 3)).tolist()
    x0, x1, d0, d1 = data["x0"], data["x1"], data["d0"], data["d1"]
    w = conv(data["weight"])
    rows = []
    if blockwise:
        cv = lambda p: [conv(p[0]), conv(p[1])]
        for i in lists[0]:
            lift0(variant, P, cv(x0[i]), cv(x1[i]), conv(d0[i]), K0i, K1, rows)
        for i in lists[1]:
            lift1(variant, P, cv(x1[i]), cv(x0[i]), conv(d1[i]), K1i, K0, rows)
        for i in lists[2]:
            sampson(variant, P, cv(x0[i]), cv(x1[i]), w, K0i, K1i, rows)
        return rows
    for k in range(3):
        i = np.asarray(lists[k], dtype=np.int64)
        if len(i) == 0:
            continue
        a0, a1 = [x0[i, 0], x0[i, 1]], [x1[i, 0], x1[i, 1]]
        if k == 0:
            lift0(variant, P, a0, a1, d0[i], K0i, K1, rows)
        elif k == 1:
            lift1(variant, P, a1, a0, d1[i], K1i, K0, rows)
        else:
            sampson(variant, P, a0, a1, w, K0i, K1i, rows)
    return rows


def _jet_rows(variant, data, lists, params, mode):
    q, t, sc, o0, o1, f0, f1 = params
    conv = (lambda v: MP.mpf(float(v))) if mode == "mp" else float
    vals = ([conv(c) for c in q], [conv(c) for c in t], conv(sc), conv(o0), conv(o1), conv(f0), conv(f1))
    return _rows(variant, data, lists, Params(variant, vals), conv, mode == "mp")


def _up(a, b):
    return a * NP - a * (a - 1) // 2 + (b - a)


def system(variant, data, lists, params, mode="mp"):
    """cost, g (11), H (66, packed upper triangle) of the problem as doubles (summed at 50
    digits, or by fsum, and rounded once), their magnitude sums S_cost = sum r^2 / 2, S_g[a]
    = sum |J_a r|, S_H[a, b] = sum |J_a J_b| over the residual rows, and the number of rows.
    params: q (4), t (3), scale, o0, o1, f0, f1 as doubles."""
    rows = _jet_rows(variant, data, lists, params, mode)
    if mode == "mp":
        tot = lambda terms: sum(terms, MP.mpf(0))
        flat = lambda x: [x]
    else:
        tot = math.fsum
        flat = lambda x: np.atleast_1d(np.asarray(x, dtype=np.float64)).tolist()
    n = NP * (NP + 1) // 2
    out = dict(rows=sum(len(flat(r.v)) for r in rows), g=np.zeros(NP), H=np.zeros(n), S_g=np.zeros(NP), S_H=np.zeros(n))
    out["cost"] = out["S_cost"] = float(tot([t for r in rows for t in flat(r.v * r.v / 2)]))
    for a in range(NP):
        terms = [t for r in rows for t in flat(r.d[a] * r.v)]
        out["g"][a] = float(tot(terms))
        out["S_g"][a] = float(tot([abs(t) for t in terms]))
        for b in range(a, NP):
            terms = [t for r in rows for t in flat(r.d[a] * r.d[b])]
            out["H"][_up(a, b)] = float(tot(terms))
            out["S_H"][_up(a, b)] = float(tot([abs(t) for t in terms]))
    return out


class RangeSums:
    """The 50-digit systems of every block range [b0, b1) of one problem's concatenated list,
    from prefix sums over the residual rows (each sum carries 50 digits, so the difference of
    two prefixes is the range's sum to ~1e-48 of the whole problem's magnitude)."""

    def __init__(self, variant, data, lists, params):
        rows = _jet_rows(variant, data, lists, params, "mp")
        n0, n1 = len(lists[0]), len(lists[1])
        # first row of block b: two rows per reprojection block, one per Sampson block
        self.first = lambda b: 2 * b if b <= n0 + n1 else 2 * (n0 + n1) + (b - n0 - n1)
        ent = [[r.v * r.v / 2 for r in rows]]
        ent += [[r.d[a] * r.v for r in rows] for a in range(NP)]
        ent += [[r.d[a] * r.d[b] for r in rows] for a in range(NP) for b in range(a, NP)]

        def prefix(terms):
            out, acc = [MP.mpf(0)], MP.mpf(0)
            for t in terms:
                acc = acc + t
                out.append(acc)
            return out

        self.sum = [prefix(e) for e in ent]
        self.mag = [prefix([abs(t) for t in e]) for e in ent]

    def system(self, b0, b1):
        i, j = self.first(b0), self.first(b1)
        X = [float(p[j] - p[i]) for p in self.sum]
        Sx = [float(p[j] - p[i]) for p in self.mag]
        return dict(rows=j - i, cost=X[0], S_cost=Sx[0], g=np.array(X[1:1 + NP]), S_g=np.array(Sx[1:1 + NP]),
                    H=np.array(X[1 + NP:]), S_H=np.array(Sx[1 + NP:]))


def jacobian(variant, data, lists, params):
    """The residuals and the Jacobian rows by jets at 50 digits: (r list, list of 11-lists)"""
    rows = _jet_rows(variant, data, lists, params, "mp")
    return [r.v for r in rows], [[MP.mpf(x) for x in r.d] for r in rows]


def plus(q, delta, ctx=MP):
    """Plus(q, delta) = (cos |delta|, sin |delta| delta / |delta|) (x) q in ctx's precision"""
    q = [ctx.mpf(float(c)) for c in q]
    n = ctx.sqrt(sum((d * d for d in delta), ctx.mpf(0)))
    if n == 0:
        return q
    sn = ctx.sin(n) / n
    return _quat_mul([ctx.cos(n)] + [sn * d for d in delta], q)


def central_jacobian(variant, data, lists, params, step="1e-25"):
    """The same Jacobian by central differences at 60 digits, the rotation through Plus
    itself: independent of the jets (truncation ~ step^2 relative)."""
    ctx = mpmath.mp.clone()
    ctx.dps = 60
    h = ctx.mpf(step)
    conv = lambda v: ctx.mpf(float(v))
    q, t, sc, o0, o1, f0, f1 = params
    base = [conv(c) for c in t] + [conv(sc), conv(o0), conv(o1), conv(f0), conv(f1)]
    cols = []
    for a in range(NP):
        if variant == 0 and a >= F0 or variant == 1 and a == F1:
            cols.append(None)  # not a parameter of the variant
            continue
        res = []
        for sgn in (1, -1):
            delta = [ctx.mpf(0)] * 3
            v = list(base)
            if a < 3:
                delta[a] = sgn * h
            else:
                v[a - 3] = v[a - 3] + sgn * h
            vals = (plus(q, delta, ctx), v[0:3], v[3], v[4], v[5], v[6], v[7])
            rows = _rows(variant, data, lists, Params(variant, vals, variables=False), conv, True)
            res.append([r.v for r in rows])
        cols.append([(p - m) / (2 * h) for p, m in zip(*res)])
    nrow = len(next(c for c in cols if c is not None))
    return [[ctx.mpf(0) if cols[a] is None else cols[a][i] for a in range(NP)] for i in range(nrow)]


def damped_system(H, g, col, radius):
    """The LM system of the doubles H (66 packed), g (11) over the active set col at 50
    digits: A = D H D + clamp(diag(D H D), 1e-6, 1e32) / radius, b = -D g, D = 1 / (1 +
    sqrt(H_aa)).  Returns (A as a list of rows, b, D, the active indices)."""
    act = [a for a in range(NP) if col[a]]
    f = lambda v: MP.mpf(float(v))
    Dg = [1 / (1 + MP.sqrt(f(H[_up(a, a)]))) for a in act]
    A = [[f(H[_up(min(a, b), max(a, b))]) * Dg[i] * Dg[j] for j, b in enumerate(act)] for i, a in enumerate(act)]
    for i in range(len(act)):
        A[i][i] += min(max(A[i][i], f(1e-6)), f(1e32)) / f(radius)
    b = [-f(g[a]) * Dg[i] for i, a in enumerate(act)]
    return A, b, Dg, act


def positive_definite(A):
    """Cholesky's test at 50 digits: every pivot is > 0 (a NaN compares false)"""
    n = len(A)
    Lw = [[MP.mpf(0)] * n for _ in range(n)]
    for j in range(n):
        dj = A[j][j] - sum((Lw[j][k] * Lw[j][k] for k in range(j)), MP.mpf(0))
        if not dj > 0:
            return False
        Lw[j][j] = MP.sqrt(dj)
        for i in range(j + 1, n):
            Lw[i][j] = (A[i][j] - sum((Lw[i][k] * Lw[j][k] for k in range(j)), MP.mpf(0))) / Lw[j][j]
    return True
