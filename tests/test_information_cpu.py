"""PairSet.information without a device: the plan and the output-extent arithmetic
(madpose_amd/csrc/host/information_plan.h) pass their stand-alone check under AddressSanitizer and
UBSan (tests/information_plan_check.cpp); the finishing arithmetic
(madpose_amd/csrc/include/mp_information.h, the text the finishing kernel runs) is held through
mp_debug_information_finish to a column-wise backward error on the 50-digit systems of
tests/lm_system_cases.py; every Python check comes before any library call; and
mp_information_set refuses bad arguments on a set whose device does not exist."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import madpose
from madpose_amd import _lib as L
from madpose_amd import synthetic
from tests import lm_reference as LR
from tests import lm_system_cases as SC
from tests.information_worker import column_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/llvm/bin/clang++"
NO_DEVICE = 10 ** 6  # no such device: a call that reached it would not return MP_EINVAL / MP_OK


def test_symbols_header_and_layout():
    lib = L.lib()
    with open(os.path.join(ROOT, "include", "madpose_mi355x.h")) as f:
        header = f.read()
    for name in ("mp_information_set", "mp_debug_information_finish", "mp_debug_information_stats"):
        assert hasattr(lib, name) and name in L.EXPORTS and f"int {name}(" in header, name
    assert ctypes.sizeof(L.mp_information_out) == 48 and "} mp_information_out;" in header
    assert [getattr(L.mp_information_out, f).offset for f in ("H", "g", "cost", "cov", "on_device",
                                                               "producer_stream")] == [0, 8, 16, 24, 32, 40]
    assert ctypes.sizeof(L.mp_information_entry) == 68 and "} mp_information_entry;" in header
    assert [getattr(L.mp_information_entry, f).offset for f in ("col", "pd", "status", "rows", "counts")] == \
        [0, 44, 48, 52, 56]
    for rel in (("host", "information_plan.h"), ("include", "mp_information.h")):
        with open(os.path.join(ROOT, "madpose_amd", "csrc", *rel)) as f:
            text = f.read()
        assert "#include <hip" not in text and "__global__" not in text  # plain C++
    assert hasattr(madpose.PairSet, "information") and hasattr(madpose, "InformationResult")


def test_plan_under_sanitizers(tmp_path):
    if not os.path.exists(CLANG):
        pytest.fail(f"{CLANG} missing: the host build of information_plan.h needs ROCm's clang")
    exe = str(tmp_path / "information_plan_check")
    cmd = [CLANG, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "madpose_amd", "csrc", "host"),
           os.path.join(ROOT, "tests", "information_plan_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().endswith("ok")


# ---- the finishing function (the column check and its constant: information_worker.column_check) ----

@pytest.fixture(scope="module")
def systems():
    """the 50-digit systems of the three variants as doubles, with their active sets"""
    out = []
    for v in (0, 1, 2):
        cx = SC.small(v)
        for j, s in enumerate(SC.formula_specs(v)):
            r = SC.reference(cx, s, "mp")
            lists = SC.effective_lists(s)
            # both reprojection types and twice as many rows as parameters: every parameter is observed
            full = len(lists[0]) > 0 and len(lists[1]) > 0 and r["rows"] >= 2 * int(np.sum(r["col"]))
            out.append(((v, j), r["H"].copy(), r["g"].copy(), np.asarray(r["col"], dtype=np.int32), full))
    return out


def test_finish_columns_against_50_digits(systems):
    """Every active column of cov against A y = e_k at 50 digits, |A y_k - e_k|_inf <= c n 2^-53
    (|A|_inf |y_k|_inf + 1) with c = 3 n + 4: check_step's constant, derived again for this
    function's operation count in information_worker.column_check's docstring (the factorisation's
    (3 n + 1) n u and 12 u <= 3 n u for the scaling, the exact right-hand side and the two products
    of the result).  Measured here: worst ratio 0.11 against c >= 22."""
    worst = 0.0
    done = 0
    for tag, H, g, col, full in systems:
        Hm, gm, cov, pd = madpose.information_finish(H, g, col)
        assert pd in (0, 1) and (pd == 1 or not full), tag
        inact = np.flatnonzero(col == 0)
        # the mask: exact zeros on the inactive entries, every other entry untouched
        for a in range(11):
            for b in range(a, 11):
                q = LR._up(a, b)
                if col[a] and col[b]:
                    assert Hm[q] == H[q]
                else:
                    assert Hm[q] == 0.0 and not np.signbit(Hm[q])
        assert np.all(gm[inact] == 0.0) and np.array_equal(gm[col != 0], g[col != 0])
        assert not np.any(cov[inact, :]) and not np.any(cov[:, inact]), tag
        if pd != 1:  # (fewer rows than parameters, or a gauge: rounding decides the last pivots)
            assert not np.any(cov)
            continue
        worst = max(worst, column_check(Hm, col, cov, tag))
        done += 1
    print(f"{done} of {len(systems)} systems inverted; worst column backward error over n u (|A||y| + 1): "
          f"{worst:.2f} (bound 3 n + 4 >= 22)")
    assert sum(1 for s in systems if s[4]) >= 12  # (four or more fully observed systems per variant)


def test_finish_matches_numpy_on_a_well_conditioned_system():
    rng = np.random.default_rng(5)
    J = rng.standard_normal((60, 11))
    J[:, 8] = 0.0
    M = J.T @ J
    col = np.ones(11, dtype=np.int32)
    col[[8, 10]] = 0
    H, g, cov, pd = madpose.information_finish(M[np.triu_indices(11)], rng.standard_normal(11), col)
    act = np.flatnonzero(col)
    assert pd == 1
    want = np.linalg.inv(M[np.ix_(act, act)])
    assert np.allclose(cov[np.ix_(act, act)], want, rtol=1e-10, atol=0)
    assert not np.any(cov[[8, 10], :]) and not np.any(cov[:, [8, 10]]) and g[8] == 0.0 and g[10] == 0.0
    column_check(H, col, cov, "random")


def test_finish_refuses_what_is_not_positive_definite():
    rng = np.random.default_rng(6)
    J = rng.standard_normal((30, 11))
    M = J.T @ J
    col = np.ones(11, dtype=np.int32)
    tri = np.triu_indices(11)
    ok = madpose.information_finish(M[tri], np.zeros(11), col)
    assert ok[3] == 1 and np.any(ok[2])
    # a zero H_aa on an active parameter
    Z = M.copy()
    Z[4, :] = Z[:, 4] = 0.0
    H, g, cov, pd = madpose.information_finish(Z[tri], np.ones(11), col)
    assert pd == 0 and not np.any(cov) and np.all(g == 1.0)
    # ... which is fine once the parameter is inactive
    c2 = col.copy()
    c2[4] = 0
    assert madpose.information_finish(Z[tri], np.ones(11), c2)[3] == 1
    # a negative diagonal; an indefinite matrix with a positive diagonal
    N = M.copy()
    N[2, 2] = -N[2, 2]
    assert madpose.information_finish(N[tri], np.zeros(11), col)[3] == 0
    Q = np.eye(11)
    Q[0, 1] = Q[1, 0] = 2.0
    H, g, cov, pd = madpose.information_finish(Q[tri], np.zeros(11), col)
    assert pd == 0 and not np.any(cov)
    # a singular one: a repeated column
    J2 = J.copy()
    J2[:, 5] = J2[:, 3]
    S = J2.T @ J2
    pd = madpose.information_finish(S[tri], np.zeros(11), col)[3]
    print("exactly repeated column: pd", pd)  # (rounding decides the last pivot; cov is zero or huge)
    # no active parameter: nothing to invert, the factorisation of nothing completes
    H, g, cov, pd = madpose.information_finish(M[tri], np.ones(11), np.zeros(11, dtype=np.int32))
    assert pd == 1 and not np.any(cov) and not np.any(H) and not np.any(g)


def test_finish_non_finite_input_is_a_value():
    rng = np.random.default_rng(7)
    J = rng.standard_normal((30, 11))
    M = J.T @ J
    tri = np.triu_indices(11)
    col = np.ones(11, dtype=np.int32)
    for bad, at in ((np.nan, (3, 3)), (np.inf, (3, 3)), (-np.inf, (0, 0)), (np.nan, (1, 7)), (np.inf, (2, 9)),
                    (-np.inf, (0, 10))):
        B = M.copy()
        B[at] = B[at[::-1]] = bad
        H, g, cov, pd = madpose.information_finish(B[tri], np.full(11, np.nan), col)
        assert pd == 0 and not np.any(cov), (bad, at)
        assert np.all(np.isnan(g))  # (g is masked, not read)
    # the same entries on an inactive parameter are masked away
    B = M.copy()
    B[9, :] = B[:, 9] = np.nan
    c2 = col.copy()
    c2[9] = 0
    H, g, cov, pd = madpose.information_finish(B[tri], np.zeros(11), c2)
    assert pd == 1 and np.all(np.isfinite(H)) and np.all(np.isfinite(cov))


# ---- Python's checks ----

class _FakeDevice:
    """An object with __cuda_array_interface__ and nothing behind it (never dereferenced here)"""

    def __init__(self, typestr, shape, strides=None, readonly=False, ptr=4096):
        self.__cuda_array_interface__ = {"typestr": typestr, "shape": tuple(shape), "strides": strides,
                                         "data": (ptr, readonly), "version": 3}


def _unopened_set(variant=0, sizes=(20, 0, 7)):
    ps = madpose.PairSet.__new__(madpose.PairSet)
    ps.variant, ps.device, ps._hyp_error = variant, 0, None
    ps._h = ctypes.c_void_p(1)
    ps._sizes = list(sizes)
    ps._norm = np.ones(len(sizes))
    return ps


def test_python_checks_before_any_library_call(monkeypatch):
    ps = _unopened_set()

    def boom():
        raise AssertionError("the library was called")
    monkeypatch.setattr(L, "lib", boom)
    m = madpose.PoseScaleOffset()
    three = [m, m, m]
    # the model count, shape and dtype
    with pytest.raises(ValueError, match="one model per pair"):
        ps.information([m])
    with pytest.raises(ValueError, match="one model per pair"):
        ps.information(np.zeros((2, 17)))
    with pytest.raises(ValueError, match="one model per entry"):
        ps.information([m], pair_ids=[0, 0])
    with pytest.raises(ValueError, match=r"pair_ids\[1\] = 3 is outside"):
        ps.information([m, m], pair_ids=[0, 3])
    with pytest.raises(ValueError, match=r"pair_ids\[0\] = -1 is outside"):
        ps.information([m], pair_ids=[-1])
    for bad in (np.zeros((3, 16)), np.zeros(17), np.zeros((3, 17), dtype=np.float32), np.zeros((3, 17, 1))):
        with pytest.raises(ValueError, match="array models must be float64"):
            ps.information(bad)
    with pytest.raises(ValueError, match="models must be a sequence"):
        ps.information(5)
    # the factor
    for bad in (0.0, -1.0, np.nan, np.inf, -np.inf, [1.0, 0.0, 1.0], [1.0, 2.0, np.nan]):
        with pytest.raises(ValueError, match="factor must be finite and positive"):
            ps.information(three, factor=bad)
    with pytest.raises(ValueError, match="one factor value per entry"):
        ps.information(three, factor=[1.0, 2.0])
    for bad in (True, "2", None):
        with pytest.raises(ValueError, match="factor must be a number"):
            ps.information(three, factor=bad)
    with pytest.raises(ValueError, match="covariance must be True or False"):
        ps.information(three, covariance=1)
    # every output: dtype, shape, contiguity, read-only, kind -- host and device
    shapes = {"out_H": (3, 66), "out_g": (3, 11), "out_cost": (3,), "out_cov": (3, 11, 11)}
    for name, shape in shapes.items():
        call = lambda a: ps.information(three, **{name: a})
        with pytest.raises(ValueError, match=f"{name} must be float64 of shape"):
            call(np.zeros(shape, dtype=np.float32))
        with pytest.raises(ValueError, match=f"{name} must be float64 of shape"):
            call(np.zeros((2,) + shape[1:]))
        with pytest.raises(ValueError, match=f"{name} must be C-contiguous"):
            call(np.zeros((6,) + shape[1:])[::2])
        ro = np.zeros(shape)
        ro.flags.writeable = False
        with pytest.raises(ValueError, match=f"{name} is read-only"):
            call(ro)
        with pytest.raises(ValueError, match=f"{name} must be a numpy array or a device array"):
            call([0.0] * 3)
        with pytest.raises(ValueError, match=f"{name} must be float64, got typestr"):
            call(_FakeDevice("<f4", shape))
        with pytest.raises(ValueError, match=f"{name} must have shape"):
            call(_FakeDevice("<f8", (4,) + shape[1:]))
        with pytest.raises(ValueError, match=f"{name} must be C-contiguous"):
            call(_FakeDevice("<f8", shape, strides=tuple(16 * int(np.prod(shape[i + 1:])) for i in range(len(shape)))))
        with pytest.raises(ValueError, match=f"{name} is read-only"):
            call(_FakeDevice("<f8", shape, readonly=True))
        with pytest.raises(ValueError, match=f"{name} has no device address"):
            call(_FakeDevice("<f8", shape, ptr=0))
        other = "out_g" if name != "out_g" else "out_H"
        with pytest.raises(ValueError, match="one kind"):
            ps.information(three, **{name: np.zeros(shape), other: _FakeDevice("<f8", shapes[other], ptr=1 << 20)})
    # overlapping outputs, host and device; touching ones are fine as far as Python is concerned
    flat = np.zeros(3 * 66 + 3 * 11)
    with pytest.raises(ValueError, match="out_H and out_g overlap"):
        ps.information(three, out_H=flat[:198].reshape(3, 66), out_g=flat[190:223].reshape(3, 11))
    with pytest.raises(ValueError, match="out_cost and out_cov overlap"):
        ps.information(three, out_cost=_FakeDevice("<f8", (3,), ptr=4096 + 8 * 362),
                       out_cov=_FakeDevice("<f8", (3, 11, 11), ptr=4096))
    with pytest.raises(ValueError, match="stream goes with device outputs"):  # (past the overlap check)
        ps.information(three, out_H=flat[:198].reshape(3, 66), out_g=flat[198:231].reshape(3, 11), stream=0)
    # the stream
    with pytest.raises(ValueError, match="stream goes with device outputs"):
        ps.information(three, stream=0)
    for bad in (-1, 1.5, True, "0"):
        with pytest.raises(ValueError, match="stream must be None"):
            ps.information(three, out_H=_FakeDevice("<f8", (3, 66)), stream=bad)
    # no row at all, and no entry: answered without the library
    H = np.full((2, 66), np.nan)
    res = ps.information([m, m], pair_ids=[1, 1], out_H=H)
    assert res.H is H and not np.any(H) and res.cov.shape == (2, 11, 11) and not np.any(res.cov)
    assert res.pd.tolist() == [-1, -1] and res.status.tolist() == [0, 0] and res.rows.tolist() == [0, 0]
    assert not np.any(res.col) and not np.any(res.counts) and not np.any(res.g) and not np.any(res.cost)
    assert ps.information([m], pair_ids=[1], covariance=False).cov is None
    with pytest.raises(ValueError, match="no covariance: pd = -1"):
        res.covariance(0)
    assert res.matrix(1).shape == (11, 11)
    res = ps.information([], pair_ids=[])
    assert res.H.shape == (0, 66) and res.g.shape == (0, 11) and res.cost.shape == (0,) and res.cov.shape == (0, 11, 11)
    assert res.col.shape == (0, 11) and res.pd.shape == (0,) and res.counts.shape == (0, 3)
    # a closed set
    ps._h = None
    with pytest.raises(ValueError, match="closed"):
        ps.information(three)


def test_result_helpers():
    """matrix and covariance on a hand-made result: the symmetric H, the active restriction, the
    focal's norm_scale per index and the variance factor 2 cost / (rows - n)"""
    rng = np.random.default_rng(9)
    J = rng.standard_normal((50, 11))
    J[:, 10] = 0.0
    M = J.T @ J
    col = np.ones(11, dtype=np.int32)
    col[10] = 0
    H, g, cov, pd = madpose.information_finish(M[np.triu_indices(11)], np.zeros(11), col)
    r = madpose.InformationResult()
    r.H, r.g, r.cost, r.cov = H[None], g[None], np.array([3.0]), cov[None]
    r.col, r.pd, r.status, r.rows = col[None], np.array([pd]), np.array([1]), np.array([50])
    r.counts, r.norm_scale, r.focal_columns = np.zeros((1, 3), np.int32), np.array([400.0]), (9,)
    assert np.array_equal(r.matrix(0)[:10, :10], M[:10, :10]) and not np.any(r.matrix(0)[10])
    C = r.covariance(0, scaled=False)
    assert C.shape == (10, 10) and np.array_equal(C, C.T)
    assert np.allclose(C, np.linalg.inv(M[:10, :10]), rtol=1e-9, atol=0)
    S = r.covariance(0)
    s = np.ones(10)
    s[9] = 400.0
    assert np.allclose(S, C * np.outer(s, s) * (2 * 3.0 / (50 - 10)), rtol=1e-14, atol=0)
    r.rows = np.array([10])
    with pytest.raises(ValueError, match="no variance factor"):
        r.covariance(0)
    assert r.covariance(0, scaled=False).shape == (10, 10)
    r.pd = np.array([0])
    with pytest.raises(ValueError, match="pd = 0"):
        r.covariance(0, scaled=False)


def _empty_set(variant=0):
    o, c = synthetic.example_options("calibrated")
    return madpose.PairSet(variant, [], o, c, device=NO_DEVICE)


@pytest.mark.parametrize("variant", [0, 1, 2, 3])
def test_c_refusals_before_any_device(variant):
    lib = L.lib()
    with _empty_set(variant) as ps:
        h = ps._h
        mods = (L.mp_model * 2)()
        bufs = [(ctypes.c_double * n)() for n in (132, 22, 2, 242)]
        out = L.mp_information_out()
        out.H, out.g, out.cost, out.cov = [ctypes.addressof(b) for b in bufs]
        ent = (L.mp_information_entry * 2)()
        i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)
        f64 = lambda *v: (ctypes.c_double * len(v))(*v)
        call = lambda **kw: lib.mp_information_set(*[kw.get(k, d) for k, d in (
            ("set", h), ("n", 0), ("ids", None), ("models", mods), ("factors", None), ("out", ctypes.byref(out)),
            ("ent", ent))])
        # no entry is the only legal call on an empty set, and it needs no device
        assert call() == L.MP_OK
        assert call(ids=i32(0), factors=f64(2.0), ent=None) == L.MP_OK
        assert call(set=None) == L.MP_EINVAL and b"null pair set" in lib.mp_last_error()
        assert call(out=None) == L.MP_EINVAL and b"null out" in lib.mp_last_error()
        assert call(n=1, ids=i32(0), ent=None) == L.MP_EINVAL and b"null entries" in lib.mp_last_error()
        for on_device in (0, 1):  # (the checks do not depend on where the outputs are)
            out.on_device = on_device
            assert call(n=-1) == L.MP_EINVAL and b"num_entries" in lib.mp_last_error()
            assert call(n=(1 << 24) + 1) == L.MP_EINVAL and b"num_entries" in lib.mp_last_error()
            assert call(n=1) == L.MP_EINVAL and b"pair count" in lib.mp_last_error()
            for bad in (0, -1, 1):
                assert call(n=1, ids=i32(bad)) == L.MP_EINVAL and b"outside the set" in lib.mp_last_error()
            for bad in (0.0, -1.0, -0.0, float("nan"), float("inf"), -float("inf")):
                assert call(n=2, ids=i32(0, 0), factors=f64(1.5, bad)) == L.MP_EINVAL
                assert b"factors[1] must be finite and > 0" in lib.mp_last_error()
        out.on_device = 0
        assert call(n=0, factors=f64(0.0)) == L.MP_OK  # (no entry: no factor is read)


def test_hooks_without_a_device():
    lib = L.lib()
    n, a, b = ctypes.c_int64(-1), ctypes.c_double(-1.0), ctypes.c_double(-1.0)
    assert lib.mp_debug_information_stats(ctypes.byref(n), ctypes.byref(a), ctypes.byref(b), 1) == L.MP_OK
    assert lib.mp_debug_information_stats(ctypes.byref(n), ctypes.byref(a), ctypes.byref(b), 0) == L.MP_OK
    assert n.value == 0 and a.value == 0.0 and b.value == 0.0
    assert lib.mp_debug_information_stats(None, None, None, 0) == L.MP_OK
    H, cov, pd = (ctypes.c_double * 66)(), (ctypes.c_double * 121)(), ctypes.c_int32()
    assert lib.mp_debug_information_finish(H, None, None, cov, ctypes.byref(pd)) == L.MP_EINVAL
    assert b"null argument" in lib.mp_last_error()
