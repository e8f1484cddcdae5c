"""One LM evaluation and one LM step of the host evaluators (mp_debug_lm_system, where = 1:
lm_eval_range_w4, 2: lm_eval_range_w8, 3: lm.cpp evaluate() as lm_refine calls it) against
tests/lm_reference.py: the per-block formulas against 50 digits, the reductions and vector
tails against float64 + fsum, the step by its backward error, and the claims that rode on
whole-run tests until now --

* "identical results either way" of the AVX2 and AVX-512 builds (host/lm.cpp
  lm_eval_avx512, host/lm_eval.h): test_w4_equals_w8_bytes;
* "the result does not depend on the pool" (host/lm.cpp): test_switches_do_not_change_the_host_lm;
* the tails of the 8-wide loops across list boundaries: test_ranges_and_tails,
  test_eval_under_sanitizers.

The reference is cross-checked first, by itself and against the oracle.  Cases, bounds and
the constants K_REF / K_ENGINE: tests/lm_system_cases.py.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from tests import lm_cases as LC
from tests import lm_reference as LR
from tests import lm_system_cases as SC
from tests.helpers import oracle_cfg, oracle_opts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/llvm/bin/clang++"
HOST = os.path.join(ROOT, "madpose_amd", "csrc", "host")

# measured on the 50-digit cases (printed by every run): the reference's float64 mode
# against its 50-digit mode, worst per-entry |dX| / (2^-53 S_X), per variant 795.6 / 173.0
# / 820.3 (SC.K_REF = 821 holds it); the host evaluators' worst per-term part on the same
# scale, per variant 296.0 / 218.1 / 801.9, identical for w4, w8 and evaluate()
HOST_WORST_MEASURED = 801.9


def have_w8():
    with open("/proc/cpuinfo") as f:
        flags = f.read()
    return all(k in flags for k in (" avx512f", " avx512dq", " avx512vl"))


def wheres():
    if not have_w8():
        print("this CPU has no AVX-512: lm_eval_range_w8 (where = 2) is not run")
        return (1, 3)
    return (1, 2, 3)


@pytest.fixture(scope="module")
def formula():
    """per variant: the context, the 50-digit problems and their references, computed once"""
    out = {}
    for v in (0, 1, 2):
        cx = SC.small(v)
        specs = SC.formula_specs(v)
        out[v] = (cx, specs, [SC.reference(cx, s, "mp") for s in specs])
    return out


# ---- the reference, by itself ----

def test_reference_cost_matches_lm_cost(formula):
    for v, (cx, specs, refs) in formula.items():
        for s, r in zip(specs, refs):
            c = LC.lm_cost(v, cx.args, cx.o, SC.config_of(s), s.model, s.lists, cx.norm_scale)
            assert abs(r["cost"] - c) <= 1e-12 * c, (v, r["cost"], c)


def test_reference_jets_against_central_differences(formula):
    """two independent routes to the Jacobian: forward-mode jets with the first-order step
    quaternion, and central differences at 60 digits through Plus itself (step 1e-25:
    truncation ~1e-50 relative, cancellation ~1e-35)"""
    for v, (cx, specs, _) in formula.items():
        for s in specs[:3] + specs[3:6]:
            lists = SC.effective_lists(s)
            _, J = LR.jacobian(v, cx.data, lists, SC.params_of(s.model, v))
            Jc = LR.central_jacobian(v, cx.data, lists, SC.params_of(s.model, v))
            assert len(J) == len(Jc) > 0
            for row, rowc in zip(J, Jc):
                scale = max(abs(x) for x in row)
                assert all(abs(a - b) <= 1e-30 * scale for a, b in zip(row, rowc)), (v, row, rowc)


def test_reference_step_against_oracle():
    """The reference's Jacobian through the oracle (Ceres' trust-region LM restated, jets of
    its own): with an iteration cap of 1 the oracle returns Plus(start, d) of its first step,
    and d must equal the step of the reference's own system (H, g at 50 digits, radius 1e4).
    In the Jacobi-scaled unknowns y = d / D the oracle's doubles may differ by kappa(A) u |y|
    ((3 n + 4) n + 2 (K_REF + rows)): the solve's backward error (check_step) and an assembly
    error of (K_REF + rows) u in A and in b, through the condition number of A, which the
    test computes; beside it 8 u of the parameter itself for forming the difference.  A wrong
    Jacobian moves y by a fraction of |y|, so the tolerance is also held below 1e-3 |y|."""
    for v in (0, 1, 2):
        cx = SC.small(v)
        rng = np.random.default_rng(700 + v)
        for sizes, kind in (((8, 8, 8), 0), ((12, 0, 9), 1), ((0, 7, 8), 0)):
            s = SC.spec(rng, cx, sizes, kind=kind)
            c = SC.config_of(s)
            c.ceres_max_num_iterations = 1
            ref, ran = oracle.least_squares(v, *cx.args, oracle_opts(cx.o), oracle_cfg(c), kind, s.lists,
                                            LC.oracle_model(s.model, v))
            assert ran
            r = SC.reference(cx, s, "mp")
            A, b, D, act = LR.damped_system(r["H"], r["g"], r["col"], 1e4)
            n = len(act)
            y = LR.MP.lu_solve(LR.MP.matrix(A), LR.MP.matrix(b))
            An = np.array([[float(x) for x in row] for row in A])
            kappa = np.linalg.norm(An, np.inf) * np.linalg.norm(np.linalg.inv(An), np.inf)
            ymax = max(abs(float(x)) for x in y)
            tol = kappa * SC.U * ymax * ((3 * n + 4) * n + 2 * (SC.K_REF + r["rows"]))
            assert tol < 1e-3 * ymax, (v, sizes, kappa)
            # the oracle's step from its result
            q0, t0, sc0, o00, o10, f00, f10 = SC.params_of(s.model, v)
            m1 = LC.model_of(ref, v)
            q1, t1, sc1, o01, o11, f01, f11 = SC.params_of(m1, v)
            qd = LR._quat_mul([float(x) for x in q1], [q0[0], -q0[1], -q0[2], -q0[3]])
            nv = np.linalg.norm(qd[1:])
            delta = np.asarray(qd[1:]) / nv * np.arctan2(nv, qd[0])
            if delta @ np.array([float(y[i]) * float(D[i]) for i in range(3)]) < 0:
                delta = -(np.asarray(qd[1:]) / nv * np.arctan2(nv, -qd[0]))  # (q and -q: one rotation)
            d_or = np.r_[delta, t1 - t0, sc1 - sc0, o01 - o00, o11 - o10, f01 - f00, f11 - f10]
            mag = np.r_[np.ones(3), np.abs(t0), abs(sc0), abs(o00), abs(o10), abs(f00), abs(f10)]
            assert not np.array_equal(d_or, np.zeros(11)), "the oracle's first step was not accepted"
            worst = 0.0
            for i, a in enumerate(act):
                err = abs(d_or[a] / float(D[i]) - float(y[i]))
                lim = tol + 8 * SC.U * mag[a] / float(D[i])
                worst = max(worst, err / lim)
                assert err <= lim, (v, sizes, a, d_or[a], float(y[i]) * float(D[i]), err, lim)
            print(f"variant {v} sizes {sizes}: kappa {kappa:.3g}, worst step error / tolerance {worst:.3g}")


def test_reference_float64_yardstick(formula):
    """k_ref: the float64 mode against the 50-digit mode, per entry in units of 2^-53 S_X;
    both modes agree to 1e-11 S_X (a guard band of the cases) and K_REF holds the measured
    value, so the engine's allowance 16 K_REF is tied to this run's own yardstick"""
    for v, (cx, specs, refs) in formula.items():
        k_ref = 0.0
        for s, r in zip(specs, refs):
            f = SC.reference(cx, s, "f64")
            assert f["rows"] == r["rows"]
            k_ref = max(k_ref, float(np.nanmax(SC.scaled_errors(f, r))))
        print(f"variant {v}: k_ref = {k_ref:.1f} (K_REF {SC.K_REF}, engine allowance {SC.K_ENGINE})")
        assert k_ref * SC.U <= 1e-11
        assert k_ref <= SC.K_REF


def test_formula_block_count(formula):
    """the 50-digit cases stay at about 600 residual blocks in all"""
    blocks = sum(len(l) for _, specs, _ in formula.values() for s in specs for l in SC.effective_lists(s))
    assert 500 <= blocks <= 600, blocks


# ---- the per-block formulas against 50 digits ----

def test_formulas_against_50_digits(formula):
    worst = {}
    for v, (cx, specs, refs) in formula.items():
        for where in wheres():
            got = SC.engine(cx, specs, where)
            for j, (g, r, s) in enumerate(zip(got, refs, specs)):
                assert g["status"] == 1 and g["pd"] == 1
                k = SC.check_system(g, r, where, (v, where, j))
                typ = "+".join(n for n, l in zip(("reproj0", "reproj1", "sampson"), SC.effective_lists(s)) if len(l))
                worst[(v, where, typ)] = max(worst.get((v, where, typ), 0.0), k)
    for key in sorted(worst):
        print("variant %d where %d %-24s worst per-term error %.1f" % (*key, worst[key]))
    print(f"host worst {max(worst.values()):.1f} (recorded {HOST_WORST_MEASURED}); allowance {SC.K_ENGINE}")


def test_single_sampson_block_is_the_jacobian_row(formula):
    """one Sampson block: g / r is the Jacobian row itself, entry by entry"""
    for v, (cx, specs, refs) in formula.items():
        s, r = specs[2], refs[2]
        assert [len(l) for l in s.lists] == [0, 0, 1]
        res, J = LR.jacobian(v, cx.data, s.lists, SC.params_of(s.model, v))
        for where in wheres():
            g = SC.engine(cx, [s], where)[0]
            rr = np.sign(float(res[0])) * np.sqrt(2 * g["cost"])
            for a in range(11):
                ja = float(J[0][a])
                if ja == 0.0:
                    assert g["g"][a] == 0.0
                else:
                    assert abs(g["g"][a] / rr - ja) <= (SC.K_ENGINE + 4) * SC.U * abs(ja), (v, where, a)


def test_w4_equals_w8_bytes(formula):
    """host/lm_eval.h: the two builds of lm_eval.inc give identical results"""
    if not have_w8():
        print("skipped: this CPU has no AVX-512, only lm_eval_range_w4 exists here")
        return
    for v, (cx, specs, _) in formula.items():
        a, b = SC.engine(cx, specs, 1, radius=1.0), SC.engine(cx, specs, 2, radius=1.0)
        for x, y in zip(a, b):
            for k in ("cost", "g", "H", "d"):
                assert np.asarray(x[k]).tobytes() == np.asarray(y[k]).tobytes(), (v, k)
    cx = SC.big(1)
    specs = [SC.spec(np.random.default_rng(5), cx, (700, 650, 699))]
    a, b = SC.engine(cx, specs, 1), SC.engine(cx, specs, 2)
    for k in ("cost", "g", "H", "d"):
        assert np.asarray(a[0][k]).tobytes() == np.asarray(b[0][k]).tobytes(), k


def test_where_2_without_avx512_is_einval():
    if have_w8():
        return
    cx = SC.small(0)
    s = SC.formula_specs(0)[3]
    with pytest.raises(Exception):
        SC.engine(cx, [s], 2)


# ---- reductions and tails against float64 + fsum ----

def sub_lists(lists, b0, b1):
    """blocks [b0, b1) of the concatenated list as three lists"""
    out, off = [], 0
    for l in lists:
        out.append(l[max(b0 - off, 0):max(min(b1 - off, len(l)), 0)])
        off += len(l)
    return out


def test_ranges_and_tails():
    """w4 and w8 over ranges [b0, b1) of the concatenated list: the list lengths, the range
    starts and the range ends take every residue modulo 8, and b0 falls inside every list.
    The ranges hold at least 16 blocks: the bound's S_cost = sum r^2 / 2 says nothing about
    the cancellation inside one residual, and on a single inlier block with |r| ~ 0.03 px of
    300 px even the float64 reference is 9e4 units away from the 50-digit value.  These
    ranges are small enough for 50 digits (prefix sums over the rows): the float64 yardstick
    is held on them too, and the engine is held to the 50-digit values."""
    for v in (0, 1, 2):
        cx = SC.small(v)
        rng = np.random.default_rng(800 + v)
        specs, ranges, refs = [], [], []
        k_ref = 0.0
        for r in range(8):
            sizes = (24 + r, 24 + (r + 3) % 8, 25 + (r + 5) % 8)
            s = SC.spec(rng, cx, sizes)
            nb = sum(sizes)
            sums = LR.RangeSums(v, cx.data, s.lists, SC.params_of(s.model, v))
            for b0 in (0, r, sizes[0] - 3, sizes[0] + 1 + r, sizes[0] + sizes[1] - 5):
                for b1 in range(b0 + 16, nb + 1):
                    specs.append(s)
                    ranges.append((b0, b1))
                    refs.append(sums.system(b0, b1))
                    if (b1 - b0) % 5 == 0:  # the yardstick on a fifth of them
                        f = LR.system(v, cx.data, sub_lists(s.lists, b0, b1), SC.params_of(s.model, v), "f64")
                        assert f["rows"] == refs[-1]["rows"]
                        k_ref = max(k_ref, float(np.nanmax(SC.scaled_errors(f, refs[-1]))))
        assert k_ref <= SC.K_REF, k_ref
        assert {b0 % 8 for b0, _ in ranges} == {b1 % 8 for _, b1 in ranges} == set(range(8))
        worst = 0.0
        for where in wheres()[:-1]:
            got = SC.engine(cx, specs, where, ranges=ranges)
            for g, r, rg in zip(got, refs, ranges):
                w = float(np.nanmax(SC.scaled_errors(g, r)))
                assert w <= SC.K_ENGINE + r["rows"], (v, where, rg, w)
                worst = max(worst, w - r["rows"])
            # an empty range adds nothing
            g = SC.engine(cx, specs[:1], where, ranges=[(7, 7)])[0]
            assert g["cost"] == 0.0 and not np.any(g["H"]) and not np.any(g["g"])
        print(f"variant {v}: {len(specs)} ranges, float64 yardstick {k_ref:.1f}, worst per-term error {worst:.1f}")


TOTALS = (255, 256, 257, 2047, 2048, 2049, 16384, 16641)


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_evaluate_chunks_and_pool(variant):
    """evaluate(): one chunk, several, the pool from 2048 blocks, and 64 -> 65 chunks where
    the partial sums move from the stack to the heap; strictly increasing lists over a pair
    of 6000 correspondences"""
    cx = SC.big(variant)
    rng = np.random.default_rng(900 + variant)
    specs = [SC.spec(rng, cx, (T // 3, T // 3, T - 2 * (T // 3))) for T in TOTALS]
    for s in specs:
        assert all(np.all(np.diff(l) > 0) for l in s.lists)
    got = SC.engine(cx, specs, 3)
    worst = 0.0
    for T, s, g in zip(TOTALS, specs, got):
        r = SC.reference(cx, s, "f64")
        assert r["rows"] == 2 * (T // 3) * 2 + T - 2 * (T // 3)
        worst = max(worst, SC.check_system(g, r, 3, (variant, T)))
    print(f"variant {variant}: totals {TOTALS}, worst per-term error {worst:.1f}")


# ---- the step ----

def test_step_backward_error(formula):
    worst = 0.0
    for v, (cx, specs, _) in formula.items():
        for radius in (1e4, 1.0, 1e-3):
            for where in (1, 3):
                for j, g in enumerate(SC.engine(cx, specs, where, radius=radius)):
                    worst = max(worst, SC.check_step(g, radius, (v, radius, where, j)))
    print(f"worst backward error over n u (|A||y| + |b|): {worst:.2f}")


def test_step_clamp():
    for v in (0, 1, 2):
        cx2, s = SC.clamp_case(v)
        r = SC.reference(cx2, s, "mp")
        for where in (1, 3):
            for radius in (1e4, 1.0):
                g = SC.engine(cx2, [s], where, radius=radius)[0]
                diag = np.array([g["H"][LR._up(a, a)] for a in range(11) if g["col"][a]])
                assert np.all(diag < 1e-6) and np.any(diag > 0)
                SC.check_system(g, r, where, (v, where))
                SC.check_step(g, radius, (v, where, radius))


def test_step_non_finite_is_a_value():
    """a NaN offset: the system is not finite, "not positive definite" on both sides, d = 0"""
    for v in (0, 1, 2):
        cx, s = SC.nan_case(v)
        for where in wheres():
            g = SC.engine(cx, [s], where)[0]
            assert g["status"] == 1 and g["pd"] == 0 and not np.any(g["d"])
            assert np.isnan(g["cost"])
            A, b, D, act = LR.damped_system(g["H"], g["g"], g["col"], 1e4)
            assert not LR.positive_definite(A)


def test_nothing_to_evaluate():
    """no residuals (status 0) and an infeasible constant bounded block (status 2): pd = -1,
    everything else zero"""
    cx = SC.small(0)
    rng = np.random.default_rng(3)
    s0 = SC.spec(rng, cx, (0, 0, 0))
    s2 = SC.spec(rng, cx, (4, 4, 4), use_shift=False, mdc=True)
    s2 = s2._replace(model=SC.with_offsets(s2.model, 0, -1e3, s2.model.offset1))
    for where in wheres():
        for s, st in ((s0, 0), (s2, 2)):
            g = SC.engine(cx, [s], where)[0]
            assert g["status"] == st and g["pd"] == -1
            assert g["cost"] == 0.0 and not np.any(g["g"]) and not np.any(g["H"]) and not np.any(g["d"])


# ---- the hook runs what lm_refine runs ----

def test_first_step_of_lm_refine_is_plus_of_the_hook_step():
    """the host LM (on_host) against the hook's where = 3, with the host build's contraction"""
    res = SC.first_step_ties(True, 3, "host")
    print(res)
    for v, (total, same) in res.items():
        assert total >= 4, (v, "too few accepted first steps: choose other seeds")
        assert same == total, (v, total, same)


# ---- switches ----

def run_worker(env_extra):
    env = {k: v for k, v in os.environ.items() if k not in ("MADPOSE_LO_THREADS", "MADPOSE_LM_WIDE", "MADPOSE_LM_ISA")}
    env.update(env_extra)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "lm_system_worker.py")], capture_output=True,
                       text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_switches_do_not_change_the_host_lm():
    """host/lm.cpp: "the result does not depend on the pool" (bench.py sets
    MADPOSE_LO_THREADS per box) nor on the wide threshold or the ISA: a 2049-block and a
    300-block problem under every setting return identical model bytes and status"""
    base = run_worker({})
    assert [x["status"] for x in base] == [1, 1]
    for env in ({"MADPOSE_LO_THREADS": "1"}, {"MADPOSE_LO_THREADS": "8"}, {"MADPOSE_LM_WIDE": "1"},
                {"MADPOSE_LM_ISA": "avx2"}):
        assert run_worker(env) == base, env


# ---- memory safety of the tails ----

def test_eval_under_sanitizers(tmp_path):
    if not os.path.exists(CLANG):
        pytest.fail(f"{CLANG} missing: the host build of the evaluation needs ROCm's clang")
    flags = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
             "-fno-omit-frame-pointer", "-mprefer-vector-width=512", "-I", HOST]
    units = [("lm_eval_w4.cpp", "-march=x86-64-v3")]
    if have_w8():
        units.append(("lm_eval_w8.cpp", "-march=x86-64-v4"))
    else:
        print("this CPU has no AVX-512: only lm_eval_range_w4 is checked")
    objs = []
    for src, march in units:
        obj = str(tmp_path / (src + ".o"))
        r = subprocess.run([CLANG] + flags + [march, "-c", os.path.join(HOST, src), "-o", obj], capture_output=True,
                           text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        objs.append(obj)
    exe = str(tmp_path / "lm_eval_check")
    cmd = [CLANG] + flags + (["-DLM_EVAL_CHECK_W8"] if have_w8() else [])
    r = subprocess.run(cmd + [os.path.join(ROOT, "tests", "lm_eval_check.cpp")] + objs + ["-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().endswith("ok")
