"""One LM evaluation and one LM step of the device LM (mp_debug_lm_system, where = 0:
lm_system_kernel runs the production setup, lm_evaluate, lm_reduce and lm_step of
kernels/lm_device.h) against tests/lm_reference.py: the three Jacobian blocks in their three
variants against 50 digits, the 256-lane reduction and the carry of the block index from
one list into the next against float64 + fsum, the masked Cholesky step by its backward
error on the active system ("the extra terms are exact zeros", LmShared), and the first
step of lm_batch_kernel against the hook's.  Cases, bounds and constants:
tests/lm_system_cases.py; the host side of the same checks: tests/test_lm_system_cpu.py.
Device and host are not compared with each other to the bit: they sum in different orders,
and each is held to the reference.
"""
import numpy as np
import pytest

import madpose
from tests import lm_reference as LR
from tests import lm_system_cases as SC

pytestmark = pytest.mark.gpu

# measured on an MI355X (printed by every run): the device's worst per-term error on the
# 50-digit cases, in units of 2^-53 S_X beside the rows' own share, per variant; the
# reference's float64 yardstick is SC.K_REF = 821 and the allowance SC.K_ENGINE = 16 K_REF
DEVICE_WORST_MEASURED = {0: 296.0, 1: 250.2, 2: 801.9}

TOTALS = (1, 63, 64, 65, 255, 256, 257, 511, 513, 1025)
SPLITS = ((100, 100, 100), (255, 2, 255), (1, 256, 1), (0, 257, 300), (300, 0, 1))


@pytest.fixture(scope="module", autouse=True)
def require_gpu():
    if madpose.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on an MI355X")


@pytest.fixture(scope="module")
def formula():
    out = {}
    for v in (0, 1, 2):
        cx = SC.small(v)
        specs = SC.formula_specs(v)
        out[v] = (cx, specs, [SC.reference(cx, s, "mp") for s in specs])
    return out


def test_formulas_against_50_digits(formula):
    worst = {}
    for v, (cx, specs, refs) in formula.items():
        got = SC.engine(cx, specs, 0)
        for j, (g, r, s) in enumerate(zip(got, refs, specs)):
            assert g["status"] == 1 and g["pd"] == 1
            k = SC.check_system(g, r, 0, (v, j))
            na = 9 + v
            assert not np.any(g["g"][na:]) and not np.any(g["d"][na:]) and not np.any(g["col"][na:])
            typ = "+".join(n for n, l in zip(("reproj0", "reproj1", "sampson"), SC.effective_lists(s)) if len(l))
            worst[(v, typ)] = max(worst.get((v, typ), 0.0), k)
    for key in sorted(worst):
        print("variant %d %-24s worst per-term error %.1f" % (*key, worst[key]))
    for v in (0, 1, 2):
        print(f"variant {v}: device worst {max(w for (vv, _), w in worst.items() if vv == v):.1f} "
              f"(recorded {DEVICE_WORST_MEASURED[v]}); K_REF {SC.K_REF}, allowance {SC.K_ENGINE}")


def test_single_sampson_block_is_the_jacobian_row(formula):
    for v, (cx, specs, refs) in formula.items():
        s = specs[2]
        res, J = LR.jacobian(v, cx.data, s.lists, SC.params_of(s.model, v))
        g = SC.engine(cx, [s], 0)[0]
        rr = np.sign(float(res[0])) * np.sqrt(2 * g["cost"])
        for a in range(11):
            ja = float(J[0][a])
            if ja == 0.0:
                assert g["g"][a] == 0.0
            else:
                assert abs(g["g"][a] / rr - ja) <= (SC.K_ENGINE + 4) * SC.U * abs(ja), (v, a)


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_reduction_and_list_carry(variant):
    """totals around the wave, the workgroup and its multiples in one list (each list type
    in turn), and splits whose list boundaries fall inside a 256-stride; one launch"""
    cx = SC.big(variant)
    rng = np.random.default_rng(1000 + variant)
    sizes = []
    for i, T in enumerate(TOTALS):
        sz = [0, 0, 0]
        sz[i % 3] = T
        sizes.append(tuple(sz))
    sizes += list(SPLITS)
    specs = [SC.spec(rng, cx, sz) for sz in sizes]
    got = SC.engine(cx, specs, 0)
    worst = 0.0
    for sz, s, g in zip(sizes, specs, got):
        r = SC.reference(cx, s, "f64")
        if sum(sz) == 1:
            # one block alone: S_cost = r^2 / 2 does not see the cancellation inside the
            # residual (test_lm_system_cpu.py::test_ranges_and_tails), so it goes against 50 digits
            r = SC.reference(cx, s, "mp")
        worst = max(worst, SC.check_system(g, r, 0, (variant, sz)))
    print(f"variant {variant}: {len(specs)} problems, worst per-term error {worst:.1f}")


def test_many_problems_one_launch():
    """40 problems of one pair in one launch, each at its own offset into the index array;
    a problem alone and the same problem among the others return identical bytes"""
    for variant in (0, 2):
        cx = SC.big(variant)
        rng = np.random.default_rng(1100 + variant)
        specs = []
        for j in range(40):
            sz = [int(rng.integers(0, 300)), int(rng.integers(0, 300)), int(rng.integers(1, 300))]
            if j % 7 == 3:
                sz[int(rng.integers(0, 2))] = 0
            specs.append(SC.spec(rng, cx, tuple(sz), kind=j % 2))
        got = SC.engine(cx, specs, 0, radius=1.0)
        for j, (s, g) in enumerate(zip(specs, got)):
            SC.check_system(g, SC.reference(cx, s, "f64"), 0, (variant, j))
        for j in (0, 17, 39):
            alone = SC.engine(cx, [specs[j]], 0, radius=1.0)[0]
            for k in ("cost", "g", "H", "d", "col", "pd"):
                assert np.asarray(alone[k]).tobytes() == np.asarray(got[j][k]).tobytes(), (variant, j, k)


def test_step_backward_error(formula):
    worst = 0.0
    for v, (cx, specs, _) in formula.items():
        for radius in (1e4, 1.0, 1e-3):
            for j, g in enumerate(SC.engine(cx, specs, 0, radius=radius)):
                worst = max(worst, SC.check_step(g, radius, (v, radius, j)))
    print(f"worst backward error over n u (|A||y| + |b|): {worst:.2f}")


def test_step_clamp():
    for v in (0, 1, 2):
        cx2, s = SC.clamp_case(v)
        r = SC.reference(cx2, s, "mp")
        for radius in (1e4, 1.0):
            g = SC.engine(cx2, [s], 0, radius=radius)[0]
            diag = np.array([g["H"][LR._up(a, a)] for a in range(11) if g["col"][a]])
            assert np.all(diag < 1e-6) and np.any(diag > 0)
            SC.check_system(g, r, 0, (v, radius))
            SC.check_step(g, radius, (v, radius))


def test_step_non_finite_is_a_value():
    for v in (0, 1, 2):
        cx, s = SC.nan_case(v)
        g = SC.engine(cx, [s], 0)[0]
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
    for s, st in ((s0, 0), (s2, 2)):
        g = SC.engine(cx, [s], 0)[0]
        assert g["status"] == st and g["pd"] == -1
        assert g["cost"] == 0.0 and not np.any(g["g"]) and not np.any(g["H"]) and not np.any(g["d"])


def test_first_step_of_lm_batch_kernel_is_plus_of_the_hook_step():
    """iteration cap 1: lm_refine_batch's model is, bit for bit, Plus(start, d) of the
    hook's d, in the product form of the kernel"""
    res = SC.first_step_ties(False, 0, SC.DEVICE_FORM)
    print(res)
    for v, (total, same) in res.items():
        assert total >= 4, (v, "too few accepted first steps: choose other seeds")
        assert same == total, (v, total, same)
