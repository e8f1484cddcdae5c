"""The cases and comparisons of tests/test_information_gpu.py (and the column check that
tests/test_information_cpu.py shares), and its device-output checks run in a process of their
own: `python -m tests.information_worker` imports torch first (one HIP runtime in the process,
INTEGRATION.md), runs every check (or those named on the command line) and prints one JSON object
{name: {"ok": bool, "seconds": s, "detail": text}} as its last line -- the pattern of
tests/residuals_worker.py, whose pairs, models and guarded buffers are used as they are.

The reference of every device-output check is the same call with host outputs."""
import functools
import sys

import numpy as np

import madpose
from madpose_amd import synthetic
from tests import lm_reference as LR
from tests import lm_system_cases as SC
from tests import refine_cases as RC
from tests import residuals_worker as W

ITEM = 4096  # rows per item (host/information_plan.h kInfoItemRows): residuals' item, so W.SIZES fit
BIG = 6000
OUTPUTS = ("H", "g", "cost", "cov")
SHAPES = {"H": (66,), "g": (11,), "cost": (), "cov": (11, 11)}

CHECKS = {}


def check(*params):
    """register a check, once per parameter tuple"""
    def reg(fn):
        name = fn.__name__.replace("check_", "", 1)
        for p in params or [()]:
            CHECKS[name + ("[" + "-".join(str(v) for v in p) + "]" if p else "")] = (fn, p)
        return fn
    return reg


def geometry(variant):
    """the kernels' variant: scale only runs on the calibrated geometry"""
    return 0 if variant == 3 else variant


# ---- the column check of the covariance (CPU and GPU) ----

def column_check(H, col, cov, tag):
    """The inverse on the function's own H: with D_a = 1 / sqrt(H_aa) and A = D H D at 50 digits
    from the doubles, and y_k = cov[:, k] with D removed (cov[a, k] / (D_a D_k)), for every active
    column k: |A y_k - e_k|_inf <= c n 2^-53 (|A|_inf |y_k|_inf + 1), c = 3 n + 4.  Returns the
    worst ratio |A y_k - e_k|_inf / (n 2^-53 (|A|_inf |y_k|_inf + 1)).

    c is SC.check_step's (Higham, Accuracy and Stability of Numerical Algorithms, Theorem 10.4:
    Cholesky and the two triangular solves give (A + dA) y = b with |dA| <= gamma_{3n+1} |L||L^T|,
    and (|L||L^T|)_ij <= sqrt(a_ii a_jj) = 1 up to rounding on the unit diagonal, so |dA y|_inf <=
    (3 n + 1) n u |A|_inf |y|_inf to first order).  The operation count beside the factorisation
    differs from lm_step's, so the remainder is derived again: D_a takes two roundings (sqrt,
    division; lm_step: three), an entry of D H D two products, so the matrix factored is A (1 +
    delta) entrywise with |delta| <= (2 + 2 * 2) u = 6 u; b = e_k is exact (lm_step: one rounding);
    the result y_a D_a D_k takes two products (lm_step: one) and carries the two roundings of each
    of its D factors, (2 + 4) u relative on y.  Together 12 u |A|_inf |y|_inf, below 3 n u (|A|_inf
    |y|_inf + 1) for n >= 6, the smallest system (six pose parameters are always active).  Hence
    (3 n + 1) n + 3 n = (3 n + 4) n: the same constant, not tuned."""
    mp = LR.MP
    act = [a for a in range(11) if col[a]]
    n = len(act)
    f = lambda v: mp.mpf(float(v))
    D = [1 / mp.sqrt(f(H[LR._up(a, a)])) for a in act]
    A = [[f(H[LR._up(min(a, b), max(a, b))]) * D[i] * D[j] for j, b in enumerate(act)] for i, a in enumerate(act)]
    nA = max(sum(abs(v) for v in row) for row in A)
    worst = 0.0
    for kk, k in enumerate(act):
        y = [f(cov[a, k]) / (D[i] * D[kk]) for i, a in enumerate(act)]
        res = max(abs(sum((A[i][j] * y[j] for j in range(n)), mp.mpf(0)) - (1 if i == kk else 0)) for i in range(n))
        ratio = float(res / (n * SC.U * (nA * max(abs(v) for v in y) + 1)))
        assert ratio <= 3 * n + 4, (tag, "column", k, "backward error over n u (|A||y| + 1)", ratio, "c", 3 * n + 4)
        worst = max(worst, ratio)
    return worst


# ---- the reference system of an entry ----

def config(variant, lo_type=0, use_shift=True, mdc=False):
    o, c = synthetic.example_options(RC.KIND[variant])
    c.LO_type = lo_type
    c.use_shift = use_shift
    c.min_depth_constraint = mdc
    return o, c


def job_use_shift(variant, c):
    """make_lm_job(.., nonminimal = false): the calibrated optimizer takes the config's flag, the
    focal ones run with their default (on), scale only has constant offsets"""
    return bool(c.use_shift) if variant == 0 else variant != 3


def gated_lists(mask, c):
    """the block lists of an entry: the set bits of residuals' mask, less what the LO type drops"""
    e = np.zeros(0, np.int32)
    bits = [np.flatnonzero((mask >> t) & 1).astype(np.int32) for t in range(3)]
    return [e if c.LO_type == 1 else bits[0], e if c.LO_type == 1 else bits[1], e if c.LO_type == 2 else bits[2]]


def problem_params(variant, row17, norm_scale):
    """q, t, scale, o0, o1, f0, f1 of a model row (user units) as the engine forms them: the
    focals over the pair's normalisation scale, the engine's own division"""
    row17 = np.asarray(row17, np.float64)
    f0 = f1 = 1.0
    if variant in (1, 2):
        f0, f1 = float(row17[15] / np.float64(norm_scale)), float(row17[16] / np.float64(norm_scale))
    if variant == 1:
        f1 = f0
    return (SC.rot_to_quat(row17[:9]), row17[9:12].copy(), float(row17[12]), float(row17[13]), float(row17[14]), f0, f1)


def reference(variant, p, o, c, norm_scale, row17, mask, mode):
    """LR.system of the entry (model row17 on pair p under residuals' mask), with its active set"""
    g = geometry(variant)
    data = SC.engine_doubles(g, RC.pair_args(variant, p), o, norm_scale)
    lists = gated_lists(mask, c)
    r = LR.system(g, data, lists, problem_params(variant, row17, norm_scale), mode)
    r["col"] = LR.active_set(g, len(lists[0]), len(lists[1]), len(lists[2]), job_use_shift(variant, c))
    r["lists"] = lists
    return r


def entry(res, e):
    """entry e of an InformationResult as the dict SC.check_system reads"""
    return dict(cost=float(res.cost[e]), g=np.asarray(res.g[e]), H=np.asarray(res.H[e]), col=res.col[e].tolist())


def entry_bytes(res, e):
    return tuple(np.ascontiguousarray(a[e]).tobytes() for a in (res.H, res.g, res.cost, res.cov, res.col, res.pd,
                                                                res.status, res.rows, res.counts))


# ---- the cases ----

class Case:
    pass


def _cut(p, idx):
    q = dict(p)
    for key in ("x0", "x1", "depth0", "depth1", "inlier_mask"):
        q[key] = p[key][idx]
    return q


@functools.lru_cache(maxsize=None)
def small_case(variant):
    """Three pairs of at most 40 correspondences cut from SC.small's pair: inliers and a few
    outliers.  Models: the synthetic ground truth and a perturbation of it (0.3 degrees, 1 %)."""
    k = Case()
    k.variant = variant
    p = SC.small(geometry(variant)).p
    inl, outl = np.flatnonzero(p["inlier_mask"]), np.flatnonzero(~p["inlier_mask"])
    rng = np.random.default_rng(900 + variant)
    k.pairs = []
    for ni, no in ((36, 4), (20, 3), (10, 2)):
        idx = np.sort(np.r_[rng.choice(inl, ni, replace=False), rng.choice(outl, no, replace=False)])
        k.pairs.append(_cut(p, idx))
    k.models, k.ids, k.kinds = [], [], []
    for i, q in enumerate(k.pairs):
        for kind, m in (("truth", RC.make_model(variant, *RC.ground_truth(variant, q))),
                        ("perturbed", RC.start_model(variant, q, rng, rot_deg=0.3, rel=0.01))):
            k.models.append(m)
            k.ids.append(i)
            k.kinds.append(kind)
    k.rows17 = np.stack([W.model_row(variant, m) for m in k.models])
    k.ne = len(k.models)
    return k


@functools.lru_cache(maxsize=None)
def size_case(variant):
    """W.case's pairs (one of every size of W.SIZES, three models each) and one pair of BIG
    correspondences under its ground truth and a perturbation."""
    w = W.case(variant)
    k = Case()
    k.variant = variant
    big = synthetic.make_pair(90 + variant, n=BIG, outlier_ratio=0.05, K1=RC.K_TF1 if variant == 2 else None)
    k.pairs = list(w.pairs) + [big]
    k.sizes = list(W.SIZES) + [BIG]
    rng = np.random.default_rng(950 + variant)
    k.models = list(w.models) + [RC.make_model(variant, *RC.ground_truth(variant, big)),
                                 RC.start_model(variant, big, rng, rot_deg=0.3, rel=0.01)]
    k.ids = list(w.ids) + [len(w.pairs)] * 2
    k.kinds = list(w.kinds) + ["truth", "perturbed"]
    k.rows17 = np.stack([W.model_row(variant, m) for m in k.models])
    k.ne = len(k.models)
    k.mix = np.array([(1.0, 1.5, 0.75, 2.0, 1.25)[e % 5] for e in range(k.ne)])
    return k


def open_set(k, o, c):
    return madpose.PairSet(k.variant, k.pairs, o, c)


# ---- 7. device outputs (the child process) ----

def device_outputs(torch, ne, names, extra=0):
    """per name: (guarded buffer, start, bytes, the (ne + extra, ...) float64 view)"""
    out = {}
    for n in names:
        per = int(np.prod(SHAPES[n], dtype=np.int64))
        nbytes = 8 * per * (ne + extra)
        buf, start = W.guarded(torch, nbytes)
        view = buf[start:start + nbytes].view(torch.float64).view((ne + extra,) + SHAPES[n])
        out[n] = (buf, start, nbytes, view)
    return out


def same_as_host(k, ps, torch, names, want, factor=1.0, **kw):
    dev = device_outputs(torch, k.ne, names)
    torch.cuda.synchronize()
    got = ps.information(k.rows17, pair_ids=k.ids, factor=factor, covariance="cov" in names,
                         **{"out_" + n: dev[n][3] for n in names}, **kw)
    torch.cuda.synchronize()
    for n in OUTPUTS:
        if n in names:
            assert getattr(got, n) is dev[n][3]
            assert dev[n][3].cpu().numpy().tobytes() == getattr(want, n).tobytes(), n
            W.assert_guards(dev[n][0], dev[n][1], dev[n][2])
        else:
            assert getattr(got, n) is None, n
    for n in ("col", "pd", "status", "rows", "counts"):
        assert getattr(got, n).tobytes() == getattr(want, n).tobytes(), n


@check((0,), (1,), (2,), (3,))
def check_device_outputs_equal_host_outputs(variant):
    torch = W._torch()
    k = size_case(variant)
    with open_set(k, *config(variant)) as ps:
        want = ps.information(k.rows17, pair_ids=k.ids)
        assert np.any(want.pd == 1) and np.any(want.pd == -1)
        same_as_host(k, ps, torch, OUTPUTS, want)
        # any subset
        for names in (("H",), ("cov",), ("g", "cost"), ("H", "cov"), ("cost",)):
            same_as_host(k, ps, torch, names, want)
        # the per-entry mix of factors
        same_as_host(k, ps, torch, OUTPUTS, ps.information(k.rows17, pair_ids=k.ids, factor=k.mix), factor=k.mix)


@check()
def check_rows_of_other_entries_keep_a_sentinel():
    """tensors larger than the call: the rows past the call's entries are not written; and a call
    on a few entries writes rows 0 .. ne - 1 only"""
    torch = W._torch()
    k = size_case(0)
    with open_set(k, *config(0)) as ps:
        sel = [e for e in range(k.ne) if k.kinds[e] == "perturbed"][4:9]
        want = ps.information(k.rows17[sel], pair_ids=[k.ids[e] for e in sel])
        big = {n: torch.full((len(sel) + 3,) + SHAPES[n], -7.5, dtype=torch.float64, device="cuda") for n in OUTPUTS}
        torch.cuda.synchronize()
        ps.information(k.rows17[sel], pair_ids=[k.ids[e] for e in sel],
                       **{"out_" + n: big[n][:len(sel)] for n in OUTPUTS})
        torch.cuda.synchronize()
        for n in OUTPUTS:
            h = big[n].cpu().numpy()
            assert h[:len(sel)].tobytes() == getattr(want, n).tobytes(), n
            assert np.all(h[len(sel):] == -7.5), n


@check()
def check_outputs_last_written_on_another_stream():
    torch = W._torch()
    k = size_case(1)
    with open_set(k, *config(1)) as ps:
        want = ps.information(k.rows17, pair_ids=k.ids)
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            ballast = torch.zeros(1 << 24, dtype=torch.float64, device="cuda")
            for _ in range(4):
                ballast = ballast * 2.0 + ballast
            dev = device_outputs(torch, k.ne, OUTPUTS)
            for n in OUTPUTS:
                dev[n][0].add_(ballast[:1].sum().to(torch.uint8))  # (adds 0, behind the ballast)
            got = ps.information(k.rows17, pair_ids=k.ids, stream=side, **{"out_" + n: dev[n][3] for n in OUTPUTS})
        torch.cuda.synchronize()
        for n in OUTPUTS:
            assert dev[n][3].cpu().numpy().tobytes() == getattr(want, n).tobytes(), n
            W.assert_guards(dev[n][0], dev[n][1], dev[n][2])
        assert got.pd.tobytes() == want.pd.tobytes()


@check()
def check_the_sets_lists_are_unchanged():
    """refine after information returns what it returned before"""
    torch = W._torch()
    k = size_case(0)
    with open_set(k, *config(0)) as ps:
        starts = [k.models[e] for e in range(k.ne) if k.kinds[e] == "perturbed"]
        ids = [k.ids[e] for e in range(k.ne) if k.kinds[e] == "perturbed"]
        before = [RC.result_key(0, r) for r in ps.refine(starts, pair_ids=ids, rounds=2)]
        dev = device_outputs(torch, k.ne, OUTPUTS)
        ps.information(k.rows17, pair_ids=k.ids, **{"out_" + n: dev[n][3] for n in OUTPUTS})
        ps.information(k.rows17, pair_ids=k.ids)
        after = [RC.result_key(0, r) for r in ps.refine(starts, pair_ids=ids, rounds=2)]
        assert before == after


@check()
def check_mixed_kinds_and_overlapping_tensors_are_refused():
    torch = W._torch()
    k = small_case(0)
    with open_set(k, *config(0)) as ps:
        ne = k.ne
        H = torch.zeros((ne, 66), dtype=torch.float64, device="cuda")
        flat = torch.zeros(ne * (66 + 11), dtype=torch.float64, device="cuda")
        call = lambda **kw: ps.information(k.rows17, pair_ids=k.ids, **kw)
        for bad, word in ((dict(out_H=H, out_g=np.zeros((ne, 11))), "one kind"),
                          (dict(out_H=np.zeros((ne, 66)), out_cov=torch.zeros((ne, 11, 11), dtype=torch.float64,
                                                                             device="cuda")), "one kind"),
                          (dict(out_H=flat[:ne * 66].view(ne, 66), out_g=flat[ne * 66 - 11:ne * 66 - 11 + ne * 11]
                                .view(ne, 11)), "out_H and out_g overlap"),
                          (dict(out_H=H, out_cost=H.view(-1)[5:5 + ne]), "out_H and out_cost overlap"),
                          (dict(out_H=H[:, :11]), "out_H must have shape"),
                          (dict(out_g=torch.zeros((ne, 22), dtype=torch.float64, device="cuda")[:, ::2]),
                           "out_g must be C-c"),
                          (dict(out_cost=torch.zeros(ne, dtype=torch.float32, device="cuda")), "out_cost must be float64"),
                          (dict(out_H=np.zeros((ne, 66)), stream=0), "stream goes with device outputs")):
            try:
                call(**bad)
            except ValueError as e:
                assert word in str(e), (word, str(e))
            else:
                raise AssertionError(f"not refused: {word}")
        torch.cuda.synchronize()
        assert not H.any().item() and not flat.any().item()  # nothing was written
        # touching ranges are taken
        got = call(out_H=flat[:ne * 66].view(ne, 66), out_g=flat[ne * 66:].view(ne, 11))
        want = call()
        torch.cuda.synchronize()
        assert got.H.cpu().numpy().tobytes() == want.H.tobytes() and got.g.cpu().numpy().tobytes() == want.g.tobytes()


@check()
def check_runs_write_device_outputs_in_place():
    """device outputs cut into many runs: every run writes its entries' rows of the caller's arrays"""
    import os
    torch = W._torch()
    k = size_case(2)
    with open_set(k, *config(2)) as ps:
        want = ps.information(k.rows17, pair_ids=k.ids)
        os.environ["MADPOSE_INFORMATION_RUN_ROWS"] = "5000"
        os.environ["MADPOSE_INFORMATION_RUN_ENTRIES"] = "4"
        try:
            same_as_host(k, ps, torch, OUTPUTS, want)
            again = ps.information(k.rows17, pair_ids=k.ids)
        finally:
            del os.environ["MADPOSE_INFORMATION_RUN_ROWS"], os.environ["MADPOSE_INFORMATION_RUN_ENTRIES"]
        for e in range(k.ne):
            assert entry_bytes(again, e) == entry_bytes(want, e), e


def main(argv):
    import io
    import json
    import time
    import traceback
    from contextlib import redirect_stdout
    torch = W._torch()  # before the library is loaded: one HIP runtime in the process
    torch.cuda.init()
    out = {}
    for name in argv or list(CHECKS):
        fn, params = CHECKS[name]
        buf, t0 = io.StringIO(), time.perf_counter()
        try:
            with redirect_stdout(buf):
                fn(*params)
            out[name] = {"ok": True, "detail": buf.getvalue()}
        except Exception as e:
            out[name] = {"ok": False, "detail": buf.getvalue() + traceback.format_exc()[-6000:]}
            stop = not isinstance(e, (AssertionError, ValueError))
        else:
            stop = False
        out[name]["seconds"] = round(time.perf_counter() - t0, 3)
        print(name, "ok" if out[name]["ok"] else "FAILED", out[name]["seconds"], flush=True)
        if stop:  # (a device error: nothing more is started on the GPU after it)
            break
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
