// The body of the device LM's kernels (lm_device.h), one least-squares problem by the
// calling workgroup; included as text in lm_batch_kernel and lm_pairs_kernel, so that
// lm_batch_kernel compiles token for token as it did with this body written in it: its
// results are pinned to the bit (tests/test_lm_device_gpu.py), and a wrapping function,
// force-inlined or not, changed them (the optimiser sees the function before the kernel).
// In scope: V; const PairData &D, const PairConst &C (the pair); const LmJob *jobs; const
// int *idx (the pair's block lists); Model *out; int *status.  Job blockIdx.x of the
// launch: out[job] = the refined model, status[job] = 1 (refined), 0 (no residuals:
// unchanged), 2 (a constant bounded block starts infeasible: unchanged).
#include "lm_setup.inc"
    if (sh.action == 0) {
        if (t0) out[blockIdx.x] = J.m;
        return;
    }
    bool act[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) act[a] = sh.col[a] >= 0;
    lm_evaluate<V, NA>(D, C, J, idx, sh.x, sh, sh.red[0]);
    // ---- trust-region loop (lane 0 decides, every lane evaluates) ----
    double radius = 1e4, decrease = 2.0;
    const int max_nonmono = J.nonmonotonic ? 5 : 0;
    double ref_cost = 0, min_cost = 0, cand_ref = 0, acc_ref = 0.0, acc_cand = 0.0;
    int n_nonmono = 0, iter = 0;
    if (t0) {
        ref_cost = min_cost = cand_ref = sh.red[0][kPack + NA];
        sh.action = (lm_gmax<NA>(sh.red[0], act) <= J.gtol) ? 0 : 2;
    }
    __syncthreads();
    while (sh.action != 0) {
        if (t0) {
            // propose a step from x (repeated while the damped system is not positive definite)
            const double *R = sh.red[sh.cur];
            int prop = 0;
            while (iter < J.max_iter) {
                ++iter;
                double d[NA];
                if (!lm_step<NA>(R, act, radius, d)) {
                    radius /= decrease;
                    decrease *= 2.0;
                    if (radius < 1e-32) break;
                    continue;
                }
#pragma unroll
                for (int a = 0; a < NA; ++a) sh.d[a] = d[a];
                // candidate = Plus(x, d), projected onto the bounds
                const LmParams &x = sh.x;
                LmParams c = x;
                {
                    const double nd = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
                    if (nd > 0) {
                        const double sn = sin(nd) / nd;
                        const double qd[4] = {cos(nd), sn * d[0], sn * d[1], sn * d[2]};
                        const double *q = x.q;
                        c.q[0] = qd[0] * q[0] - qd[1] * q[1] - qd[2] * q[2] - qd[3] * q[3];
                        c.q[1] = qd[0] * q[1] + qd[1] * q[0] + qd[2] * q[3] - qd[3] * q[2];
                        c.q[2] = qd[0] * q[2] - qd[1] * q[3] + qd[2] * q[0] + qd[3] * q[1];
                        c.q[3] = qd[0] * q[3] + qd[1] * q[2] - qd[2] * q[1] + qd[3] * q[0];
                    }
#pragma unroll
                    for (int k = 0; k < 3; ++k) c.t[k] = x.t[k] + d[3 + k];
                    auto upd = [&](int slot, double v, double dv) {
                        if (sh.col[slot] < 0) return v;
                        v += dv;
                        return (sh.has_lo[slot] && v < sh.lo[slot]) ? sh.lo[slot] : v;
                    };
                    c.s = upd(kLS, c.s, d[kLS]);
                    c.o0 = upd(kLO0, c.o0, d[kLO0]);
                    c.o1 = upd(kLO1, c.o1, d[kLO1]);
                    if (NA > kLF0) c.f0 = upd(kLF0, c.f0, d[NA > kLF0 ? kLF0 : 0]);
                    if (NA > kLF1) c.f1 = upd(kLF1, c.f1, d[NA > kLF1 ? kLF1 : 0]);
                    lm_quat_to_rot(c.q, c.R);
                }
                double step2 = 0;
                {
                    const double dd[12] = {c.q[0] - x.q[0], c.q[1] - x.q[1], c.q[2] - x.q[2], c.q[3] - x.q[3],
                                           c.t[0] - x.t[0], c.t[1] - x.t[1], c.t[2] - x.t[2], c.s - x.s,
                                           c.o0 - x.o0,     c.o1 - x.o1,     c.f0 - x.f0,     c.f1 - x.f1};
#pragma unroll
                    for (int k = 0; k < 12; ++k) step2 += dd[k] * dd[k];
                }
                if (sqrt(step2) <= J.ptol * (sqrt(lm_amb_norm2(x)) + J.ptol)) break; // parameter tolerance
                sh.c = c;
                prop = 1;
                break;
            }
            sh.prop = prop;
        }
        __syncthreads();
        if (sh.prop == 0) break;
        lm_evaluate<V, NA>(D, C, J, idx, sh.c, sh, sh.red[sh.cur ^ 1]);
        if (t0) {
            const double *R = sh.red[sh.cur], *Rc = sh.red[sh.cur ^ 1];
            const double cost = R[kPack + NA], cand_cost = Rc[kPack + NA];
            sh.action = 2;
            if (fabs(cost - cand_cost) <= J.ftol * cost) {
                sh.action = 0; // function tolerance
            } else {
                double d[NA];
#pragma unroll
                for (int a = 0; a < NA; ++a) d[a] = sh.d[a];
                double gd = 0, jd2 = 0;
#pragma unroll
                for (int a = 0; a < NA; ++a) {
                    gd += (act[a] ? R[kPack + a] : 0.0) * d[a];
#pragma unroll
                    for (int b2 = 0; b2 < NA; ++b2) {
                        const double h = (act[a] && act[b2]) ? R[a <= b2 ? lm_up(a, b2, NA) : lm_up(b2, a, NA)] : 0.0;
                        jd2 += d[a] * h * d[b2];
                    }
                }
                const double mcc = -(gd + 0.5 * jd2);
                const double rho = (mcc > 0 && isfinite(cand_cost))
                                       ? fmax((cost - cand_cost) / mcc, (ref_cost - cand_cost) / (acc_ref + mcc))
                                       : -1.0;
                if (rho > 1e-3) {
                    sh.x = sh.c;
                    sh.cur ^= 1;
                    // Ceres TrustRegionStepEvaluator::StepAccepted
                    acc_cand += mcc;
                    acc_ref += mcc;
                    if (cand_cost < min_cost) {
                        min_cost = cand_cost;
                        n_nonmono = 0;
                        cand_ref = cand_cost;
                        acc_cand = 0.0;
                        sh.best = sh.x;
                    } else {
                        ++n_nonmono;
                        if (cand_cost > cand_ref) {
                            cand_ref = cand_cost;
                            acc_cand = 0.0;
                        }
                    }
                    if (n_nonmono == max_nonmono) {
                        ref_cost = cand_ref;
                        acc_ref = acc_cand;
                    }
                    radius = fmin(1e16, radius / fmax(1.0 / 3.0, 1.0 - pow(2.0 * rho - 1.0, 3.0)));
                    decrease = 2.0;
                    if (lm_gmax<NA>(Rc, act) <= J.gtol) sh.action = 0;
                } else {
                    radius /= decrease;
                    decrease *= 2.0;
                    if (radius < 1e-32) sh.action = 0;
                }
            }
            if (iter >= J.max_iter) sh.action = 0;
        }
        __syncthreads();
    }
    if (t0) {
        Model m = J.m;
        const LmParams &b = sh.best;
        lm_quat_to_rot(b.q, m.R);
        for (int k = 0; k < 3; ++k) m.t[k] = b.t[k];
        m.scale = b.s;
        m.offset0 = b.o0;
        m.offset1 = b.o1;
        m.focal0 = b.f0;
        m.focal1 = (V == kSF) ? b.f0 : b.f1;
        out[blockIdx.x] = m;
    }
