// The setup of one device LM problem (lm_refine's in host/lm.cpp): the first part of
// lm_problem.inc's body, a file of its own so that lm_system_kernel (the test hook of one
// evaluation and one step, lm_device.h) runs the same text.  In scope and results as
// lm_problem.inc describes; after it: NA, kPack, sh (x, best, col, has_lo, lo, cur,
// action: 0 = nothing to do, status[job] written), J, t0, behind a barrier.
    constexpr int NA = V == kCal ? kLF0 : (V == kSF ? kLF0 + 1 : kLNFull);
    constexpr int kPack = LmShared<NA>::kPack;
    __shared__ LmShared<NA> sh;
    const LmJob &J = jobs[blockIdx.x]; // (read in place: uniform, kept out of registers)
    const bool t0 = threadIdx.x == 0;
    // ---- setup (lm_refine in host/lm.cpp) ----
    if (t0) {
        const bool has_o0 = J.n0 > 0, has_s_o1 = J.n1 > 0;
        for (int k = 0; k < kLNFull; ++k) {
            sh.col[k] = -1;
            sh.has_lo[k] = 0;
            sh.lo[k] = 0.0;
        }
        for (int k = 0; k < 6; ++k) sh.col[k] = k;
        if (has_s_o1) {
            sh.col[kLS] = kLS;
            sh.has_lo[kLS] = 1;
            sh.lo[kLS] = 1e-2;
        }
        if (has_o0 && J.use_shift) sh.col[kLO0] = kLO0;
        if (has_s_o1 && J.use_shift) sh.col[kLO1] = kLO1;
        if (J.min_depth_constraint) {
            sh.has_lo[kLO0] = sh.has_lo[kLO1] = 1;
            sh.lo[kLO0] = -C.min_depth[0] + 1e-2;
            sh.lo[kLO1] = -C.min_depth[1] + 1e-2;
        }
        if (V == kSF) sh.col[kLF0] = kLF0;
        if (V == kTF) {
            sh.col[kLF0] = kLF0;
            sh.col[kLF1] = kLF1;
            sh.has_lo[kLF0] = sh.has_lo[kLF1] = 1;
            sh.lo[kLF0] = sh.lo[kLF1] = 1e-6;
        }
        LmParams &x = sh.x;
        lm_rot_to_quat(J.m.R, x.q);
        lm_quat_to_rot(x.q, x.R);
        for (int k = 0; k < 3; ++k) x.t[k] = J.m.t[k];
        x.s = J.m.scale;
        x.o0 = J.m.offset0;
        x.o1 = J.m.offset1;
        x.f0 = J.m.focal0;
        x.f1 = J.m.focal1;
        sh.best = x;
        sh.cur = 0;
        sh.action = 1;
        if (J.n0 + J.n1 + J.n2 == 0) sh.action = 0;
        // constant bounded blocks must start feasible (Ceres Program::IsFeasible)
        if (!J.use_shift && J.min_depth_constraint) {
            if (has_o0 && x.o0 < sh.lo[kLO0]) sh.action = 0;
            if (has_s_o1 && x.o1 < sh.lo[kLO1]) sh.action = 0;
        }
        if (J.n0 + J.n1 + J.n2 == 0)
            status[blockIdx.x] = 0;
        else
            status[blockIdx.x] = sh.action ? 1 : 2;
    }
    __syncthreads();
