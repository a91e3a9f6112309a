// The row block of the trajectory smoothers (csrc/mvmc_smooth.hip: finished tracklets; csrc/mvmc_smooth_window.hip: live sessions):
// FK, the stage-1 residual and its analytic Jacobian of ONE row on ONE wave, and the prior's coefficients.  Included inside the
// including file's anonymous namespace, after mvmc_common.h, mvmc_track.hip and mvmc_ik1.hip (MVMC_DEVICE_ONLY).
#pragma once
constexpr int SK = MVMC_SMOOTH_K;                 // 39 stage-1 parameters (Ik1Tables::act[0])
constexpr int SK2 = SK * SK;
constexpr int SKH = SK * (SK + 1) / 2;            // packed triangle
constexpr int SM_BLK = MVMC_SMOOTH_BLOCK_DOUBLES;  // per frame: J^T J upper (SKH), J^T r (SK), E
constexpr int SM_WORK = MVMC_SMOOTH_WORK_DOUBLES;  // per frame: L_tt lower (SKH), L_{t+1,t}, L_{t+2,t} (SK2 each), y / d, g, diag A (SK each)
constexpr int W_L1 = SKH, W_L2 = SKH + SK2, W_Y = SKH + 2 * SK2, W_G = W_Y + SK, W_D = W_G + SK;
static_assert(W_D + SK <= SM_WORK, "smoothing workspace layout");
static_assert(SKH + SK + 1 <= SM_BLK, "smoothing block layout");

// upper-triangle index (s <= t) of the packed J^T J, and the packed lower triangle (r >= c) of the factor
__device__ __forceinline__ int sm_up(int s, int t) { return s * SK - s * (s - 1) / 2 + (t - s); }
__device__ __forceinline__ int sm_lo(int r, int c) { return r * (r + 1) / 2 + c; }

// ---- blocks ----
struct SmBlkLds {
    double Rl[18 * 9], Rg[18 * 9], pos[18 * 3], ax[18 * 9];   // local and global rotations, joints, rotation axes (global frame)
    double W[NOBS * 6], t[NOBS * 3];
    double D[NOBS * 3 * SK], WD[NOBS * 3 * SK];
    int mq[MVMC_SMOOTH_MAX_VIEWS], mc[MVMC_SMOOTH_MAX_VIEWS];
    int nv;
};

// FK of one row on the calling wave: x the row's 68 parameters -> L.Rl, L.Rg (local and global rotations) and L.pos (joints); AXES: L.ax
// too, the Euler axes of every joint in the global frame.  L.pos is complete on return; L.ax needs one MVMC_WAVE_SYNC more.  Tab: the
// tables' type -- Ik1Tables, or any struct with its parents, side_map and dirs (a copy of them in LDS).
template <bool AXES, class Lds, class Tab>
__device__ __forceinline__ void sm_row_fk(const Tab& T, Lds& L, const double* __restrict__ x) {
    const int lane = threadIdx.x & 63;
    if (lane < 18) {
        euler_to_rot(x + 3 + 3 * lane, &L.Rl[9 * lane]);
        if constexpr (AXES) {   // the Euler axes in the parent's frame (oracle/trf_np.py: ik_jacobian): x, Rx y, Rx Ry z
            const double a0 = x[3 + 3 * lane], a1 = x[4 + 3 * lane];
            const double ca = cos(a0), sa = sin(a0), cb = cos(a1), sb = sin(a1);
            double* A = &L.ax[9 * lane];
            A[0] = 1.0; A[1] = 0.0; A[2] = 0.0;
            A[3] = 0.0; A[4] = ca; A[5] = sa;
            A[6] = sb; A[7] = -sa * cb; A[8] = ca * cb;
        }
    }
    if (lane < 3) L.pos[lane] = x[lane];
    MVMC_WAVE_SYNC();
    if (lane < 9) L.Rg[lane] = L.Rl[lane];
    MVMC_WAVE_SYNC();
    for (int j = 1; j < 18; ++j) {
        const int p = T.parents[j];
        const double* Gp = &L.Rg[9 * p];
        if (lane < 9) {
            const int r = lane / 3, c = lane - 3 * r;
            const double* Rj = &L.Rl[9 * j];
            L.Rg[9 * j + lane] = Gp[3 * r] * Rj[c] + Gp[3 * r + 1] * Rj[3 + c] + Gp[3 * r + 2] * Rj[6 + c];
        } else if (lane < 12) {
            const int e = lane - 9;
            const double len = x[57 + T.side_map[j]];
            const double o0 = T.dirs[3 * j] * len, o1 = T.dirs[3 * j + 1] * len, o2 = T.dirs[3 * j + 2] * len;
            L.pos[3 * j + e] = Gp[3 * e] * o0 + Gp[3 * e + 1] * o1 + Gp[3 * e + 2] * o2 + L.pos[3 * p + e];
        }
        MVMC_WAVE_SYNC();
    }
    if constexpr (AXES) {
        double axl[9];
        if (lane < 18) {
#pragma unroll
            for (int e = 0; e < 9; ++e) axl[e] = L.ax[9 * lane + e];
        }
        MVMC_WAVE_SYNC();
        if (lane < 18) {   // axes into the global frame: R_parent a (the root's parent frame is the world)
            const int p = T.parents[lane];
            for (int c = 0; c < 3; ++c)
                for (int e = 0; e < 3; ++e)
                    L.ax[9 * lane + 3 * c + e] = p < 0 ? axl[3 * c + e]
                                                       : L.Rg[9 * p + 3 * e] * axl[3 * c] + L.Rg[9 * p + 3 * e + 1] * axl[3 * c + 1] +
                                                             L.Rg[9 * p + 3 * e + 2] * axl[3 * c + 2];
        }
    }
}

// One (view, observed joint) pair: kp the view's pose (17,3), P its camera (3,4), obs the joint's row of it (17: the mid spine of the
// shoulders and hips, its score their product), X the joint -> the observation (ob0, ob1), its score s, and the projection (u, vv)
// with its depth w
__device__ __forceinline__ void sm_pair(const double* __restrict__ kp, const double* __restrict__ P, int obs, double X0, double X1,
                                        double X2, double& ob0, double& ob1, double& s, double& w, double& u, double& vv) {
    if (obs < 17) { ob0 = kp[obs * 3]; ob1 = kp[obs * 3 + 1]; s = kp[obs * 3 + 2]; }
    else {
        const double sh0 = 0.5 * (kp[5 * 3] + kp[6 * 3]), hp0 = 0.5 * (kp[11 * 3] + kp[12 * 3]);
        const double sh1 = 0.5 * (kp[5 * 3 + 1] + kp[6 * 3 + 1]), hp1 = 0.5 * (kp[11 * 3 + 1] + kp[12 * 3 + 1]);
        ob0 = 0.5 * (sh0 + hp0); ob1 = 0.5 * (sh1 + hp1);
        s = kp[5 * 3 + 2] * kp[6 * 3 + 2];
        s *= kp[11 * 3 + 2] * kp[12 * 3 + 2];
    }
    const double h0 = P[0] * X0 + P[1] * X1 + P[2] * X2 + P[3];
    const double h1 = P[4] * X0 + P[5] * X1 + P[6] * X2 + P[7];
    const double h2 = P[8] * X0 + P[9] * X1 + P[10] * X2 + P[11];
    w = 1e-5 + h2;
    u = h0 / w;
    vv = h1 / w;
}

// The robust loss on one (selected view, observed joint) pair (include/mvmc.h: MVMC_SMOOTH_LOSS_*; tests/smooth_robust_np.py): e2 the
// squared length of the PLAIN pixel residual, delta = loss_px -> rho and the weight w of the reweighted model.  Huber's e = 0 is inside.
template <int LOSS>
__device__ __forceinline__ void sm_rho_w(double e2, double delta, double& rho, double& w) {
    if constexpr (LOSS == MVMC_SMOOTH_LOSS_HUBER) {
        const double e = sqrt(e2);
        if (e <= delta) { rho = 0.5 * e2; w = 1.0; }
        else { rho = delta * (e - 0.5 * delta); w = delta / e; }
    } else if constexpr (LOSS == MVMC_SMOOTH_LOSS_CAUCHY) {
        const double q = e2 / (delta * delta);
        rho = 0.5 * delta * delta * log1p(q);
        w = 1.0 / (1.0 + q);
    } else {
        rho = 0.5 * e2; w = 1.0;
    }
}

// One row on the calling wave: members (C) pose indices or -1, Prig the row's rig (C,3,4), x the row's 68 parameters -> out (SM_BLK).
// LOSS = MVMC_SMOOTH_LOSS_NONE is the arithmetic without a loss, operation for operation (loss_px is not read).  With a loss the pair's
// rho and w are taken in registers inside the view loop: W_k and t_k carry w s^2, E = sum s^2 rho; the score stays outside the loss, and
// a pair whose score is 0 contributes nothing whatever its residual.  The reductions and the LDS are the same for every LOSS.
// CONTACT (default false: none of the three last arguments is read, the code is the one without the parameter): the foot-contact term
// of the row, 1/2 wc |X_K - a|^2 for foot f = 0 (K = MVMC_SMOOTH_FOOT_L), 1 (MVMC_SMOOTH_FOOT_R) when cmask[f] != 0, a = anchors + 3 f
// (include/mvmc.h: mvmc_smooth_blocks_contact).  It is quadratic in X_K, so it joins the observed joint's own W_k (+ wc I), t_k
// (+ wc (X_K - a)) after the views' reduction, in the lane that owns them, and E (left, then right); it stays outside the loss.  A
// row whose mask is (0, 0) runs the code without the term, operation for operation; a row with a mask and no view runs the whole row
// with an empty view loop instead of the no-data return.
// FLOOR (default false: nrm and wf are not read, the code is the one without the parameter; needs CONTACT): the term is anisotropic
// about the unit floor normal nrm (3) of the row's sequence (include/mvmc.h: mvmc_smooth_blocks_floor): with c = X_K - a,
// W_k += wc I + (wf - wc) n n^T, t_k += wc c + (wf - wc)(n . c) n, E += 1/2 wc |c|^2 + 1/2 (wf - wc)(n . c)^2 -- the CONTACT term
// first, operation for operation, then the rank-one part in the same lane; no LDS and no barrier more.  A NaN normal: CONTACT's row.
template <int LOSS, bool CONTACT = false, bool FLOOR = false>
__device__ __forceinline__ void sm_row_block(const Ik1Tables& T, SmBlkLds& L, const double* __restrict__ kps17,
                                             const double* __restrict__ Prig, int C, int Pmax, const int32_t* __restrict__ members,
                                             const double* __restrict__ x, double* __restrict__ out, double loss_px,
                                             const int32_t* __restrict__ cmask = nullptr, const double* __restrict__ anchors = nullptr,
                                             double wc = 0.0, const double* __restrict__ nrm = nullptr, double wf = 0.0) {
    static_assert(CONTACT || !FLOOR, "the floor is a form of the contact term");
    const int lane = threadIdx.x & 63;
    bool on[2] = {false, false};
    if constexpr (CONTACT) { on[0] = uni((int)cmask[0]) != 0; on[1] = uni((int)cmask[1]) != 0; }
    bool fl = false;
    double n0 = 0.0, n1 = 0.0, n2 = 0.0;
    if constexpr (FLOOR) {
        n0 = uni(nrm[0]); n1 = uni(nrm[1]); n2 = uni(nrm[2]);
        fl = n0 == n0 && n1 == n1 && n2 == n2;
    }
    if (lane == 0) {
        int n = 0;
        for (int c = 0; c < C; ++c) {
            const int m = members[c];
            if (m >= 0 && n < MVMC_SMOOTH_MAX_VIEWS) { L.mq[n] = m; L.mc[n] = (m / Pmax) % C; ++n; }
        }
        L.nv = n;
    }
    MVMC_WAVE_SYNC();
    const int nv = uni(L.nv);
    if (nv == 0 && !(on[0] || on[1])) {   // no data: the prior alone places the frame
        for (int i = lane; i < SM_BLK; i += 64) out[i] = 0.0;
        return;
    }
    sm_row_fk<true>(T, L, x);
    // residual and the per-joint blocks: lane (k, r) = observed joint k in the views r, r + 4, ... (as ik1_eval)
    const int k = lane & 15, r = lane >> 4;
    const double X0 = L.pos[3 * kIkSkel[k]], X1 = L.pos[3 * kIkSkel[k] + 1], X2 = L.pos[3 * kIkSkel[k] + 2];
    const int obs = kIkObs[k];
    double f2 = 0.0, o[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int v = r; v < nv; v += 4) {
        const double* kp = kps17 + (size_t)L.mq[v] * 51;
        const double* P = Prig + (size_t)L.mc[v] * 12;
        double ob0, ob1, s, w, u, vv;
        sm_pair(kp, P, obs, X0, X1, X2, ob0, ob1, s, w, u, vv);
        // the pair's terms: f2 += its cost, W_k += cw (du du^T + dv dv^T), t_k += ct (du gu + dv gv)
        double cw, ct, gu, gv;
        if constexpr (LOSS == MVMC_SMOOTH_LOSS_NONE) {
            const double fu = (u - ob0) * s, fv = (vv - ob1) * s;
            f2 += fu * fu + fv * fv;
            cw = s * s; ct = s; gu = fu; gv = fv;
        } else {
            const double ru = u - ob0, rv = vv - ob1;
            double rho, wl;
            sm_rho_w<LOSS>(ru * ru + rv * rv, loss_px, rho, wl);
            const bool live = s != 0.0;
            f2 += live ? s * s * rho : 0.0;
            cw = ct = live ? wl * (s * s) : 0.0; gu = ru; gv = rv;
        }
        double du[3], dv[3];
        for (int c = 0; c < 3; ++c) {
            du[c] = (P[c] - u * P[8 + c]) / w;
            dv[c] = (P[4 + c] - vv * P[8 + c]) / w;
        }
        o[0] += cw * (du[0] * du[0] + dv[0] * dv[0]);
        o[1] += cw * (du[0] * du[1] + dv[0] * dv[1]);
        o[2] += cw * (du[0] * du[2] + dv[0] * dv[2]);
        o[3] += cw * (du[1] * du[1] + dv[1] * dv[1]);
        o[4] += cw * (du[1] * du[2] + dv[1] * dv[2]);
        o[5] += cw * (du[2] * du[2] + dv[2] * dv[2]);
        o[6] += ct * (du[0] * gu + dv[0] * gv);
        o[7] += ct * (du[1] * gu + dv[1] * gv);
        o[8] += ct * (du[2] * gu + dv[2] * gv);
    }
    double E = LOSS == MVMC_SMOOTH_LOSS_NONE ? 0.5 * wave_sum(f2) : wave_sum(f2);   // 1/2 sum (s e)^2, or sum s^2 rho
#pragma unroll
    for (int e = 0; e < 9; ++e) {
        o[e] += xor_lane<16>(o[e]);
        o[e] += xor_lane<32>(o[e]);
    }
    if constexpr (CONTACT) {
        for (int f = 0; f < 2; ++f) {   // left, then right
            if (!on[f]) continue;
            const int K = f == 0 ? MVMC_SMOOTH_FOOT_L : MVMC_SMOOTH_FOOT_R;
            const double* a = anchors + 3 * f;
            const double c0 = L.pos[3 * K] - a[0], c1 = L.pos[3 * K + 1] - a[1], c2 = L.pos[3 * K + 2] - a[2];
            E += 0.5 * wc * (c0 * c0 + c1 * c1 + c2 * c2);   // (every lane: E stays wave-uniform)
            if (lane < NOBS && kIkSkel[lane] == K) {         // the lane of the ankle's observed-joint slot
                o[0] += wc; o[3] += wc; o[5] += wc;
                o[6] += wc * c0; o[7] += wc * c1; o[8] += wc * c2;
            }
            if constexpr (FLOOR) {
                if (fl) {   // the rank-one part along the normal
                    const double dw = wf - wc, nc = n0 * c0 + n1 * c1 + n2 * c2;
                    E += 0.5 * dw * (nc * nc);
                    if (lane < NOBS && kIkSkel[lane] == K) {
                        o[0] += dw * (n0 * n0); o[1] += dw * (n0 * n1); o[2] += dw * (n0 * n2);
                        o[3] += dw * (n1 * n1); o[4] += dw * (n1 * n2); o[5] += dw * (n2 * n2);
                        o[6] += dw * nc * n0; o[7] += dw * nc * n1; o[8] += dw * nc * n2;
                    }
                }
            }
        }
    }
    if (lane < NOBS) {
#pragma unroll
        for (int e = 0; e < 6; ++e) L.W[lane * 6 + e] = o[e];
#pragma unroll
        for (int e = 0; e < 3; ++e) L.t[lane * 3 + e] = o[6 + e];
    }
    MVMC_WAVE_SYNC();
    // D_k (3 x 39) = d X_k / d x: translation, then per active Euler column cross(axis, X_k - X_a) when joint a is a strict ancestor
    for (int i = lane; i < NOBS * SK; i += 64) {
        const int kk = i / SK, col = i - kk * SK, K = kIkSkel[kk];
        double d0 = 0.0, d1 = 0.0, d2 = 0.0;
        const int act = T.act[0][col];
        if (act < 3) { d0 = act == 0; d1 = act == 1; d2 = act == 2; }
        else {
            const int a = (act - 3) / 3, c = (act - 3) - 3 * ((act - 3) / 3);
            if ((T.anc[K] >> a) & 1) {
                const double* A = &L.ax[9 * a + 3 * c];
                const double l0 = L.pos[3 * K] - L.pos[3 * a], l1 = L.pos[3 * K + 1] - L.pos[3 * a + 1], l2 = L.pos[3 * K + 2] - L.pos[3 * a + 2];
                d0 = A[1] * l2 - A[2] * l1;
                d1 = A[2] * l0 - A[0] * l2;
                d2 = A[0] * l1 - A[1] * l0;
            }
        }
        L.D[(kk * 3) * SK + col] = d0;
        L.D[(kk * 3 + 1) * SK + col] = d1;
        L.D[(kk * 3 + 2) * SK + col] = d2;
    }
    MVMC_WAVE_SYNC();
    for (int i = lane; i < NOBS * SK; i += 64) {
        const int kk = i / SK, col = i - kk * SK;
        const double* Wk = &L.W[kk * 6];
        const double a0 = L.D[(kk * 3) * SK + col], a1 = L.D[(kk * 3 + 1) * SK + col], a2 = L.D[(kk * 3 + 2) * SK + col];
        L.WD[(kk * 3) * SK + col] = Wk[0] * a0 + Wk[1] * a1 + Wk[2] * a2;
        L.WD[(kk * 3 + 1) * SK + col] = Wk[1] * a0 + Wk[3] * a1 + Wk[4] * a2;
        L.WD[(kk * 3 + 2) * SK + col] = Wk[2] * a0 + Wk[4] * a1 + Wk[5] * a2;
    }
    MVMC_WAVE_SYNC();
    for (int i = lane; i < SKH; i += 64) {
        int s = 0, rem = i;
        while (rem >= SK - s) { rem -= SK - s; ++s; }
        const int t = s + rem;
        double h = 0.0;
        for (int q = 0; q < NOBS * 3; ++q) h += L.D[q * SK + s] * L.WD[q * SK + t];
        out[i] = h;
    }
    if (lane < SK) {
        double g = 0.0;
        for (int q = 0; q < NOBS * 3; ++q) g += L.D[q * SK + lane] * L.t[q];
        out[SKH + lane] = g;
    }
    if (lane == 0) {
        out[SKH + SK] = E;
        for (int i = SKH + SK + 1; i < SM_BLK; ++i) out[i] = 0.0;
    }
}

// prior Hessian coefficient between local frames i and j of n (|i - j| <= 2): velocity (Dv^T Dv) and acceleration (Da^T Da) terms
__device__ __forceinline__ double sm_cv(int i, int j, int n) {
    const int hi = i > j ? i : j, lo = i < j ? i : j;
    double s = 0.0;
    for (int k = hi < 1 ? 1 : hi; k <= lo + 1 && k < n; ++k) {   // term k: x_k - x_{k-1}
        const double a = (i == k) ? 1.0 : -1.0, b = (j == k) ? 1.0 : -1.0;
        s += a * b;
    }
    return s;
}
__device__ __forceinline__ double sm_ca(int i, int j, int n) {
    const int hi = i > j ? i : j, lo = i < j ? i : j;
    double s = 0.0;
    for (int c = hi - 1 < 1 ? 1 : hi - 1; c <= lo + 1 && c + 1 < n; ++c) {   // term c: x_{c+1} - 2 x_c + x_{c-1}
        const double a = (i == c) ? -2.0 : 1.0, b = (j == c) ? -2.0 : 1.0;
        s += a * b;
    }
    return s;
}

// the prior's gradient at local frame i, parameter q (column cx of x): Dv^T Dv x and Da^T Da x through the differences
__device__ __forceinline__ double sm_prior_grad(const double* __restrict__ x, int i, int n, int cx, double wv, double wa) {
    double gv = 0.0, ga = 0.0;
    if (i >= 1) gv += x[(size_t)i * 68 + cx] - x[(size_t)(i - 1) * 68 + cx];
    if (i + 1 < n) gv -= x[(size_t)(i + 1) * 68 + cx] - x[(size_t)i * 68 + cx];
    for (int c = i - 1; c <= i + 1; ++c) {
        if (c < 1 || c + 1 >= n) continue;
        const double acc = (x[(size_t)(c + 1) * 68 + cx] - 2.0 * x[(size_t)c * 68 + cx]) + x[(size_t)(c - 1) * 68 + cx];
        ga += (c == i ? -2.0 : 1.0) * acc;
    }
    return wv * gv + wa * ga;
}

// the (loss, loss_px) pair of the *_robust entries: a loss of the three, and with one a loss_px that is a finite number > 0
inline bool sm_loss_ok(int loss, double loss_px) {
    if (loss < MVMC_SMOOTH_LOSS_NONE || loss > MVMC_SMOOTH_LOSS_CAUCHY) return false;
    return loss == MVMC_SMOOTH_LOSS_NONE || (loss_px > 0.0 && loss_px <= 1.7976931348623157e308);   // (NaN fails both)
}

inline bool sm_tables(const mvmcSkeleton* skel_host, Ik1Tables* T) {
    SkelDev sk;
    if (!skel_to_dev(skel_host, &sk) || sk.n_side != MVMC_N_SIDE) return false;
    ik1_build_tables_host(*T, sk);
    return T->na[0] == SK;
}
