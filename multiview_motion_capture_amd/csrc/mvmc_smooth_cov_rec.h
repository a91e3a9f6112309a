// The backward recursion of the smoothers' covariance (Takahashi's selected inverse over the block-banded factor that sm_sweep leaves
// in the workspace), shared by csrc/mvmc_smooth_cov.hip (finished tracklets: every row of the identity, outputs for every row) and
// csrc/mvmc_smooth_window_cov.hip (live sessions: the window's free rows, outputs for the emitted row alone).  Included inside the
// including file's anonymous namespace, after mvmc_smooth_row.h and mvmc_smooth_sweep.h.  The algorithm, the wave assignment and the
// LDS budget are described at the head of csrc/mvmc_smooth_cov.hip.
#pragma once

constexpr int SC_J = 18;                              // every skeleton joint
constexpr int SC_INFO = MVMC_SMOOTH_COV_INFO_DOUBLES;

struct ScRowLds {
    double Rl[18 * 9], Rg[18 * 9], pos[18 * 3], ax[18 * 9];   // as SmBlkLds
    double D[SC_J * 3 * SK];                                  // D_K (3 x 39) of the 18 joints
    int mq[MVMC_SMOOTH_MAX_VIEWS];
    int nv;
};

struct ScLds {
    SmSweepLds sw;
    double T[SK2];                                            // L_tt of the row (lower triangle, row-major 39 x 39)
    double L1[SK2], L2[SK2];                                  // L_{t+1,t}, L_{t+2,t} of the row, staged from the workspace
    ScRowLds row;
};

// One row on the calling wave: FK and D_K = d X_K / d x (3 x 39) of every joint K -- sm_row_block's construction (Euler axes in the
// global frame, cross(axis, X_K - X_a) for the strict ancestors a of K, the identity for the root translation) through T.anc[K] --
// and the number of (selected view, observed joint) pairs whose score is not zero.
__device__ __forceinline__ int sc_row_tables(const Ik1Tables& T, ScRowLds& L, const double* __restrict__ kps17, int C,
                                             const int32_t* __restrict__ members, const double* __restrict__ x) {
    const int lane = threadIdx.x & 63;
    if (lane == 0) {
        int n = 0;
        for (int c = 0; c < C; ++c) {
            const int m = members[c];
            if (m >= 0 && n < MVMC_SMOOTH_MAX_VIEWS) L.mq[n++] = m;
        }
        L.nv = n;
    }
    if (lane < 18) {
        euler_to_rot(x + 3 + 3 * lane, &L.Rl[9 * lane]);
        const double a0 = x[3 + 3 * lane], a1 = x[4 + 3 * lane];
        const double ca = cos(a0), sa = sin(a0), cb = cos(a1), sb = sin(a1);
        double* A = &L.ax[9 * lane];
        A[0] = 1.0; A[1] = 0.0; A[2] = 0.0;
        A[3] = 0.0; A[4] = ca; A[5] = sa;
        A[6] = sb; A[7] = -sa * cb; A[8] = ca * cb;
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
    MVMC_WAVE_SYNC();
    for (int i = lane; i < SC_J * SK; i += 64) {
        const int K = i / SK, col = i - K * SK;
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
        L.D[(K * 3) * SK + col] = d0;
        L.D[(K * 3 + 1) * SK + col] = d1;
        L.D[(K * 3 + 2) * SK + col] = d2;
    }
    // the residual pairs that count: lane (k, r) = observed joint k in the views r, r + 4, ... (sm_row_block's layout and score)
    const int nv = uni(L.nv);
    const int obs = kIkObs[lane & 15];
    int cnt = 0;
    for (int v = lane >> 4; v < nv; v += 4) {
        const double* kp = kps17 + (size_t)L.mq[v] * 51;
        double s;
        if (obs < 17) s = kp[obs * 3 + 2];
        else {
            s = kp[5 * 3 + 2] * kp[6 * 3 + 2];
            s *= kp[11 * 3 + 2] * kp[12 * 3 + 2];
        }
        cnt += s != 0.0;
    }
    return cnt;
}

// X <- sign X T^-1 on the calling wave (T lower triangular in LDS): a row per lane in registers, T read as an LDS broadcast
__device__ __forceinline__ void sc_right_solve(double* __restrict__ X, const double* __restrict__ Tl, double sign) {
    const int lane = threadIdx.x & 63;
    const int row = lane < SK ? lane : SK - 1;
    double v[SK];
#pragma unroll
    for (int c = 0; c < SK; ++c) v[c] = X[row * SK + c];
#pragma unroll
    for (int c = SK - 1; c >= 0; --c) {
        double s = v[c];
#pragma unroll
        for (int q = SK - 1; q > c; --q) s -= v[q] * Tl[q * SK + c];
        v[c] = s / Tl[c * SK + c];
    }
    if (lane < SK) {
#pragma unroll
        for (int c = 0; c < SK; ++c) X[lane * SK + c] = sign * v[c];
    }
}

// The recursion r = m - 1 .. r_stop over the factor of sm_sweep (every thread calls; the factor in wk is complete and read-only).  The
// m free rows: x + r 68 their parameters, bk + r SM_BLK their data blocks, wk + r SM_WORK their factor rows, members_of(r) their
// members (C).  only < 0: every row r visited writes jc + r 108 and pv + r 39; only >= 0: row ``only`` alone writes, at jc and pv.
// e_acc: this lane's share of sum_t tr(Sigma_tt H_t) over the rows visited; n_acc: this lane's share of their residual pairs (wave 3).
template <class MembersOf>
__device__ __forceinline__ void sc_recursion(ScLds& S, const Ik1Tables& T, const double* __restrict__ x, const double* __restrict__ bk,
                                             const double* __restrict__ wk, int m, int r_stop, int only, const double* __restrict__ kps17,
                                             int C, MembersOf members_of, double* __restrict__ jc, double* __restrict__ pv, double& e_acc,
                                             int& n_acc) {
    SmSweepLds& L = S.sw;
    const int tid = threadIdx.x, wave = tid >> 6;
    // the six blocks of the sweep in rotating roles
    static_assert(offsetof(SmSweepLds, S) == 5 * SK2 * sizeof(double), "the sweep's six blocks are contiguous");
    double* const B0 = &L.B[0][0];
    int iS11 = 0, iS21 = 1, iS22 = 2, iX1 = 3, iX2 = 4, iM = 5;
    for (int r = m - 1; r >= r_stop; --r) {
        const double* wt = wk + (size_t)r * SM_WORK;
        const double *L1 = S.L1, *L2 = S.L2;
        const bool h1 = r + 1 < m, h2 = r + 2 < m;
        const int o = only < 0 ? r : (r == only ? 0 : -1);   // where the row's outputs go, -1: nowhere
        double *S11 = B0 + iS11 * SK2, *S21 = B0 + iS21 * SK2, *S22 = B0 + iS22 * SK2, *X1 = B0 + iX1 * SK2, *X2 = B0 + iX2 * SK2,
               *M = B0 + iM * SK2;
        // phase A: the row's factor blocks into LDS; G1 = S11 L1 + S21^T L2 and G2 = S21 L1 + S22 L2, one output per lane and pass
        for (int i = tid; i < SK2; i += SM_THREADS) {
            const int rr = i / SK, cc = i - rr * SK;
            S.T[i] = cc <= rr ? wt[sm_lo(rr, cc)] : 0.0;
            if (h1) S.L1[i] = wt[W_L1 + i];
            if (h2) S.L2[i] = wt[W_L2 + i];
        }
        __syncthreads();
        if (h1)
            for (int i = tid; i < SK2; i += SM_THREADS) {
                const int rr = i / SK, cc = i - rr * SK;
                double g1 = 0.0, s1 = 0.0, g2 = 0.0, s2 = 0.0;   // four independent chains in one pass over q
                if (h2)
                    for (int q = 0; q < SK; ++q) {
                        const double l1 = L1[q * SK + cc], l2 = L2[q * SK + cc];
                        g1 += S11[rr * SK + q] * l1;
                        s1 += S21[q * SK + rr] * l2;
                        g2 += S21[rr * SK + q] * l1;
                        s2 += S22[rr * SK + q] * l2;
                    }
                else
                    for (int q = 0; q < SK; ++q) g1 += S11[rr * SK + q] * L1[q * SK + cc];
                X1[i] = g1 + s1;
                X2[i] = g2 + s2;
            }
        __syncthreads();
        // phase B: Sigma_{t+1,t} = -G1 T^-1 (wave 0), Sigma_{t+2,t} = -G2 T^-1 (wave 1), T^-1 = I T^-1 into the dead S22 (wave 2),
        // the row's FK, D_K and residual count (wave 3)
        if (wave == 0) {
            if (h1) sc_right_solve(X1, S.T, -1.0);
        } else if (wave == 1) {
            if (h2) sc_right_solve(X2, S.T, -1.0);
        } else if (wave == 2) {
            const int lane = tid & 63;
            if (lane < SK) {
#pragma unroll
                for (int c = 0; c < SK; ++c) S22[lane * SK + c] = c == lane ? 1.0 : 0.0;
            }
            MVMC_WAVE_SYNC();
            sc_right_solve(S22, S.T, 1.0);
        } else {
            n_acc += sc_row_tables(T, S.row, kps17, C, members_of(r), x + (size_t)r * 68);
        }
        __syncthreads();
        // phase C: M = T^-T - Sigma_{t+1,t}^T L1 - Sigma_{t+2,t}^T L2
        for (int i = tid; i < SK2; i += SM_THREADS) {
            const int rr = i / SK, cc = i - rr * SK;
            double s1 = 0.0, s2 = 0.0;
            if (h2)
                for (int q = 0; q < SK; ++q) {
                    s1 += X1[q * SK + rr] * L1[q * SK + cc];
                    s2 += X2[q * SK + rr] * L2[q * SK + cc];
                }
            else if (h1)
                for (int q = 0; q < SK; ++q) s1 += X1[q * SK + rr] * L1[q * SK + cc];
            M[i] = (S22[cc * SK + rr] - s1) - s2;
        }
        __syncthreads();
        // phase D: Sigma_tt = M T^-1 on wave 0, then made symmetric: the recursion carries the antisymmetric part of a rounding
        // error forward with a gain above one (1.85 per row measured in the restatement: 1e19 after 150 rows), the symmetric part
        // with a gain below one
        if (wave == 0) sc_right_solve(M, S.T, 1.0);
        __syncthreads();
        for (int i = tid; i < SK2; i += SM_THREADS) {
            const int rr = i / SK, cc = i - rr * SK;
            if (rr > cc) {
                const double a = 0.5 * (M[rr * SK + cc] + M[cc * SK + rr]);
                M[rr * SK + cc] = a;
                M[cc * SK + rr] = a;
            }
        }
        __syncthreads();
        // phase E: the row's outputs while Sigma_tt (in M) is in LDS.  U = D Sigma_tt (54 x 39) into the two dead blocks S21 (joints
        // 0..8) and S22 (joints 9..17); p_q; this lane's share of tr(Sigma_tt H_t)
        if (o >= 0) {
            for (int i = tid; i < SC_J * 3 * SK; i += SM_THREADS) {
                const int a = i / SK, q = i - a * SK;
                const double* Da = &S.row.D[a * SK];
                double u = 0.0;
                for (int p = 0; p < SK; ++p) u += Da[p] * M[p * SK + q];
                if (a < 27) S21[i] = u;
                else S22[i - 27 * SK] = u;
            }
            if (tid < SK) pv[(size_t)o * SK + tid] = M[tid * SK + tid];
        }
        {
            const double* H = bk + (size_t)r * SM_BLK;
            for (int i = tid; i < SK2; i += SM_THREADS) {
                const int rr = i / SK, cc = i - rr * SK;
                e_acc += M[i] * H[rr <= cc ? sm_up(rr, cc) : sm_up(cc, rr)];
            }
        }
        __syncthreads();
        if (o >= 0 && tid < SC_J * 6) {   // C_K = U_K D_K^T: the six values (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)
            const int K = tid / 6, e = tid - 6 * K;
            const int a = e < 3 ? 0 : e < 5 ? 1 : 2, b = e < 3 ? e : e < 5 ? e - 2 : 2;
            const double* U = K < 9 ? &S21[(K * 3 + a) * SK] : &S22[((K - 9) * 3 + a) * SK];
            const double* Db = &S.row.D[(K * 3 + b) * SK];
            double c = 0.0;
            for (int q = 0; q < SK; ++q) c += U[q] * Db[q];
            jc[(size_t)o * (SC_J * 6) + tid] = c;
        }
        __syncthreads();
        // the next row up: S11 <- Sigma_tt, S21 <- Sigma_{t+1,t}, S22 <- S11; the three others are free
        const int oS11 = iS11, oS21 = iS21, oS22 = iS22, oX2 = iX2;
        iS11 = iM; iS21 = iX1; iS22 = oS11; iX1 = oS21; iX2 = oS22; iM = oX2;
    }
}
