// The block-banded Levenberg-Marquardt sweep of the trajectory smoothers (csrc/mvmc_smooth.hip: finished tracklets, all the rows of an
// identity free; csrc/mvmc_smooth_window.hip: live sessions, the last m rows free after h frozen rows of history): one 256-lane
// workgroup solves (A + mu diag A) d = -g, A = the rows' data blocks + the exact prior Hessian, 39 x 39 blocks with two sub-diagonals
// (each prior block diagonal).  Included inside the including file's anonymous namespace, after mvmc_smooth_row.h.
//   forward  per free row: S = A_tt + mu diag(A_tt) - P1 P1^T - P2 P2^T, b = -g_t - P1 y1 - P2 y2, N1 = A_{t+1,t} - Q P1^T,
//            N2 = A_{t+2,t} on all four waves; the Cholesky of S on wave 0 with lane = row, the row in registers and every column
//            broadcast through v_readlane (no LDS round trip, no barrier per column), the forward substitution of b in the same
//            registers; N1 <- N1 L^-T on wave 0 and N2 <- N2 L^-T on wave 1 (a row per lane in registers, L_tt read as an LDS
//            broadcast) while waves 2 and 3 write L_tt out; the five 39 x 39 LDS blocks and the three y vectors rotate by index, nothing
//            is copied.  The frozen history enters through the gradient's stencils and the prior's interior coefficients only.
//   back     L^T d = y on wave 0 without a barrier: lane = column of L_tt in registers, d broadcast through v_readlane.
//   sums     the predicted reduction (-d.g + mu d^T diag(A) d) / 2 and |d|_inf.
// Every sum runs in a fixed order inside the workgroup's own lanes.
#pragma once
constexpr int SM_THREADS = 256;

struct SmSweepLds {
    double B[5][SK2];         // L(t,t-1), L(t,t-2), L(t+1,t-1), L(t+1,t), L(t+2,t) in rotating roles
    double S[SK2];            // the diagonal block being factored (lower triangle), then L_tt
    double y[3][SK];          // y_{t-1}, y_{t-2}, b in rotating roles
    double wv[SK], wa[SK];
    double red[SM_THREADS], red2[SM_THREADS], red3[SM_THREADS];
    int colx[SK];             // column of x (0..67) of each stage-1 parameter
    int fail;
};

struct SmStep {
    double pred, dmax;        // predicted reduction of E, |d|_inf
    int fail;                 // a pivot of the Cholesky was not positive and finite
};

__device__ __forceinline__ double rl64(double v, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}

// fixed-order sum over the workgroup (every thread calls)
__device__ double sm_wg_sum(double* red, double s) {
    const int tid = threadIdx.x;
    red[tid] = s;
    __syncthreads();
    for (int w = SM_THREADS / 2; w >= 1; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// colx and the prior's weights per stage-1 parameter (every thread calls)
__device__ __forceinline__ void sm_sweep_tables(SmSweepLds& L, const Ik1Tables& T, double root_vel, double root_acc, double ang_vel,
                                                double ang_acc) {
    const int tid = threadIdx.x;
    if (tid < SK) {
        const int a = T.act[0][tid];
        L.colx[tid] = a;
        L.wv[tid] = a < 3 ? root_vel : ang_vel;
        L.wa[tid] = a < 3 ? root_acc : ang_acc;
    }
    __syncthreads();
}

// 1/2 sum w_v |x_t - x_{t-1}|^2 + 1/2 sum w_a |x_{t+1} - 2 x_t + x_{t-1}|^2 over the nw rows of x: every term whose stencil touches a
// free row (rows >= h)
__device__ double sm_prior_energy(SmSweepLds& L, const double* __restrict__ x, int nw, int h) {
    double s = 0.0;
    for (int i = threadIdx.x; i < nw * SK; i += SM_THREADS) {
        const int t = i / SK, q = i - t * SK, cx = L.colx[q];
        const double* xr = x + (size_t)t * 68 + cx;
        if (t >= 1 && t >= h) {
            const double dv = xr[0] - xr[-68];
            s += L.wv[q] * dv * dv;
        }
        if (t >= 1 && t + 1 < nw) {
            const double da = (xr[68] - 2.0 * xr[0]) + xr[-68];
            s += L.wa[q] * da * da;
        }
    }
    return 0.5 * sm_wg_sum(L.red, s);
}

// sum of the E of the m row blocks at blk + r blk_stride
__device__ double sm_data_energy(SmSweepLds& L, const double* __restrict__ blk, size_t blk_stride, int m) {
    double s = 0.0;
    for (int r = threadIdx.x; r < m; r += SM_THREADS) s += blk[(size_t)r * blk_stride + SKH + SK];
    return sm_wg_sum(L.red, s);
}

// One solve (every thread calls): the m free rows are the rows h .. h + m - 1 of the nw rows of x; row r reads its block at
// blk + r blk_stride and writes L_tt, L_{t+1,t}, L_{t+2,t}, d (over y), g and diag A at fac + r fac_stride (SM_WORK layout).
__device__ __forceinline__ SmStep sm_sweep(SmSweepLds& L, const double* __restrict__ blk, size_t blk_stride, double* __restrict__ fac,
                                           size_t fac_stride, const double* __restrict__ x, int m, int h, int nw, double mu) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    // ---- forward sweep over the free rows: L y = -g ----
    int iP1 = 0, iP2 = 1, iQ = 2, iN1 = 3, iN2 = 4, iy1 = 0, iy2 = 1, ib = 2;
    for (int i = tid; i < SK2; i += SM_THREADS) { L.B[0][i] = 0.0; L.B[1][i] = 0.0; L.B[2][i] = 0.0; }
    if (tid < SK) { L.y[0][tid] = 0.0; L.y[1][tid] = 0.0; }
    if (tid == 0) L.fail = 0;
    __syncthreads();
    for (int r = 0; r < m; ++r) {
        const int t = h + r;                       // the row's index among the nw rows (the prior's coefficients and stencils)
        const double* bt = blk + (size_t)r * blk_stride;
        double* wt = fac + (size_t)r * fac_stride;
        const double *P1 = L.B[iP1], *P2 = L.B[iP2], *Q = L.B[iQ], *y1 = L.y[iy1], *y2 = L.y[iy2];
        double *N1 = L.B[iN1], *N2 = L.B[iN2], *bb = L.y[ib];
        // phase A: S = A_tt + mu diag(A_tt) - P1 P1^T - P2 P2^T (lower); b = -g_t - P1 y1 - P2 y2; N1 = A_{t+1,t} - Q P1^T; N2 = A_{t+2,t}
        for (int i = tid; i < SKH; i += SM_THREADS) {
            int rr = 0;
            while ((rr + 1) * (rr + 2) / 2 <= i) ++rr;
            const int cc = i - rr * (rr + 1) / 2;
            double a = bt[sm_up(cc, rr)];
            if (rr == cc) {
                a += L.wv[rr] * sm_cv(t, t, nw) + L.wa[rr] * sm_ca(t, t, nw);
                wt[W_D + rr] = a;
                a += mu * a;
            }
            double s1 = 0.0, s2 = 0.0;
            if (r >= 1)
                for (int q = 0; q < SK; ++q) s1 += P1[rr * SK + q] * P1[cc * SK + q];
            if (r >= 2)
                for (int q = 0; q < SK; ++q) s2 += P2[rr * SK + q] * P2[cc * SK + q];
            L.S[rr * SK + cc] = (a - s1) - s2;
        }
        if (tid >= 192 && tid < 192 + SK) {
            const int q0 = tid - 192;
            const double g = bt[SKH + q0] + sm_prior_grad(x, t, nw, L.colx[q0], L.wv[q0], L.wa[q0]);
            wt[W_G + q0] = g;
            double s1 = 0.0, s2 = 0.0;
            for (int q = 0; q < SK; ++q) s1 += P1[q0 * SK + q] * y1[q];
            for (int q = 0; q < SK; ++q) s2 += P2[q0 * SK + q] * y2[q];
            bb[q0] = (-g - s1) - s2;
        }
        if (r + 1 < m)
            for (int i = tid; i < SK2; i += SM_THREADS) {
                const int rr = i / SK, cc = i - rr * SK;
                const double a = rr == cc ? L.wv[rr] * sm_cv(t + 1, t, nw) + L.wa[rr] * sm_ca(t + 1, t, nw) : 0.0;
                double s1 = 0.0;
                if (r >= 1)
                    for (int q = 0; q < SK; ++q) s1 += Q[rr * SK + q] * P1[cc * SK + q];
                N1[i] = a - s1;
                N2[i] = (r + 2 < m && rr == cc) ? L.wa[rr] * sm_ca(t + 2, t, nw) : 0.0;
            }
        __syncthreads();
        // phase B, wave 0: Cholesky of S with lane = row, the row in registers, each column broadcast through v_readlane; the
        // forward substitution of b in the same registers
        if (wave == 0) {
            double a[SK];
            const int row = lane < SK ? lane : SK - 1;
#pragma unroll
            for (int c = 0; c < SK; ++c) a[c] = (lane < SK && c <= lane) ? L.S[row * SK + c] : (c == lane ? 1.0 : 0.0);
            double bv = lane < SK ? bb[row] : 0.0;
            int bad = 0;
#pragma unroll
            for (int j = 0; j < SK; ++j) {
                const double piv = rl64(a[j], j);
                if (!(piv > 0.0 && piv < __longlong_as_double(0x7ff0000000000000LL))) bad = 1;
                const double rt = piv > 0.0 ? sqrt(piv) : 0.0;
                const double l = lane == j ? rt : a[j] / rt;
                a[j] = l;
#pragma unroll
                for (int k = j + 1; k < SK; ++k) a[k] -= l * rl64(l, k);
            }
#pragma unroll
            for (int j = 0; j < SK; ++j) {
                const double yj = rl64(bv / a[j], j);
                if (lane == j) bv = yj;
                if (lane > j) bv -= a[j] * yj;
            }
            if (lane < SK) {
#pragma unroll
                for (int c = 0; c < SK; ++c)
                    if (c <= lane) L.S[lane * SK + c] = a[c];
                bb[lane] = bv;
                wt[W_Y + lane] = bv;
            }
            if (bad && lane == 0) L.fail = 1;
        }
        __syncthreads();
        // phase C: N1 <- N1 L^-T on wave 0, N2 <- N2 L^-T on wave 1 (a row per lane in registers, L read as an LDS broadcast);
        // waves 2 and 3 write L_tt to the factor
        if (wave < 2 && r + 1 < m && (wave == 0 || r + 2 < m)) {
            double* Nw = wave == 0 ? N1 : N2;
            const int row = lane < SK ? lane : SK - 1;
            double v[SK];
#pragma unroll
            for (int c = 0; c < SK; ++c) v[c] = Nw[row * SK + c];
#pragma unroll
            for (int c = 0; c < SK; ++c) {
                double s = v[c];
#pragma unroll
                for (int q = 0; q < c; ++q) s -= v[q] * L.S[c * SK + q];
                v[c] = s / L.S[c * SK + c];
            }
            if (lane < SK) {
#pragma unroll
                for (int c = 0; c < SK; ++c) Nw[lane * SK + c] = v[c];
            }
        } else if (wave >= 2) {
            for (int i = tid - 128; i < SKH; i += 128) {
                int rr = 0;
                while ((rr + 1) * (rr + 2) / 2 <= i) ++rr;
                wt[i] = L.S[rr * SK + (i - rr * (rr + 1) / 2)];
            }
        }
        __syncthreads();
        // the factor's off-diagonal blocks to the workspace (read only from here on), and the roles rotate by index
        for (int i = tid; i < SK2; i += SM_THREADS) {
            wt[W_L1 + i] = N1[i];
            wt[W_L2 + i] = N2[i];
        }
        const int oP1 = iP1, oP2 = iP2, oy2 = iy2;
        iP2 = iQ; iP1 = iN1; iQ = iN2; iN1 = oP1; iN2 = oP2;
        iy2 = iy1; iy1 = ib; ib = oy2;
    }
    __syncthreads();
    // ---- back substitution on wave 0, no barrier: L^T d = y; lane = column of L_tt in registers, d broadcast by v_readlane ----
    if (wave == 0) {
        double d1 = 0.0, d2 = 0.0;
        const int col = lane < SK ? lane : SK - 1;
        for (int r = m - 1; r >= 0; --r) {
            double* wt = fac + (size_t)r * fac_stride;
            double bv = wt[W_Y + col];
            if (r + 1 < m) {
                double s1 = 0.0;
#pragma unroll
                for (int q = 0; q < SK; ++q) s1 += wt[W_L1 + q * SK + col] * rl64(d1, q);
                bv -= s1;
            }
            if (r + 2 < m) {
                double s2 = 0.0;
#pragma unroll
                for (int q = 0; q < SK; ++q) s2 += wt[W_L2 + q * SK + col] * rl64(d2, q);
                bv -= s2;
            }
            double c[SK];
#pragma unroll
            for (int j = 0; j < SK; ++j) c[j] = j >= col ? wt[sm_lo(j, col)] : 1.0;
#pragma unroll
            for (int j = SK - 1; j >= 0; --j) {
                const double dj = rl64(bv / c[j], j);
                if (lane == j) bv = dj;
                if (lane < j) bv -= c[j] * dj;
            }
            d2 = d1;
            d1 = lane < SK ? bv : 0.0;
            if (lane < SK) wt[W_Y + lane] = bv;
        }
    }
    __syncthreads();
    // ---- predicted reduction -(d.g + d^T A d / 2) = (-d.g + mu d^T diag(A) d) / 2, |d|_inf ----
    double sg = 0.0, sd = 0.0, dm = 0.0;
    for (int i = tid; i < m * SK; i += SM_THREADS) {
        const int r = i / SK, q = i - r * SK;
        const double* wt = fac + (size_t)r * fac_stride;
        const double dd = wt[W_Y + q];
        sg += dd * wt[W_G + q];
        sd += dd * dd * wt[W_D + q];
        dm = fmax(dm, fabs(dd));
    }
    L.red[tid] = sg;
    L.red2[tid] = sd;
    L.red3[tid] = dm;
    __syncthreads();
    for (int w = SM_THREADS / 2; w >= 1; w >>= 1) {
        if (tid < w) {
            L.red[tid] += L.red[tid + w];
            L.red2[tid] += L.red2[tid + w];
            L.red3[tid] = fmax(L.red3[tid], L.red3[tid + w]);
        }
        __syncthreads();
    }
    SmStep o;
    o.pred = 0.5 * (-L.red[0] + mu * L.red2[0]);
    o.dmax = L.red3[0];
    o.fail = L.fail;
    __syncthreads();
    return o;
}
