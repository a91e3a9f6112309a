// Trajectory smoothing of finished tracklets (multiview_motion_capture_amd/smoothing.py; algorithm restated in tests/smooth_np.py): one
// Levenberg-Marquardt solve per identity over every frame from its first to its last, E = the IK's stage-1 data term of every frame with
// selected views + a diagonal velocity / acceleration prior on the 39 stage-1 parameters.  No counterpart in the reference, whose only
// temporal element is the IK's warm start.
//   blocks  ONE wave per (identity, frame): FK, the stage-1 residual and its analytic Jacobian (angular velocity x lever arm through the
//           projection), reduced per observed joint first (W_k = sum_v s^2 (du du^T + dv dv^T), t_k = sum_v s (du fu + dv fv)), then
//           J^T J = sum_k D_k^T W_k D_k and J^T r = sum_k D_k^T t_k with D_k = d X_k / d x (3 x 39): the upper triangle, J^T r and E_t of
//           the frame into one of two block buffers (the other holds the blocks of the accepted point);
//   step    ONE 256-lane workgroup per identity: the accept / reject decision on the last trial (E summed in a fixed order), then the
//           block-banded Cholesky of (A + mu diag(A)) -- A = the data blocks + the exact prior Hessian, two off-diagonal blocks per row,
//           each prior block diagonal -- a forward sweep that keeps the last two block rows in LDS and writes the factor to the caller's
//           workspace, back-substitution, and the next trial point.
// Every sum runs in a fixed order inside one identity's own lanes: an identity's numbers depend on nothing else in the launch.
#define MVMC_DEVICE_ONLY
#include "mvmc_common.h"
#include "mvmc_track.hip"
#include "mvmc_ik1.hip"
#undef MVMC_DEVICE_ONLY

namespace {

#include "mvmc_smooth_row.h"

constexpr int SM_THREADS = 256;

__global__ void __launch_bounds__(64) smooth_blocks_kernel(Ik1Tables T, const double* __restrict__ kps17, const double* __restrict__ Pmats,
                                                           int C, int Pmax, const int32_t* __restrict__ rig_of,
                                                           const int32_t* __restrict__ members, const double* __restrict__ xe,
                                                           const int32_t* __restrict__ id_of, const int32_t* __restrict__ ctl,
                                                           int n_frames, double* __restrict__ blk) {
    __shared__ SmBlkLds L;
    const int f = blockIdx.x;
    const int id = uni((int)id_of[f]);
    if (uni((int)ctl[id * 4]) != 0) return;                      // stopped identity: nothing to evaluate
    const int buf = 1 - uni((int)ctl[id * 4 + 1]);               // the buffer that does not hold the accepted point's blocks
    sm_row_block(T, L, kps17, Pmats + (size_t)rig_of[f] * C * 12, C, Pmax, members + (size_t)f * C, xe + (size_t)f * 68,
                 blk + ((size_t)buf * n_frames + f) * SM_BLK);
}

// ---- step ----
struct SmStepLds {
    double S[SK2];            // the diagonal block being factored (lower triangle used), then L_tt
    double P1[SK2], P2[SK2];  // L(t, t-1), L(t, t-2)
    double Q[SK2];            // L(t+1, t-1)
    double N1[SK2], N2[SK2];  // L(t+1, t), L(t+2, t)
    double y1[SK], y2[SK], b[SK];
    double wv[SK], wa[SK];
    double red[SM_THREADS], red2[SM_THREADS], red3[SM_THREADS];
    int colx[SK];             // column of x (0..67) of each stage-1 parameter
    int fail;
};

// 1/2 sum w_v |x_t - x_{t-1}|^2 + 1/2 sum w_a |x_{t+1} - 2 x_t + x_{t-1}|^2 of one identity (every thread calls; fixed order)
__device__ double sm_prior_energy(SmStepLds& L, const double* __restrict__ x, int n) {
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int i = tid; i < n * SK; i += SM_THREADS) {
        const int t = i / SK, q = i - t * SK, cx = L.colx[q];
        if (t >= 1) {
            const double dv = x[(size_t)t * 68 + cx] - x[(size_t)(t - 1) * 68 + cx];
            s += L.wv[q] * dv * dv;
        }
        if (t >= 1 && t + 1 < n) {
            const double da = (x[(size_t)(t + 1) * 68 + cx] - 2.0 * x[(size_t)t * 68 + cx]) + x[(size_t)(t - 1) * 68 + cx];
            s += L.wa[q] * da * da;
        }
    }
    L.red[tid] = s;
    __syncthreads();
    for (int w = SM_THREADS / 2; w >= 1; w >>= 1) {
        if (tid < w) L.red[tid] += L.red[tid + w];
        __syncthreads();
    }
    const double r = 0.5 * L.red[0];
    __syncthreads();
    return r;
}

// sum of the blocks' E over the identity's frames (fixed order)
__device__ double sm_data_energy(SmStepLds& L, const double* __restrict__ blk, int n) {
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int t = tid; t < n; t += SM_THREADS) s += blk[(size_t)t * SM_BLK + SKH + SK];
    L.red[tid] = s;
    __syncthreads();
    for (int w = SM_THREADS / 2; w >= 1; w >>= 1) {
        if (tid < w) L.red[tid] += L.red[tid + w];
        __syncthreads();
    }
    const double r = L.red[0];
    __syncthreads();
    return r;
}

__global__ void __launch_bounds__(SM_THREADS) smooth_step_kernel(Ik1Tables T, double* __restrict__ xall, double* __restrict__ xtall,
                                                                 const double* __restrict__ blk, const int32_t* __restrict__ id_lo,
                                                                 int n_frames, double root_vel, double root_acc, double ang_vel,
                                                                 double ang_acc, double mu0, double ftol, double xtol, int max_iter,
                                                                 int phase, int32_t* __restrict__ ctl, double* __restrict__ info,
                                                                 double* __restrict__ work) {
    __shared__ SmStepLds L;
    const int tid = threadIdx.x, id = blockIdx.x;
    int32_t* cl = ctl + id * 4;
    if (uni((int)cl[0]) != 0) return;   // stopped: wave-uniform for the whole workgroup
    const int lo = id_lo[id], n = id_lo[id + 1] - lo;
    double* inf = info + (size_t)id * MVMC_SMOOTH_INFO_DOUBLES;
    double* x = xall + (size_t)lo * 68;
    double* xt = xtall + (size_t)lo * 68;
    double* wk = work + (size_t)lo * SM_WORK;
    if (tid < SK) {
        const int a = T.act[0][tid];
        L.colx[tid] = a;
        L.wv[tid] = a < 3 ? root_vel : ang_vel;
        L.wa[tid] = a < 3 ? root_acc : ang_acc;
    }
    __syncthreads();
    int cur = uni((int)cl[1]);
    const double* bcur;
    double mu;
    int trials, n_acc;
    if (phase == 0) {   // the start: the blocks at x0 are in buffer 1 - cur
        cur = 1 - cur;
        bcur = blk + ((size_t)cur * n_frames + lo) * SM_BLK;
        const double Ed = sm_data_energy(L, bcur, n), Ep = sm_prior_energy(L, x, n);
        if (tid < MVMC_SMOOTH_INFO_DOUBLES) inf[tid] = tid < 8 ? 0.0 : -1.0;
        __syncthreads();
        if (tid == 0) { inf[0] = Ed; inf[1] = Ep; inf[2] = Ed; inf[3] = Ep; cl[1] = cur; }
        mu = mu0;
        trials = 0;
        n_acc = 0;
    } else {            // the decision on the trial whose blocks are in buffer 1 - cur
        const double* btr = blk + ((size_t)(1 - cur) * n_frames + lo) * SM_BLK;
        const double Etd = sm_data_energy(L, btr, n), Etp = sm_prior_energy(L, xt, n);
        const double Ed = inf[2], Ep = inf[3];
        const double E = Ed + Ep, Et = Etd + Etp;
        mu = inf[6];
        trials = (int)inf[4];
        n_acc = (int)inf[5];
        __syncthreads();
        const bool acc = Et < E;
        if (tid == 0) inf[8 + trials] = acc ? 1.0 : 0.0;
        ++trials;
        bool stop = false;
        if (acc) {
            for (int i = tid; i < n * 68; i += SM_THREADS) x[i] = xt[i];
            cur = 1 - cur;
            mu /= 10.0;
            ++n_acc;
            if (tid == 0) { inf[2] = Etd; inf[3] = Etp; cl[1] = cur; }
            if (E - Et < ftol * E) stop = true;
        } else {
            mu *= 10.0;
        }
        if (stop) {
            if (tid == 0) { inf[4] = trials; inf[5] = n_acc; inf[6] = mu; inf[7] = 4.0; cl[0] = 1; }
            return;
        }
        bcur = blk + ((size_t)cur * n_frames + lo) * SM_BLK;
    }
    if (trials >= max_iter) {
        if (tid == 0) { inf[4] = trials; inf[5] = n_acc; inf[6] = mu; inf[7] = 1.0; cl[0] = 1; }
        return;
    }
    // ---- forward sweep: L y = -g ----
    for (int i = tid; i < SK2; i += SM_THREADS) { L.P1[i] = 0.0; L.P2[i] = 0.0; L.Q[i] = 0.0; }
    if (tid < SK) { L.y1[tid] = 0.0; L.y2[tid] = 0.0; }
    if (tid == 0) L.fail = 0;
    __syncthreads();
    for (int t = 0; t < n; ++t) {
        const double* bt = bcur + (size_t)t * SM_BLK;
        double* wt = wk + (size_t)t * SM_WORK;
        // S = A_tt + mu diag(A_tt) - P1 P1^T - P2 P2^T (lower triangle); b = -g_t - P1 y1 - P2 y2
        for (int i = tid; i < SKH; i += SM_THREADS) {
            int rr = 0;
            while ((rr + 1) * (rr + 2) / 2 <= i) ++rr;
            const int cc = i - rr * (rr + 1) / 2;
            double a = bt[sm_up(cc, rr)];
            if (rr == cc) {
                a += L.wv[rr] * sm_cv(t, t, n) + L.wa[rr] * sm_ca(t, t, n);
                wt[W_D + rr] = a;
                a += mu * a;
            }
            double s1 = 0.0, s2 = 0.0;
            for (int q = 0; q < SK; ++q) s1 += L.P1[rr * SK + q] * L.P1[cc * SK + q];
            for (int q = 0; q < SK; ++q) s2 += L.P2[rr * SK + q] * L.P2[cc * SK + q];
            L.S[rr * SK + cc] = (a - s1) - s2;
        }
        if (tid < SK) {
            const double g = bt[SKH + tid] + sm_prior_grad(x, t, n, L.colx[tid], L.wv[tid], L.wa[tid]);
            wt[W_G + tid] = g;
            double s1 = 0.0, s2 = 0.0;
            for (int q = 0; q < SK; ++q) s1 += L.P1[tid * SK + q] * L.y1[q];
            for (int q = 0; q < SK; ++q) s2 += L.P2[tid * SK + q] * L.y2[q];
            L.b[tid] = (-g - s1) - s2;
        }
        // N1 = A_{t+1,t} - Q P1^T, N2 = A_{t+2,t} (both prior blocks are diagonal)
        if (t + 1 < n)
            for (int i = tid; i < SK2; i += SM_THREADS) {
                const int rr = i / SK, cc = i - rr * SK;
                double a = rr == cc ? L.wv[rr] * sm_cv(t + 1, t, n) + L.wa[rr] * sm_ca(t + 1, t, n) : 0.0;
                double s1 = 0.0;
                for (int q = 0; q < SK; ++q) s1 += L.Q[rr * SK + q] * L.P1[cc * SK + q];
                L.N1[i] = a - s1;
                L.N2[i] = (t + 2 < n && rr == cc) ? L.wa[rr] * sm_ca(t + 2, t, n) : 0.0;
            }
        __syncthreads();
        // Cholesky of S and the forward substitution of b: one wave, lane = row
        if (tid < 64) {
            for (int j = 0; j < SK; ++j) {
                double s = 0.0;
                if (tid >= j && tid < SK) {
                    s = L.S[tid * SK + j];
                    for (int q = 0; q < j; ++q) s -= L.S[tid * SK + q] * L.S[j * SK + q];
                }
                if (tid == j) L.S[j * SK + j] = s > 0.0 ? sqrt(s) : 0.0;
                if (tid == j && !(s > 0.0 && s < __longlong_as_double(0x7ff0000000000000LL))) L.fail = 1;
                MVMC_WAVE_SYNC();
                if (tid > j && tid < SK) L.S[tid * SK + j] = s / L.S[j * SK + j];
                MVMC_WAVE_SYNC();
            }
            for (int j = 0; j < SK; ++j) {
                const double yj = L.b[j] / L.S[j * SK + j];
                MVMC_WAVE_SYNC();
                if (tid == j) L.b[j] = yj;
                if (tid > j && tid < SK) L.b[tid] -= L.S[tid * SK + j] * yj;
                MVMC_WAVE_SYNC();
            }
        }
        __syncthreads();
        // N1 <- N1 L^-T, N2 <- N2 L^-T: one row per lane
        if (t + 1 < n && tid < 2 * SK) {
            double* Rw = (tid < SK ? L.N1 : L.N2) + (tid < SK ? tid : tid - SK) * SK;
            for (int c = 0; c < SK; ++c) {
                double s = Rw[c];
                for (int q = 0; q < c; ++q) s -= Rw[q] * L.S[c * SK + q];
                Rw[c] = s / L.S[c * SK + c];
            }
        }
        __syncthreads();
        for (int i = tid; i < SKH; i += SM_THREADS) {
            int rr = 0;
            while ((rr + 1) * (rr + 2) / 2 <= i) ++rr;
            wt[i] = L.S[rr * SK + (i - rr * (rr + 1) / 2)];
        }
        for (int i = tid; i < SK2; i += SM_THREADS) {
            wt[W_L1 + i] = L.N1[i];
            wt[W_L2 + i] = L.N2[i];
            L.P2[i] = L.Q[i];
            L.P1[i] = L.N1[i];
            L.Q[i] = L.N2[i];
        }
        if (tid < SK) {
            wt[W_Y + tid] = L.b[tid];
            L.y2[tid] = L.y1[tid];
            L.y1[tid] = L.b[tid];
        }
        __syncthreads();
    }
    // ---- back substitution: L^T d = y (d over y in the workspace; d_{t+1}, d_{t+2} in y1, y2) ----
    if (tid < SK) { L.y1[tid] = 0.0; L.y2[tid] = 0.0; }
    __syncthreads();
    for (int t = n - 1; t >= 0; --t) {
        double* wt = wk + (size_t)t * SM_WORK;
        if (tid < SK) {
            double z = wt[W_Y + tid];
            double s1 = 0.0, s2 = 0.0;
            if (t + 1 < n)
                for (int q = 0; q < SK; ++q) s1 += wt[W_L1 + q * SK + tid] * L.y1[q];
            if (t + 2 < n)
                for (int q = 0; q < SK; ++q) s2 += wt[W_L2 + q * SK + tid] * L.y2[q];
            L.b[tid] = (z - s1) - s2;
        }
        for (int i = tid; i < SKH; i += SM_THREADS) {
            int rr = 0;
            while ((rr + 1) * (rr + 2) / 2 <= i) ++rr;
            L.S[rr * SK + (i - rr * (rr + 1) / 2)] = wt[i];
        }
        __syncthreads();
        if (tid < 64) {
            for (int j = SK - 1; j >= 0; --j) {
                const double dj = L.b[j] / L.S[j * SK + j];
                MVMC_WAVE_SYNC();
                if (tid == j) L.b[j] = dj;
                if (tid < j) L.b[tid] -= L.S[j * SK + tid] * dj;
                MVMC_WAVE_SYNC();
            }
        }
        __syncthreads();
        if (tid < SK) {
            wt[W_Y + tid] = L.b[tid];
            L.y2[tid] = L.y1[tid];
            L.y1[tid] = L.b[tid];
        }
        __syncthreads();
    }
    // ---- predicted reduction -(d.g + d^T A d / 2) = (-d.g + mu d^T diag(A) d) / 2, |d|_inf; then the trial point ----
    double sg = 0.0, sd = 0.0, dm = 0.0;
    for (int i = tid; i < n * SK; i += SM_THREADS) {
        const int t = i / SK, q = i - t * SK;
        const double* wt = wk + (size_t)t * SM_WORK;
        const double d = wt[W_Y + q];
        sg += d * wt[W_G + q];
        sd += d * d * wt[W_D + q];
        dm = fmax(dm, fabs(d));
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
    const double E = inf[2] + inf[3];
    const double pred = 0.5 * (-L.red[0] + mu * L.red2[0]);
    const double dmax = L.red3[0];
    const int fail = uni(L.fail);
    int why = 0;
    if (fail || !(dmax == dmax)) why = 5;
    else if (dmax < xtol) why = 2;
    else if (pred < ftol * E) why = 3;
    if (why) {
        if (tid == 0) { inf[4] = trials; inf[5] = n_acc; inf[6] = mu; inf[7] = why; cl[0] = 1; }
        return;
    }
    for (int i = tid; i < n * 68; i += SM_THREADS) xt[i] = x[i];
    __syncthreads();
    for (int i = tid; i < n * SK; i += SM_THREADS) {
        const int t = i / SK, q = i - t * SK;
        xt[(size_t)t * 68 + L.colx[q]] = x[(size_t)t * 68 + L.colx[q]] + wk[(size_t)t * SM_WORK + W_Y + q];
    }
    if (tid == 0) { inf[4] = trials; inf[5] = n_acc; inf[6] = mu; inf[7] = 0.0; }
}


}  // namespace

extern "C" int mvmc_smooth_blocks(const mvmcSkeleton* skel_host, const double* kps17, int n_views, int p_max, const double* Pmats,
                                  const int32_t* rig_of, const int32_t* members, const double* x, const int32_t* id_of, const int32_t* ctl,
                                  int n_frames, double* blk, mvmcStream_t stream) {
    if (!skel_host || n_frames < 0 || n_views <= 0 || n_views > MVMC_SMOOTH_MAX_VIEWS || p_max <= 0) return MVMC_ERR_ARG;
    if (n_frames == 0) return MVMC_OK;
    if (!kps17 || !Pmats || !rig_of || !members || !x || !id_of || !ctl || !blk) return MVMC_ERR_ARG;
    Ik1Tables T;
    if (!sm_tables(skel_host, &T)) return MVMC_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(smooth_blocks_kernel, dim3(n_frames), dim3(64), 0, (hipStream_t)stream, T, kps17, Pmats, n_views, p_max, rig_of,
                       members, x, id_of, ctl, n_frames, blk);
    MVMC_CHECK_LAUNCH();
    return MVMC_OK;
}

extern "C" int mvmc_smooth_step(const mvmcSkeleton* skel_host, double* x, double* x_trial, const double* blk, const int32_t* id_lo,
                                int n_ids, int n_frames, double root_vel, double root_acc, double ang_vel, double ang_acc, double mu0,
                                double ftol, double xtol, int max_iter, int phase, int32_t* ctl, double* info, double* work,
                                mvmcStream_t stream) {
    if (!skel_host || n_ids < 0 || n_frames < 0 || phase < 0 || max_iter < 0 || max_iter > MVMC_SMOOTH_INFO_DOUBLES - 8) return MVMC_ERR_ARG;
    if (!(root_vel >= 0.0) || !(root_acc >= 0.0) || !(ang_vel >= 0.0) || !(ang_acc >= 0.0) || !(mu0 > 0.0)) return MVMC_ERR_ARG;
    if (n_ids == 0) return MVMC_OK;
    if (!x || !x_trial || !blk || !id_lo || !ctl || !info || !work) return MVMC_ERR_ARG;
    Ik1Tables T;
    if (!sm_tables(skel_host, &T)) return MVMC_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(smooth_step_kernel, dim3(n_ids), dim3(SM_THREADS), 0, (hipStream_t)stream, T, x, x_trial, blk, id_lo, n_frames,
                       root_vel, root_acc, ang_vel, ang_acc, mu0, ftol, xtol, max_iter, phase, ctl, info, work);
    MVMC_CHECK_LAUNCH();
    return MVMC_OK;
}
