// Body fit of finished tracklets (multiview_motion_capture_amd/body_fit.py; algorithm restated in tests/body_fit_np.py): one side-length
// vector per identity, every frame's pose re-solved against it.  No counterpart in the reference, whose IK fits the lengths again on
// every frame (inverse_kinematics.py:380-433).
//   observe   per (problem, camera): the pose nearest to the record's joints (reprojection_error, motion_capture.py:403-414, the
//             distance mvmc_st_affinity uses), then one pass per problem that settles two problems of one frame claiming one pose;
//   lengths   Levenberg-Marquardt on the identity's 11 side lengths with every root and angle fixed: ONE 64-lane workgroup per identity
//             runs the whole loop; the sums over its problems are per-lane partials in a fixed problem order and a fixed butterfly, so
//             an identity's numbers depend on nothing else in the launch;
//   pose      stage 1 of PoseSolver.solve (solve_pose_reproj, :202-238) with a calibration per problem: the stand-alone IK kernel's
//             device code (ik1_solve) with the problem's rig selected by offsetting the projection matrices.
#define MVMC_DEVICE_ONLY
#include "mvmc_common.h"
#include "mvmc_track.hip"
#include "mvmc_ik1.hip"
#undef MVMC_DEVICE_ONLY

namespace {

constexpr int BF_NS = MVMC_N_SIDE;
constexpr int BF_NH = BF_NS * (BF_NS + 1) / 2;   // upper triangle of J^T J
constexpr int BF_WORK = MVMC_BODY_WORK_DOUBLES;   // per problem: global rotations, bone vectors R_parent dir, joint positions

__device__ __forceinline__ double bf_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

// ---- observation selection ----
__global__ void body_dist_kernel(const double* __restrict__ kps17, const int32_t* __restrict__ counts, const double* __restrict__ Pmats,
                                 const int32_t* __restrict__ frame_of, const int32_t* __restrict__ rig_of, const double* __restrict__ joints,
                                 int B, int C, int Pmax, int n_frames, int n_rigs, double min_score, double max_dist,
                                 int32_t* __restrict__ choice, double* __restrict__ dist) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * C) return;
    const int b = idx / C, c = idx - b * C;
    const int f = frame_of[b], r = rig_of[b];
    int best = -1;
    double bd = __longlong_as_double(0x7ff0000000000000LL);
    if (f >= 0 && f < n_frames && r >= 0 && r < n_rigs) {
        const int n = counts[(size_t)f * C + c];
        const double* P = Pmats + ((size_t)r * C + c) * 12;
        for (int p = 0; p < n && p < Pmax; ++p) {
            const int q = (f * C + c) * Pmax + p;
            const double d = reproj_error(joints + (size_t)b * 54, kps17 + (size_t)q * 51, P, min_score);
            if (d < max_dist && d < bd) { best = q; bd = d; }   // (NaN: no joint above min_score, never a candidate)
        }
    }
    choice[idx] = best;
    dist[idx] = bd;
}

// one problem per thread: a pose another problem of the same frame holds at a smaller distance (equal: lower rank) is given up
__global__ void body_resolve_kernel(const int32_t* __restrict__ choice, const double* __restrict__ dist, const int32_t* __restrict__ order,
                                    const int32_t* __restrict__ grp_lo, const int32_t* __restrict__ grp_hi, const int32_t* __restrict__ rank,
                                    int B, int C, int32_t* __restrict__ members, int32_t* __restrict__ n_views) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int lo = grp_lo[b], hi = grp_hi[b], rb = rank[b];
    int nv = 0;
    for (int c = 0; c < C; ++c) {
        const int q = choice[(size_t)b * C + c];
        bool keep = q >= 0;
        if (keep) {
            const double d = dist[(size_t)b * C + c];
            for (int i = lo; i < hi && keep; ++i) {
                const int b2 = order[i];
                if (b2 == b || choice[(size_t)b2 * C + c] != q) continue;
                const double d2 = dist[(size_t)b2 * C + c];
                if (d2 < d || (d2 == d && rank[b2] < rb)) keep = false;
            }
        }
        members[(size_t)b * C + c] = keep ? q : -1;
        nv += keep;
    }
    n_views[b] = nv;
}

// ---- length step ----
struct BfLds {
    double dirs[18 * 3];
    int parents[18], side[18];
    double lens[BF_NS], trial[BF_NS], delta[BF_NS];
    double H[BF_NH], g[BF_NS], E;        // at lens
    double Ht[BF_NH], gt[BF_NS], Et;     // at trial
    int flag;
};

__device__ __forceinline__ int bf_hidx(int s, int t) { return s * BF_NS - s * (s - 1) / 2 + (t - s); }   // s <= t

__device__ __forceinline__ double bf_wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return __shfl(v, 0, 64);   // (lanes round differently: lane 0's sum for everyone)
}

// global rotations and bone vectors of problem p (work: this lane's own rows, written and read by the same lane)
__device__ void bf_basis(const BfLds& L, const double* __restrict__ x, double* __restrict__ w) {
    double* Rg = w;
    double* bv = w + 162;
    for (int j = 0; j < 18; ++j) {
        double R[9];
        euler_to_rot(x + 3 + 3 * j, R);
        const int p = L.parents[j];
        if (p < 0) {
            for (int e = 0; e < 9; ++e) Rg[e] = R[e];
            bv[0] = bv[1] = bv[2] = 0.0;
            continue;
        }
        const double* Rp = Rg + 9 * p;
        for (int a = 0; a < 3; ++a)
            for (int c = 0; c < 3; ++c) Rg[9 * j + 3 * a + c] = Rp[3 * a] * R[c] + Rp[3 * a + 1] * R[3 + c] + Rp[3 * a + 2] * R[6 + c];
        for (int a = 0; a < 3; ++a)
            bv[3 * j + a] = Rp[3 * a] * L.dirs[3 * j] + Rp[3 * a + 1] * L.dirs[3 * j + 1] + Rp[3 * a + 2] * L.dirs[3 * j + 2];
    }
}

// E, H = J^T J, g = J^T r of the identity at lengths ln (LDS), into (Hout, gout, Eout) of L; every lane calls
__device__ void bf_eval(BfLds& L, const double* ln, double* Hout, double* gout, double* Eout, const double* __restrict__ kps17,
                        const double* __restrict__ Pmats, const int32_t* __restrict__ rig_of, const int32_t* __restrict__ members,
                        const double* __restrict__ params, double* __restrict__ work, int lo, int hi, int C, int Pmax) {
    const int lane = threadIdx.x & 63;
    double H[BF_NH], g[BF_NS], E = 0.0;
#pragma unroll
    for (int i = 0; i < BF_NH; ++i) H[i] = 0.0;
#pragma unroll
    for (int i = 0; i < BF_NS; ++i) g[i] = 0.0;
    for (int p = lo + lane; p < hi; p += 64) {
        const double* x = params + (size_t)p * 68;
        double* w = work + (size_t)p * BF_WORK;
        const double* bv = w + 162;
        double* X = w + 216;
        X[0] = x[0]; X[1] = x[1]; X[2] = x[2];
        for (int j = 1; j < 18; ++j) {
            const int pj = L.parents[j];
            const double l = ln[L.side[j]];
            for (int a = 0; a < 3; ++a) X[3 * j + a] = X[3 * pj + a] + bv[3 * j + a] * l;
        }
        const double* Pbase = Pmats + (size_t)rig_of[p] * C * 12;
        for (int c = 0; c < C; ++c) {
            const int m = members[(size_t)p * C + c];
            if (m < 0) continue;
            const double* P = Pbase + ((m / Pmax) % C) * 12;
            const double* kp = kps17 + (size_t)m * 51;
            for (int r = 0; r < NOBS; ++r) {
                const int k = kIkSkel[r], ob = kIkObs[r];
                double ox, oy, ow;
                if (ob == 17) {
                    ox = 0.5 * (0.5 * (kp[15] + kp[18]) + 0.5 * (kp[33] + kp[36]));
                    oy = 0.5 * (0.5 * (kp[16] + kp[19]) + 0.5 * (kp[34] + kp[37]));
                    ow = kp[17] * kp[20];
                    ow *= kp[35] * kp[38];
                } else {
                    ox = kp[3 * ob]; oy = kp[3 * ob + 1]; ow = kp[3 * ob + 2];
                }
                const double X0 = X[3 * k], X1 = X[3 * k + 1], X2 = X[3 * k + 2];
                const double h0 = P[0] * X0 + P[1] * X1 + P[2] * X2 + P[3];
                const double h1 = P[4] * X0 + P[5] * X1 + P[6] * X2 + P[7];
                const double wd = P[8] * X0 + P[9] * X1 + P[10] * X2 + P[11] + 1e-5;
                const double u = h0 / wd, v = h1 / wd;
                const double ru = (u - ox) * ow, rv = (v - oy) * ow;
                E += ru * ru + rv * rv;
                double du[3], dv[3];
                for (int a = 0; a < 3; ++a) { du[a] = (P[a] - u * P[8 + a]) / wd; dv[a] = (P[4 + a] - v * P[8 + a]) / wd; }
                double ju[BF_NS], jv[BF_NS];
#pragma unroll
                for (int s = 0; s < BF_NS; ++s) { ju[s] = 0.0; jv[s] = 0.0; }
                for (int j = k; j != 0; j = L.parents[j]) {
                    const double cu = du[0] * bv[3 * j] + du[1] * bv[3 * j + 1] + du[2] * bv[3 * j + 2];
                    const double cv = dv[0] * bv[3 * j] + dv[1] * bv[3 * j + 1] + dv[2] * bv[3 * j + 2];
                    const int sj = L.side[j];
#pragma unroll
                    for (int s = 0; s < BF_NS; ++s)
                        if (s == sj) { ju[s] += cu; jv[s] += cv; }
                }
#pragma unroll
                for (int s = 0; s < BF_NS; ++s) {
                    ju[s] *= ow; jv[s] *= ow;
                    g[s] += ju[s] * ru + jv[s] * rv;
                }
#pragma unroll
                for (int s = 0; s < BF_NS; ++s)
#pragma unroll
                    for (int t = s; t < BF_NS; ++t) H[bf_hidx(s, t)] += ju[s] * ju[t] + jv[s] * jv[t];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < BF_NH; ++i) H[i] = bf_wave_sum(H[i]);
#pragma unroll
    for (int i = 0; i < BF_NS; ++i) g[i] = bf_wave_sum(g[i]);
    E = 0.5 * bf_wave_sum(E);
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < BF_NH; ++i) Hout[i] = H[i];
#pragma unroll
        for (int i = 0; i < BF_NS; ++i) gout[i] = g[i];
        *Eout = E;
    }
    MVMC_WAVE_SYNC();
}

// (H + mu diag(H)) d = -g on the free slots (Cholesky; held slots: d = 0); lane 0 only.  Returns the model's predicted reduction.
__device__ double bf_solve(const double* H, const double* g, int free, double mu, double* d) {
    double M[BF_NS][BF_NS], y[BF_NS];
    for (int s = 0; s < BF_NS; ++s) {
        const bool fs = (free >> s) & 1;
        for (int t = 0; t < BF_NS; ++t) {
            const bool ft = (free >> t) & 1;
            const double h = H[s <= t ? bf_hidx(s, t) : bf_hidx(t, s)];
            M[s][t] = (fs && ft) ? (s == t ? h + mu * h : h) : (s == t ? 1.0 : 0.0);
        }
        y[s] = fs ? -g[s] : 0.0;
    }
    for (int j = 0; j < BF_NS; ++j) {
        double a = M[j][j];
        for (int k = 0; k < j; ++k) a -= M[j][k] * M[j][k];
        a = sqrt(a);
        M[j][j] = a;
        for (int i = j + 1; i < BF_NS; ++i) {
            double b = M[i][j];
            for (int k = 0; k < j; ++k) b -= M[i][k] * M[j][k];
            M[i][j] = b / a;
        }
    }
    for (int i = 0; i < BF_NS; ++i) {
        double b = y[i];
        for (int k = 0; k < i; ++k) b -= M[i][k] * y[k];
        y[i] = b / M[i][i];
    }
    for (int i = BF_NS - 1; i >= 0; --i) {
        double b = y[i];
        for (int k = i + 1; k < BF_NS; ++k) b -= M[k][i] * d[k];
        d[i] = b / M[i][i];
    }
    double dg = 0.0, dHd = 0.0;
    for (int s = 0; s < BF_NS; ++s) {
        if (!((free >> s) & 1)) { d[s] = 0.0; continue; }
        dg += d[s] * g[s];
        for (int t = 0; t < BF_NS; ++t)
            if ((free >> t) & 1) dHd += d[s] * H[s <= t ? bf_hidx(s, t) : bf_hidx(t, s)] * d[t];
    }
    return -(dg + 0.5 * dHd);
}

__global__ void __launch_bounds__(64) body_lengths_kernel(SkelDev sk, const double* __restrict__ kps17, const double* __restrict__ Pmats,
                                                          const int32_t* __restrict__ rig_of, const int32_t* __restrict__ members,
                                                          const double* __restrict__ params, const int32_t* __restrict__ id_lo, int C,
                                                          int Pmax, double* __restrict__ lens, int32_t* __restrict__ free_mask,
                                                          int fix_free, int max_iter, double mu0, double ftol, double xtol,
                                                          double* __restrict__ info, double* __restrict__ work) {
    __shared__ BfLds L;
    const int lane = threadIdx.x & 63, id = blockIdx.x;
    const int lo = id_lo[id], hi = id_lo[id + 1];
    if (lane < 18) {
        L.parents[lane] = sk.parents[lane];
        L.side[lane] = sk.side_map[lane];
        for (int a = 0; a < 3; ++a) L.dirs[3 * lane + a] = sk.dirs[lane][a];
    }
    if (lane < BF_NS) L.lens[lane] = lens[(size_t)id * BF_NS + lane];
    double* inf = info + (size_t)id * MVMC_BODY_INFO_DOUBLES;
    if (lane < MVMC_BODY_INFO_DOUBLES) inf[lane] = lane < 4 ? 0.0 : -1.0;
    MVMC_WAVE_SYNC();
    for (int p = lo + lane; p < hi; p += 64) bf_basis(L, params + (size_t)p * 68, work + (size_t)p * BF_WORK);
    bf_eval(L, L.lens, L.H, L.g, &L.E, kps17, Pmats, rig_of, members, params, work, lo, hi, C, Pmax);
    int free;
    if (fix_free) free = free_mask[id];
    else {
        free = 0;
        for (int s = 0; s < BF_NS; ++s)
            if (L.H[bf_hidx(s, s)] > 0.0) free |= 1 << s;
        if (lane == 0) free_mask[id] = free;
    }
    free = uni(free);
    const double E0 = uni(L.E);
    int n_acc = 0, it = 0;
    double mu = mu0;
    if (free != 0) {
        for (; it < max_iter; ++it) {
            if (lane == 0) {
                double dmax = 0.0;
                const double pred = bf_solve(L.H, L.g, free, mu, L.delta);
                for (int s = 0; s < BF_NS; ++s) { L.trial[s] = L.lens[s] + L.delta[s]; dmax = fmax(dmax, fabs(L.delta[s])); }
                L.flag = (dmax < xtol || pred < ftol * L.E) ? 1 : 0;
            }
            MVMC_WAVE_SYNC();
            if (uni(L.flag)) break;
            bf_eval(L, L.trial, L.Ht, L.gt, &L.Et, kps17, Pmats, rig_of, members, params, work, lo, hi, C, Pmax);
            const double E = uni(L.E), Et = uni(L.Et);
            const bool acc = Et < E;
            if (lane == 0) inf[4 + it] = acc ? 1.0 : 0.0;
            if (acc) {
                if (lane < BF_NS) { L.lens[lane] = L.trial[lane]; L.g[lane] = L.gt[lane]; }
                for (int i = lane; i < BF_NH; i += 64) L.H[i] = L.Ht[i];
                if (lane == 0) L.E = Et;
                MVMC_WAVE_SYNC();
                mu /= 10.0;
                ++n_acc;
                if (E - Et < ftol * E) { ++it; break; }
            } else {
                mu *= 10.0;
            }
        }
    }
    if (lane < BF_NS) lens[(size_t)id * BF_NS + lane] = L.lens[lane];
    if (lane == 0) { inf[0] = E0; inf[1] = L.E; inf[2] = (double)it; inf[3] = (double)n_acc; }
}

// ---- pose step: ik1_solve with the problem's rig ----
__global__ void __launch_bounds__(64, MVMC_SMALL_WPS)
body_pose_kernel(SkelDev skarg, const double* __restrict__ kps17, const double* __restrict__ Pmats, const int32_t* __restrict__ rig_of,
                 int n_rigs, const int32_t* __restrict__ members, int B, int V, int vcap, int C, int Pmax, const double* __restrict__ init,
                 int max_nfev, double* __restrict__ params_out, double* __restrict__ joints_out, double* __restrict__ info_out,
                 double* __restrict__ scratch, int stage_mask) {
    __shared__ Ik1Shared S;
    __shared__ Ik1Tables T;
    extern __shared__ __attribute__((aligned(16))) int bf_members[];
    const int lane = threadIdx.x & 63, b = blockIdx.x;
    const int r = uni((int)rig_of[b]);
    if (r < 0 || r >= n_rigs) {   // no calibration: NaN, as a problem with fewer than two views
        for (int i = lane; i < 68; i += 64) params_out[(size_t)b * 68 + i] = bf_nan();
        if (lane < 54) joints_out[(size_t)b * 54 + lane] = bf_nan();
        if (info_out && lane < 8) info_out[(size_t)b * 8 + lane] = bf_nan();
        return;
    }
    ik1_build_tables(T, skarg);
    ik1_solve(S, bf_members, reinterpret_cast<unsigned short*>(bf_members + vcap), vcap, T, kps17, Pmats + (size_t)r * C * 12, members, b, V,
              C, Pmax, init, nullptr, max_nfev, max_nfev, params_out, joints_out, info_out, scratch, stage_mask | 4, nullptr, nullptr);
}

}  // namespace

extern "C" int mvmc_body_observe(const double* kps17, const int32_t* counts, int n_frames, int n_views, int p_max, const double* Pmats,
                                 int n_rigs, const int32_t* frame_of, const int32_t* rig_of, const double* joints, const int32_t* order,
                                 const int32_t* grp_lo, const int32_t* grp_hi, const int32_t* rank, int n_problems, double min_score,
                                 double max_dist, int32_t* choice, double* dist, int32_t* members, int32_t* n_views_out,
                                 mvmcStream_t stream) {
    if (n_problems < 0 || n_frames <= 0 || n_views <= 0 || p_max <= 0 || n_rigs <= 0) return MVMC_ERR_ARG;
    if (n_problems == 0) return MVMC_OK;
    if (!kps17 || !counts || !Pmats || !frame_of || !rig_of || !joints || !order || !grp_lo || !grp_hi || !rank || !choice || !dist ||
        !members || !n_views_out)
        return MVMC_ERR_ARG;
    const long long pairs = (long long)n_problems * n_views;
    if (pairs > 0x7fffffffLL || (long long)n_frames * n_views * p_max > 0x7fffffffLL) return MVMC_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(body_dist_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, st, kps17, counts, Pmats, frame_of, rig_of,
                       joints, n_problems, n_views, p_max, n_frames, n_rigs, min_score, max_dist, choice, dist);
    MVMC_CHECK_LAUNCH();
    hipLaunchKernelGGL(body_resolve_kernel, dim3((n_problems + 255) / 256), dim3(256), 0, st, choice, dist, order, grp_lo, grp_hi, rank,
                       n_problems, n_views, members, n_views_out);
    MVMC_CHECK_LAUNCH();
    return MVMC_OK;
}

extern "C" int mvmc_body_lengths(const mvmcSkeleton* skel_host, const double* kps17, int n_views, int p_max, const double* Pmats,
                                 const int32_t* rig_of, const int32_t* members, const double* params, const int32_t* id_lo, int n_ids,
                                 double* lens, int32_t* free_mask, int fix_free, int max_iter, double mu0, double ftol, double xtol,
                                 double* info, double* work, mvmcStream_t stream) {
    if (!skel_host || n_ids < 0 || n_views <= 0 || p_max <= 0 || max_iter < 0 || max_iter > MVMC_BODY_INFO_DOUBLES - 4) return MVMC_ERR_ARG;
    if (n_ids == 0) return MVMC_OK;
    if (!kps17 || !Pmats || !rig_of || !members || !params || !id_lo || !lens || !free_mask || !info || !work) return MVMC_ERR_ARG;
    SkelDev sk;
    if (!skel_to_dev(skel_host, &sk)) return MVMC_ERR_ARG;
    if (sk.n_side != MVMC_N_SIDE) return MVMC_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(body_lengths_kernel, dim3(n_ids), dim3(64), 0, (hipStream_t)stream, sk, kps17, Pmats, rig_of, members, params, id_lo,
                       n_views, p_max, lens, free_mask, fix_free, max_iter, mu0, ftol, xtol, info, work);
    MVMC_CHECK_LAUNCH();
    return MVMC_OK;
}

extern "C" int mvmc_ik_solve_stages_rigs(const mvmcSkeleton* skel_host, const double* kps17, const double* Pmats, int n_rigs,
                                         const int32_t* rig_of_problem, const int32_t* members, int n_problems, int v_max, int n_views,
                                         int p_max, const double* init_params, int stage_mask, int max_nfev, double* params_out,
                                         double* joints_out, double* info_out, double* scratch, mvmcStream_t stream) {
    if (stage_mask < 1 || stage_mask > 3 || max_nfev < 1 || n_rigs < 1 || v_max <= 0 || n_views <= 0 || p_max <= 0) return MVMC_ERR_ARG;
    if (n_problems <= 0) return n_problems == 0 ? MVMC_OK : MVMC_ERR_ARG;   // (before the pointers, as the two entries above: empty tables may be NULL)
    if (!skel_host || !kps17 || !Pmats || !rig_of_problem || !members || !init_params || !params_out || !joints_out || !scratch)
        return MVMC_ERR_ARG;
    SkelDev sk;
    if (!skel_to_dev(skel_host, &sk)) return MVMC_ERR_ARG;
    if (sk.n_side != MVMC_N_SIDE) return MVMC_ERR_UNSUPPORTED;
    const int vcap = v_max;
    if (vcap > 64 || n_views > 65535) return MVMC_ERR_UNSUPPORTED;
    const size_t lds = ((size_t)vcap * 6 + 15) / 16 * 16;
    hipLaunchKernelGGL(body_pose_kernel, dim3(n_problems), dim3(64), lds, (hipStream_t)stream, sk, kps17, Pmats, rig_of_problem, n_rigs,
                       members, n_problems, v_max, vcap, n_views, p_max, init_params, max_nfev, params_out, joints_out, info_out, scratch,
                       stage_mask);
    MVMC_CHECK_LAUNCH();
    return MVMC_OK;
}
