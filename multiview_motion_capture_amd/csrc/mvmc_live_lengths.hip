// One skeleton per live identity, estimated as frames arrive (multiview_motion_capture_amd/live_smoothing.py: lengths="auto";
// include/mvmc.h: mvmc_live_lengths_apply / _update; restated in tests/live_lengths_np.py, which is the definition).  No counterpart in
// the reference, whose IK fits the lengths again on every frame (inverse_kinematics.py:380-433).
//   apply   before the tick's window launch, one lane per (item, length): a new identity's state from its first row; the running
//           skeleton l into the data row of every other identity;
//   update  after the window launch, ONE 64-lane workgroup per item: the rows that moved behind the lag since the last tick (one in
//           the common case) each add the normal equations of mvmc_body_lengths' residual in the 11 lengths, linearised at the row's
//           own lengths, to the identity's A and b; then (A + prior I) l = b + prior l0 and l goes into the rows the next tick solves
//           again.  body_lengths_kernel's lane-per-problem mapping would idle 63 lanes on one row, so here the lanes share the row's
//           (member, observation row) pairs: the row's global rotations, bone vectors and joints are made once and passed through LDS,
//           every lane accumulates its pairs in registers over all the tick's rows, and ONE butterfly (bf_wave_sum's) adds the lanes.
//           The 11 x 11 solve runs over LDS with the lanes on the entries of the matrix.
// Every sum runs in a fixed order inside one identity's own lanes, no atomics: an identity's bits depend on nothing else in the launch.
#include "mvmc_common.h"
#include "mvmc_ik_shared.h"

namespace {

constexpr int LL_NS = MVMC_N_SIDE;
constexpr int LL_NH = LL_NS * (LL_NS + 1) / 2;
constexpr int LL_STATE = MVMC_LIVE_LEN_STATE_DOUBLES, LL_INFO = MVMC_LIVE_LEN_INFO_DOUBLES;
constexpr int LL_ITEM = MVMC_SMOOTH_WIN_ITEM_INTS, LL_RING = MVMC_SMOOTH_WIN_RING;
// the state's layout (include/mvmc.h)
constexpr int LL_A = 0, LL_B = LL_NH, LL_L = LL_B + LL_NS, LL_L0 = LL_L + LL_NS, LL_NEXT = LL_L0 + LL_NS, LL_CONTRIB = LL_NEXT + 1,
              LL_COMMITTED = LL_NEXT + 2, LL_CROW = LL_NEXT + 3;
static_assert(LL_CROW + 1 == LL_STATE, "lens_state: A, b, l, l0 and four counters");
static_assert(LL_INFO == 5 + LL_NS + 1, "linfo: status, rows, contributed, committed, committed_row, l, 1/2 sum r^2");
static_assert(MVMC_SMOOTH_MAX_VIEWS <= 64, "a row's members are counted by one ballot");

__device__ __forceinline__ double ll_nan() { return __longlong_as_double(0x7ff8000000000000LL); }
__device__ __forceinline__ int ll_hidx(int s, int t) { return s * LL_NS - s * (s - 1) / 2 + (t - s); }   // s <= t (bf_hidx)
__device__ __forceinline__ double ll_inf() { return __longlong_as_double(0x7ff0000000000000LL); }
__device__ __forceinline__ bool ll_pos_finite(double v) { return v > 0.0 && v < ll_inf(); }

__device__ __forceinline__ double ll_wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return __shfl(v, 0, 64);   // (lanes round differently: lane 0's sum for everyone)
}

__global__ void live_lengths_apply_kernel(const int32_t* __restrict__ items, int n_items, double* __restrict__ new_params, int n_new,
                                          double* __restrict__ state, int n_slots) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n_items * LL_NS) return;
    const int it = idx / LL_NS, s = idx - it * LL_NS;
    const int32_t* im = items + (size_t)it * LL_ITEM;
    const int slot = im[0], is_data = im[3], reset = im[4], src = im[5];
    if (slot < 0 || slot >= n_slots || !is_data || src < 0 || src >= n_new) return;
    double* S = state + (size_t)slot * LL_STATE;
    double* x = new_params + (size_t)src * 68 + 57;
    if (!reset) {
        x[s] = S[LL_L + s];
        return;
    }
    for (int i = s; i < LL_NH; i += LL_NS) S[LL_A + i] = 0.0;
    S[LL_B + s] = 0.0;
    S[LL_L + s] = x[s];
    S[LL_L0 + s] = x[s];
    if (s == 0) { S[LL_NEXT] = 0.0; S[LL_CONTRIB] = 0.0; S[LL_COMMITTED] = 0.0; S[LL_CROW] = -1.0; }
}

struct LlLds {
    double dirs[18 * 3];
    int parents[18], side[18];
    double R[18 * 9], Rg[18 * 9], bv[18 * 3], X[18 * 3];   // the row: local and global rotations, bone vectors R_parent dir, joints
    double lr[LL_NS];                                      // the row's own lengths
    double A[LL_NH], b[LL_NS], l[LL_NS], l0[LL_NS];
    double M[LL_NS * LL_NS], y[LL_NS];                     // the solve
};

__global__ void __launch_bounds__(64) live_lengths_update_kernel(SkelDev sk, const double* __restrict__ kps17, const double* __restrict__ Pmats,
                                                                 int C, int Pmax, int n_rigs, const int32_t* __restrict__ items,
                                                                 double* __restrict__ rows, const int32_t* __restrict__ members,
                                                                 const int32_t* __restrict__ count, int n_slots, int lag, double prior,
                                                                 int commit, double* __restrict__ state, double* __restrict__ linfo) {
    __shared__ LlLds L;
    const int lane = threadIdx.x & 63, it = blockIdx.x;
    const int32_t* im = items + (size_t)it * LL_ITEM;
    const int slot = uni((int)im[0]), rig = uni((int)im[1]), d = uni((int)im[2]);
    double* inf = linfo + (size_t)it * LL_INFO;
    // (a malformed item is never followed out of bounds: status 6, NaN, nothing else written)
    bool bad = slot < 0 || slot >= n_slots || rig < 0 || rig >= n_rigs || d < 1;
    int n = 0, next = 0;
    double* S = state;
    if (!bad) {
        S = state + (size_t)slot * LL_STATE;
        n = uni((int)count[slot * 2]);
        const double nx = uni(S[LL_NEXT]);
        bad = n < 1 || !(nx >= 0.0 && nx <= (double)n);
        if (!bad) {
            next = (int)nx;
            bad = n - next > LL_RING;
        }
    }
    if (bad) {
        if (lane < LL_INFO) inf[lane] = lane == 0 ? 6.0 : ll_nan();
        return;
    }
    if (lane < 18) {
        L.parents[lane] = sk.parents[lane];
        L.side[lane] = sk.side_map[lane];
        for (int a = 0; a < 3; ++a) L.dirs[3 * lane + a] = sk.dirs[lane][a];
    }
    for (int i = lane; i < LL_NH; i += 64) L.A[i] = S[LL_A + i];
    if (lane < LL_NS) { L.b[lane] = S[LL_B + lane]; L.l[lane] = S[LL_L + lane]; L.l0[lane] = S[LL_L0 + lane]; }
    int contributed = (int)uni(S[LL_CONTRIB]), committed = uni(S[LL_COMMITTED]) != 0.0 ? 1 : 0;
    double crow = uni(S[LL_CROW]);
    MVMC_WAVE_SYNC();

    // ---- the rows that moved behind the lag: this lane's pairs of all of them, in row order ----
    double H[LL_NH], g[LL_NS], E = 0.0;
#pragma unroll
    for (int i = 0; i < LL_NH; ++i) H[i] = 0.0;
#pragma unroll
    for (int i = 0; i < LL_NS; ++i) g[i] = 0.0;
    int n_rows = 0;
    const int lo = d > 1 && n - d > next ? n - d : next;
    const double* Pbase = Pmats + (size_t)rig * C * 12;
    for (int r = lo; r < n - lag && !committed; ++r) {
        const size_t at = (size_t)slot * LL_RING + r % LL_RING;
        const int32_t* mrow = members + at * C;
        const int mine = lane < C ? mrow[lane] : -1;
        if (__popcll(__ballot(mine >= 0)) < 2) continue;   // a missing row, or a data row with fewer than two views
        const double* x = rows + at * 68;
        MVMC_WAVE_SYNC();   // (the previous row's pairs have read the LDS)
        if (lane < 18) euler_to_rot(x + 3 + 3 * lane, L.R + 9 * lane);
        if (lane < LL_NS) L.lr[lane] = x[57 + lane];
        MVMC_WAVE_SYNC();
        if (lane < 9) L.Rg[lane] = L.R[lane];
        if (lane >= 16 && lane < 19) { L.bv[lane - 16] = 0.0; L.X[lane - 16] = x[lane - 16]; }
        MVMC_WAVE_SYNC();
        for (int j = 1; j < 18; ++j) {   // (parents come first: skel_to_dev)
            const int p = L.parents[j];
            const double* Rp = L.Rg + 9 * p;
            if (lane < 9) {
                const int a = lane / 3, c = lane - 3 * a;
                L.Rg[9 * j + lane] = Rp[3 * a] * L.R[9 * j + c] + Rp[3 * a + 1] * L.R[9 * j + 3 + c] + Rp[3 * a + 2] * L.R[9 * j + 6 + c];
            } else if (lane >= 16 && lane < 19) {
                const int a = lane - 16;
                const double v = Rp[3 * a] * L.dirs[3 * j] + Rp[3 * a + 1] * L.dirs[3 * j + 1] + Rp[3 * a + 2] * L.dirs[3 * j + 2];
                L.bv[3 * j + a] = v;
                L.X[3 * j + a] = L.X[3 * p + a] + v * L.lr[L.side[j]];
            }
            MVMC_WAVE_SYNC();
        }
        for (int q = lane; q < C * NOBS; q += 64) {
            const int m = mrow[q / NOBS], ro = q % NOBS;
            if (m < 0) continue;
            const double* P = Pbase + ((m / Pmax) % C) * 12;
            const double* kp = kps17 + (size_t)m * 51;
            const int k = kIkSkel[ro], ob = kIkObs[ro];
            double ox, oy, ow;
            if (ob == 17) {
                ox = 0.5 * (0.5 * (kp[15] + kp[18]) + 0.5 * (kp[33] + kp[36]));
                oy = 0.5 * (0.5 * (kp[16] + kp[19]) + 0.5 * (kp[34] + kp[37]));
                ow = kp[17] * kp[20];
                ow *= kp[35] * kp[38];
            } else {
                ox = kp[3 * ob]; oy = kp[3 * ob + 1]; ow = kp[3 * ob + 2];
            }
            const double X0 = L.X[3 * k], X1 = L.X[3 * k + 1], X2 = L.X[3 * k + 2];
            const double h0 = P[0] * X0 + P[1] * X1 + P[2] * X2 + P[3];
            const double h1 = P[4] * X0 + P[5] * X1 + P[6] * X2 + P[7];
            const double wd = P[8] * X0 + P[9] * X1 + P[10] * X2 + P[11] + 1e-5;
            const double u = h0 / wd, v = h1 / wd;
            const double ru = (u - ox) * ow, rv = (v - oy) * ow;
            E += ru * ru + rv * rv;
            double du[3], dv[3];
            for (int a = 0; a < 3; ++a) { du[a] = (P[a] - u * P[8 + a]) / wd; dv[a] = (P[4 + a] - v * P[8 + a]) / wd; }
            double ju[LL_NS], jv[LL_NS];
#pragma unroll
            for (int s = 0; s < LL_NS; ++s) { ju[s] = 0.0; jv[s] = 0.0; }
            for (int j = k; j != 0; j = L.parents[j]) {
                const double cu = du[0] * L.bv[3 * j] + du[1] * L.bv[3 * j + 1] + du[2] * L.bv[3 * j + 2];
                const double cv = dv[0] * L.bv[3 * j] + dv[1] * L.bv[3 * j + 1] + dv[2] * L.bv[3 * j + 2];
                const int sj = L.side[j];
#pragma unroll
                for (int s = 0; s < LL_NS; ++s)
                    if (s == sj) { ju[s] += cu; jv[s] += cv; }
            }
            double tu = -ru, tv = -rv;   // J l_r - r of the two residuals
#pragma unroll
            for (int s = 0; s < LL_NS; ++s) {
                ju[s] *= ow; jv[s] *= ow;
                tu += ju[s] * L.lr[s]; tv += jv[s] * L.lr[s];
            }
#pragma unroll
            for (int s = 0; s < LL_NS; ++s) g[s] += ju[s] * tu + jv[s] * tv;
#pragma unroll
            for (int s = 0; s < LL_NS; ++s)
#pragma unroll
                for (int t = s; t < LL_NS; ++t) H[ll_hidx(s, t)] += ju[s] * ju[t] + jv[s] * jv[t];
        }
        ++n_rows;
    }
    if (n - lag > next) next = n - lag;

    // ---- the solve: (A + prior I) l = b + prior l0, right-looking Cholesky over LDS ----
    int status = 0;
    if (n_rows > 0) {
#pragma unroll
        for (int i = 0; i < LL_NH; ++i) H[i] = ll_wave_sum(H[i]);
#pragma unroll
        for (int i = 0; i < LL_NS; ++i) g[i] = ll_wave_sum(g[i]);
        E = 0.5 * ll_wave_sum(E);
        MVMC_WAVE_SYNC();
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < LL_NH; ++i) L.A[i] += H[i];
#pragma unroll
            for (int i = 0; i < LL_NS; ++i) L.b[i] += g[i];
        }
        MVMC_WAVE_SYNC();
        for (int i = lane; i < LL_NS * LL_NS; i += 64) {
            const int s = i / LL_NS, t = i - s * LL_NS;
            L.M[i] = L.A[s <= t ? ll_hidx(s, t) : ll_hidx(t, s)] + (s == t ? prior : 0.0);
        }
        if (lane < LL_NS) L.y[lane] = L.b[lane] + prior * L.l0[lane];
        MVMC_WAVE_SYNC();
        bool ok = true;
        for (int j = 0; j < LL_NS && ok; ++j) {   // column j of the factor, the forward substitution riding along
            const double a = L.M[j * LL_NS + j];
            ok = ll_pos_finite(a);
            if (!ok) break;
            const double sq = sqrt(a);
            MVMC_WAVE_SYNC();
            if (lane > j && lane < LL_NS) L.M[lane * LL_NS + j] /= sq;
            if (lane == j) { L.M[j * LL_NS + j] = sq; L.y[j] /= sq; }
            MVMC_WAVE_SYNC();
            for (int i = lane; i < LL_NS * LL_NS; i += 64) {
                const int s = i / LL_NS, t = i - s * LL_NS;
                if (s > j && t > j && t <= s) L.M[i] -= L.M[s * LL_NS + j] * L.M[t * LL_NS + j];
            }
            if (lane > j && lane < LL_NS) L.y[lane] -= L.M[lane * LL_NS + j] * L.y[j];
            MVMC_WAVE_SYNC();
        }
        if (ok) {
            for (int j = LL_NS - 1; j >= 0; --j) {   // back substitution with the factor's transpose
                if (lane == j) L.y[j] /= L.M[j * LL_NS + j];
                MVMC_WAVE_SYNC();
                if (lane < j) L.y[lane] -= L.M[j * LL_NS + lane] * L.y[j];
                MVMC_WAVE_SYNC();
            }
            // every length finite, and > 0 where the slot has curvature (slot 7 has none: the prior holds it at l0, which may be 0)
            const int s = lane < LL_NS ? lane : 0;
            const double v = L.y[s];
            ok = __popcll(__ballot(lane < LL_NS && fabs(v) < ll_inf() && (v > 0.0 || !(L.A[ll_hidx(s, s)] > 0.0)))) == LL_NS;
        }
        if (ok) {
            if (lane < LL_NS) L.l[lane] = L.y[lane];
        } else {
            status = 1;
        }
        contributed += n_rows;
        if (commit > 0 && contributed >= commit) { committed = 1; crow = (double)(n - lag); }
        MVMC_WAVE_SYNC();
    } else {
        E = 0.0;
    }

    // ---- the state, the rows the next tick solves again, the report ----
    for (int i = lane; i < LL_NH; i += 64) S[LL_A + i] = L.A[i];
    if (lane < LL_NS) { S[LL_B + lane] = L.b[lane]; S[LL_L + lane] = L.l[lane]; }
    if (lane == 0) { S[LL_NEXT] = (double)next; S[LL_CONTRIB] = (double)contributed; S[LL_COMMITTED] = (double)committed; S[LL_CROW] = crow; }
    const int first = n - lag > 0 ? n - lag : 0;
    for (int i = lane; i < (n - first) * LL_NS; i += 64) {
        const int r = first + i / LL_NS, s = i % LL_NS;
        rows[((size_t)slot * LL_RING + r % LL_RING) * 68 + 57 + s] = L.l[s];
    }
    if (lane == 0) { inf[0] = (double)status; inf[1] = (double)n_rows; inf[2] = (double)contributed; inf[3] = (double)committed; inf[4] = crow; }
    if (lane < LL_NS) inf[5 + lane] = L.l[lane];
    if (lane == 0) inf[5 + LL_NS] = E;
}

}  // namespace

extern "C" int mvmc_live_lengths_apply(const int32_t* items, int n_items, double* new_params, int n_new, double* lens_state, int n_slots,
                                       mvmcStream_t stream) {
    if (n_items < 0 || n_new < 0 || n_slots < 0) return MVMC_ERR_ARG;
    if (n_items == 0) return MVMC_OK;
    if (!items || !lens_state || (n_new > 0 && !new_params)) return MVMC_ERR_ARG;
    if ((long long)n_items * LL_NS > 0x7fffffffLL) return MVMC_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(live_lengths_apply_kernel, dim3((n_items * LL_NS + 255) / 256), dim3(256), 0, (hipStream_t)stream, items, n_items,
                       new_params, n_new, lens_state, n_slots);
    MVMC_CHECK_LAUNCH();
    return MVMC_OK;
}

extern "C" int mvmc_live_lengths_update(const mvmcSkeleton* skel_host, const double* kps17, int n_views, int p_max, const double* Pmats,
                                        int n_rigs, const int32_t* items, int n_items, double* rows, const int32_t* members,
                                        const int32_t* count, int n_slots, int lag, double prior, int commit, double* lens_state,
                                        double* linfo, mvmcStream_t stream) {
    if (!skel_host || n_items < 0 || n_slots < 0 || n_rigs < 1 || n_views <= 0 || n_views > MVMC_SMOOTH_MAX_VIEWS || p_max <= 0)
        return MVMC_ERR_ARG;
    if (lag < 0 || lag >= MVMC_SMOOTH_WIN_MAX || commit < 0 || !(prior > 0.0 && prior <= 1.7976931348623157e308)) return MVMC_ERR_ARG;
    if (n_items == 0) return MVMC_OK;
    if (!kps17 || !Pmats || !items || !rows || !members || !count || !lens_state || !linfo) return MVMC_ERR_ARG;
    SkelDev sk;
    if (!skel_to_dev(skel_host, &sk)) return MVMC_ERR_ARG;
    if (sk.n_side != MVMC_N_SIDE) return MVMC_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(live_lengths_update_kernel, dim3(n_items), dim3(64), 0, (hipStream_t)stream, sk, kps17, Pmats, n_views, p_max, n_rigs,
                       items, rows, members, count, n_slots, lag, prior, commit, lens_state, linfo);
    MVMC_CHECK_LAUNCH();
    return MVMC_OK;
}
