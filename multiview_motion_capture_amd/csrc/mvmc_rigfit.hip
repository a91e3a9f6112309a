// Rig refinement (multiview_motion_capture_amd/rig_refine.py; algorithm restated in tests/rig_refine_np.py): a bundle adjustment of
// every sequence's cameras over the keypoints of its tracked people.  No counterpart in the reference.
//   start     per candidate point: the DLT of the views that see it (dlt_point, the arithmetic of mvmc_dlt) with the point's own rig,
//             and its reprojection distance in every such view;
//   accum     per TILE of MVMC_RIG_TILE points (one wave, one point per lane): the damped point blocks V* = L L^T, per free camera
//             Y = W L^-T, and the tile's part of the Schur complement as ONE symmetric product over the stacked rows [Y; z^T]
//             (z = L^-1 g_p) staged in LDS -- on the matrix cores (v_mfma_f64_16x16x4_f64) or, variant 0, as FMAs over the same LDS
//             rows; the camera blocks J_c J_c^T (with the residual as last row: U_c, g_c) the same way from the camera-row table;
//   solve     one workgroup per sequence: the tile parts summed IN TILE ORDER, S = U* - sum Y Y^T by Cholesky, the trial cameras;
//   backsub   per tile: the points' steps, the trial points and the trial cost;
//   decide    one workgroup per sequence: accept / reject, the gauge rescale, mu, the stop rules.
// The tiles of a sequence are cut from its own points, every sum has a fixed order and there are no atomics: a sequence's numbers
// depend on nothing else in the launch.  A sequence that has stopped (ctl[0] != 0) idles.
// Robust loss (the _robust entries; restated in tests/rig_robust_np.py): rg_obs, rg_point and the two tile kernels take the loss as a
// compile-time parameter.  With a loss an observation's rows a, b, ju, jv and its residual are multiplied by sqrt(w) as the lane forms
// them and the tile's E is the sum of rho; everything staged in LDS, part, red, the solve and the decision are what they are without
// one.  LOSS = MVMC_RIG_LOSS_NONE is the arithmetic without a loss, operation for operation.
// Intrinsic unknowns (the _intr entries; restated in tests/rig_intr_np.py): the four trial kernels take NI, the number of intrinsic
// unknowns per camera, as a compile-time parameter beside LOSS; the entries without intrinsics are NI = 0.  Per camera with
// islot >= 0, NI = 1 (phi: K00, K01, K11 <- e^phi x themselves) or 3 (and the additive dcx, dcy on K02, K12) more unknowns.  Their
// rows of an observation are closed-form from rg_obs: d(u, v)/dphi = (u - cx, v - cy), d/dcx = (1, 0), d/dcy = (0, 1), times
// sqrt(w) with a loss.  Camera 0's pose stays held; its intrinsics may be free (slot -1, islot >= 0).
// LAYOUT of the reduced system, for every NI: one contiguous block per camera in camera order, its 6 pose columns if slot >= 0, then
// its NI intrinsic columns if islot >= 0 (rg_col; with NI = 0 and slot ascending with the camera that is column 6 slot + r);
// M = 6 (C - 1) + NI C columns at the most, identity past a sequence's own; red = S (M x M), g (M), d (M).  Only the sign of slot
// and islot is read.  A table with more free columns than M breaks include/mvmc.h's contract: its sequence idles in every kernel.
// part (PD per tile): the lower block triangle of [Y; z^T] [Y; z^T]^T (z^T is row M), then per camera with a free unknown, in camera
// order, the NR (NR + 1) / 2 products of its NR = 7 + NI rows (6 pose rows, NI intrinsic rows, the residual; rows of unknowns that
// are not free are zero), upper triangle; then E of the tile.  There is room for C - 1 such cameras with NI = 0 and for C otherwise.
// LDS of accum: with NI = 0 both tables are resident and the observations are evaluated once.  With NI > 0 they are not resident
// together (C = 8, NI = 3 would need about 201 KB): the tile stages [Y; z^T], multiplies, and then stages the camera rows into the
// SAME LDS from a second evaluation of the observations: max(Mp x 1,552 B, C NR x 1,040 B), 124,160 B at C = 8, NI = 3.
// Prior (NI > 0 alone; NI = 0 compiles every term of it out): E_prior = 1/2 sum (phi / sigma_f)^2 + 1/2 sum (dcx^2 + dcy^2) /
// sigma_c^2 about the input K (K0: fx, cx, cy per camera), phi = log(K00 / fx0) -- accumulated over the call.  It is part of every
// E read or written and of the diagonal and gradient of the intrinsic columns (added per sequence in the solve kernel, in camera
// order); sigma = +inf is no term.  On acceptance the trial K is taken over with the trial pose.
#include "mvmc_common.h"
#include "mvmc_dlt_point.h"

#include <type_traits>

namespace {

constexpr int RG_TILE = MVMC_RIG_TILE;
constexpr int RG_LD = 3 * RG_TILE + 2;    // row stride of the Y table (doubles): 388 dwords = 4 mod 64 banks
constexpr int RG_LDJ = 2 * RG_TILE + 2;   // row stride of the camera-row table
constexpr int RG_CAM = MVMC_RIG_CAM_DOUBLES;
constexpr int RG_INFO = MVMC_RIG_INFO_DOUBLES;
constexpr int RG_TRIALS = 8, RG_COSTS = 8 + MVMC_RIG_MAX_ITER;
typedef double rg_d4 __attribute__((ext_vector_type(4)));

// nq: the cameras that part has row products for
struct RgDims { int nq, M, Mp, nb, nblk, PD, RD; };
template <int NI>
__host__ __device__ inline RgDims rg_dims(int C) {
    constexpr int NR = 7 + NI;
    RgDims d;
    d.nq = NI ? C : C - 1;
    d.M = 6 * (C - 1) + NI * C;
    d.Mp = (d.M + 1 + 15) / 16 * 16;      // rows of [Y; z^T], padded to the matrix core's 16
    d.nb = d.Mp / 16;
    d.nblk = d.nb * (d.nb + 1) / 2;       // lower block triangle
    d.PD = (d.nblk * 256 + NR * (NR + 1) / 2 * d.nq + 1 + 1) / 2 * 2;
    d.RD = d.M * d.M + 2 * d.M;
    return d;
}
// columns of the sequence in front of camera c's block (c = C: all of them).  isl is not read with NI = 0.
template <int NI>
__device__ __forceinline__ int rg_col(const int32_t* __restrict__ sl, const int32_t* __restrict__ isl, int c) {
    int off = 0;
    for (int k = 0; k < c; ++k) {
        off += sl[k] >= 0 ? 6 : 0;
        if constexpr (NI > 0) off += isl[k] >= 0 ? NI : 0;
    }
    return off;
}

__device__ __forceinline__ double rg_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

// one observation: residual, the point rows a, b of the Jacobian (R^T du, R^T dv), and y = R X, du, dv for the camera rows
// with a loss: rho of the plain residual, and ru, rv, a, b, du, dv (so ju, jv) times sqrt(w)
// NI > 0: the intrinsic rows iu, iv (NI of each)
struct RgObs { double ru, rv, a[3], b[3], y[3], du[3], dv[3], rho, iu[3], iv[3]; };
template <int LOSS, int NI = 0>
__device__ __forceinline__ void rg_obs(const double* __restrict__ cam, const double* X, double ou, double ov, double delta, RgObs& o) {
    const double* K = cam;
    const double* R = cam + 9;
    const double* t = cam + 18;
    double xc[3], p[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) { o.y[r] = R[3 * r] * X[0] + R[3 * r + 1] * X[1] + R[3 * r + 2] * X[2]; xc[r] = o.y[r] + t[r]; }
#pragma unroll
    for (int r = 0; r < 3; ++r) p[r] = K[3 * r] * xc[0] + K[3 * r + 1] * xc[1] + K[3 * r + 2] * xc[2];
    const double u = p[0] / p[2], v = p[1] / p[2];
    o.ru = u - ou; o.rv = v - ov;
#pragma unroll
    for (int k = 0; k < 3; ++k) { o.du[k] = (K[k] - u * K[6 + k]) / p[2]; o.dv[k] = (K[3 + k] - v * K[6 + k]) / p[2]; }
    double sw = 1.0;
    if constexpr (LOSS != MVMC_RIG_LOSS_NONE) {
        const double s2 = o.ru * o.ru + o.rv * o.rv;
        if constexpr (LOSS == MVMC_RIG_LOSS_HUBER) {
            const double s = sqrt(s2);
            if (s <= delta) { o.rho = 0.5 * s2; sw = 1.0; }
            else { o.rho = delta * (s - 0.5 * delta); sw = sqrt(delta / s); }
        } else {
            const double q = s2 / (delta * delta);
            o.rho = 0.5 * delta * delta * log1p(q);
            sw = sqrt(1.0 / (1.0 + q));
        }
        o.ru *= sw; o.rv *= sw;
#pragma unroll
        for (int k = 0; k < 3; ++k) { o.du[k] *= sw; o.dv[k] *= sw; }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        o.a[k] = R[k] * o.du[0] + R[3 + k] * o.du[1] + R[6 + k] * o.du[2];
        o.b[k] = R[k] * o.dv[0] + R[3 + k] * o.dv[1] + R[6 + k] * o.dv[2];
    }
    if constexpr (NI > 0) { o.iu[0] = sw * (u - K[2]); o.iv[0] = sw * (v - K[5]); }
    if constexpr (NI == 3) { o.iu[1] = sw; o.iv[1] = 0.0; o.iu[2] = 0.0; o.iv[2] = sw; }
}
// camera rows: ju = (y x du, du), jv = (y x dv, dv)
__device__ __forceinline__ void rg_cam_rows(const RgObs& o, double* ju, double* jv) {
    ju[0] = o.y[1] * o.du[2] - o.y[2] * o.du[1]; ju[1] = o.y[2] * o.du[0] - o.y[0] * o.du[2]; ju[2] = o.y[0] * o.du[1] - o.y[1] * o.du[0];
    jv[0] = o.y[1] * o.dv[2] - o.y[2] * o.dv[1]; jv[1] = o.y[2] * o.dv[0] - o.y[0] * o.dv[2]; jv[2] = o.y[0] * o.dv[1] - o.y[1] * o.dv[0];
#pragma unroll
    for (int k = 0; k < 3; ++k) { ju[3 + k] = o.du[k]; jv[3 + k] = o.dv[k]; }
}

// the point's block at (X, cams): V (upper, 6), g_p, sum r^2 (with a loss: sum rho); then V* = V + mu diag V = L L^T.
// l = {l00, l10, l11, l20, l21, l22}
struct RgPoint { double V[6], g[3], rr, l[6]; };
template <int LOSS>
__device__ __forceinline__ void rg_point(const double* __restrict__ cams, const double* __restrict__ uvp, int C, const double* X, double mu,
                                         double delta, RgPoint& P) {
#pragma unroll
    for (int k = 0; k < 6; ++k) P.V[k] = 0.0;
    P.g[0] = P.g[1] = P.g[2] = 0.0;
    P.rr = 0.0;
    for (int c = 0; c < C; ++c) {
        const double ou = uvp[2 * c], ov = uvp[2 * c + 1];
        if (!(ou == ou)) continue;
        RgObs o;
        rg_obs<LOSS>(cams + c * RG_CAM, X, ou, ov, delta, o);
        P.V[0] += o.a[0] * o.a[0] + o.b[0] * o.b[0]; P.V[1] += o.a[0] * o.a[1] + o.b[0] * o.b[1]; P.V[2] += o.a[0] * o.a[2] + o.b[0] * o.b[2];
        P.V[3] += o.a[1] * o.a[1] + o.b[1] * o.b[1]; P.V[4] += o.a[1] * o.a[2] + o.b[1] * o.b[2]; P.V[5] += o.a[2] * o.a[2] + o.b[2] * o.b[2];
#pragma unroll
        for (int k = 0; k < 3; ++k) P.g[k] += o.a[k] * o.ru + o.b[k] * o.rv;
        if constexpr (LOSS == MVMC_RIG_LOSS_NONE) P.rr += o.ru * o.ru + o.rv * o.rv;
        else P.rr += o.rho;
    }
    const double v00 = P.V[0] + mu * P.V[0], v11 = P.V[3] + mu * P.V[3], v22 = P.V[5] + mu * P.V[5];
    P.l[0] = sqrt(v00);
    P.l[1] = P.V[1] / P.l[0];
    P.l[2] = sqrt(v11 - P.l[1] * P.l[1]);
    P.l[3] = P.V[2] / P.l[0];
    P.l[4] = (P.V[4] - P.l[3] * P.l[1]) / P.l[2];
    P.l[5] = sqrt(v22 - P.l[3] * P.l[3] - P.l[4] * P.l[4]);
}
// y L^T = w (a row of W L^-T), and L y = w
__device__ __forceinline__ void rg_fwd(const double* l, const double* w, double* y) {
    y[0] = w[0] / l[0];
    y[1] = (w[1] - l[1] * y[0]) / l[2];
    y[2] = (w[2] - l[3] * y[0] - l[4] * y[1]) / l[5];
}
__device__ __forceinline__ void rg_bwd(const double* l, const double* y, double* x) {   // L^T x = y
    x[2] = y[2] / l[5];
    x[1] = (y[1] - l[4] * x[2]) / l[2];
    x[0] = (y[0] - l[1] * x[1] - l[3] * x[2]) / l[0];
}

// ---- start values ----
__global__ void __launch_bounds__(256) rig_start_kernel(const double* __restrict__ obs, const int32_t* __restrict__ rig_of,
                                                        const double* __restrict__ Pmats, int N, int C, int n_rigs, double min_score,
                                                        double* __restrict__ X0, double* __restrict__ dist) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int r = rig_of[i];
    double o[4] = {rg_nan(), rg_nan(), rg_nan(), rg_nan()};
    const double* ob = obs + (size_t)i * C * 3;
    const double* Pr = Pmats + (size_t)(r < 0 || r >= n_rigs ? 0 : r) * C * 12;
    if (r >= 0 && r < n_rigs)
        dlt_point(C, min_score, [&](int v, double (&kp)[3], const double*& Pc) {
            if (!(ob[3 * v + 2] > min_score)) return false;
            kp[0] = ob[3 * v]; kp[1] = ob[3 * v + 1]; kp[2] = ob[3 * v + 2];
            Pc = Pr + v * 12;
            return true;
        }, o);
    for (int k = 0; k < 4; ++k) X0[(size_t)i * 4 + k] = o[k];
    for (int v = 0; v < C; ++v) {
        double d = rg_nan();
        if (ob[3 * v + 2] > min_score) {
            const double* P = Pr + v * 12;
            const double h0 = P[0] * o[0] + P[1] * o[1] + P[2] * o[2] + P[3];
            const double h1 = P[4] * o[0] + P[5] * o[1] + P[6] * o[2] + P[7];
            const double h2 = P[8] * o[0] + P[9] * o[1] + P[10] * o[2] + P[11];
            const double eu = h0 / h2 - ob[3 * v], ev = h1 / h2 - ob[3 * v + 1];
            d = sqrt(eu * eu + ev * ev);
        }
        dist[(size_t)i * C + v] = d;
    }
}

// ---- the tile's part of the reduced system ----
// part (PD per tile): the lower block triangle of [Y; z^T] [Y; z^T]^T in 16 x 16 blocks (block (bi, bj), bj <= bi, at bi (bi + 1) / 2
// + bj, row-major), then per camera with a free unknown the NR (NR + 1) / 2 products of the rows (J_c; r) (upper triangle), then
// E = 1/2 sum r^2 of the tile (with a loss: sum rho).
template <bool MFMA, int LOSS, int NI>
__global__ void __launch_bounds__(64) rig_accum_kernel(const double* __restrict__ X, const double* __restrict__ uv,
                                                       const int32_t* __restrict__ tile, const int32_t* __restrict__ slot,
                                                       const int32_t* __restrict__ islot, const double* __restrict__ cams,
                                                       const int32_t* __restrict__ ctl, const double* __restrict__ info, int N, int S,
                                                       int C, double mu0, double delta, double* __restrict__ part) {
    static_assert(MFMA || NI == 0, "the FMA variant of the stacked product exists without intrinsic unknowns alone");
    extern __shared__ __attribute__((aligned(16))) double rg_lds[];
    constexpr int NR = 7 + NI, QN = NR * (NR + 1) / 2;
    const RgDims D = rg_dims<NI>(C);
    double* sY = rg_lds;
    double* sJ = NI == 0 ? rg_lds + D.Mp * RG_LD : rg_lds;   // NI > 0: in the same LDS, after [Y; z^T] has been multiplied
    const int lane = threadIdx.x & 63, tl = blockIdx.x;
    const int s = uni((int)tile[4 * tl]), lo = uni((int)tile[4 * tl + 1]), n = uni((int)tile[4 * tl + 2]);
    if (s < 0 || s >= S || lo < 0 || n < 0 || n > RG_TILE || lo + n > N) return;
    if (ctl[4 * s] != 0) return;
    const double mu = ctl[4 * s + 1] == 0 ? mu0 : info[(size_t)s * RG_INFO + 2];
    const double* cm = cams + (size_t)s * C * RG_CAM;
    const int32_t* sl = slot + (size_t)s * C;
    const int32_t* isl = NI > 0 ? islot + (size_t)s * C : nullptr;
    if (rg_col<NI>(sl, isl, C) > D.M) return;
    const int i = lo + lane;                 // read by the lanes < n alone
    double Xp[3] = {0.0, 0.0, 0.0};
    const double* uvp = uv + (size_t)i * C * 2;
    RgPoint P;
    // a lane's observations: their rows of [Y; z^T] (WY), their camera rows (WJ), or both
    auto stage = [&](auto wy, auto wj) {
        constexpr bool WY = decltype(wy)::value, WJ = decltype(wj)::value;
        int off = 0, q = 0;
        for (int c = 0; c < C; ++c) {
            bool pf = sl[c] >= 0, jf = false;
            if constexpr (NI > 0) jf = isl[c] >= 0;
            int row = off;
            double* jr = sJ + NR * q * RG_LDJ + 2 * lane;
            off += (pf ? 6 : 0) + (jf ? NI : 0);
            q += pf || jf;
            const double ou = uvp[2 * c], ov = uvp[2 * c + 1];
            if (!(pf || jf) || !(ou == ou)) continue;
            RgObs o;
            rg_obs<LOSS, NI>(cm + c * RG_CAM, Xp, ou, ov, delta, o);
            auto put = [&](int ry, int rj, double xu, double xv) {
                if constexpr (WY) {
                    const double w[3] = {xu * o.a[0] + xv * o.b[0], xu * o.a[1] + xv * o.b[1], xu * o.a[2] + xv * o.b[2]};
                    double y[3];
                    rg_fwd(P.l, w, y);
                    for (int k = 0; k < 3; ++k) sY[ry * RG_LD + 3 * lane + k] = y[k];
                }
                if constexpr (WJ) { jr[rj * RG_LDJ] = xu; jr[rj * RG_LDJ + 1] = xv; }
            };
            if (pf) {
                double ju[6], jv[6];
                rg_cam_rows(o, ju, jv);
#pragma unroll
                for (int r = 0; r < 6; ++r) put(row + r, r, ju[r], jv[r]);
                row += 6;
            }
            if constexpr (NI > 0)
                if (jf) {
#pragma unroll
                    for (int r = 0; r < NI; ++r) put(row + r, 6 + r, o.iu[r], o.iv[r]);
                }
            if constexpr (WJ) { jr[(NR - 1) * RG_LDJ] = o.ru; jr[(NR - 1) * RG_LDJ + 1] = o.rv; }
        }
    };
    auto clear_rows = [&]() {
        for (int r = 0; r < NR * D.nq; ++r) { sJ[r * RG_LDJ + 2 * lane] = 0.0; sJ[r * RG_LDJ + 2 * lane + 1] = 0.0; }
    };
    for (int r = 0; r < D.Mp; ++r)
        for (int k = 0; k < 3; ++k) sY[r * RG_LD + 3 * lane + k] = 0.0;
    if constexpr (NI == 0) clear_rows();
    double rr = 0.0;
    if (lane < n) {
        for (int k = 0; k < 3; ++k) Xp[k] = X[(size_t)i * 3 + k];
        rg_point<LOSS>(cm, uvp, C, Xp, mu, delta, P);
        rr = P.rr;
        double z[3];
        rg_fwd(P.l, P.g, z);
        for (int k = 0; k < 3; ++k) sY[D.M * RG_LD + 3 * lane + k] = z[k];
        stage(std::true_type{}, std::bool_constant<NI == 0>{});
    }
    MVMC_WAVE_SYNC();
    double* out = part + (size_t)tl * D.PD;
    const int li = lane & 15, lq = lane >> 4;
    for (int bi = 0; bi < D.nb; ++bi)
        for (int bj = 0; bj <= bi; ++bj) {
            double* ob = out + (bi * (bi + 1) / 2 + bj) * 256;
            if constexpr (MFMA) {
                // lane l gives A[i = l % 16][k = l / 16] and B[k = l / 16][j = l % 16], receives D[i = l / 16 + 4 v][j = l % 16]
                const double* ra = sY + (16 * bi + li) * RG_LD + lq;
                const double* rb = sY + (16 * bj + li) * RG_LD + lq;
                rg_d4 acc = {0.0, 0.0, 0.0, 0.0};
                for (int k0 = 0; k0 < 3 * RG_TILE; k0 += 4) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ra[k0], rb[k0], acc, 0, 0, 0);
#pragma unroll
                for (int v = 0; v < 4; ++v) ob[(lq + 4 * v) * 16 + li] = acc[v];
            } else {
                const double* rb = sY + (16 * bj + li) * RG_LD;
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const double* ra = sY + (16 * bi + lq + 4 * v) * RG_LD;
                    double acc = 0.0;
                    for (int k = 0; k < 3 * RG_TILE; ++k) acc = fma(ra[k], rb[k], acc);
                    ob[(lq + 4 * v) * 16 + li] = acc;
                }
            }
        }
    if constexpr (NI > 0) {
        MVMC_WAVE_SYNC();
        clear_rows();
        if (lane < n) stage(std::false_type{}, std::true_type{});
        MVMC_WAVE_SYNC();
    }
    for (int e = lane; e < QN * D.nq; e += 64) {
        const int q = e / QN, w = e - QN * q;
        int a = 0, rem = w;
        while (rem >= NR - a) { rem -= NR - a; ++a; }
        const double* ra = sJ + (NR * q + a) * RG_LDJ;
        const double* rb = sJ + (NR * q + a + rem) * RG_LDJ;
        double acc = 0.0;
        for (int k = 0; k < 2 * RG_TILE; ++k) acc = fma(ra[k], rb[k], acc);
        out[D.nblk * 256 + e] = acc;
    }
    double E = wave_sum(rr);
    if constexpr (LOSS == MVMC_RIG_LOSS_NONE) E = 0.5 * E;
    if (lane == 0) out[D.nblk * 256 + QN * D.nq] = E;
}

__device__ void rg_rodrigues(const double* w, double* Q) {
    const double t2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], th = sqrt(t2);
    double a, b;
    if (th < 1e-8) { a = 1.0 - t2 / 6.0; b = 0.5 - t2 / 24.0; }
    else { a = sin(th) / th; b = (1.0 - cos(th)) / t2; }
    const double W[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double ww = 0.0;
            for (int k = 0; k < 3; ++k) ww += W[3 * i + k] * W[3 * k + j];
            Q[3 * i + j] = (i == j ? 1.0 : 0.0) + a * W[3 * i + j] + b * ww;
        }
}
__device__ void rg_centre(const double* cam, double* c) {
    const double* R = cam + 9;
    const double* t = cam + 18;
    for (int k = 0; k < 3; ++k) c[k] = -(R[k] * t[0] + R[3 + k] * t[1] + R[6 + k] * t[2]);
}

// E_prior at cams, in camera order
template <int NI>
__device__ double rg_prior(const double* __restrict__ cm, const double* __restrict__ k0, const int32_t* __restrict__ isl, int C, double sf,
                           double sc) {
    double e = 0.0;
    for (int c = 0; c < C; ++c) {
        if (isl[c] < 0) continue;
        const double* K = cm + c * RG_CAM;
        const double phi = log(K[0] / k0[3 * c]) / sf;
        e += 0.5 * (phi * phi);
        if constexpr (NI == 3) {
            const double dx = (K[2] - k0[3 * c + 1]) / sc, dy = (K[5] - k0[3 * c + 2]) / sc;
            e += 0.5 * (dx * dx + dy * dy);
        }
    }
    return e;
}
// the gauge camera: the first whose pose is free (-1: there is none)
__device__ int rg_gauge_cam(const int32_t* __restrict__ sl, int C) {
    for (int c = 0; c < C; ++c)
        if (sl[c] >= 0) return c;
    return -1;
}

// ---- the sequence's reduced system and its solution ----
// red (RD per sequence): S (M x M, row-major; identity on the columns the sequence does not use), g (M), d (M)
template <int NI>
__global__ void __launch_bounds__(256) rig_solve_kernel(const int32_t* __restrict__ seq, const int32_t* __restrict__ slot,
                                                        const int32_t* __restrict__ islot, const double* __restrict__ cams,
                                                        double* __restrict__ camt, int32_t* __restrict__ ctl,
                                                        double* __restrict__ info, const double* __restrict__ part,
                                                        double* __restrict__ red, const double* __restrict__ K0, int T, int C,
                                                        int max_iter, double mu0, double sf, double sc) {
    extern __shared__ __attribute__((aligned(16))) double rg_lds[];
    __shared__ int bad;
    // of a column: its camera (-1: not the sequence's), its row among the camera's NR, the camera's place in part
    constexpr int MMAX = 6 * (MVMC_RIG_MAX_CAMS - 1) + NI * MVMC_RIG_MAX_CAMS;
    __shared__ int ccam[MMAX], crow[MMAX], cq[MMAX];
    constexpr int NR = 7 + NI, QN = NR * (NR + 1) / 2;
    const RgDims D = rg_dims<NI>(C);
    const int M = D.M;
    double* sP = rg_lds;
    double* sS = sP + D.PD;
    double* sg = sS + M * M;
    double* sd = sg + M;
    double* sgc = sd + M;
    double* sdU = sgc + M;
    double* spw = sdU + M;       // NI > 0: the prior's diagonal term of the column
    double* ssx = spw + M;       // NI > 0: the column's scale in |d|_inf: 1, and 1 / fx for dcx, dcy
    const int s = blockIdx.x, tid = threadIdx.x;
    if (ctl[4 * s] != 0) return;
    const int it = ctl[4 * s + 1];
    const int t0 = seq[4 * s], nt = seq[4 * s + 1];
    if (t0 < 0 || nt < 0 || t0 + nt > T) return;
    const double* cm = cams + (size_t)s * C * RG_CAM;
    const int32_t* sl = slot + (size_t)s * C;
    const int32_t* isl = NI > 0 ? islot + (size_t)s * C : nullptr;
    const double* k0 = NI > 0 ? K0 + (size_t)s * C * 3 : nullptr;
    if (rg_col<NI>(sl, isl, C) > M) return;
    for (int e = tid; e < D.PD; e += 256) {
        double acc = 0.0;
        for (int t = 0; t < nt; ++t) acc += part[(size_t)(t0 + t) * D.PD + e];
        sP[e] = acc;
    }
    if (tid == 0) {
        bad = 0;
        int col = 0, q = 0;
        for (int c = 0; c < C; ++c) {
            bool pf = sl[c] >= 0, jf = false;
            if constexpr (NI > 0) jf = isl[c] >= 0;
            if (pf)
                for (int r = 0; r < 6; ++r) { ccam[col] = c; crow[col] = r; cq[col] = q; ++col; }
            if (jf)
                for (int r = 0; r < NI; ++r) { ccam[col] = c; crow[col] = 6 + r; cq[col] = q; ++col; }
            q += pf || jf;
        }
        for (; col < M; ++col) { ccam[col] = -1; crow[col] = 0; cq[col] = 0; }
    }
    __syncthreads();
    double* inf = info + (size_t)s * RG_INFO;
    const double mu = it == 0 ? mu0 : inf[2];
    const double* sC = sP + D.nblk * 256;
    if (it == 0 && tid == 0) {
        double E = sC[QN * D.nq];
        if constexpr (NI > 0) E = E + rg_prior<NI>(cm, k0, isl, C, sf, sc);
        const int ref = rg_gauge_cam(sl, C);
        inf[0] = E; inf[1] = E; inf[2] = mu0; inf[RG_COSTS] = E;
        double c0[3], cr[3] = {0.0, 0.0, 0.0};
        rg_centre(cm, c0);
        if (ref >= 0) rg_centre(cm + ref * RG_CAM, cr);
        inf[3] = sqrt((cr[0] - c0[0]) * (cr[0] - c0[0]) + (cr[1] - c0[1]) * (cr[1] - c0[1]) + (cr[2] - c0[2]) * (cr[2] - c0[2]));
    }
    if (it >= max_iter) {
        if (tid == 0) ctl[4 * s] = MVMC_RIG_STOP_MAX_ITER;
        return;
    }
    auto Tm = [&](int i, int j) {   // i >= j
        const int bi = i >> 4, bj = j >> 4;
        return sP[(bi * (bi + 1) / 2 + bj) * 256 + (i & 15) * 16 + (j & 15)];
    };
    auto qr = [&](int a, int b) { return a * NR - a * (a - 1) / 2 + (b - a); };   // a <= b < NR, of QN
    double* rd = red + (size_t)s * D.RD;
    for (int i = tid; i < M; i += 256) {
        const int c = ccam[i], a = crow[i];
        double gc = 0.0, dU = 0.0, g = 0.0;
        if (c >= 0) {
            gc = sC[QN * cq[i] + qr(a, NR - 1)];
            dU = sC[QN * cq[i] + qr(a, a)];
            if constexpr (NI > 0) {
                const double* K = cm + c * RG_CAM;
                double pw = 0.0, pg = 0.0, sx = 1.0;
                if (a == 6) { pw = 1.0 / (sf * sf); pg = log(K[0] / k0[3 * c]) / sf / sf; }
                else if (a > 6) { pw = 1.0 / (sc * sc); pg = (K[a == 7 ? 2 : 5] - k0[3 * c + a - 6]) / sc / sc; sx = 1.0 / K[0]; }
                gc = gc + pg;
                dU = dU + pw;
                spw[i] = pw; ssx[i] = sx;
            }
            g = gc - Tm(M, i);
        } else if constexpr (NI > 0) {
            spw[i] = 0.0; ssx[i] = 1.0;
        }
        sgc[i] = gc; sdU[i] = dU; sg[i] = g;
        rd[M * M + i] = g;
    }
    __syncthreads();
    for (int idx = tid; idx < M * M; idx += 256) {
        const int i = idx / M, j = idx - i * M;
        const int ci = ccam[i], cj = ccam[j];
        double v;
        if (ci < 0 || cj < 0) v = i == j ? 1.0 : 0.0;
        else {
            v = -Tm(i > j ? i : j, i > j ? j : i);
            if (ci == cj) {
                const int a = crow[i], b = crow[j];
                double u = sC[QN * cq[i] + qr(a < b ? a : b, a < b ? b : a)];
                if constexpr (NI > 0)
                    if (i == j) u += spw[i];
                v += u;
                if (i == j) v += mu * u;
            }
        }
        sS[idx] = v;
        rd[idx] = v;
    }
    __syncthreads();
    // right-looking Cholesky of S, lower triangle in place
    for (int j = 0; j < M; ++j) {
        if (tid == 0) {
            const double d = sS[j * M + j];
            if (!(d > 0.0)) bad = 1;
            sS[j * M + j] = sqrt(d);
        }
        __syncthreads();
        if (bad) break;
        const double dj = sS[j * M + j];
        __syncthreads();
        for (int i = j + 1 + tid; i < M; i += 256) sS[i * M + j] /= dj;
        __syncthreads();
        const int w = M - j - 1;
        for (int idx = tid; idx < w * w; idx += 256) {
            const int i = j + 1 + idx / w, k = j + 1 + idx % w;
            if (k <= i) sS[i * M + k] -= sS[i * M + j] * sS[k * M + j];
        }
        __syncthreads();
    }
    if (tid == 0) {
        ctl[4 * s + 3] = bad;
        double dg = 0.0, dDd = 0.0, dmax = 0.0;
        if (!bad) {
            for (int i = 0; i < M; ++i) {
                double b = -sg[i];
                for (int k = 0; k < i; ++k) b -= sS[i * M + k] * sd[k];
                sd[i] = b / sS[i * M + i];
            }
            for (int i = M - 1; i >= 0; --i) {
                double b = sd[i];
                for (int k = i + 1; k < M; ++k) b -= sS[k * M + i] * sd[k];
                sd[i] = b / sS[i * M + i];
            }
            for (int i = 0; i < M; ++i) {
                dg += sd[i] * sgc[i];
                dDd += sd[i] * sd[i] * sdU[i];
                if constexpr (NI > 0) dmax = fmax(dmax, fabs(sd[i]) * ssx[i]);
                else dmax = fmax(dmax, fabs(sd[i]));
            }
        } else {
            for (int i = 0; i < M; ++i) sd[i] = 0.0;
        }
        inf[4] = dg; inf[5] = dDd; inf[6] = dmax;
        for (int i = 0; i < M; ++i) rd[M * M + M + i] = sd[i];
    }
    __syncthreads();
    if (tid < C) {
        const double* ci = cm + tid * RG_CAM;
        double* co = camt + ((size_t)s * C + tid) * RG_CAM;
        for (int k = 0; k < RG_CAM; ++k) co[k] = ci[k];
        int o = rg_col<NI>(sl, isl, tid);
        if (sl[tid] >= 0 && !bad) {
            double Q[9];
            rg_rodrigues(sd + o, Q);
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) co[9 + 3 * i + j] = Q[3 * i] * ci[9 + j] + Q[3 * i + 1] * ci[12 + j] + Q[3 * i + 2] * ci[15 + j];
            for (int k = 0; k < 3; ++k) co[18 + k] = ci[18 + k] + sd[o + 3 + k];
        }
        if constexpr (NI > 0) {
            if (sl[tid] >= 0) o += 6;
            if (isl[tid] >= 0 && !bad) {
                const double e = exp(sd[o]);
                co[0] = ci[0] * e; co[1] = ci[1] * e; co[4] = ci[4] * e;
                if constexpr (NI == 3) { co[2] = ci[2] + sd[o + 1]; co[5] = ci[5] + sd[o + 2]; }
            }
        }
    }
}

// ---- the points' steps, the trial points and the trial cost.  part2 (4 per tile): E_trial, d_p . g_p, d_p^T diag(V) d_p, |d_p|_inf ----
template <int LOSS, int NI>
__global__ void __launch_bounds__(64) rig_backsub_kernel(const double* __restrict__ X, double* __restrict__ Xt, const double* __restrict__ uv,
                                                         const int32_t* __restrict__ tile, const int32_t* __restrict__ slot,
                                                         const int32_t* __restrict__ islot, const double* __restrict__ cams,
                                                         const double* __restrict__ camt, const int32_t* __restrict__ ctl,
                                                         const double* __restrict__ info, const double* __restrict__ red, int N, int S,
                                                         int C, double delta, double* __restrict__ part2) {
    const RgDims D = rg_dims<NI>(C);
    const int lane = threadIdx.x & 63, tl = blockIdx.x;
    const int s = uni((int)tile[4 * tl]), lo = uni((int)tile[4 * tl + 1]), n = uni((int)tile[4 * tl + 2]);
    if (s < 0 || s >= S || lo < 0 || n < 0 || n > RG_TILE || lo + n > N) return;
    if (ctl[4 * s] != 0 || ctl[4 * s + 3] != 0) return;
    const double mu = info[(size_t)s * RG_INFO + 2];
    const double* cm = cams + (size_t)s * C * RG_CAM;
    const double* ct = camt + (size_t)s * C * RG_CAM;
    const int32_t* sl = slot + (size_t)s * C;
    const int32_t* isl = NI > 0 ? islot + (size_t)s * C : nullptr;
    if (rg_col<NI>(sl, isl, C) > D.M) return;
    const double* dc = red + (size_t)s * D.RD + D.M * D.M + D.M;
    double Et = 0.0, dg = 0.0, dDd = 0.0, dmax = 0.0;
    if (lane < n) {
        const int i = lo + lane;
        const double Xp[3] = {X[(size_t)i * 3], X[(size_t)i * 3 + 1], X[(size_t)i * 3 + 2]};
        const double* uvp = uv + (size_t)i * C * 2;
        RgPoint P;
        rg_point<LOSS>(cm, uvp, C, Xp, mu, delta, P);
        double rhs[3] = {-P.g[0], -P.g[1], -P.g[2]};
        int off = 0;
        for (int c = 0; c < C; ++c) {
            bool pf = sl[c] >= 0, jf = false;
            if constexpr (NI > 0) jf = isl[c] >= 0;
            const double* d = dc + off;
            off += (pf ? 6 : 0) + (jf ? NI : 0);
            const double ou = uvp[2 * c], ov = uvp[2 * c + 1];
            if (!(pf || jf) || !(ou == ou)) continue;
            RgObs o;
            rg_obs<LOSS, NI>(cm + c * RG_CAM, Xp, ou, ov, delta, o);
            double su = 0.0, sv = 0.0;
            if (pf) {
                double ju[6], jv[6];
                rg_cam_rows(o, ju, jv);
#pragma unroll
                for (int r = 0; r < 6; ++r) { su += ju[r] * d[r]; sv += jv[r] * d[r]; }
                d += 6;
            }
            if constexpr (NI > 0)
                if (jf) {
#pragma unroll
                    for (int r = 0; r < NI; ++r) { su += o.iu[r] * d[r]; sv += o.iv[r] * d[r]; }
                }
            for (int k = 0; k < 3; ++k) rhs[k] -= o.a[k] * su + o.b[k] * sv;
        }
        double y[3], dp[3];
        rg_fwd(P.l, rhs, y);
        rg_bwd(P.l, y, dp);
        const double Xn[3] = {Xp[0] + dp[0], Xp[1] + dp[1], Xp[2] + dp[2]};
        for (int k = 0; k < 3; ++k) Xt[(size_t)i * 3 + k] = Xn[k];
        dg = dp[0] * P.g[0] + dp[1] * P.g[1] + dp[2] * P.g[2];
        dDd = dp[0] * dp[0] * P.V[0] + dp[1] * dp[1] * P.V[3] + dp[2] * dp[2] * P.V[5];
        dmax = fmax(fabs(dp[0]), fmax(fabs(dp[1]), fabs(dp[2])));
        for (int c = 0; c < C; ++c) {
            const double ou = uvp[2 * c], ov = uvp[2 * c + 1];
            if (!(ou == ou)) continue;
            RgObs o;
            rg_obs<LOSS>(ct + c * RG_CAM, Xn, ou, ov, delta, o);
            if constexpr (LOSS == MVMC_RIG_LOSS_NONE) Et += o.ru * o.ru + o.rv * o.rv;
            else Et += o.rho;
        }
    }
    Et = wave_sum(Et);
    if constexpr (LOSS == MVMC_RIG_LOSS_NONE) Et = 0.5 * Et;
    dg = wave_sum(dg);
    dDd = wave_sum(dDd);
    dmax = wave_max_dpp(dmax);
    if (lane == 0) {
        double* o = part2 + (size_t)tl * 4;
        o[0] = Et; o[1] = dg; o[2] = dDd; o[3] = dmax;
    }
}

// ---- accept or reject, the gauge rescale, the stop rules.  NI > 0: the prior of the trial cameras in the trial cost, and the trial K
// taken over on acceptance ----
template <int NI>
__global__ void __launch_bounds__(256) rig_decide_kernel(double* __restrict__ X, const double* __restrict__ Xt, const int32_t* __restrict__ seq,
                                                         const int32_t* __restrict__ slot, const int32_t* __restrict__ islot,
                                                         double* __restrict__ cams, const double* __restrict__ camt,
                                                         int32_t* __restrict__ ctl, double* __restrict__ info,
                                                         const double* __restrict__ part2, const double* __restrict__ K0, int N, int T,
                                                         int C, int max_iter, double ftol, double xtol, double sf, double sc) {
    __shared__ double sh[8];
    __shared__ int accept;
    const int s = blockIdx.x, tid = threadIdx.x;
    if (ctl[4 * s] != 0) return;
    const int t0 = seq[4 * s], nt = seq[4 * s + 1], p0 = seq[4 * s + 2], np = seq[4 * s + 3];
    if (t0 < 0 || nt < 0 || t0 + nt > T || p0 < 0 || np < 0 || p0 + np > N) return;
    double* inf = info + (size_t)s * RG_INFO;
    const int32_t* sl = slot + (size_t)s * C;
    const int32_t* isl = NI > 0 ? islot + (size_t)s * C : nullptr;
    if (rg_col<NI>(sl, isl, C) > rg_dims<NI>(C).M) return;
    const double* ct = camt + (size_t)s * C * RG_CAM;
    double* cm = cams + (size_t)s * C * RG_CAM;
    const int bad = ctl[4 * s + 3];
    if (tid < 64) {
        double Et = 0.0, dg = 0.0, dDd = 0.0, dmax = 0.0;
        if (!bad)
            for (int t = tid; t < nt; t += 64) {
                const double* p = part2 + (size_t)(t0 + t) * 4;
                Et += p[0]; dg += p[1]; dDd += p[2]; dmax = fmax(dmax, p[3]);
            }
        Et = wave_sum(Et); dg = wave_sum(dg); dDd = wave_sum(dDd); dmax = wave_max_dpp(dmax);
        if (tid == 0) {
            int it = ctl[4 * s + 1], stop = 0, acc = 0;
            const double E = inf[1], mu = inf[2];
            if (bad) {
                inf[RG_TRIALS + it] = 0.0;
                inf[RG_COSTS + it + 1] = E;
                inf[2] = mu * 10.0;
                ++it;
            } else {
                if constexpr (NI > 0) Et += rg_prior<NI>(ct, K0 + (size_t)s * C * 3, isl, C, sf, sc);
                dg += inf[4]; dDd += inf[5]; dmax = fmax(dmax, inf[6]);
                const double pred = 0.5 * (mu * dDd - dg);
                inf[7] = pred;
                if (dmax < xtol) stop = MVMC_RIG_STOP_XTOL;
                else if (pred < ftol * E) stop = MVMC_RIG_STOP_FTOL;
                else {
                    acc = Et < E;
                    inf[RG_TRIALS + it] = acc ? 1.0 : 0.0;
                    inf[RG_COSTS + it + 1] = acc ? Et : E;
                    ++it;
                    if (acc) {
                        inf[1] = Et;
                        inf[2] = mu / 10.0;
                        ctl[4 * s + 2] += 1;
                        if (E - Et < ftol * E) stop = MVMC_RIG_STOP_FTOL;
                        // gauge: |c_ref - c_0| back to its input length, about c_0
                        const int ref = rg_gauge_cam(sl, C);
                        double c0[3], cr[3];
                        rg_centre(ct, c0);
                        rg_centre(ct + (ref < 0 ? 0 : ref) * RG_CAM, cr);
                        const double len = sqrt((cr[0] - c0[0]) * (cr[0] - c0[0]) + (cr[1] - c0[1]) * (cr[1] - c0[1]) + (cr[2] - c0[2]) * (cr[2] - c0[2]));
                        sh[0] = inf[3] / len; sh[1] = c0[0]; sh[2] = c0[1]; sh[3] = c0[2];
                    } else {
                        inf[2] = mu * 10.0;
                    }
                }
            }
            if (stop == 0 && it >= max_iter) stop = MVMC_RIG_STOP_MAX_ITER;
            ctl[4 * s + 1] = it;
            ctl[4 * s] = stop;
            accept = acc;
        }
    }
    __syncthreads();
    if (!accept) return;
    const double gs = sh[0], c0[3] = {sh[1], sh[2], sh[3]};
    for (int i = tid; i < np; i += 256)
        for (int k = 0; k < 3; ++k) X[(size_t)(p0 + i) * 3 + k] = c0[k] + gs * (Xt[(size_t)(p0 + i) * 3 + k] - c0[k]);
    if (tid < C) {
        const double* ci = ct + tid * RG_CAM;
        double* co = cm + tid * RG_CAM;
        if constexpr (NI > 0)
            if (isl[tid] >= 0)
                for (int k = 0; k < 9; ++k) co[k] = ci[k];
        if (sl[tid] >= 0) {
            double cc[3];
            rg_centre(ci, cc);
            for (int k = 0; k < 3; ++k) cc[k] = c0[k] + gs * (cc[k] - c0[k]);
            for (int k = 9; k < 18; ++k) co[k] = ci[k];
            for (int r = 0; r < 3; ++r) co[18 + r] = -(ci[9 + 3 * r] * cc[0] + ci[9 + 3 * r + 1] * cc[1] + ci[9 + 3 * r + 2] * cc[2]);
        }
    }
}

// ---- the weights of the loss at (X, cams): w (N,C), NaN where the camera does not observe the point; points outside every tile are
// not written ----
template <int LOSS>
__global__ void __launch_bounds__(64) rig_weights_kernel(const double* __restrict__ X, const double* __restrict__ uv,
                                                         const int32_t* __restrict__ tile, const double* __restrict__ cams, int N, int S, int C,
                                                         double delta, double* __restrict__ w) {
    const int lane = threadIdx.x & 63, tl = blockIdx.x;
    const int s = uni((int)tile[4 * tl]), lo = uni((int)tile[4 * tl + 1]), n = uni((int)tile[4 * tl + 2]);
    if (s < 0 || s >= S || lo < 0 || n < 0 || n > RG_TILE || lo + n > N) return;
    if (lane >= n) return;
    const int i = lo + lane;
    const double* cm = cams + (size_t)s * C * RG_CAM;
    const double Xp[3] = {X[(size_t)i * 3], X[(size_t)i * 3 + 1], X[(size_t)i * 3 + 2]};
    const double* uvp = uv + (size_t)i * C * 2;
    for (int c = 0; c < C; ++c) {
        const double ou = uvp[2 * c], ov = uvp[2 * c + 1];
        double wc = rg_nan();
        if (ou == ou) {
            RgObs o;
            rg_obs<MVMC_RIG_LOSS_NONE>(cm + c * RG_CAM, Xp, ou, ov, delta, o);
            const double s2 = o.ru * o.ru + o.rv * o.rv;
            if constexpr (LOSS == MVMC_RIG_LOSS_HUBER) {
                const double sr = sqrt(s2);
                wc = sr <= delta ? 1.0 : delta / sr;
            } else if constexpr (LOSS == MVMC_RIG_LOSS_CAUCHY) {
                wc = 1.0 / (1.0 + s2 / (delta * delta));
            } else {
                wc = 1.0;
            }
        }
        w[(size_t)i * C + c] = wc;
    }
}

template <int NI>
size_t rg_accum_lds(int C) {
    const RgDims D = rg_dims<NI>(C);
    const size_t y = (size_t)D.Mp * RG_LD, j = (size_t)(7 + NI) * D.nq * RG_LDJ;
    return (NI == 0 ? y + j : y > j ? y : j) * sizeof(double);
}
template <int NI>
size_t rg_solve_lds(int C) {
    const RgDims D = rg_dims<NI>(C);
    return ((size_t)D.PD + (size_t)D.M * D.M + (NI == 0 ? 4 : 6) * D.M) * sizeof(double);
}

// the checks that every entry with tiles shares: sizes, the camera count, the trial cap and the loss
bool rg_args_ok(int n_points, int n_tiles, int n_seqs, int n_views, int max_iter, int loss, double loss_px) {
    if (n_points < 0 || n_tiles < 0 || n_seqs < 0 || n_views < 2 || n_views > MVMC_RIG_MAX_CAMS || max_iter < 0 || max_iter > MVMC_RIG_MAX_ITER)
        return false;
    if (loss < MVMC_RIG_LOSS_NONE || loss > MVMC_RIG_LOSS_CAUCHY) return false;
    return loss == MVMC_RIG_LOSS_NONE || (loss_px > 0.0 && loss_px <= 1.7976931348623157e308);   // (NaN fails both)
}
bool rg_intr_ok(int n_intr, double sf, double sc) { return (n_intr == 1 || n_intr == 3) && sf > 0.0 && sc > 0.0; }   // (NaN fails)

// f(LOSS, NI) as integral constants for the run-time (loss, n_intr); n_intr is 0, 1 or 3
template <class F>
auto rg_dispatch(int loss, int n_intr, F f) {
    auto ni = [&](auto L) {
        return n_intr == 1 ? f(L, std::integral_constant<int, 1>{}) : n_intr == 3 ? f(L, std::integral_constant<int, 3>{})
                                                                                  : f(L, std::integral_constant<int, 0>{});
    };
    return loss == MVMC_RIG_LOSS_HUBER    ? ni(std::integral_constant<int, MVMC_RIG_LOSS_HUBER>{})
           : loss == MVMC_RIG_LOSS_CAUCHY ? ni(std::integral_constant<int, MVMC_RIG_LOSS_CAUCHY>{})
                                          : ni(std::integral_constant<int, MVMC_RIG_LOSS_NONE>{});
}
long long rg_doubles(int n_views, int n_intr, bool red) {
    if (n_views < 2 || n_views > MVMC_RIG_MAX_CAMS) return -1;
    return rg_dispatch(MVMC_RIG_LOSS_NONE, n_intr, [&](auto, auto I) {
        const RgDims D = rg_dims<decltype(I)::value>(n_views);
        return (long long)(red ? D.RD : D.PD);
    });
}

template <bool MFMA, int LOSS, int NI>
int rg_accumulate(hipStream_t st, const double* X, const double* uv, const int32_t* tile, const int32_t* seq, const int32_t* slot,
                  const int32_t* islot, const double* cams, double* cams_trial, int32_t* ctl, double* info, const double* K0, int n_points,
                  int n_tiles, int n_seqs, int n_views, int max_iter, double mu0, double delta, double sf, double sc, double* part,
                  double* red) {
    const size_t la = rg_accum_lds<NI>(n_views), ls = rg_solve_lds<NI>(n_views);
    if (la > 65536 && hipFuncSetAttribute((const void*)rig_accum_kernel<MFMA, LOSS, NI>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)la) != hipSuccess)
        return MVMC_ERR_LAUNCH;
    if (ls > 65536 && hipFuncSetAttribute((const void*)rig_solve_kernel<NI>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ls) !=
                          hipSuccess)
        return MVMC_ERR_LAUNCH;
    if (n_tiles > 0) {
        hipLaunchKernelGGL((rig_accum_kernel<MFMA, LOSS, NI>), dim3(n_tiles), dim3(64), la, st, X, uv, tile, slot, islot, cams, ctl, info,
                           n_points, n_seqs, n_views, mu0, delta, part);
        MVMC_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(rig_solve_kernel<NI>, dim3(n_seqs), dim3(256), ls, st, seq, slot, islot, cams, cams_trial, ctl, info, part, red, K0,
                       n_tiles, n_views, max_iter, mu0, sf, sc);
    MVMC_CHECK_LAUNCH();
    return MVMC_OK;
}

template <int LOSS, int NI>
int rg_step(hipStream_t st, double* X, double* X_trial, const double* uv, const int32_t* tile, const int32_t* seq, const int32_t* slot,
            const int32_t* islot, double* cams, const double* cams_trial, int32_t* ctl, double* info, const double* red, const double* K0,
            int n_points, int n_tiles, int n_seqs, int n_views, int max_iter, double ftol, double xtol, double delta, double sf, double sc,
            double* part2) {
    if (n_tiles > 0) {
        hipLaunchKernelGGL((rig_backsub_kernel<LOSS, NI>), dim3(n_tiles), dim3(64), 0, st, X, X_trial, uv, tile, slot, islot, cams,
                           cams_trial, ctl, info, red, n_points, n_seqs, n_views, delta, part2);
        MVMC_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(rig_decide_kernel<NI>, dim3(n_seqs), dim3(256), 0, st, X, X_trial, seq, slot, islot, cams, cams_trial, ctl, info,
                       part2, K0, n_points, n_tiles, n_views, max_iter, ftol, xtol, sf, sc);
    MVMC_CHECK_LAUNCH();
    return MVMC_OK;
}

// The six trial entries end here: n_intr = 0 (islot, K0 not read) for those without intrinsics; the _intr entries have checked
// rg_intr_ok.  The FMA variant of the stacked product (variant 0) exists with n_intr = 0 alone.
int rg_accumulate_entry(const double* X, const double* uv, const int32_t* tile, const int32_t* seq, const int32_t* slot, const double* cams,
                        double* cams_trial, int32_t* ctl, double* info, int n_points, int n_tiles, int n_seqs, int n_views, int max_iter,
                        double mu0, int variant, double* part, double* red, int loss, double loss_px, int n_intr, const int32_t* islot,
                        const double* K0, double sf, double sc, mvmcStream_t stream) {
    if (!rg_args_ok(n_points, n_tiles, n_seqs, n_views, max_iter, loss, loss_px) || variant < (n_intr ? 1 : 0) || variant > 1)
        return MVMC_ERR_ARG;
    if (n_seqs == 0) return MVMC_OK;
    if (!X || !uv || !tile || !seq || !slot || !cams || !cams_trial || !ctl || !info || !part || !red || (n_intr && (!islot || !K0)))
        return MVMC_ERR_ARG;
    return rg_dispatch(loss, n_intr, [&](auto L, auto I) {
        constexpr int LOSS = decltype(L)::value, NI = decltype(I)::value;
        auto run = [&](auto MF) {
            return rg_accumulate<decltype(MF)::value, LOSS, NI>((hipStream_t)stream, X, uv, tile, seq, slot, islot, cams, cams_trial, ctl, info,
                                                                K0, n_points, n_tiles, n_seqs, n_views, max_iter, mu0, loss_px, sf, sc, part,
                                                                red);
        };
        if constexpr (NI == 0)
            if (variant == 0) return run(std::false_type{});
        return run(std::true_type{});
    });
}

int rg_step_entry(double* X, double* X_trial, const double* uv, const int32_t* tile, const int32_t* seq, const int32_t* slot, double* cams,
                  const double* cams_trial, int32_t* ctl, double* info, const double* red, int n_points, int n_tiles, int n_seqs,
                  int n_views, int max_iter, double ftol, double xtol, double* part2, int loss, double loss_px, int n_intr,
                  const int32_t* islot, const double* K0, double sf, double sc, mvmcStream_t stream) {
    if (!rg_args_ok(n_points, n_tiles, n_seqs, n_views, max_iter, loss, loss_px)) return MVMC_ERR_ARG;
    if (n_seqs == 0) return MVMC_OK;
    if (!X || !X_trial || !uv || !tile || !seq || !slot || !cams || !cams_trial || !ctl || !info || !red || !part2 ||
        (n_intr && (!islot || !K0)))
        return MVMC_ERR_ARG;
    return rg_dispatch(loss, n_intr, [&](auto L, auto I) {
        return rg_step<decltype(L)::value, decltype(I)::value>((hipStream_t)stream, X, X_trial, uv, tile, seq, slot, islot, cams, cams_trial,
                                                               ctl, info, red, K0, n_points, n_tiles, n_seqs, n_views, max_iter, ftol, xtol,
                                                               loss_px, sf, sc, part2);
    });
}

}  // namespace

extern "C" long long mvmc_rig_part_doubles(int n_views) { return rg_doubles(n_views, 0, false); }
extern "C" long long mvmc_rig_red_doubles(int n_views) { return rg_doubles(n_views, 0, true); }
extern "C" long long mvmc_rig_part_doubles_intr(int n_views, int n_intr) {
    return n_intr == 1 || n_intr == 3 ? rg_doubles(n_views, n_intr, false) : -1;
}
extern "C" long long mvmc_rig_red_doubles_intr(int n_views, int n_intr) {
    return n_intr == 1 || n_intr == 3 ? rg_doubles(n_views, n_intr, true) : -1;
}

extern "C" int mvmc_rig_start(const double* obs, const int32_t* rig_of, const double* Pmats, int n_points, int n_views, int n_rigs,
                              double min_score, double* X0, double* dist, mvmcStream_t stream) {
    if (n_points < 0 || n_views < 2 || n_views > MVMC_RIG_MAX_CAMS || n_rigs <= 0) return MVMC_ERR_ARG;
    if (n_points == 0) return MVMC_OK;
    if (!obs || !rig_of || !Pmats || !X0 || !dist) return MVMC_ERR_ARG;
    hipLaunchKernelGGL(rig_start_kernel, dim3((n_points + 255) / 256), dim3(256), 0, (hipStream_t)stream, obs, rig_of, Pmats, n_points,
                       n_views, n_rigs, min_score, X0, dist);
    MVMC_CHECK_LAUNCH();
    return MVMC_OK;
}


extern "C" int mvmc_rig_accumulate(const double* X, const double* uv, const int32_t* tile, const int32_t* seq, const int32_t* slot,
                                   const double* cams, double* cams_trial, int32_t* ctl, double* info, int n_points, int n_tiles,
                                   int n_seqs, int n_views, int max_iter, double mu0, int variant, double* part, double* red,
                                   mvmcStream_t stream) {
    return rg_accumulate_entry(X, uv, tile, seq, slot, cams, cams_trial, ctl, info, n_points, n_tiles, n_seqs, n_views, max_iter, mu0,
                               variant, part, red, MVMC_RIG_LOSS_NONE, 0.0, 0, nullptr, nullptr, 0.0, 0.0, stream);
}

extern "C" int mvmc_rig_step(double* X, double* X_trial, const double* uv, const int32_t* tile, const int32_t* seq, const int32_t* slot,
                             double* cams, const double* cams_trial, int32_t* ctl, double* info, const double* red, int n_points,
                             int n_tiles, int n_seqs, int n_views, int max_iter, double ftol, double xtol, double* part2,
                             mvmcStream_t stream) {
    return rg_step_entry(X, X_trial, uv, tile, seq, slot, cams, cams_trial, ctl, info, red, n_points, n_tiles, n_seqs, n_views, max_iter,
                         ftol, xtol, part2, MVMC_RIG_LOSS_NONE, 0.0, 0, nullptr, nullptr, 0.0, 0.0, stream);
}

extern "C" int mvmc_rig_accumulate_robust(const double* X, const double* uv, const int32_t* tile, const int32_t* seq, const int32_t* slot,
                                          const double* cams, double* cams_trial, int32_t* ctl, double* info, int n_points, int n_tiles,
                                          int n_seqs, int n_views, int max_iter, double mu0, int variant, double* part, double* red,
                                          int loss, double loss_px, mvmcStream_t stream) {
    return rg_accumulate_entry(X, uv, tile, seq, slot, cams, cams_trial, ctl, info, n_points, n_tiles, n_seqs, n_views, max_iter, mu0,
                               variant, part, red, loss, loss_px, 0, nullptr, nullptr, 0.0, 0.0, stream);
}

extern "C" int mvmc_rig_step_robust(double* X, double* X_trial, const double* uv, const int32_t* tile, const int32_t* seq,
                                    const int32_t* slot, double* cams, const double* cams_trial, int32_t* ctl, double* info,
                                    const double* red, int n_points, int n_tiles, int n_seqs, int n_views, int max_iter, double ftol,
                                    double xtol, double* part2, int loss, double loss_px, mvmcStream_t stream) {
    return rg_step_entry(X, X_trial, uv, tile, seq, slot, cams, cams_trial, ctl, info, red, n_points, n_tiles, n_seqs, n_views, max_iter,
                         ftol, xtol, part2, loss, loss_px, 0, nullptr, nullptr, 0.0, 0.0, stream);
}

extern "C" int mvmc_rig_accumulate_intr(const double* X, const double* uv, const int32_t* tile, const int32_t* seq, const int32_t* slot,
                                        const double* cams, double* cams_trial, int32_t* ctl, double* info, int n_points, int n_tiles,
                                        int n_seqs, int n_views, int max_iter, double mu0, int variant, double* part, double* red,
                                        int loss, double loss_px, int n_intr, const int32_t* islot, const double* K0, double focal_sigma,
                                        double centre_sigma, mvmcStream_t stream) {
    if (!rg_intr_ok(n_intr, focal_sigma, centre_sigma)) return MVMC_ERR_ARG;
    return rg_accumulate_entry(X, uv, tile, seq, slot, cams, cams_trial, ctl, info, n_points, n_tiles, n_seqs, n_views, max_iter, mu0,
                               variant, part, red, loss, loss_px, n_intr, islot, K0, focal_sigma, centre_sigma, stream);
}

extern "C" int mvmc_rig_step_intr(double* X, double* X_trial, const double* uv, const int32_t* tile, const int32_t* seq,
                                  const int32_t* slot, double* cams, const double* cams_trial, int32_t* ctl, double* info,
                                  const double* red, int n_points, int n_tiles, int n_seqs, int n_views, int max_iter, double ftol,
                                  double xtol, double* part2, int loss, double loss_px, int n_intr, const int32_t* islot, const double* K0,
                                  double focal_sigma, double centre_sigma, mvmcStream_t stream) {
    if (!rg_intr_ok(n_intr, focal_sigma, centre_sigma)) return MVMC_ERR_ARG;
    return rg_step_entry(X, X_trial, uv, tile, seq, slot, cams, cams_trial, ctl, info, red, n_points, n_tiles, n_seqs, n_views, max_iter,
                         ftol, xtol, part2, loss, loss_px, n_intr, islot, K0, focal_sigma, centre_sigma, stream);
}

extern "C" int mvmc_rig_weights(const double* X, const double* uv, const int32_t* tile, const double* cams, int n_points, int n_tiles,
                                int n_seqs, int n_views, int loss, double loss_px, double* w, mvmcStream_t stream) {
    if (!rg_args_ok(n_points, n_tiles, n_seqs, n_views, 0, loss, loss_px)) return MVMC_ERR_ARG;
    if (n_tiles == 0 || n_seqs == 0) return MVMC_OK;
    if (!X || !uv || !tile || !cams || !w) return MVMC_ERR_ARG;
    return rg_dispatch(loss, 0, [&](auto L, auto) -> int {
        hipLaunchKernelGGL(rig_weights_kernel<decltype(L)::value>, dim3(n_tiles), dim3(64), 0, (hipStream_t)stream, X, uv, tile, cams,
                           n_points, n_seqs, n_views, loss_px, w);
        MVMC_CHECK_LAUNCH();
        return MVMC_OK;
    });
}
