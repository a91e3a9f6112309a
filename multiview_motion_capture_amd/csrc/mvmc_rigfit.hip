// Rig refinement (multiview_motion_capture_amd/rig_refine.py; algorithm restated in tests/rig_refine_np.py): a bundle adjustment of
// every sequence's cameras over the keypoints of its tracked people.  No counterpart in the reference.
//   start     per candidate point: the DLT of the views that see it (dlt_point, the arithmetic of mvmc_dlt) with the point's own rig,
//             and its reprojection distance in every such view;
//   accum     per TILE of MVMC_RIG_TILE points (one wave, one point per lane): the damped point blocks V* = L L^T, per free camera
//             Y = W L^-T, and the tile's part of the Schur complement as ONE symmetric product over the stacked rows [Y; z^T]
//             (z = L^-1 g_p) staged in LDS -- on the matrix cores (v_mfma_f64_16x16x4_f64) or, variant 0, as FMAs over the same LDS
//             rows; the camera blocks J_c J_c^T (with the residual as seventh row: U_c, g_c) the same way from a second LDS table;
//   solve     one workgroup per sequence: the tile parts summed IN TILE ORDER, S = U* - sum Y Y^T by Cholesky, the trial cameras;
//   backsub   per tile: the points' steps, the trial points and the trial cost;
//   decide    one workgroup per sequence: accept / reject, the gauge rescale, mu, the stop rules.
// The tiles of a sequence are cut from its own points, every sum has a fixed order and there are no atomics: a sequence's numbers
// depend on nothing else in the launch.  A sequence that has stopped (ctl[0] != 0) idles.
// Robust loss (the _robust entries; restated in tests/rig_robust_np.py): rg_obs, rg_point and the two tile kernels take the loss as a
// compile-time parameter.  With a loss an observation's rows a, b, ju, jv and its residual are multiplied by sqrt(w) as the lane forms
// them and the tile's E is the sum of rho; everything staged in LDS, part, red, the solve and the decision are what they are without
// one.  LOSS = MVMC_RIG_LOSS_NONE is the arithmetic without a loss, operation for operation.
// Intrinsic unknowns (the _intr entries; restated in tests/rig_intr_np.py): kernels of their own at the end of this file, the code
// above is what it was.  Per camera with islot >= 0, NI = 1 (phi: K00, K01, K11 <- e^phi x themselves) or 3 (and dcx, dcy) more
// unknowns with a Gaussian prior about the input K.  LAYOUT of their reduced system: one contiguous block per camera in camera order,
// its 6 pose columns if slot >= 0, then its NI intrinsic columns if islot >= 0; M = 6 (C - 1) + NI C, identity past a sequence's
// own columns; red = S (M x M), g (M), d (M).  [Y; z^T] and the camera rows share one LDS allocation, one after the other.
#include "mvmc_common.h"
#include "mvmc_dlt_point.h"

namespace {

constexpr int RG_TILE = MVMC_RIG_TILE;
constexpr int RG_LD = 3 * RG_TILE + 2;    // row stride of the Y table (doubles): 388 dwords = 4 mod 64 banks
constexpr int RG_LDJ = 2 * RG_TILE + 2;   // row stride of the camera-row table
constexpr int RG_CAM = MVMC_RIG_CAM_DOUBLES;
constexpr int RG_INFO = MVMC_RIG_INFO_DOUBLES;
constexpr int RG_TRIALS = 8, RG_COSTS = 8 + MVMC_RIG_MAX_ITER;
typedef double rg_d4 __attribute__((ext_vector_type(4)));

struct RgDims { int nf, M, Mp, nb, nblk, PD, RD; };
__host__ __device__ inline RgDims rg_dims(int C) {
    RgDims d;
    d.nf = C - 1;
    d.M = 6 * d.nf;
    d.Mp = (d.M + 1 + 15) / 16 * 16;      // rows of [Y; z^T], padded to the matrix core's 16
    d.nb = d.Mp / 16;
    d.nblk = d.nb * (d.nb + 1) / 2;       // lower block triangle
    d.PD = (d.nblk * 256 + 28 * d.nf + 1 + 1) / 2 * 2;
    d.RD = d.M * d.M + 2 * d.M;
    return d;
}
__device__ __forceinline__ int rg_q7(int i, int j) { return i * 7 - i * (i - 1) / 2 + (j - i); }   // i <= j < 7, of 28

__device__ __forceinline__ double rg_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

// one observation: residual, the point rows a, b of the Jacobian (R^T du, R^T dv), and y = R X, du, dv for the camera rows
// with a loss: rho of the plain residual, and ru, rv, a, b, du, dv (so ju, jv) times sqrt(w)
struct RgObs { double ru, rv, a[3], b[3], y[3], du[3], dv[3], rho; };
template <int LOSS>
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
    if constexpr (LOSS != MVMC_RIG_LOSS_NONE) {
        const double s2 = o.ru * o.ru + o.rv * o.rv;
        double sw;
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
// + bj, row-major), then per slot the 28 products of the rows (J_c; r) (upper triangle, rg_q7), then E = 1/2 sum r^2 of the tile
// (with a loss: sum rho).
template <bool MFMA, int LOSS>
__global__ void __launch_bounds__(64) rig_accum_kernel(const double* __restrict__ X, const double* __restrict__ uv,
                                                       const int32_t* __restrict__ tile, const int32_t* __restrict__ slot,
                                                       const double* __restrict__ cams, const int32_t* __restrict__ ctl,
                                                       const double* __restrict__ info, int N, int S, int C, double mu0,
                                                       double delta, double* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) double rg_lds[];
    const RgDims D = rg_dims(C);
    double* sY = rg_lds;
    double* sJ = rg_lds + D.Mp * RG_LD;
    const int lane = threadIdx.x & 63, tl = blockIdx.x;
    const int s = uni((int)tile[4 * tl]), lo = uni((int)tile[4 * tl + 1]), n = uni((int)tile[4 * tl + 2]);
    if (s < 0 || s >= S || lo < 0 || n < 0 || n > RG_TILE || lo + n > N) return;
    if (ctl[4 * s] != 0) return;
    const double mu = ctl[4 * s + 1] == 0 ? mu0 : info[(size_t)s * RG_INFO + 2];
    const double* cm = cams + (size_t)s * C * RG_CAM;
    const int32_t* sl = slot + (size_t)s * C;
    for (int r = 0; r < D.Mp; ++r)
        for (int k = 0; k < 3; ++k) sY[r * RG_LD + 3 * lane + k] = 0.0;
    for (int r = 0; r < 7 * D.nf; ++r) { sJ[r * RG_LDJ + 2 * lane] = 0.0; sJ[r * RG_LDJ + 2 * lane + 1] = 0.0; }
    double rr = 0.0;
    if (lane < n) {
        const int i = lo + lane;
        const double Xp[3] = {X[(size_t)i * 3], X[(size_t)i * 3 + 1], X[(size_t)i * 3 + 2]};
        const double* uvp = uv + (size_t)i * C * 2;
        RgPoint P;
        rg_point<LOSS>(cm, uvp, C, Xp, mu, delta, P);
        rr = P.rr;
        double z[3];
        rg_fwd(P.l, P.g, z);
        for (int k = 0; k < 3; ++k) sY[D.M * RG_LD + 3 * lane + k] = z[k];
        for (int c = 0; c < C; ++c) {
            const int q = sl[c];
            const double ou = uvp[2 * c], ov = uvp[2 * c + 1];
            if (q < 0 || q >= D.nf || !(ou == ou)) continue;
            RgObs o;
            rg_obs<LOSS>(cm + c * RG_CAM, Xp, ou, ov, delta, o);
            double ju[6], jv[6];
            rg_cam_rows(o, ju, jv);
#pragma unroll
            for (int r = 0; r < 6; ++r) {
                const double w[3] = {ju[r] * o.a[0] + jv[r] * o.b[0], ju[r] * o.a[1] + jv[r] * o.b[1], ju[r] * o.a[2] + jv[r] * o.b[2]};
                double y[3];
                rg_fwd(P.l, w, y);
                for (int k = 0; k < 3; ++k) sY[(6 * q + r) * RG_LD + 3 * lane + k] = y[k];
                sJ[(7 * q + r) * RG_LDJ + 2 * lane] = ju[r];
                sJ[(7 * q + r) * RG_LDJ + 2 * lane + 1] = jv[r];
            }
            sJ[(7 * q + 6) * RG_LDJ + 2 * lane] = o.ru;
            sJ[(7 * q + 6) * RG_LDJ + 2 * lane + 1] = o.rv;
        }
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
    for (int e = lane; e < 28 * D.nf; e += 64) {
        const int q = e / 28, w = e - 28 * q;
        int i = 0, rem = w;
        while (rem >= 7 - i) { rem -= 7 - i; ++i; }
        const double* ra = sJ + (7 * q + i) * RG_LDJ;
        const double* rb = sJ + (7 * q + i + rem) * RG_LDJ;
        double acc = 0.0;
        for (int k = 0; k < 2 * RG_TILE; ++k) acc = fma(ra[k], rb[k], acc);
        out[D.nblk * 256 + e] = acc;
    }
    double E = wave_sum(rr);
    if constexpr (LOSS == MVMC_RIG_LOSS_NONE) E = 0.5 * E;
    if (lane == 0) out[D.nblk * 256 + 28 * D.nf] = E;
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

// ---- the sequence's reduced system and its solution ----
// red (RD per sequence): S (M x M, row-major; identity on the slots the sequence does not use), g (M), d (M)
__global__ void __launch_bounds__(256) rig_solve_kernel(const int32_t* __restrict__ seq, const int32_t* __restrict__ slot,
                                                        const double* __restrict__ cams, double* __restrict__ camt,
                                                        int32_t* __restrict__ ctl, double* __restrict__ info,
                                                        const double* __restrict__ part, double* __restrict__ red, int T, int C,
                                                        int max_iter, double mu0) {
    extern __shared__ __attribute__((aligned(16))) double rg_lds[];
    __shared__ int bad;
    const RgDims D = rg_dims(C);
    const int M = D.M;
    double* sP = rg_lds;
    double* sS = sP + D.PD;
    double* sg = sS + M * M;
    double* sd = sg + M;
    double* sgc = sd + M;
    double* sdU = sgc + M;
    const int s = blockIdx.x, tid = threadIdx.x;
    if (ctl[4 * s] != 0) return;
    const int it = ctl[4 * s + 1];
    const int t0 = seq[4 * s], nt = seq[4 * s + 1];
    if (t0 < 0 || nt < 0 || t0 + nt > T) return;
    for (int e = tid; e < D.PD; e += 256) {
        double acc = 0.0;
        for (int t = 0; t < nt; ++t) acc += part[(size_t)(t0 + t) * D.PD + e];
        sP[e] = acc;
    }
    if (tid == 0) bad = 0;
    __syncthreads();
    double* inf = info + (size_t)s * RG_INFO;
    const double* cm = cams + (size_t)s * C * RG_CAM;
    const int32_t* sl = slot + (size_t)s * C;
    int nfs = 0, ref = -1;
    for (int c = 0; c < C; ++c)
        if (sl[c] >= 0) { if (sl[c] == 0) ref = c; ++nfs; }
    const double mu = it == 0 ? mu0 : inf[2];
    if (it == 0 && tid == 0) {
        const double E = sP[D.nblk * 256 + 28 * D.nf];
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
    const double* sC = sP + D.nblk * 256;
    double* rd = red + (size_t)s * D.RD;
    for (int idx = tid; idx < M * M; idx += 256) {
        const int i = idx / M, j = idx - i * M;
        const int si = i / 6, sj = j / 6;
        double v;
        if (si >= nfs || sj >= nfs) v = i == j ? 1.0 : 0.0;
        else {
            v = -Tm(i > j ? i : j, i > j ? j : i);
            if (si == sj) {
                const int a = i - 6 * si, b = j - 6 * sj;
                const double u = sC[28 * si + rg_q7(a < b ? a : b, a < b ? b : a)];
                v += u;
                if (i == j) v += mu * u;
            }
        }
        sS[idx] = v;
        rd[idx] = v;
    }
    for (int i = tid; i < M; i += 256) {
        const int si = i / 6, a = i - 6 * si;
        const bool use = si < nfs;
        const double gc = use ? sC[28 * si + rg_q7(a, 6)] : 0.0;
        sgc[i] = gc;
        sdU[i] = use ? sC[28 * si + rg_q7(a, a)] : 0.0;
        const double g = use ? gc - Tm(M, i) : 0.0;
        sg[i] = g;
        rd[M * M + i] = g;
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
                dmax = fmax(dmax, fabs(sd[i]));
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
        const int q = sl[tid];
        if (q >= 0 && q < D.nf && !bad) {
            double Q[9];
            rg_rodrigues(sd + 6 * q, Q);
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) co[9 + 3 * i + j] = Q[3 * i] * ci[9 + j] + Q[3 * i + 1] * ci[12 + j] + Q[3 * i + 2] * ci[15 + j];
            for (int k = 0; k < 3; ++k) co[18 + k] = ci[18 + k] + sd[6 * q + 3 + k];
        }
    }
}

// ---- the points' steps, the trial points and the trial cost.  part2 (4 per tile): E_trial, d_p . g_p, d_p^T diag(V) d_p, |d_p|_inf ----
template <int LOSS>
__global__ void __launch_bounds__(64) rig_backsub_kernel(const double* __restrict__ X, double* __restrict__ Xt, const double* __restrict__ uv,
                                                         const int32_t* __restrict__ tile, const int32_t* __restrict__ slot,
                                                         const double* __restrict__ cams, const double* __restrict__ camt,
                                                         const int32_t* __restrict__ ctl, const double* __restrict__ info,
                                                         const double* __restrict__ red, int N, int S, int C, double delta,
                                                         double* __restrict__ part2) {
    const RgDims D = rg_dims(C);
    const int lane = threadIdx.x & 63, tl = blockIdx.x;
    const int s = uni((int)tile[4 * tl]), lo = uni((int)tile[4 * tl + 1]), n = uni((int)tile[4 * tl + 2]);
    if (s < 0 || s >= S || lo < 0 || n < 0 || n > RG_TILE || lo + n > N) return;
    if (ctl[4 * s] != 0 || ctl[4 * s + 3] != 0) return;
    const double mu = info[(size_t)s * RG_INFO + 2];
    const double* cm = cams + (size_t)s * C * RG_CAM;
    const double* ct = camt + (size_t)s * C * RG_CAM;
    const int32_t* sl = slot + (size_t)s * C;
    const double* dc = red + (size_t)s * D.RD + D.M * D.M + D.M;
    double Et = 0.0, dg = 0.0, dDd = 0.0, dmax = 0.0;
    if (lane < n) {
        const int i = lo + lane;
        const double Xp[3] = {X[(size_t)i * 3], X[(size_t)i * 3 + 1], X[(size_t)i * 3 + 2]};
        const double* uvp = uv + (size_t)i * C * 2;
        RgPoint P;
        rg_point<LOSS>(cm, uvp, C, Xp, mu, delta, P);
        double rhs[3] = {-P.g[0], -P.g[1], -P.g[2]};
        for (int c = 0; c < C; ++c) {
            const int q = sl[c];
            const double ou = uvp[2 * c], ov = uvp[2 * c + 1];
            if (q < 0 || q >= D.nf || !(ou == ou)) continue;
            RgObs o;
            rg_obs<LOSS>(cm + c * RG_CAM, Xp, ou, ov, delta, o);
            double ju[6], jv[6];
            rg_cam_rows(o, ju, jv);
            double su = 0.0, sv = 0.0;
#pragma unroll
            for (int r = 0; r < 6; ++r) { su += ju[r] * dc[6 * q + r]; sv += jv[r] * dc[6 * q + r]; }
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

// ---- accept or reject, the gauge rescale, the stop rules ----
__global__ void __launch_bounds__(256) rig_decide_kernel(double* __restrict__ X, const double* __restrict__ Xt, const int32_t* __restrict__ seq,
                                                         const int32_t* __restrict__ slot, double* __restrict__ cams,
                                                         const double* __restrict__ camt, int32_t* __restrict__ ctl,
                                                         double* __restrict__ info, const double* __restrict__ part2, int N, int T, int C,
                                                         int max_iter, double ftol, double xtol) {
    __shared__ double sh[8];
    __shared__ int accept;
    const int s = blockIdx.x, tid = threadIdx.x;
    if (ctl[4 * s] != 0) return;
    const int t0 = seq[4 * s], nt = seq[4 * s + 1], p0 = seq[4 * s + 2], np = seq[4 * s + 3];
    if (t0 < 0 || nt < 0 || t0 + nt > T || p0 < 0 || np < 0 || p0 + np > N) return;
    double* inf = info + (size_t)s * RG_INFO;
    const int32_t* sl = slot + (size_t)s * C;
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
                        int ref = 0;
                        for (int c = 0; c < C; ++c)
                            if (sl[c] == 0) ref = c;
                        double c0[3], cr[3];
                        rg_centre(ct, c0);
                        rg_centre(ct + ref * RG_CAM, cr);
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
    const double sc = sh[0], c0[3] = {sh[1], sh[2], sh[3]};
    for (int i = tid; i < np; i += 256)
        for (int k = 0; k < 3; ++k) X[(size_t)(p0 + i) * 3 + k] = c0[k] + sc * (Xt[(size_t)(p0 + i) * 3 + k] - c0[k]);
    if (tid < C && sl[tid] >= 0) {
        const double* ci = ct + tid * RG_CAM;
        double* co = cm + tid * RG_CAM;
        double cc[3];
        rg_centre(ci, cc);
        for (int k = 0; k < 3; ++k) cc[k] = c0[k] + sc * (cc[k] - c0[k]);
        for (int k = 9; k < 18; ++k) co[k] = ci[k];
        for (int r = 0; r < 3; ++r) co[18 + r] = -(ci[9 + 3 * r] * cc[0] + ci[9 + 3 * r + 1] * cc[1] + ci[9 + 3 * r + 2] * cc[2]);
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

size_t rg_accum_lds(int C) {
    const RgDims D = rg_dims(C);
    return ((size_t)D.Mp * RG_LD + (size_t)7 * D.nf * RG_LDJ) * sizeof(double);
}
size_t rg_solve_lds(int C) {
    const RgDims D = rg_dims(C);
    return ((size_t)D.PD + (size_t)D.M * D.M + 4 * D.M) * sizeof(double);
}

bool rg_loss_ok(int loss, double loss_px) {
    if (loss < MVMC_RIG_LOSS_NONE || loss > MVMC_RIG_LOSS_CAUCHY) return false;
    return loss == MVMC_RIG_LOSS_NONE || (loss_px > 0.0 && loss_px <= 1.7976931348623157e308);   // (NaN fails both)
}

template <bool MFMA, int LOSS>
int rg_launch_accum(hipStream_t st, size_t la, int n_tiles, const double* X, const double* uv, const int32_t* tile, const int32_t* slot,
                    const double* cams, const int32_t* ctl, const double* info, int n_points, int n_seqs, int n_views, double mu0,
                    double delta, double* part) {
    if (la > 65536 && hipFuncSetAttribute((const void*)rig_accum_kernel<MFMA, LOSS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)la) !=
                          hipSuccess)
        return MVMC_ERR_LAUNCH;
    if (n_tiles > 0) {
        hipLaunchKernelGGL((rig_accum_kernel<MFMA, LOSS>), dim3(n_tiles), dim3(64), la, st, X, uv, tile, slot, cams, ctl, info, n_points,
                           n_seqs, n_views, mu0, delta, part);
        MVMC_CHECK_LAUNCH();
    }
    return MVMC_OK;
}

int rg_accumulate(const double* X, const double* uv, const int32_t* tile, const int32_t* seq, const int32_t* slot, const double* cams,
                  double* cams_trial, int32_t* ctl, double* info, int n_points, int n_tiles, int n_seqs, int n_views, int max_iter,
                  double mu0, int variant, double* part, double* red, int loss, double loss_px, mvmcStream_t stream) {
    if (n_points < 0 || n_tiles < 0 || n_seqs < 0 || n_views < 2 || n_views > MVMC_RIG_MAX_CAMS || max_iter < 0 ||
        max_iter > MVMC_RIG_MAX_ITER || variant < 0 || variant > 1 || !rg_loss_ok(loss, loss_px))
        return MVMC_ERR_ARG;
    if (n_seqs == 0) return MVMC_OK;
    if (!X || !uv || !tile || !seq || !slot || !cams || !cams_trial || !ctl || !info || !part || !red) return MVMC_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const size_t la = rg_accum_lds(n_views), ls = rg_solve_lds(n_views);
    if (ls > 65536 && hipFuncSetAttribute((const void*)rig_solve_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ls) != hipSuccess)
        return MVMC_ERR_LAUNCH;
    int rc;
#define RG_ACCUM(MF, LS) rg_launch_accum<MF, LS>(st, la, n_tiles, X, uv, tile, slot, cams, ctl, info, n_points, n_seqs, n_views, mu0, loss_px, part)
    if (loss == MVMC_RIG_LOSS_HUBER) rc = variant ? RG_ACCUM(true, MVMC_RIG_LOSS_HUBER) : RG_ACCUM(false, MVMC_RIG_LOSS_HUBER);
    else if (loss == MVMC_RIG_LOSS_CAUCHY) rc = variant ? RG_ACCUM(true, MVMC_RIG_LOSS_CAUCHY) : RG_ACCUM(false, MVMC_RIG_LOSS_CAUCHY);
    else rc = variant ? RG_ACCUM(true, MVMC_RIG_LOSS_NONE) : RG_ACCUM(false, MVMC_RIG_LOSS_NONE);
#undef RG_ACCUM
    if (rc != MVMC_OK) return rc;
    hipLaunchKernelGGL(rig_solve_kernel, dim3(n_seqs), dim3(256), ls, st, seq, slot, cams, cams_trial, ctl, info, part, red, n_tiles,
                       n_views, max_iter, mu0);
    MVMC_CHECK_LAUNCH();
    return MVMC_OK;
}

int rg_step(double* X, double* X_trial, const double* uv, const int32_t* tile, const int32_t* seq, const int32_t* slot, double* cams,
            const double* cams_trial, int32_t* ctl, double* info, const double* red, int n_points, int n_tiles, int n_seqs, int n_views,
            int max_iter, double ftol, double xtol, double* part2, int loss, double loss_px, mvmcStream_t stream) {
    if (n_points < 0 || n_tiles < 0 || n_seqs < 0 || n_views < 2 || n_views > MVMC_RIG_MAX_CAMS || max_iter < 0 ||
        max_iter > MVMC_RIG_MAX_ITER || !rg_loss_ok(loss, loss_px))
        return MVMC_ERR_ARG;
    if (n_seqs == 0) return MVMC_OK;
    if (!X || !X_trial || !uv || !tile || !seq || !slot || !cams || !cams_trial || !ctl || !info || !red || !part2) return MVMC_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (n_tiles > 0) {
#define RG_BACKSUB(LS) hipLaunchKernelGGL(rig_backsub_kernel<LS>, dim3(n_tiles), dim3(64), 0, st, X, X_trial, uv, tile, slot, cams, cams_trial, \
                                          ctl, info, red, n_points, n_seqs, n_views, loss_px, part2)
        if (loss == MVMC_RIG_LOSS_HUBER) RG_BACKSUB(MVMC_RIG_LOSS_HUBER);
        else if (loss == MVMC_RIG_LOSS_CAUCHY) RG_BACKSUB(MVMC_RIG_LOSS_CAUCHY);
        else RG_BACKSUB(MVMC_RIG_LOSS_NONE);
#undef RG_BACKSUB
        MVMC_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(rig_decide_kernel, dim3(n_seqs), dim3(256), 0, st, X, X_trial, seq, slot, cams, cams_trial, ctl, info, part2,
                       n_points, n_tiles, n_views, max_iter, ftol, xtol);
    MVMC_CHECK_LAUNCH();
    return MVMC_OK;
}

// ==== intrinsic unknowns (the _intr entries; restated in tests/rig_intr_np.py) ====
// Per camera with free intrinsics NI = 1 or 3 more unknowns: phi (K00, K01, K11 <- e^phi x themselves) and, NI = 3, the additive
// dcx, dcy on K02, K12.  Their rows of an observation are closed-form from rg_obs: d(u, v)/dphi = (u - cx, v - cy), d/dcx = (1, 0),
// d/dcy = (0, 1), times sqrt(w) with a loss.  Camera 0's pose stays held; its intrinsics may be free (slot -1, islot >= 0).
// Layout of the reduced system: one contiguous block per camera in camera order -- its 6 pose columns if slot >= 0, then its NI
// intrinsic columns if islot >= 0 -- M = 6 (C - 1) + NI C columns at the most; columns past a sequence's own are identity.  red is
// S (M x M), g (M), d (M) as without intrinsics.
// part (PD per tile): the lower block triangle of [Y; z^T] [Y; z^T]^T (z^T is row M), then PER CAMERA (not per slot) the
// NR (NR + 1) / 2 products of its NR = 7 + NI rows (6 pose rows, NI intrinsic rows, the residual; rows of unknowns that are not
// free are zero), upper triangle, then E of the tile.
// LDS: the two tables are not resident together (C = 8, NI = 3 would need about 201 KB).  The tile stages [Y; z^T], multiplies,
// and then stages the camera rows into the SAME LDS from a second evaluation of the observations: max(Mp x 1,552 B, C NR x 1,040 B),
// 124,160 B at C = 8, NI = 3.
// Prior: E_prior = 1/2 sum (phi / sigma_f)^2 + 1/2 sum (dcx^2 + dcy^2) / sigma_c^2 about the input K (K0: fx, cx, cy per camera),
// phi = log(K00 / fx0) -- accumulated over the call.  It is part of every E read or written and of the diagonal and gradient of the
// intrinsic columns (added per sequence in the solve kernel, in camera order); sigma = +inf is no term.
template <int NI>
__host__ __device__ inline RgDims rg_dims_intr(int C) {
    constexpr int NR = 7 + NI;
    RgDims d;
    d.nf = C - 1;
    d.M = 6 * d.nf + NI * C;
    d.Mp = (d.M + 1 + 15) / 16 * 16;
    d.nb = d.Mp / 16;
    d.nblk = d.nb * (d.nb + 1) / 2;
    d.PD = (d.nblk * 256 + NR * (NR + 1) / 2 * C + 1 + 1) / 2 * 2;
    d.RD = d.M * d.M + 2 * d.M;
    return d;
}
// columns of the sequence in front of camera c's block (c = C: all of them)
template <int NI>
__device__ __forceinline__ int rg_col(const int32_t* __restrict__ sl, const int32_t* __restrict__ isl, int c) {
    int off = 0;
    for (int k = 0; k < c; ++k) off += (sl[k] >= 0 ? 6 : 0) + (isl[k] >= 0 ? NI : 0);
    return off;
}

// rg_obs and the intrinsic rows iu, iv of the observation
template <int NI>
struct RgObsI : RgObs { double iu[NI], iv[NI]; };
template <int LOSS, int NI>
__device__ __forceinline__ void rg_obs_intr(const double* __restrict__ cam, const double* X, double ou, double ov, double delta,
                                            RgObsI<NI>& o) {
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
    o.rho = 0.0;
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
    o.iu[0] = sw * (u - K[2]); o.iv[0] = sw * (v - K[5]);
    if constexpr (NI == 3) { o.iu[1] = sw; o.iv[1] = 0.0; o.iu[2] = 0.0; o.iv[2] = sw; }
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

template <int LOSS, int NI>
__global__ void __launch_bounds__(64) rig_accum_intr_kernel(const double* __restrict__ X, const double* __restrict__ uv,
                                                            const int32_t* __restrict__ tile, const int32_t* __restrict__ slot,
                                                            const int32_t* __restrict__ islot, const double* __restrict__ cams,
                                                            const int32_t* __restrict__ ctl, const double* __restrict__ info, int N, int S,
                                                            int C, double mu0, double delta, double* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) double rg_lds[];
    constexpr int NR = 7 + NI, QN = NR * (NR + 1) / 2;
    const RgDims D = rg_dims_intr<NI>(C);
    double* sY = rg_lds;     // first [Y; z^T] ...
    double* sJ = rg_lds;     // ... then, in the same LDS, the camera rows
    const int lane = threadIdx.x & 63, tl = blockIdx.x;
    const int s = uni((int)tile[4 * tl]), lo = uni((int)tile[4 * tl + 1]), n = uni((int)tile[4 * tl + 2]);
    if (s < 0 || s >= S || lo < 0 || n < 0 || n > RG_TILE || lo + n > N) return;
    if (ctl[4 * s] != 0) return;
    const double mu = ctl[4 * s + 1] == 0 ? mu0 : info[(size_t)s * RG_INFO + 2];
    const double* cm = cams + (size_t)s * C * RG_CAM;
    const int32_t* sl = slot + (size_t)s * C;
    const int32_t* isl = islot + (size_t)s * C;
    if (rg_col<NI>(sl, isl, C) > D.M) return;
    for (int r = 0; r < D.Mp; ++r)
        for (int k = 0; k < 3; ++k) sY[r * RG_LD + 3 * lane + k] = 0.0;
    double rr = 0.0;
    const int i = lo + lane;                 // read by the lanes < n alone
    double Xp[3] = {0.0, 0.0, 0.0};
    const double* uvp = uv + (size_t)i * C * 2;
    if (lane < n) {
        for (int k = 0; k < 3; ++k) Xp[k] = X[(size_t)i * 3 + k];
        RgPoint P;
        rg_point<LOSS>(cm, uvp, C, Xp, mu, delta, P);
        rr = P.rr;
        double z[3];
        rg_fwd(P.l, P.g, z);
        for (int k = 0; k < 3; ++k) sY[D.M * RG_LD + 3 * lane + k] = z[k];
        int off = 0;
        for (int c = 0; c < C; ++c) {
            const bool pf = sl[c] >= 0, jf = isl[c] >= 0;
            int row = off;
            off += (pf ? 6 : 0) + (jf ? NI : 0);
            const double ou = uvp[2 * c], ov = uvp[2 * c + 1];
            if (!(pf || jf) || !(ou == ou)) continue;
            RgObsI<NI> o;
            rg_obs_intr<LOSS, NI>(cm + c * RG_CAM, Xp, ou, ov, delta, o);
            auto put = [&](int r, double xu, double xv) {
                const double w[3] = {xu * o.a[0] + xv * o.b[0], xu * o.a[1] + xv * o.b[1], xu * o.a[2] + xv * o.b[2]};
                double y[3];
                rg_fwd(P.l, w, y);
                for (int k = 0; k < 3; ++k) sY[r * RG_LD + 3 * lane + k] = y[k];
            };
            if (pf) {
                double ju[6], jv[6];
                rg_cam_rows(o, ju, jv);
#pragma unroll
                for (int r = 0; r < 6; ++r) put(row + r, ju[r], jv[r]);
                row += 6;
            }
            if (jf) {
#pragma unroll
                for (int r = 0; r < NI; ++r) put(row + r, o.iu[r], o.iv[r]);
            }
        }
    }
    MVMC_WAVE_SYNC();
    double* out = part + (size_t)tl * D.PD;
    const int li = lane & 15, lq = lane >> 4;
    for (int bi = 0; bi < D.nb; ++bi)
        for (int bj = 0; bj <= bi; ++bj) {
            double* ob = out + (bi * (bi + 1) / 2 + bj) * 256;
            // lane l gives A[i = l % 16][k = l / 16] and B[k = l / 16][j = l % 16], receives D[i = l / 16 + 4 v][j = l % 16]
            const double* ra = sY + (16 * bi + li) * RG_LD + lq;
            const double* rb = sY + (16 * bj + li) * RG_LD + lq;
            rg_d4 acc = {0.0, 0.0, 0.0, 0.0};
            for (int k0 = 0; k0 < 3 * RG_TILE; k0 += 4) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ra[k0], rb[k0], acc, 0, 0, 0);
#pragma unroll
            for (int v = 0; v < 4; ++v) ob[(lq + 4 * v) * 16 + li] = acc[v];
        }
    // second pass over the same LDS: per camera the rows (J_c; r), NR rows of RG_LDJ
    MVMC_WAVE_SYNC();
    for (int r = 0; r < NR * C; ++r) { sJ[r * RG_LDJ + 2 * lane] = 0.0; sJ[r * RG_LDJ + 2 * lane + 1] = 0.0; }
    if (lane < n) {
        for (int c = 0; c < C; ++c) {
            const bool pf = sl[c] >= 0, jf = isl[c] >= 0;
            const double ou = uvp[2 * c], ov = uvp[2 * c + 1];
            if (!(pf || jf) || !(ou == ou)) continue;
            RgObsI<NI> o;
            rg_obs_intr<LOSS, NI>(cm + c * RG_CAM, Xp, ou, ov, delta, o);
            double* row = sJ + NR * c * RG_LDJ + 2 * lane;
            if (pf) {
                double ju[6], jv[6];
                rg_cam_rows(o, ju, jv);
#pragma unroll
                for (int r = 0; r < 6; ++r) { row[r * RG_LDJ] = ju[r]; row[r * RG_LDJ + 1] = jv[r]; }
            }
            if (jf) {
#pragma unroll
                for (int r = 0; r < NI; ++r) { row[(6 + r) * RG_LDJ] = o.iu[r]; row[(6 + r) * RG_LDJ + 1] = o.iv[r]; }
            }
            row[(NR - 1) * RG_LDJ] = o.ru;
            row[(NR - 1) * RG_LDJ + 1] = o.rv;
        }
    }
    MVMC_WAVE_SYNC();
    for (int e = lane; e < QN * C; e += 64) {
        const int c = e / QN, w = e - QN * c;
        int a = 0, rem = w;
        while (rem >= NR - a) { rem -= NR - a; ++a; }
        const double* ra = sJ + (NR * c + a) * RG_LDJ;
        const double* rb = sJ + (NR * c + a + rem) * RG_LDJ;
        double acc = 0.0;
        for (int k = 0; k < 2 * RG_TILE; ++k) acc = fma(ra[k], rb[k], acc);
        out[D.nblk * 256 + e] = acc;
    }
    double E = wave_sum(rr);
    if constexpr (LOSS == MVMC_RIG_LOSS_NONE) E = 0.5 * E;
    if (lane == 0) out[D.nblk * 256 + QN * C] = E;
}

template <int NI>
__global__ void __launch_bounds__(256) rig_solve_intr_kernel(const int32_t* __restrict__ seq, const int32_t* __restrict__ slot,
                                                             const int32_t* __restrict__ islot, const double* __restrict__ cams,
                                                             double* __restrict__ camt, int32_t* __restrict__ ctl,
                                                             double* __restrict__ info, const double* __restrict__ part,
                                                             double* __restrict__ red, const double* __restrict__ K0, int T, int C,
                                                             int max_iter, double mu0, double sf, double sc) {
    extern __shared__ __attribute__((aligned(16))) double rg_lds[];
    __shared__ int bad;
    __shared__ int ccam[6 * (MVMC_RIG_MAX_CAMS - 1) + NI * MVMC_RIG_MAX_CAMS], crow[6 * (MVMC_RIG_MAX_CAMS - 1) + NI * MVMC_RIG_MAX_CAMS];
    constexpr int NR = 7 + NI, QN = NR * (NR + 1) / 2;
    const RgDims D = rg_dims_intr<NI>(C);
    const int M = D.M;
    double* sP = rg_lds;
    double* sS = sP + D.PD;
    double* sg = sS + M * M;
    double* sd = sg + M;
    double* sgc = sd + M;
    double* sdU = sgc + M;
    double* spw = sdU + M;       // the prior's diagonal term of the column
    double* ssx = spw + M;       // the column's scale in |d|_inf: 1, and 1 / fx for dcx, dcy
    const int s = blockIdx.x, tid = threadIdx.x;
    if (ctl[4 * s] != 0) return;
    const int it = ctl[4 * s + 1];
    const int t0 = seq[4 * s], nt = seq[4 * s + 1];
    if (t0 < 0 || nt < 0 || t0 + nt > T) return;
    const double* cm = cams + (size_t)s * C * RG_CAM;
    const double* k0 = K0 + (size_t)s * C * 3;
    const int32_t* sl = slot + (size_t)s * C;
    const int32_t* isl = islot + (size_t)s * C;
    const int Ms = rg_col<NI>(sl, isl, C);
    if (Ms > M) return;
    for (int e = tid; e < D.PD; e += 256) {
        double acc = 0.0;
        for (int t = 0; t < nt; ++t) acc += part[(size_t)(t0 + t) * D.PD + e];
        sP[e] = acc;
    }
    if (tid == 0) {
        bad = 0;
        int col = 0;
        for (int c = 0; c < C; ++c) {
            if (sl[c] >= 0)
                for (int r = 0; r < 6; ++r) { ccam[col] = c; crow[col] = r; ++col; }
            if (isl[c] >= 0)
                for (int r = 0; r < NI; ++r) { ccam[col] = c; crow[col] = 6 + r; ++col; }
        }
        for (; col < M; ++col) { ccam[col] = -1; crow[col] = 0; }
    }
    __syncthreads();
    double* inf = info + (size_t)s * RG_INFO;
    int ref = -1;
    for (int c = C - 1; c >= 0; --c)
        if (sl[c] >= 0) ref = c;
    const double mu = it == 0 ? mu0 : inf[2];
    const double* sC = sP + D.nblk * 256;
    if (it == 0 && tid == 0) {
        const double E = sC[QN * C] + rg_prior<NI>(cm, k0, isl, C, sf, sc);
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
    auto q = [&](int a, int b) { return a * NR - a * (a - 1) / 2 + (b - a); };   // a <= b < NR
    double* rd = red + (size_t)s * D.RD;
    for (int i = tid; i < M; i += 256) {
        const int c = ccam[i], a = crow[i];
        double gc = 0.0, dU = 0.0, pw = 0.0, sx = 1.0, g = 0.0;
        if (c >= 0) {
            const double* K = cm + c * RG_CAM;
            double pg = 0.0;
            if (a == 6) { pw = 1.0 / (sf * sf); pg = log(K[0] / k0[3 * c]) / sf / sf; }
            else if (a > 6) { pw = 1.0 / (sc * sc); pg = (K[a == 7 ? 2 : 5] - k0[3 * c + a - 6]) / sc / sc; sx = 1.0 / K[0]; }
            gc = sC[QN * c + q(a, NR - 1)] + pg;
            dU = sC[QN * c + q(a, a)] + pw;
            g = gc - Tm(M, i);
        }
        sgc[i] = gc; sdU[i] = dU; spw[i] = pw; ssx[i] = sx; sg[i] = g;
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
                double u = sC[QN * ci + q(a < b ? a : b, a < b ? b : a)];
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
                dmax = fmax(dmax, fabs(sd[i]) * ssx[i]);
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
        if (sl[tid] >= 0) o += 6;
        if (isl[tid] >= 0 && !bad) {
            const double e = exp(sd[o]);
            co[0] = ci[0] * e; co[1] = ci[1] * e; co[4] = ci[4] * e;
            if constexpr (NI == 3) { co[2] = ci[2] + sd[o + 1]; co[5] = ci[5] + sd[o + 2]; }
        }
    }
}

template <int LOSS, int NI>
__global__ void __launch_bounds__(64) rig_backsub_intr_kernel(const double* __restrict__ X, double* __restrict__ Xt,
                                                              const double* __restrict__ uv, const int32_t* __restrict__ tile,
                                                              const int32_t* __restrict__ slot, const int32_t* __restrict__ islot,
                                                              const double* __restrict__ cams, const double* __restrict__ camt,
                                                              const int32_t* __restrict__ ctl, const double* __restrict__ info,
                                                              const double* __restrict__ red, int N, int S, int C, double delta,
                                                              double* __restrict__ part2) {
    const RgDims D = rg_dims_intr<NI>(C);
    const int lane = threadIdx.x & 63, tl = blockIdx.x;
    const int s = uni((int)tile[4 * tl]), lo = uni((int)tile[4 * tl + 1]), n = uni((int)tile[4 * tl + 2]);
    if (s < 0 || s >= S || lo < 0 || n < 0 || n > RG_TILE || lo + n > N) return;
    if (ctl[4 * s] != 0 || ctl[4 * s + 3] != 0) return;
    const double mu = info[(size_t)s * RG_INFO + 2];
    const double* cm = cams + (size_t)s * C * RG_CAM;
    const double* ct = camt + (size_t)s * C * RG_CAM;
    const int32_t* sl = slot + (size_t)s * C;
    const int32_t* isl = islot + (size_t)s * C;
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
            const bool pf = sl[c] >= 0, jf = isl[c] >= 0;
            const double* d = dc + off;
            off += (pf ? 6 : 0) + (jf ? NI : 0);
            const double ou = uvp[2 * c], ov = uvp[2 * c + 1];
            if (!(pf || jf) || !(ou == ou)) continue;
            RgObsI<NI> o;
            rg_obs_intr<LOSS, NI>(cm + c * RG_CAM, Xp, ou, ov, delta, o);
            double su = 0.0, sv = 0.0;
            if (pf) {
                double ju[6], jv[6];
                rg_cam_rows(o, ju, jv);
#pragma unroll
                for (int r = 0; r < 6; ++r) { su += ju[r] * d[r]; sv += jv[r] * d[r]; }
                d += 6;
            }
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

// rig_decide_kernel with the prior of the trial cameras in the trial cost, and the trial K taken over on acceptance
template <int NI>
__global__ void __launch_bounds__(256) rig_decide_intr_kernel(double* __restrict__ X, const double* __restrict__ Xt,
                                                              const int32_t* __restrict__ seq, const int32_t* __restrict__ slot,
                                                              const int32_t* __restrict__ islot, double* __restrict__ cams,
                                                              const double* __restrict__ camt, int32_t* __restrict__ ctl,
                                                              double* __restrict__ info, const double* __restrict__ part2,
                                                              const double* __restrict__ K0, int N, int T, int C, int max_iter, double ftol,
                                                              double xtol, double sf, double sc) {
    __shared__ double sh[8];
    __shared__ int accept;
    const int s = blockIdx.x, tid = threadIdx.x;
    if (ctl[4 * s] != 0) return;
    const int t0 = seq[4 * s], nt = seq[4 * s + 1], p0 = seq[4 * s + 2], np = seq[4 * s + 3];
    if (t0 < 0 || nt < 0 || t0 + nt > T || p0 < 0 || np < 0 || p0 + np > N) return;
    double* inf = info + (size_t)s * RG_INFO;
    const int32_t* sl = slot + (size_t)s * C;
    const int32_t* isl = islot + (size_t)s * C;
    if (rg_col<NI>(sl, isl, C) > rg_dims_intr<NI>(C).M) return;
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
                Et += rg_prior<NI>(ct, K0 + (size_t)s * C * 3, isl, C, sf, sc);
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
                        int ref = 0;
                        for (int c = C - 1; c >= 0; --c)
                            if (sl[c] >= 0) ref = c;
                        double c0[3], cr[3];
                        rg_centre(ct, c0);
                        rg_centre(ct + ref * RG_CAM, cr);
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
    const double sc_ = sh[0], c0[3] = {sh[1], sh[2], sh[3]};
    for (int i = tid; i < np; i += 256)
        for (int k = 0; k < 3; ++k) X[(size_t)(p0 + i) * 3 + k] = c0[k] + sc_ * (Xt[(size_t)(p0 + i) * 3 + k] - c0[k]);
    if (tid < C) {
        const double* ci = ct + tid * RG_CAM;
        double* co = cm + tid * RG_CAM;
        if (isl[tid] >= 0)
            for (int k = 0; k < 9; ++k) co[k] = ci[k];
        if (sl[tid] >= 0) {
            double cc[3];
            rg_centre(ci, cc);
            for (int k = 0; k < 3; ++k) cc[k] = c0[k] + sc_ * (cc[k] - c0[k]);
            for (int k = 9; k < 18; ++k) co[k] = ci[k];
            for (int r = 0; r < 3; ++r) co[18 + r] = -(ci[9 + 3 * r] * cc[0] + ci[9 + 3 * r + 1] * cc[1] + ci[9 + 3 * r + 2] * cc[2]);
        }
    }
}

template <int NI>
size_t rg_accum_lds_intr(int C) {
    const RgDims D = rg_dims_intr<NI>(C);
    const size_t a = (size_t)D.Mp * RG_LD, b = (size_t)(7 + NI) * C * RG_LDJ;
    return (a > b ? a : b) * sizeof(double);
}
template <int NI>
size_t rg_solve_lds_intr(int C) {
    const RgDims D = rg_dims_intr<NI>(C);
    return ((size_t)D.PD + (size_t)D.M * D.M + 6 * D.M) * sizeof(double);
}

bool rg_intr_ok(int n_intr, double sf, double sc) { return (n_intr == 1 || n_intr == 3) && sf > 0.0 && sc > 0.0; }   // (NaN fails)

template <int LOSS, int NI>
int rg_accumulate_intr(hipStream_t st, const double* X, const double* uv, const int32_t* tile, const int32_t* seq, const int32_t* slot,
                       const int32_t* islot, const double* cams, double* cams_trial, int32_t* ctl, double* info, const double* K0,
                       int n_points, int n_tiles, int n_seqs, int n_views, int max_iter, double mu0, double delta, double sf, double sc,
                       double* part, double* red) {
    const size_t la = rg_accum_lds_intr<NI>(n_views), ls = rg_solve_lds_intr<NI>(n_views);
    if (la > 65536 && hipFuncSetAttribute((const void*)rig_accum_intr_kernel<LOSS, NI>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)la) != hipSuccess)
        return MVMC_ERR_LAUNCH;
    if (ls > 65536 && hipFuncSetAttribute((const void*)rig_solve_intr_kernel<NI>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ls) !=
                          hipSuccess)
        return MVMC_ERR_LAUNCH;
    if (n_tiles > 0) {
        hipLaunchKernelGGL((rig_accum_intr_kernel<LOSS, NI>), dim3(n_tiles), dim3(64), la, st, X, uv, tile, slot, islot, cams, ctl, info,
                           n_points, n_seqs, n_views, mu0, delta, part);
        MVMC_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(rig_solve_intr_kernel<NI>, dim3(n_seqs), dim3(256), ls, st, seq, slot, islot, cams, cams_trial, ctl, info, part, red,
                       K0, n_tiles, n_views, max_iter, mu0, sf, sc);
    MVMC_CHECK_LAUNCH();
    return MVMC_OK;
}

template <int LOSS, int NI>
int rg_step_intr(hipStream_t st, double* X, double* X_trial, const double* uv, const int32_t* tile, const int32_t* seq, const int32_t* slot,
                 const int32_t* islot, double* cams, const double* cams_trial, int32_t* ctl, double* info, const double* red,
                 const double* K0, int n_points, int n_tiles, int n_seqs, int n_views, int max_iter, double ftol, double xtol, double delta,
                 double sf, double sc, double* part2) {
    if (n_tiles > 0) {
        hipLaunchKernelGGL((rig_backsub_intr_kernel<LOSS, NI>), dim3(n_tiles), dim3(64), 0, st, X, X_trial, uv, tile, slot, islot, cams,
                           cams_trial, ctl, info, red, n_points, n_seqs, n_views, delta, part2);
        MVMC_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(rig_decide_intr_kernel<NI>, dim3(n_seqs), dim3(256), 0, st, X, X_trial, seq, slot, islot, cams, cams_trial, ctl,
                       info, part2, K0, n_points, n_tiles, n_views, max_iter, ftol, xtol, sf, sc);
    MVMC_CHECK_LAUNCH();
    return MVMC_OK;
}

// the (loss, n_intr) instantiation of F
#define RG_INTR_DISPATCH(F, ...)                                                                                          \
    (n_intr == 1 ? (loss == MVMC_RIG_LOSS_HUBER    ? F<MVMC_RIG_LOSS_HUBER, 1>(__VA_ARGS__)                               \
                    : loss == MVMC_RIG_LOSS_CAUCHY ? F<MVMC_RIG_LOSS_CAUCHY, 1>(__VA_ARGS__)                              \
                                                   : F<MVMC_RIG_LOSS_NONE, 1>(__VA_ARGS__))                               \
                 : (loss == MVMC_RIG_LOSS_HUBER    ? F<MVMC_RIG_LOSS_HUBER, 3>(__VA_ARGS__)                               \
                    : loss == MVMC_RIG_LOSS_CAUCHY ? F<MVMC_RIG_LOSS_CAUCHY, 3>(__VA_ARGS__)                              \
                                                   : F<MVMC_RIG_LOSS_NONE, 3>(__VA_ARGS__)))

}  // namespace

extern "C" long long mvmc_rig_part_doubles_intr(int n_views, int n_intr) {
    if (n_views < 2 || n_views > MVMC_RIG_MAX_CAMS || (n_intr != 1 && n_intr != 3)) return -1;
    return n_intr == 1 ? rg_dims_intr<1>(n_views).PD : rg_dims_intr<3>(n_views).PD;
}

extern "C" long long mvmc_rig_red_doubles_intr(int n_views, int n_intr) {
    if (n_views < 2 || n_views > MVMC_RIG_MAX_CAMS || (n_intr != 1 && n_intr != 3)) return -1;
    return n_intr == 1 ? rg_dims_intr<1>(n_views).RD : rg_dims_intr<3>(n_views).RD;
}

extern "C" int mvmc_rig_accumulate_intr(const double* X, const double* uv, const int32_t* tile, const int32_t* seq, const int32_t* slot,
                                        const double* cams, double* cams_trial, int32_t* ctl, double* info, int n_points, int n_tiles,
                                        int n_seqs, int n_views, int max_iter, double mu0, int variant, double* part, double* red,
                                        int loss, double loss_px, int n_intr, const int32_t* islot, const double* K0, double focal_sigma,
                                        double centre_sigma, mvmcStream_t stream) {
    if (n_points < 0 || n_tiles < 0 || n_seqs < 0 || n_views < 2 || n_views > MVMC_RIG_MAX_CAMS || max_iter < 0 ||
        max_iter > MVMC_RIG_MAX_ITER || variant != 1 || !rg_loss_ok(loss, loss_px) || !rg_intr_ok(n_intr, focal_sigma, centre_sigma))
        return MVMC_ERR_ARG;
    if (n_seqs == 0) return MVMC_OK;
    if (!X || !uv || !tile || !seq || !slot || !cams || !cams_trial || !ctl || !info || !part || !red || !islot || !K0) return MVMC_ERR_ARG;
    return RG_INTR_DISPATCH(rg_accumulate_intr, (hipStream_t)stream, X, uv, tile, seq, slot, islot, cams, cams_trial, ctl, info, K0,
                            n_points, n_tiles, n_seqs, n_views, max_iter, mu0, loss_px, focal_sigma, centre_sigma, part, red);
}

extern "C" int mvmc_rig_step_intr(double* X, double* X_trial, const double* uv, const int32_t* tile, const int32_t* seq,
                                  const int32_t* slot, double* cams, const double* cams_trial, int32_t* ctl, double* info,
                                  const double* red, int n_points, int n_tiles, int n_seqs, int n_views, int max_iter, double ftol,
                                  double xtol, double* part2, int loss, double loss_px, int n_intr, const int32_t* islot, const double* K0,
                                  double focal_sigma, double centre_sigma, mvmcStream_t stream) {
    if (n_points < 0 || n_tiles < 0 || n_seqs < 0 || n_views < 2 || n_views > MVMC_RIG_MAX_CAMS || max_iter < 0 ||
        max_iter > MVMC_RIG_MAX_ITER || !rg_loss_ok(loss, loss_px) || !rg_intr_ok(n_intr, focal_sigma, centre_sigma))
        return MVMC_ERR_ARG;
    if (n_seqs == 0) return MVMC_OK;
    if (!X || !X_trial || !uv || !tile || !seq || !slot || !cams || !cams_trial || !ctl || !info || !red || !part2 || !islot || !K0)
        return MVMC_ERR_ARG;
    return RG_INTR_DISPATCH(rg_step_intr, (hipStream_t)stream, X, X_trial, uv, tile, seq, slot, islot, cams, cams_trial, ctl, info, red,
                            K0, n_points, n_tiles, n_seqs, n_views, max_iter, ftol, xtol, loss_px, focal_sigma, centre_sigma, part2);
}

extern "C" long long mvmc_rig_part_doubles(int n_views) {
    if (n_views < 2 || n_views > MVMC_RIG_MAX_CAMS) return -1;
    return rg_dims(n_views).PD;
}

extern "C" long long mvmc_rig_red_doubles(int n_views) {
    if (n_views < 2 || n_views > MVMC_RIG_MAX_CAMS) return -1;
    return rg_dims(n_views).RD;
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
    return rg_accumulate(X, uv, tile, seq, slot, cams, cams_trial, ctl, info, n_points, n_tiles, n_seqs, n_views, max_iter, mu0, variant,
                         part, red, MVMC_RIG_LOSS_NONE, 0.0, stream);
}

extern "C" int mvmc_rig_step(double* X, double* X_trial, const double* uv, const int32_t* tile, const int32_t* seq, const int32_t* slot,
                             double* cams, const double* cams_trial, int32_t* ctl, double* info, const double* red, int n_points,
                             int n_tiles, int n_seqs, int n_views, int max_iter, double ftol, double xtol, double* part2,
                             mvmcStream_t stream) {
    return rg_step(X, X_trial, uv, tile, seq, slot, cams, cams_trial, ctl, info, red, n_points, n_tiles, n_seqs, n_views, max_iter, ftol,
                   xtol, part2, MVMC_RIG_LOSS_NONE, 0.0, stream);
}

extern "C" int mvmc_rig_accumulate_robust(const double* X, const double* uv, const int32_t* tile, const int32_t* seq, const int32_t* slot,
                                          const double* cams, double* cams_trial, int32_t* ctl, double* info, int n_points, int n_tiles,
                                          int n_seqs, int n_views, int max_iter, double mu0, int variant, double* part, double* red,
                                          int loss, double loss_px, mvmcStream_t stream) {
    return rg_accumulate(X, uv, tile, seq, slot, cams, cams_trial, ctl, info, n_points, n_tiles, n_seqs, n_views, max_iter, mu0, variant,
                         part, red, loss, loss_px, stream);
}

extern "C" int mvmc_rig_step_robust(double* X, double* X_trial, const double* uv, const int32_t* tile, const int32_t* seq,
                                    const int32_t* slot, double* cams, const double* cams_trial, int32_t* ctl, double* info,
                                    const double* red, int n_points, int n_tiles, int n_seqs, int n_views, int max_iter, double ftol,
                                    double xtol, double* part2, int loss, double loss_px, mvmcStream_t stream) {
    return rg_step(X, X_trial, uv, tile, seq, slot, cams, cams_trial, ctl, info, red, n_points, n_tiles, n_seqs, n_views, max_iter, ftol,
                   xtol, part2, loss, loss_px, stream);
}

extern "C" int mvmc_rig_weights(const double* X, const double* uv, const int32_t* tile, const double* cams, int n_points, int n_tiles,
                                int n_seqs, int n_views, int loss, double loss_px, double* w, mvmcStream_t stream) {
    if (n_points < 0 || n_tiles < 0 || n_seqs < 0 || n_views < 2 || n_views > MVMC_RIG_MAX_CAMS || !rg_loss_ok(loss, loss_px))
        return MVMC_ERR_ARG;
    if (n_tiles == 0 || n_seqs == 0) return MVMC_OK;
    if (!X || !uv || !tile || !cams || !w) return MVMC_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (loss == MVMC_RIG_LOSS_HUBER)
        hipLaunchKernelGGL(rig_weights_kernel<MVMC_RIG_LOSS_HUBER>, dim3(n_tiles), dim3(64), 0, st, X, uv, tile, cams, n_points, n_seqs,
                           n_views, loss_px, w);
    else if (loss == MVMC_RIG_LOSS_CAUCHY)
        hipLaunchKernelGGL(rig_weights_kernel<MVMC_RIG_LOSS_CAUCHY>, dim3(n_tiles), dim3(64), 0, st, X, uv, tile, cams, n_points, n_seqs,
                           n_views, loss_px, w);
    else
        hipLaunchKernelGGL(rig_weights_kernel<MVMC_RIG_LOSS_NONE>, dim3(n_tiles), dim3(64), 0, st, X, uv, tile, cams, n_points, n_seqs,
                           n_views, loss_px, w);
    MVMC_CHECK_LAUNCH();
    return MVMC_OK;
}
