// Lens distortion at the door of the pipeline: raw detector pixels -> pinhole pixels (mvmc_lens_undistort) and back
// (mvmc_lens_distort).  No counterpart in the reference, whose only projection is project_3d_points_to_image_plane_without_distortion.
// One pass over the (F, C, n_points, 3) keypoint triples; everything downstream stays a pinhole pipeline.  tests/lens_np.py restates
// the models, the Newton inverse and the accept rule in NumPy.
//
// Layout.  A WAVE owns a frame (four frames in flight per 256-lane workgroup, frames taken grid-stride), so every dropped[f, c] is
// written once by one wave from ballots -- no atomics, bit-identical from run to run.  Lane l of a chunk takes triple base + l of the
// frame: a wave instruction moves 64 consecutive triples, 768 contiguous bytes in float32 as one 12-byte load per lane (the triples
// are 4-byte aligned only; a 16-byte vector would straddle them).  The frame's lens rows (C x 128 B) are staged in the wave's slice of
// LDS and staged again only when the wave's next frame names another rig.  The waves of a workgroup never meet: no workgroup barrier.
// The model is read per lane but branched on OUTSIDE the Newton loops; lanes of one camera agree, and a rig with one model for all
// cameras runs one loop per chunk.  The loops have a fixed trip bound; they leave early only when a ballot says no lane still iterates.
#include "mvmc_common.h"

namespace {

constexpr int kLensWaves = 4;
constexpr double kLensStop = 1e-13;

template <typename T>
struct LensTri {
    T x, y, s;
};

struct LensRow {
    int model;
    double fx, fy, cx, cy, skew, k[8];
};

// Brown-Conrady forward map at (x, y) with its Jacobian (symmetric: j12 = j21).  k = {k1, k2, p1, p2, k3, k4, k5, k6}.
__device__ __forceinline__ void brown_eval(const double* k, double x, double y, double& X, double& Y, double& j11, double& j12,
                                           double& j22, double& rad) {
    const double k1 = k[0], k2 = k[1], p1 = k[2], p2 = k[3], k3 = k[4], k4 = k[5], k5 = k[6], k6 = k[7];
    const double xx = x * x, yy = y * y, xy = x * y, r2 = xx + yy;
    const double num = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3));
    const double den = 1.0 + r2 * (k4 + r2 * (k5 + r2 * k6));
    const double nump = k1 + r2 * (2.0 * k2 + 3.0 * k3 * r2);
    const double denp = k4 + r2 * (2.0 * k5 + 3.0 * k6 * r2);
    const double iden = 1.0 / den;
    rad = num * iden;
    const double radp = (nump - rad * denp) * iden;   // d rad / d r^2
    X = x * rad + 2.0 * p1 * xy + p2 * (r2 + 2.0 * xx);
    Y = y * rad + p1 * (r2 + 2.0 * yy) + 2.0 * p2 * xy;
    j11 = rad + 2.0 * xx * radp + 2.0 * p1 * y + 6.0 * p2 * x;
    j12 = 2.0 * xy * radp + 2.0 * p1 * x + 2.0 * p2 * y;
    j22 = rad + 2.0 * yy * radp + 6.0 * p1 * y + 2.0 * p2 * x;
}

// Kannala-Brandt: theta_d(theta) and its derivative.  k = {k1, k2, k3, k4}.
__device__ __forceinline__ void fisheye_eval(const double* k, double th, double& thd, double& dthd) {
    const double t2 = th * th;
    thd = th * (1.0 + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3]))));
    dthd = 1.0 + t2 * (3.0 * k[0] + t2 * (5.0 * k[1] + t2 * (7.0 * k[2] + t2 * 9.0 * k[3])));
}

// (xd, yd) distorted normalised -> (x, y) ideal normalised; false = no valid pre-image (the accept rule of include/mvmc.h).
__device__ __forceinline__ bool brown_inverse(const double* k, double xd, double yd, double& x, double& y) {
    x = xd;
    y = yd;
    bool ok = true, conv = false;
    double X, Y, j11, j12, j22, rad;
    for (int it = 0; it < MVMC_LENS_MAX_ITER; ++it) {
        brown_eval(k, x, y, X, Y, j11, j12, j22, rad);
        if (!conv) {
            const double det = j11 * j22 - j12 * j12;
            ok = ok && det > 0.0 && rad > 0.0;
            const double f1 = X - xd, f2 = Y - yd, idet = 1.0 / det;
            const double dx = -(j22 * f1 - j12 * f2) * idet, dy = -(j11 * f2 - j12 * f1) * idet;
            x += dx;
            y += dy;
            conv = fabs(dx) + fabs(dy) <= kLensStop * (1.0 + fabs(x) + fabs(y));
        }
        if (__ballot(ok && !conv) == 0ull) break;   // wave-uniform: every lane has converged or is rejected whatever follows
    }
    brown_eval(k, x, y, X, Y, j11, j12, j22, rad);
    return ok && conv && j11 * j22 - j12 * j12 > 0.0 && rad > 0.0 && isfinite(x) && isfinite(y);
}

__device__ __forceinline__ bool fisheye_inverse(const double* k, double xd, double yd, double& x, double& y) {
    const double thd = sqrt(xd * xd + yd * yd);
    double th = thd, g, dg;
    bool ok = true, conv = false;
    for (int it = 0; it < MVMC_LENS_MAX_ITER; ++it) {
        fisheye_eval(k, th, g, dg);
        if (!conv) {
            ok = ok && dg > 0.0;
            const double d = -(g - thd) / dg;
            th += d;
            conv = fabs(d) <= kLensStop * (1.0 + fabs(th));
        }
        if (__ballot(ok && !conv) == 0ull) break;
    }
    fisheye_eval(k, th, g, dg);
    const double scale = thd > 0.0 ? tan(th) / thd : 1.0;
    x = xd * scale;
    y = yd * scale;
    return ok && conv && dg > 0.0 && th >= 0.0 && th < MVMC_LENS_FISHEYE_MAX_THETA && isfinite(x) && isfinite(y);
}

template <typename T, bool INVERSE>
__global__ __launch_bounds__(64 * kLensWaves) void lens_kernel(const LensTri<T>* in, int F, int C, int n_points, const double* lens,
                                                               const int32_t* rig_of_frame, int R, LensTri<T>* out,
                                                               int32_t* dropped) {
    extern __shared__ double s_lens[];   // (kLensWaves, C, MVMC_LENS_DOUBLES)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double* L = s_lens + (size_t)wave * C * MVMC_LENS_DOUBLES;
    const int total = C * n_points;
    int staged = -1;
    for (long long f = (long long)blockIdx.x * kLensWaves + wave; f < F; f += (long long)gridDim.x * kLensWaves) {
        const int rig = __builtin_amdgcn_readfirstlane(rig_of_frame ? rig_of_frame[f] : 0);
        const LensTri<T>* src = in + (size_t)f * total;
        LensTri<T>* dst = out + (size_t)f * total;
        int32_t* drop_row = dropped + (size_t)f * C;
        if (rig < 0 || rig >= R) {   // no calibration is read: the frame comes out empty and says so
            const LensTri<T> z = {T(0), T(0), T(0)};
            for (int i = lane; i < total; i += 64) dst[i] = z;
            for (int c = lane; c < C; c += 64) drop_row[c] = -1;
            continue;
        }
        if (rig != staged) {
            MVMC_WAVE_SYNC();
            const double* row = lens + (size_t)rig * C * MVMC_LENS_DOUBLES;
            for (int e = lane; e < C * MVMC_LENS_DOUBLES; e += 64) L[e] = row[e];
            MVMC_WAVE_SYNC();
            staged = rig;
        }
        int cur = 0, cnt = 0;   // the camera whose count is open, and the count (wave-uniform)
        for (int base = 0; base < total; base += 64) {
            const int i = base + lane;
            const bool active = i < total;
            const int c = active ? i / n_points : 0;
            bool drop = false;
            if (active) {
                const LensTri<T> t = src[i];
                LensTri<T> o = t;
                const double* row = L + c * MVMC_LENS_DOUBLES;
                const int model = (int)row[0];
                if ((model == MVMC_LENS_BROWN || model == MVMC_LENS_FISHEYE) && t.s > T(0)) {
                    const double fx = row[1], fy = row[2], cx = row[3], cy = row[4], skew = row[5];
                    const double* k = row + 6;
                    const double yd = ((double)t.y - cy) / fy, xd = ((double)t.x - cx - skew * yd) / fx;
                    double x, y;
                    bool ok = true;
                    if (INVERSE) {
                        if (model == MVMC_LENS_BROWN)
                            ok = brown_inverse(k, xd, yd, x, y);
                        else
                            ok = fisheye_inverse(k, xd, yd, x, y);
                    } else if (model == MVMC_LENS_BROWN) {
                        double j11, j12, j22, rad;
                        brown_eval(k, xd, yd, x, y, j11, j12, j22, rad);
                    } else {
                        const double r = sqrt(xd * xd + yd * yd);
                        double thd, dthd;
                        fisheye_eval(k, atan(r), thd, dthd);
                        const double scale = r > 0.0 ? thd / r : 1.0;
                        x = xd * scale;
                        y = yd * scale;
                    }
                    if (ok) {
                        o.x = (T)(fx * x + skew * y + cx);
                        o.y = (T)(fy * y + cy);
                    } else {
                        o.x = o.y = o.s = T(0);
                        drop = true;
                    }
                }
                dst[i] = o;
            }
            const int c_hi = (min(base + 63, total - 1)) / n_points;
            for (int cc = base / n_points; cc <= c_hi; ++cc) {
                const int n = __popcll(__ballot(drop && c == cc));
                if (cc != cur) {
                    if (lane == 0) drop_row[cur] = cnt;
                    cur = cc;
                    cnt = 0;
                }
                cnt += n;
            }
        }
        if (lane == 0) drop_row[cur] = cnt;
    }
}

template <bool INVERSE>
int lens_launch(const void* kps_in, int dtype, int n_frames, int n_views, int n_points, const double* lens, const int32_t* rig_of_frame,
                int n_rigs, void* kps_out, int32_t* dropped, mvmcStream_t stream) {
    if (!kps_in || !kps_out || !lens || !dropped) return MVMC_ERR_ARG;
    if (dtype != MVMC_F32 && dtype != MVMC_F64) return MVMC_ERR_ARG;
    if (n_frames < 0 || n_views <= 0 || n_points <= 0 || n_rigs < 1) return MVMC_ERR_ARG;
    if ((long long)n_views * n_points > 0x7fffffffll) return MVMC_ERR_ARG;
    if (n_frames == 0) return MVMC_OK;
    const size_t shm = (size_t)kLensWaves * n_views * MVMC_LENS_DOUBLES * sizeof(double);
    if (shm > 64 * 1024) return MVMC_ERR_UNSUPPORTED;
    const long long want = ((long long)n_frames + kLensWaves - 1) / kLensWaves;
    const dim3 grid((unsigned)(want < 2048 ? want : 2048)), block(64 * kLensWaves);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == MVMC_F32)
        hipLaunchKernelGGL((lens_kernel<float, INVERSE>), grid, block, shm, s, (const LensTri<float>*)kps_in, n_frames, n_views,
                           n_points, lens, rig_of_frame, n_rigs, (LensTri<float>*)kps_out, dropped);
    else
        hipLaunchKernelGGL((lens_kernel<double, INVERSE>), grid, block, shm, s, (const LensTri<double>*)kps_in, n_frames, n_views,
                           n_points, lens, rig_of_frame, n_rigs, (LensTri<double>*)kps_out, dropped);
    MVMC_CHECK_LAUNCH();
    return MVMC_OK;
}

}  // namespace

extern "C" int mvmc_lens_undistort(const void* kps_in, int dtype, int n_frames, int n_views, int n_points, const double* lens,
                                   const int32_t* rig_of_frame, int n_rigs, void* kps_out, int32_t* dropped, mvmcStream_t stream) {
    return lens_launch<true>(kps_in, dtype, n_frames, n_views, n_points, lens, rig_of_frame, n_rigs, kps_out, dropped, stream);
}

extern "C" int mvmc_lens_distort(const void* kps_in, int dtype, int n_frames, int n_views, int n_points, const double* lens,
                                 const int32_t* rig_of_frame, int n_rigs, void* kps_out, int32_t* dropped, mvmcStream_t stream) {
    return lens_launch<false>(kps_in, dtype, n_frames, n_views, n_points, lens, rig_of_frame, n_rigs, kps_out, dropped, stream);
}
