// The DLT of one point (TR-1/TR-2), shared by the triangulation kernels (mvmc_geom.hip) and the rig refinement's start values
// (mvmc_rigfit.hip).
#pragma once
#include "mvmc_common.h"

// ------------------------------------------------------------------------------------------------
// DLT: one thread per (problem, joint).  The 2V x 4 system is reduced to its 4x4 normal matrix in
// fp64 registers and the null vector is the eigenvector of the smallest eigenvalue (== last right
// singular vector of A, mv_math_util.py:235-236): inverse iteration on L D L^T; where the spectral gap is
// small or a pivot vanishes, the smallest eigenvalue by cyclic Jacobi and the iteration shifted to it.
// ------------------------------------------------------------------------------------------------
// Upper triangle of a symmetric 4 x 4 matrix: entry (r, c), r <= c, at index U4(r, c) of ten doubles.
__host__ __device__ constexpr int U4(int r, int c) { return r <= c ? r * 4 - r * (r - 1) / 2 + (c - r) : c * 4 - c * (c - 1) / 2 + (r - c); }
// One Jacobi rotation (P, Q) of the cyclic sweep, EIGENVALUES ONLY (no eigenvector accumulation: ten doubles of state where the matrix
// pair of the first version held thirty-two -- that fallback alone took the kernel from 82 to 164 VGPRs, i.e. from six waves per SIMD
// to three; the eigenvector now comes from two or three inverse iterations shifted to the eigenvalue found here).
template <int P, int Q>
__device__ __forceinline__ void jacobi_rot4_ev(double (&b)[10]) {
    const double apq = b[U4(P, Q)];
    if (fabs(apq) < 1e-300) return;
    const double theta = (b[U4(Q, Q)] - b[U4(P, P)]) / (2.0 * apq);
    const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k == P || k == Q) continue;
        const double akp = b[U4(k, P)], akq = b[U4(k, Q)];
        b[U4(k, P)] = c * akp - s * akq;
        b[U4(k, Q)] = s * akp + c * akq;
    }
    b[U4(P, P)] -= t * apq;
    b[U4(Q, Q)] += t * apq;
    b[U4(P, Q)] = 0.0;
}

// One triangulated point from the views `get(v, kp, Pc)` hands out (v = 0 .. V-1; false = no such member): kp <- {x, y, score},
// Pc -> the view's 3x4 projection.  out[0..2] = X, out[3] = mean score of the views used; NaN when the cluster is empty.
// mv_math_util.py:152-187 (triangulate_point_groups_from_multiple_views_linear) + :215-240 (the DLT of one point).
// VU > 0: the view loops are unrolled VU times behind `v < V` tests (V <= VU), for callers whose `get` serves view v out of registers.
template <int VU = 0, typename Get>
__device__ __forceinline__ void dlt_point(int V, double min_score, Get get, double* __restrict__ o) {
    // upper triangle of the normal matrix A^T A (rows r1 = x P_3 - P_1, r2 = y P_3 - P_2 of every view used).  ONE pass over the views in
    // the common case: the views with score >= min_score are accumulated while all views are counted; only a point that fewer than
    // two such views see ("< 2 valid views -> resort to all views", mv_math_util.py:177-182) is accumulated again over all of them.
    // (The first version counted in a pass of its own: the members, slots and keypoints of every view were read twice.)
    double a00, a01, a02, a03, a11, a12, a13, a22, a23, a33;
    double ssum = 0.0;
    int nused = 0, n_all = 0, n_ok = 0;
    auto accumulate = [&](bool use_all) {
    a00 = 0.0; a01 = 0.0; a02 = 0.0; a03 = 0.0; a11 = 0.0; a12 = 0.0; a13 = 0.0; a22 = 0.0; a23 = 0.0; a33 = 0.0;
    ssum = 0.0; nused = 0; n_all = 0; n_ok = 0;
    auto view = [&](int v) {
        double kp[3]; const double* Pc;
        if (!get(v, kp, Pc)) return;
        const double x = kp[0], y = kp[1], sc = kp[2];
        ++n_all;
        const bool ok = sc >= min_score;
        n_ok += ok ? 1 : 0;
        if (!use_all && !ok) return;
        const double p0 = x * Pc[8] - Pc[0], p1 = x * Pc[9] - Pc[1], p2 = x * Pc[10] - Pc[2], p3 = x * Pc[11] - Pc[3];
        const double q0 = y * Pc[8] - Pc[4], q1 = y * Pc[9] - Pc[5], q2 = y * Pc[10] - Pc[6], q3 = y * Pc[11] - Pc[7];
        // two fused multiply-adds per entry (the sum p p + q q + a in one chain: a third fewer instructions than product, fma, add)
        a00 = fma(p0, p0, fma(q0, q0, a00)); a01 = fma(p0, p1, fma(q0, q1, a01)); a02 = fma(p0, p2, fma(q0, q2, a02));
        a03 = fma(p0, p3, fma(q0, q3, a03)); a11 = fma(p1, p1, fma(q1, q1, a11)); a12 = fma(p1, p2, fma(q1, q2, a12));
        a13 = fma(p1, p3, fma(q1, q3, a13)); a22 = fma(p2, p2, fma(q2, q2, a22)); a23 = fma(p2, p3, fma(q2, q3, a23));
        a33 = fma(p3, p3, fma(q3, q3, a33));
        ssum += sc;
        ++nused;
    };
    if constexpr (VU > 0) {
#pragma unroll
        for (int v = 0; v < VU; ++v)
            if (v < V) view(v);
    } else {
        for (int v = 0; v < V; ++v) view(v);
    }
    };
    accumulate(false);
    if (n_all == 0) {
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
        o[0] = o[1] = o[2] = o[3] = nan;
        return;
    }
    const bool use_all = n_ok < 2;
    if (use_all) accumulate(true);
    // The right singular vector of the smallest singular value (mv_math_util.py:152-160: SVD of the 2 nv x 4 system, last row of V^T) =
    // the eigenvector of the smallest eigenvalue of the normal matrix a.  Inverse iteration on a = L D L^T started from e4: the first
    // iterate is L^-T e4, i.e. the inhomogeneous least-squares point (X, 1); every further solve multiplies the error by
    // lambda_min / lambda_2 (~1e-5 for pixel noise against a real baseline), so three to five solves reach 1e-13 -- ~300 flops where
    // the cyclic Jacobi sweeps this replaces took ~3,000 and left the kernel ALU bound at 13 TFLOP/s.  A point
    // seen by fewer than two views has a rank-deficient matrix (a pivot vanishes): the Jacobi path below keeps handling those.
    const double tr = a00 + a11 + a22 + a33;
    double e0 = 0.0, e1 = 0.0, e2 = 0.0, e3 = 1.0;
    // inverse iteration on (a - sigma I) = L D L^T from the start vector e; false = a pivot vanished or the iterates did not settle
    // (reciprocals by v_rcp_f64 + two Newton steps, ~1 ulp: the factors and the normalisation only steer an iteration whose fixed point
    // does not depend on them, and an IEEE division is ~28 dependent instructions -- a dozen of them were 40 % of a point's instructions)
    // -> 0 settled, 1 not settled after max_it solves, 2 a pivot vanished (no solve was made: e is untouched)
    auto inverse_iteration = [&](double sigma, int max_it) -> int {
        const double floor_ = 1e-13 * tr;
        const double d0 = a00 - sigma, i0 = fast_rcp64(d0);
        const double l10 = a01 * i0, l20 = a02 * i0, l30 = a03 * i0;
        const double d1 = (a11 - sigma) - l10 * a01, i1 = fast_rcp64(d1);
        const double l21 = (a12 - l20 * a01) * i1, l31 = (a13 - l30 * a01) * i1;
        const double d2 = (a22 - sigma) - l20 * a02 - l21 * l21 * d1, i2 = fast_rcp64(d2);
        const double l32 = (a23 - l30 * a02 - l31 * l21 * d1) * i2;
        double d3 = (a33 - sigma) - l30 * a03 - l31 * l31 * d1 - l32 * l32 * d2;
        if (!(d0 > floor_ && d1 > floor_ && d2 > floor_)) return 2;
        // (the last pivot is ~lambda_min - sigma: rounding may push it to zero or below for consistent observations; its size only scales
        // the iterates, their direction comes from L)
        const double tiny = 1e-30 * tr + 1e-300;
        if (!(d3 > tiny)) d3 = tiny;
        const double i3 = fast_rcp64(d3);
        double x0 = e0, x1 = e1, x2 = e2, x3 = e3;
        bool conv = false;
        double ch_prev = 1.0;
        for (int it = 0; it < max_it; ++it) {
            // L y = x;  z = y / D;  L^T w = z
            const double y0 = x0, y1 = x1 - l10 * y0, y2 = x2 - l20 * y0 - l21 * y1, y3 = x3 - l30 * y0 - l31 * y1 - l32 * y2;
            const double w3 = y3 * i3;
            const double w2 = y2 * i2 - l32 * w3;
            const double w1 = y1 * i1 - l21 * w2 - l31 * w3;
            const double w0 = y0 * i0 - l10 * w1 - l20 * w2 - l30 * w3;
            // normalised by the component of largest magnitude (sign included): converged iterates repeat
            double m = w0;
            if (fabs(w1) > fabs(m)) m = w1;
            if (fabs(w2) > fabs(m)) m = w2;
            if (fabs(w3) > fabs(m)) m = w3;
            const double inv = fast_rcp64(m);   // (the bare v_rcp_f64 will not do although the factor only scales the iterate: its error,
                                                // ~1e-8 and not a smooth function of m, keeps consecutive iterates 1e-9 apart for ever:
                                                // every point then fell through to the Jacobi path, 6.3 ms instead of 1.2)
            const double n0 = w0 * inv, n1 = w1 * inv, n2 = w2 * inv, n3 = w3 * inv;
            const double ch = fmax(fmax(fabs(n0 - x0), fabs(n1 - x1)), fmax(fabs(n2 - x2), fabs(n3 - x3)));
            x0 = n0; x1 = n1; x2 = n2; x3 = n3;
            // settled: the iterate repeats to 1e-13 -- or, the changes shrinking geometrically (by lambda_min / lambda_2 per solve), the
            // NEXT change would: ch (ch / ch_prev) <= 1e-13 with the ratio itself below 1e-3.  The second test saves the solve that
            // only confirms (three solves instead of four at the usual gap of ~1e-5); the iterate it stops at is within that product of
            // the fixed point.
            if (it > 0 && (ch <= 1e-13 || (it > 1 && ch <= 1e-3 * ch_prev && ch * ch <= 1e-13 * ch_prev))) { conv = true; break; }
            ch_prev = ch;
        }
        e0 = x0; e1 = x1; e2 = x2; e3 = x3;
        return conv ? 0 : 1;
    };
    // not settled after eight solves = a small spectral gap (clusters of mismatched poses, gross outliers: lambda_min / lambda_2 > ~0.03;
    // 15 % of the points of the Shelf clusters, none of the synthetic ones), or a vanished pivot: the smallest eigenvalue by cyclic
    // Jacobi on the upper triangle, then the same iteration shifted to just below it -- the error then shrinks by
    // 1e-14 tr / (lambda_2 - lambda_min) per solve, whatever the ratio of the two
    if (inverse_iteration(0.0, 8) != 0) {
        double b[10] = {a00, a01, a02, a03, a11, a12, a13, a22, a23, a33};
        for (int sweep = 0; sweep < 16; ++sweep) {
            const double off = b[1] * b[1] + b[2] * b[2] + b[3] * b[3] + b[5] * b[5] + b[6] * b[6] + b[8] * b[8];
            if (off <= 1e-36 * tr * tr) break;
            jacobi_rot4_ev<0, 1>(b); jacobi_rot4_ev<0, 2>(b); jacobi_rot4_ev<0, 3>(b);
            jacobi_rot4_ev<1, 2>(b); jacobi_rot4_ev<1, 3>(b); jacobi_rot4_ev<2, 3>(b);
        }
        const double lmin = fmin(fmin(b[0], b[4]), fmin(b[7], b[9]));
        accumulate(use_all);   // (the matrix again, from the views: keeping it live across the sweeps would cost twenty registers of the hot path's budget)
        e0 = 0.0; e1 = 0.0; e2 = 0.0; e3 = 1.0;
        // A pivot that vanishes even in the shifted matrix = the null space has more than one dimension (a point one view sees, two
        // views on one line of sight): the reference returns whichever null vector LAPACK happens to produce, there is no point to
        // agree on -- NaN, never the start vector (0, 0, 0, 1) dressed up as the point (0, 0, 0)
        const int st = inverse_iteration(lmin - 1e-14 * tr, 8);
        if (st == 2 || !(e3 == e3)) { e0 = e1 = e2 = 0.0; e3 = 0.0; }   // (0 / 0 below gives NaN)
    }
    const double rw = 1.0 / e3;     // (one IEEE division; the three quotients differ from e / e3 by an ulp at most)
    o[0] = e0 * rw; o[1] = e1 * rw; o[2] = e2 * rw;
    o[3] = ssum / (double)nused;
}
