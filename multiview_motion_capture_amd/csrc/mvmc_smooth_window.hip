// Fixed-lag smoothing of live sessions (multiview_motion_capture_amd/live_smoothing.py; algorithm restated in tests/live_smooth_np.py):
// a whole tick of every live identity of every session in ONE launch, one 256-lane workgroup per identity, over state that stays on the
// device between ticks (per identity slot a ring of MVMC_SMOOTH_WIN_RING rows of 68 parameters and of members, the row count and the
// first frame).  The objective is mvmc_smooth.hip's; the problem is the last min(W, rows) rows of the identity, with the up to two rows
// before them as frozen history.  No counterpart in the reference.
//   append  the tick's new rows: d - 1 missing rows and the newest one (a data row from the tracker's table, or missing), a missing row
//           = a copy of the identity's last row;
//   per trial, inside the launch: the row blocks of the free rows on the workgroup's four waves (mvmc_smooth_row.h), the accept /
//           reject decision, one block-banded solve over the free rows (mvmc_smooth_sweep.h, the sweep the offline smoother runs too),
//           the next trial point.
// mvmc_smooth_window_robust: the same launch with the row blocks of the robust loss (mvmc_smooth_row.h: sm_row_block<LOSS>); the LDS
// and the workspace are the same for every loss.
// mvmc_smooth_window_contact: the same launch with foot contacts (live_smoothing.py: contacts="auto"; restated in
// tests/live_smooth_contact_np.py), smooth_window_kernel<LOSS, true>.  Per identity slot two more rings stay on the device: a label per
// row and foot (0 left ankle, 1 right ankle) and an anchor (3 doubles, NaN without a label).
//   append  the new rows' labels are 0 and their anchors NaN (a reset slot's whole rings);
//   blocks  every free row's stored label and anchor go to sm_row_block<LOSS, true>: 1/2 wc |ankle - a|^2, outside the loss;
//   after the last trial: FK of the free rows at their final values, a row per wave at a time, the two ankles into a small LDS array;
//           then wave f = foot f, one lane per window row: rows with index <= n - 1 - lag are frozen and keep their label and anchor;
//           the rows after them are labelled again (mvmc_smooth_contact.hip's rule: central-difference speed, one-sided at the
//           identity's first and newest row, the ground gate); one ballot of the <= 34 labels and one wave-uniform walk of its bits in
//           row order with the open run's start and sums in uniform registers: a run whose first visible row is frozen keeps that row's
//           anchor, another one is dropped when shorter than min_run, else gets the mean of its rows' ankles; every lane stores its
//           own row.  The emitted row (n - 1 - lag, frozen from this tick on) goes to cinfo with E_contact at the start and the end.
// Every sum runs in a fixed order inside one identity's own lanes: an identity's numbers depend on nothing else in the launch.
#define MVMC_DEVICE_ONLY
#include "mvmc_common.h"
#include "mvmc_track.hip"
#include "mvmc_ik1.hip"
#undef MVMC_DEVICE_ONLY

namespace {

#include "mvmc_smooth_row.h"
#include "mvmc_smooth_sweep.h"

constexpr int SW_MAXW = MVMC_SMOOTH_WIN_MAX;
constexpr int SW_RING = MVMC_SMOOTH_WIN_RING;
constexpr int SW_ROWS = SW_MAXW + 2;                      // window + history
constexpr int SW_ITEM = MVMC_SMOOTH_WIN_ITEM_INTS;
constexpr int SW_INFO = MVMC_SMOOTH_WIN_INFO_DOUBLES;
constexpr int SW_CINFO = MVMC_SMOOTH_LIVE_CONTACT_DOUBLES;
// workspace of one item (doubles): x and the trial point (SW_ROWS x 68 each), then per free row two block buffers and the factor
constexpr int SW_X = 0, SW_XT = SW_ROWS * 68, SW_PER_ITEM = 2 * SW_ROWS * 68;
constexpr int SW_PER_ROW = 2 * SM_BLK + SM_WORK;
static_assert(SW_RING >= 2 * SW_MAXW + 2, "ring: a jump of up to W frames keeps the rows that leave the window");

union SwLds {
    SmBlkLds blk[4];          // the blocks phase: one row block per wave
    SmSweepLds sw;            // the sweep (the phases do not overlap in time)
};
static_assert(sizeof(SwLds) <= 160 * 1024, "LDS of one workgroup");

// the contact arguments of smooth_window_kernel<LOSS, true> (the plain instantiations take none: their signature is the one it was)
struct SwContact {
    int32_t* lab;      // (n_slots, SW_RING, 2)
    double* anc;       // (n_slots, SW_RING, 2, 3)
    double* out;       // (n_items, SW_CINFO)
    double wc, speed, g0, g1, g2, g_off, height;
    int lag, min_run, use_ground;
};
__device__ __forceinline__ const SwContact& sw_contact(const SwContact& c) { return c; }

// the LDS of the contact instantiations beside SwLds: the free rows' two ankles (window row t: ank + 6 t) and the (row, foot) terms
// and the FK's tables (a copy: the contact passes read them here, so that the kernel's Ik1Tables argument is read where it was)
struct SwContactLds {
    double ank[SW_ROWS * 6], term[SW_ROWS * 2];
    double dirs[18 * 3];
    signed char parents[18], side_map[18];
};
static_assert(sizeof(SwLds) + sizeof(SwContactLds) <= 160 * 1024, "LDS of one workgroup with contacts");
__device__ __forceinline__ SwContactLds& sw_contact_lds() {
    __shared__ SwContactLds K;
    return K;
}

template <int LOSS, bool CONTACT, class... CA>
__global__ void __launch_bounds__(SM_THREADS) smooth_window_kernel(
    Ik1Tables T, const double* __restrict__ kps17, const double* __restrict__ Pmats, int C, int Pmax, int n_rigs,
    const int32_t* __restrict__ items, const double* __restrict__ new_params, const int32_t* __restrict__ new_members, int n_new,
    double* __restrict__ rows, int32_t* __restrict__ members, int32_t* __restrict__ count, int n_slots, int W, int n_iter,
    double root_vel, double root_acc, double ang_vel, double ang_acc, double mu0, double ftol, double xtol, double* __restrict__ info,
    double* __restrict__ work, int work_rows, double loss_px, CA... ca) {
    static_assert(sizeof...(CA) == (CONTACT ? 1 : 0), "one SwContact with contacts, nothing without");
    __shared__ SwLds LL;
    const int tid = threadIdx.x, wave = tid >> 6, it = blockIdx.x;
    const int32_t* im = items + (size_t)it * SW_ITEM;
    const int slot = uni((int)im[0]), rig = uni((int)im[1]), d = uni((int)im[2]), is_data = uni((int)im[3]), reset = uni((int)im[4]);
    const int src = uni((int)im[5]), f0 = uni((int)im[6]), row_lo = uni((int)im[7]);
    double* inf = info + (size_t)it * SW_INFO;
    if (tid < SW_INFO) inf[tid] = tid < 8 ? 0.0 : -1.0;
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    if constexpr (CONTACT) {   // {label L, R, anchor L (3), R (3), E_contact at the start, at the end}: no label until one is made
        double* co = sw_contact(ca...).out + (size_t)it * SW_CINFO;
        if (tid < SW_CINFO) co[tid] = tid >= 2 && tid < 8 ? qnan : 0.0;
        SwContactLds& K = sw_contact_lds();
        if (tid < 54) K.dirs[tid] = T.dirs[tid];
        if (tid >= 64 && tid < 82) { K.parents[tid - 64] = T.parents[tid - 64]; K.side_map[tid - 64] = T.side_map[tid - 64]; }
    }
    // (a malformed item is skipped, never followed out of bounds: stop reason 6)
    if (slot < 0 || slot >= n_slots || rig < 0 || rig >= n_rigs || d < 1 || d > W || (is_data && (src < 0 || src >= n_new)) ||
        (reset && !is_data) || row_lo < 0 || row_lo + W > work_rows) {
        if (tid == 0) inf[7] = 6.0;
        return;
    }
    double* ring = rows + (size_t)slot * SW_RING * 68;
    int32_t* mring = members + (size_t)slot * SW_RING * C;
    const int n_old = reset ? 0 : uni((int)count[slot * 2]);
    if (n_old < 0 || (!reset && n_old < 1)) {
        if (tid == 0) inf[7] = 6.0;
        return;
    }
    const int n = reset ? 1 : n_old + d;
    // ---- append: missing rows are copies of the identity's last row, the newest row is the table's when it has data ----
    {
        const int first = reset ? 0 : n_old;
        double last = 0.0;
        if (tid < 68 && n_old >= 1) last = ring[((n_old - 1) % SW_RING) * 68 + tid];
        for (int r = first; r < n; ++r) {
            const bool data = is_data && r == n - 1;
            if (tid < 68) ring[(r % SW_RING) * 68 + tid] = data ? new_params[(size_t)src * 68 + tid] : last;
            if (tid >= 128 && tid < 128 + C) mring[(r % SW_RING) * C + tid - 128] = data ? new_members[(size_t)src * C + tid - 128] : -1;
        }
        if (tid == 0) {
            count[slot * 2] = n;
            if (reset) count[slot * 2 + 1] = f0;
        }
        if constexpr (CONTACT) {   // the new rows carry no label (a reset slot: none of its ring does)
            const SwContact& c = sw_contact(ca...);
            int32_t* lring = c.lab + (size_t)slot * SW_RING * 2;
            double* aring = c.anc + (size_t)slot * SW_RING * 6;
            if (reset) {
                for (int i = tid; i < SW_RING * 2; i += SM_THREADS) lring[i] = 0;
                for (int i = tid; i < SW_RING * 6; i += SM_THREADS) aring[i] = qnan;
            } else {
                for (int r = first; r < n; ++r) {
                    if (tid >= 192 && tid < 194) lring[(r % SW_RING) * 2 + tid - 192] = 0;
                    if (tid >= 200 && tid < 206) aring[(r % SW_RING) * 6 + tid - 200] = qnan;
                }
            }
        }
    }
    if (n < 2) return;   // one row: nothing to solve
    const int m = n < W ? n : W, h = (n - m) < 2 ? (n - m) : 2, nw = h + m, lo = n - nw;
    double* x = work + (size_t)it * SW_PER_ITEM + SW_X;
    double* xt = work + (size_t)it * SW_PER_ITEM + SW_XT;
    double* rowwk = work + (size_t)gridDim.x * SW_PER_ITEM + (size_t)row_lo * SW_PER_ROW;   // this item's W rows
    __syncthreads();
    for (int i = tid; i < nw * 68; i += SM_THREADS) {
        const int t = i / 68, c = i - t * 68;
        const double v = ring[((lo + t) % SW_RING) * 68 + c];
        x[i] = v;
        xt[i] = v;
    }
    SmSweepLds& L = LL.sw;
    const double* Prig = Pmats + (size_t)rig * C * 12;
    // per free row r (0..m-1): blocks buffer b at rowwk + r SW_PER_ROW + b SM_BLK, the factor after them
    auto blocks_of = [&](int r, int b) -> double* { return rowwk + (size_t)r * SW_PER_ROW + (size_t)b * SM_BLK; };
    double* fac = rowwk + 2 * SM_BLK;
    __syncthreads();
    // the row blocks of the free rows at the point p into buffer b: a row per wave at a time
    auto eval_blocks = [&](const double* p, int b) {
        __syncthreads();   // (the LDS changes hands: sweep -> blocks; p is complete)
        for (int r = wave; r < m; r += 4) {
            const int at = (lo + h + r) % SW_RING;
            if constexpr (CONTACT) {
                const SwContact& c = sw_contact(ca...);
                sm_row_block<LOSS, true>(T, LL.blk[wave], kps17, Prig, C, Pmax, mring + (size_t)at * C, p + (size_t)(h + r) * 68,
                                         blocks_of(r, b), loss_px, c.lab + ((size_t)slot * SW_RING + at) * 2,
                                         c.anc + ((size_t)slot * SW_RING + at) * 6, c.wc);
            } else {
                sm_row_block<LOSS>(T, LL.blk[wave], kps17, Prig, C, Pmax, mring + (size_t)at * C, p + (size_t)(h + r) * 68,
                                   blocks_of(r, b), loss_px);
            }
        }
        __syncthreads();
    };
    // contacts: E_contact of the free rows at p under their stored labels and anchors -> cinfo[at] (FK of the free rows, a row per
    // wave at a time; the terms one lane each; thread 0 adds them in (row, foot) order).  The ankles stay in the LDS array.
    [[maybe_unused]] auto contact_energy = [&](const double* p, int at_out) {
        if constexpr (CONTACT) {
            const SwContact& c = sw_contact(ca...);
            SwContactLds& K = sw_contact_lds();
            const int lane = tid & 63;
            __syncthreads();   // (the LDS changes hands: sweep -> FK; p is complete)
            for (int r = wave; r < m; r += 4) {
                sm_row_fk<false>(K, LL.blk[wave], p + (size_t)(h + r) * 68);
                if (lane < 6) K.ank[(h + r) * 6 + lane] = LL.blk[wave].pos[3 * (lane < 3 ? MVMC_SMOOTH_FOOT_L : MVMC_SMOOTH_FOOT_R) + lane % 3];
                MVMC_WAVE_SYNC();   // (pos is read before the next row's FK writes it)
            }
            __syncthreads();
            if (tid < 2 * m) {
                const int r = tid >> 1, f = tid & 1;
                const size_t at = (size_t)slot * SW_RING + (lo + h + r) % SW_RING;
                double e = 0.0;
                if (c.lab[at * 2 + f] != 0) {
                    const double* a = c.anc + at * 6 + 3 * f;
                    const double* q = K.ank + (h + r) * 6 + 3 * f;
                    const double c0 = q[0] - a[0], c1 = q[1] - a[1], c2 = q[2] - a[2];
                    e = 0.5 * c.wc * (c0 * c0 + c1 * c1 + c2 * c2);
                }
                K.term[tid] = e;
            }
            __syncthreads();
            if (tid == 0) {
                double E = 0.0;
                for (int i = 0; i < 2 * m; ++i) E += K.term[i];
                c.out[(size_t)it * SW_CINFO + at_out] = E;
            }
        }
    };
    contact_energy(x, 8);
    eval_blocks(x, 0);
    sm_sweep_tables(L, T, root_vel, root_acc, ang_vel, ang_acc);   // (the blocks phase overwrote them)
    int cur = 0, trials = 0, n_acc = 0, why = 1;
    double mu = mu0;
    double Ed = sm_data_energy(L, blocks_of(0, 0), SW_PER_ROW, m), Ep = sm_prior_energy(L, x, nw, h);
    if (tid == 0) { inf[0] = Ed; inf[1] = Ep; }

    for (int iter = 0; iter < n_iter; ++iter) {
        const SmStep st = sm_sweep(L, blocks_of(0, cur), SW_PER_ROW, fac, SW_PER_ROW, x, m, h, nw, mu);
        const double E = Ed + Ep, pred = st.pred, dmax = st.dmax;
        if (st.fail || !(dmax == dmax) || dmax == __longlong_as_double(0x7ff0000000000000LL)) { why = 5; break; }
        if (dmax < xtol) { why = 2; break; }
        if (pred < ftol * E) { why = 3; break; }
        for (int i = tid; i < m * SK; i += SM_THREADS) {
            const int r = i / SK, q = i - r * SK, at = (h + r) * 68 + L.colx[q];
            xt[at] = x[at] + fac[(size_t)r * SW_PER_ROW + W_Y + q];
        }
        eval_blocks(xt, 1 - cur);
        sm_sweep_tables(L, T, root_vel, root_acc, ang_vel, ang_acc);   // (the blocks phase overwrote them)
        const double Etd = sm_data_energy(L, blocks_of(0, 1 - cur), SW_PER_ROW, m), Etp = sm_prior_energy(L, xt, nw, h);
        const double Et = Etd + Etp;
        const bool acc = Et < E;
        if (tid == 0) inf[8 + trials] = acc ? 1.0 : 0.0;
        ++trials;
        if (acc) {
            for (int i = tid; i < nw * 68; i += SM_THREADS) x[i] = xt[i];
            cur = 1 - cur;
            mu /= 10.0;
            ++n_acc;
            Ed = Etd;
            Ep = Etp;
            __syncthreads();
            if (E - Et < ftol * E) { why = 4; break; }
        } else {
            for (int i = tid; i < nw * 68; i += SM_THREADS) xt[i] = x[i];
            mu *= 10.0;
            __syncthreads();
        }
    }
    __syncthreads();
    // the free rows back into the ring
    for (int i = tid; i < m * 68; i += SM_THREADS) {
        const int r = i / 68, c = i - r * 68;
        ring[((lo + h + r) % SW_RING) * 68 + c] = x[(h + r) * 68 + c];
    }
    if (tid == 0) { inf[2] = Ed; inf[3] = Ep; inf[4] = trials; inf[5] = n_acc; inf[6] = mu; inf[7] = why; }
    if constexpr (CONTACT) {
        const SwContact& c = sw_contact(ca...);
        SwContactLds& K = sw_contact_lds();
        contact_energy(x, 9);   // (also: the free rows' ankles at the final values; every read of the stored labels is done)
        __syncthreads();
        if (wave < 2) {   // wave f = foot f, lane t = window row t (nw <= 34)
            const int f = wave, t = tid & 63, i = lo + t;             // i: the row's index in the identity
            const int first = n - c.lag > 0 ? n - c.lag : 0;          // the first tentative row: everything before it is frozen
            const bool in = t < nw, tent = in && i >= first;
            int32_t* lab = c.lab + ((size_t)slot * SW_RING + (in ? i % SW_RING : 0)) * 2 + f;
            double* anc = c.anc + ((size_t)slot * SW_RING + (in ? i % SW_RING : 0)) * 6 + 3 * f;
            const double* p = K.ank + 3 * f;                          // window row t: p + 6 t (free rows only)
            int on = 0;
            double a0 = qnan, a1 = qnan, a2 = qnan;                    // the row's anchor
            if (in && !tent) {
                on = *lab != 0;
                if (on) { a0 = anc[0]; a1 = anc[1]; a2 = anc[2]; }
            }
            if (tent) {   // (both neighbours are free rows: the window is longer than the lag)
                const int a = (i > 0 ? i - 1 : i) - lo, b = (i + 1 < n ? i + 1 : i) - lo;
                const double d0 = p[6 * b] - p[6 * a], d1 = p[6 * b + 1] - p[6 * a + 1], d2 = p[6 * b + 2] - p[6 * a + 2];
                double v = sqrt(dadd(dadd(dmul(d0, d0), dmul(d1, d1)), dmul(d2, d2)));
                if (b - a == 2) v = dmul(0.5, v);
                on = v < c.speed;
                if (on && c.use_ground)
                    on = dadd(dadd(dadd(dmul(c.g0, p[6 * t]), dmul(c.g1, p[6 * t + 1])), dmul(c.g2, p[6 * t + 2])), -c.g_off) < c.height;
            }
            const double q0 = tent && on ? p[6 * t] : 0.0, q1 = tent && on ? p[6 * t + 1] : 0.0, q2 = tent && on ? p[6 * t + 2] : 0.0;
            const unsigned long long bal = __ballot(on != 0);
            const unsigned blo = (unsigned)uni((int)(unsigned)bal), bhi = (unsigned)uni((int)(unsigned)(bal >> 32));
            int start = -1;
            double s0 = 0.0, s1 = 0.0, s2 = 0.0, k0 = 0.0, k1 = 0.0, k2 = 0.0;
            // the run [start, end) is complete: a frozen first row's anchor, or dropped, or the mean of its rows
            auto close = [&](int end) {
                const bool mine = t >= start && t < end;
                if (lo + start < first) {
                    if (mine) { a0 = k0; a1 = k1; a2 = k2; }
                } else if (end - start < c.min_run) {
                    if (mine) on = 0;
                } else {
                    const double len = (double)(end - start);
                    if (mine) { a0 = s0 / len; a1 = s1 / len; a2 = s2 / len; }
                }
                start = -1;
            };
            for (int j = 0; j < nw; ++j) {   // wave-uniform: every lane walks the same bits and holds the same sums
                const double r0 = __shfl(q0, j), r1 = __shfl(q1, j), r2 = __shfl(q2, j);
                const double f0_ = __shfl(a0, j), f1_ = __shfl(a1, j), f2_ = __shfl(a2, j);
                if (((j < 32 ? blo >> j : bhi >> (j - 32)) & 1u) != 0u) {
                    if (start < 0) { start = j; s0 = 0.0; s1 = 0.0; s2 = 0.0; k0 = f0_; k1 = f1_; k2 = f2_; }
                    s0 += r0; s1 += r1; s2 += r2;
                } else if (start >= 0) {
                    close(j);
                }
            }
            if (start >= 0) close(nw);
            if (tent) {
                *lab = on;
                anc[0] = on ? a0 : qnan; anc[1] = on ? a1 : qnan; anc[2] = on ? a2 : qnan;
            }
            if (in && i == n - 1 - c.lag) {   // the emitted row: frozen, its stored label and anchor
                double* co = c.out + (size_t)it * SW_CINFO;
                co[f] = (double)on;
                co[2 + 3 * f] = a0; co[3 + 3 * f] = a1; co[4 + 3 * f] = a2;
            }
        }
    }
}

}  // namespace

extern "C" long long mvmc_smooth_window_work_doubles(int n_items, int window) {
    if (n_items < 0 || window < 2 || window > SW_MAXW) return -1;
    return (long long)n_items * (SW_PER_ITEM + (long long)window * SW_PER_ROW);
}

extern "C" int mvmc_smooth_window_robust(const mvmcSkeleton* skel_host, const double* kps17, int n_views, int p_max, const double* Pmats,
                                         int n_rigs, const int32_t* items, int n_items, const double* new_params,
                                         const int32_t* new_members, int n_new, double* rows, int32_t* members, int32_t* count,
                                         int n_slots, int window, int n_iter, double root_vel, double root_acc, double ang_vel,
                                         double ang_acc, double mu0, double ftol, double xtol, double* info, double* work,
                                         long long work_doubles, int loss, double loss_px, mvmcStream_t stream) {
    if (!skel_host || n_items < 0 || n_new < 0 || n_slots < 0 || n_rigs < 1 || n_views <= 0 || n_views > MVMC_SMOOTH_MAX_VIEWS ||
        p_max <= 0)
        return MVMC_ERR_ARG;
    if (window < 2 || window > SW_MAXW || n_iter < 1 || n_iter > SW_INFO - 8) return MVMC_ERR_ARG;
    if (!(root_vel >= 0.0) || !(root_acc >= 0.0) || !(ang_vel >= 0.0) || !(ang_acc >= 0.0) || !(mu0 > 0.0)) return MVMC_ERR_ARG;
    if (!sm_loss_ok(loss, loss_px)) return MVMC_ERR_ARG;
    if (n_items == 0) return MVMC_OK;
    if (!kps17 || !Pmats || !items || !rows || !members || !count || !info || !work || (n_new > 0 && (!new_params || !new_members)))
        return MVMC_ERR_ARG;
    if (work_doubles < mvmc_smooth_window_work_doubles(n_items, window)) return MVMC_ERR_ARG;
    Ik1Tables T;
    if (!sm_tables(skel_host, &T)) return MVMC_ERR_UNSUPPORTED;
    auto kernel = loss == MVMC_SMOOTH_LOSS_HUBER    ? smooth_window_kernel<MVMC_SMOOTH_LOSS_HUBER, false>
                  : loss == MVMC_SMOOTH_LOSS_CAUCHY ? smooth_window_kernel<MVMC_SMOOTH_LOSS_CAUCHY, false>
                                                    : smooth_window_kernel<MVMC_SMOOTH_LOSS_NONE, false>;
    hipLaunchKernelGGL(kernel, dim3(n_items), dim3(SM_THREADS), 0, (hipStream_t)stream, T, kps17, Pmats, n_views, p_max, n_rigs, items,
                       new_params, new_members, n_new, rows, members, count, n_slots, window, n_iter, root_vel, root_acc, ang_vel,
                       ang_acc, mu0, ftol, xtol, info, work, n_items * window, loss_px);
    MVMC_CHECK_LAUNCH();
    return MVMC_OK;
}

extern "C" int mvmc_smooth_window_contact(const mvmcSkeleton* skel_host, const double* kps17, int n_views, int p_max, const double* Pmats,
                                          int n_rigs, const int32_t* items, int n_items, const double* new_params,
                                          const int32_t* new_members, int n_new, double* rows, int32_t* members, int32_t* count,
                                          int n_slots, int window, int n_iter, double root_vel, double root_acc, double ang_vel,
                                          double ang_acc, double mu0, double ftol, double xtol, double* info, double* work,
                                          long long work_doubles, int loss, double loss_px, int32_t* contact, double* anchors, int lag,
                                          double contact_weight, double contact_speed, int contact_min_frames, int use_ground,
                                          const double* ground, double contact_height, double* cinfo, mvmcStream_t stream) {
    const double big = 1.7976931348623157e308;   // (a NaN fails every comparison below)
    if (!skel_host || n_items < 0 || n_new < 0 || n_slots < 0 || n_rigs < 1 || n_views <= 0 || n_views > MVMC_SMOOTH_MAX_VIEWS ||
        p_max <= 0)
        return MVMC_ERR_ARG;
    if (window < 2 || window > SW_MAXW || n_iter < 1 || n_iter > SW_INFO - 8) return MVMC_ERR_ARG;
    if (!(root_vel >= 0.0) || !(root_acc >= 0.0) || !(ang_vel >= 0.0) || !(ang_acc >= 0.0) || !(mu0 > 0.0)) return MVMC_ERR_ARG;
    if (!sm_loss_ok(loss, loss_px)) return MVMC_ERR_ARG;
    if (lag < 0 || lag >= window || contact_min_frames < 1 || lag + 1 < contact_min_frames) return MVMC_ERR_ARG;
    if (!(contact_weight >= 0.0 && contact_weight <= big) || !(contact_speed >= -big && contact_speed <= big)) return MVMC_ERR_ARG;
    if (use_ground) {
        if (!ground || !(contact_height >= -big && contact_height <= big)) return MVMC_ERR_ARG;
        for (int i = 0; i < 4; ++i)
            if (!(ground[i] >= -big && ground[i] <= big)) return MVMC_ERR_ARG;
    }
    if (n_items == 0) return MVMC_OK;
    if (!kps17 || !Pmats || !items || !rows || !members || !count || !info || !work || (n_new > 0 && (!new_params || !new_members)))
        return MVMC_ERR_ARG;
    if (!contact || !anchors || !cinfo) return MVMC_ERR_ARG;
    if (work_doubles < mvmc_smooth_window_work_doubles(n_items, window)) return MVMC_ERR_ARG;
    Ik1Tables T;
    if (!sm_tables(skel_host, &T)) return MVMC_ERR_UNSUPPORTED;
    const bool g = use_ground != 0;
    const SwContact ca{contact, anchors, cinfo, contact_weight, contact_speed, g ? ground[0] : 0.0, g ? ground[1] : 0.0,
                       g ? ground[2] : 0.0, g ? ground[3] : 0.0, g ? contact_height : 0.0, lag, contact_min_frames, g ? 1 : 0};
    auto kernel = loss == MVMC_SMOOTH_LOSS_HUBER    ? smooth_window_kernel<MVMC_SMOOTH_LOSS_HUBER, true, SwContact>
                  : loss == MVMC_SMOOTH_LOSS_CAUCHY ? smooth_window_kernel<MVMC_SMOOTH_LOSS_CAUCHY, true, SwContact>
                                                    : smooth_window_kernel<MVMC_SMOOTH_LOSS_NONE, true, SwContact>;
    hipLaunchKernelGGL(kernel, dim3(n_items), dim3(SM_THREADS), 0, (hipStream_t)stream, T, kps17, Pmats, n_views, p_max, n_rigs, items,
                       new_params, new_members, n_new, rows, members, count, n_slots, window, n_iter, root_vel, root_acc, ang_vel,
                       ang_acc, mu0, ftol, xtol, info, work, n_items * window, loss_px, ca);
    MVMC_CHECK_LAUNCH();
    return MVMC_OK;
}

extern "C" int mvmc_smooth_window(const mvmcSkeleton* skel_host, const double* kps17, int n_views, int p_max, const double* Pmats,
                                  int n_rigs, const int32_t* items, int n_items, const double* new_params, const int32_t* new_members,
                                  int n_new, double* rows, int32_t* members, int32_t* count, int n_slots, int window, int n_iter,
                                  double root_vel, double root_acc, double ang_vel, double ang_acc, double mu0, double ftol, double xtol,
                                  double* info, double* work, long long work_doubles, mvmcStream_t stream) {
    return mvmc_smooth_window_robust(skel_host, kps17, n_views, p_max, Pmats, n_rigs, items, n_items, new_params, new_members, n_new, rows,
                                     members, count, n_slots, window, n_iter, root_vel, root_acc, ang_vel, ang_acc, mu0, ftol, xtol, info,
                                     work, work_doubles, MVMC_SMOOTH_LOSS_NONE, 0.0, stream);
}
