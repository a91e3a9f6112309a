// Re-linking of the records of one person (multiview_motion_capture_amd/relinking.py; include/mvmc.h: mvmc_relink).  The reference has
// no counterpart: its tracker never joins two tracklets.  Per sequence the records are nodes in (first frame, track id) order; record A
// may be followed by record B when 1 <= gap = B.first - A.last <= max_gap, at the cost (metres)
//     mean_k | A.last_joints[k] + v gap - B.first_joints[k] |,   v = the mean of the defined end / start velocities of A and B,
// allowed when cost <= min(max_dist, near_dist + speed gap).  The links taken minimise sum cost + max_dist (records without a
// successor): an optimal assignment on the n x 2n matrix [allowed costs, RL_BIG elsewhere | max_dist on the diagonal, RL_BIG elsewhere].
//
// ONE launch, one 256-lane workgroup per sequence:
//   1. all lanes build the n x n real part of the matrix (LDS for n <= RL_LDS_N, the caller's workspace beyond); the dummy part is
//      never stored;
//   2. Kuhn-Munkres with potentials, rows in record order (assign_rows of mvmc_stitch.hip, for n <= 512 instead of 16): a column
//      belongs to lane (j - 1) mod 256, which alone touches its v / minv / used / way; the minimum of an augmenting step (value, then
//      lowest column: the sequential scan's "first minimum wins") by a shuffle butterfly per wave and four LDS words across the waves.
//      The arithmetic per column is the sequential algorithm's, so the result is its result bit for bit;
//   3. pointer jumping along the links: chain head and position in the chain of every record.
// Every loop is bounded; status 1 = an assignment hit its bound, 2 = a malformed sequence row (nothing is read or written for it).
// Steps 2 and 3 are one function (assign_and_chain) that the re-identification by bone lengths further down runs as well
// (mvmc_reid_signature, mvmc_reid_link: the same nodes and choice, another cost).
#include "mvmc_common.h"

namespace {

constexpr int RL_THREADS = 256;
constexpr int RL_CAP = MVMC_RELINK_MAX_RECORDS;
constexpr int RL_LDS_N = 64;             // the n x n costs stay in LDS up to here (32 KB)
constexpr int RL_PER = RL_CAP / RL_THREADS;
constexpr double RL_BIG = 1e6;           // a link that is not allowed: finite, beyond any sum of allowed costs
constexpr double RL_INF = 1e300;
constexpr int RL_REC = MVMC_RELINK_REC_DOUBLES;
static_assert(RL_CAP % RL_THREADS == 0, "records per lane of the pointer jumping");

struct RelinkArgs {
    const double* rec;        // (N, RL_REC): last joints (54), first joints (54), centroids {last, k back, first, k on} (4 x 3)
    const int32_t* frames;    // (N, 4): first frame, last frame, frames spanned by the end velocity, by the start velocity (0: undefined)
    const int32_t* seq;       // (S, 4): first record, records, offset into work (doubles), 0
    int n_records, max_gap;
    double max_dist, near_dist, speed;
    int32_t *succ, *head, *pos;
    double* link_cost;
    int32_t* status;
    double* work;
    long long work_doubles;
};

// the cost of the link a -> b (rows of rec / frames), RL_BIG when it is not allowed
__device__ inline double link_cost_of(const RelinkArgs& A, int a, int b) {
#pragma clang fp contract(off)
    const int32_t* fa = A.frames + (size_t)a * 4;
    const int32_t* fb = A.frames + (size_t)b * 4;
    const int gap = fb[0] - fa[1];
    if (a == b || gap < 1 || gap > A.max_gap) return RL_BIG;
    const double* ra = A.rec + (size_t)a * RL_REC;
    const double* rb = A.rec + (size_t)b * RL_REC;
    double v[3] = {0.0, 0.0, 0.0};
    const int da = fa[2], db = fb[3];
    for (int c = 0; c < 3; ++c) {
        const double va = da > 0 ? (ra[108 + c] - ra[111 + c]) / (double)da : 0.0;
        const double vb = db > 0 ? (rb[117 + c] - rb[114 + c]) / (double)db : 0.0;
        v[c] = (da > 0 && db > 0) ? (va + vb) / 2.0 : (da > 0 ? va : (db > 0 ? vb : 0.0));
    }
    const double g = (double)gap;
    double sum = 0.0;
    for (int k = 0; k < 18; ++k) {
        const double dx = (ra[3 * k] + v[0] * g) - rb[54 + 3 * k];
        const double dy = (ra[3 * k + 1] + v[1] * g) - rb[54 + 3 * k + 1];
        const double dz = (ra[3 * k + 2] + v[2] * g) - rb[54 + 3 * k + 2];
        sum += sqrt(dx * dx + dy * dy + dz * dz);
    }
    const double c = sum / 18.0;
    const double gate = fmin(A.max_dist, A.near_dist + A.speed * g);
    return (isfinite(c) && c <= gate) ? c : RL_BIG;
}

// (value, column) minimum over the wave: the smaller value, the lower column among equals; every lane gets it
__device__ __forceinline__ void wave_min_col(double& v, int& j) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double ov = __shfl_xor(v, off);
        const int oj = __shfl_xor(j, off);
        if (ov < v || (ov == v && oj < j)) { v = ov; j = oj; }
    }
}

// Steps 2 and 3 of a sequence of n >= 1 records (relink_kernel and reid_link_kernel run these instructions): the assignment on the
// n x 2n matrix  [real(i, j) | dummy on the diagonal, RL_BIG elsewhere], then the chains.  real(i, j) reads the n x n part, which
// every lane of the workgroup has finished writing (the barrier below orders it); off = the sequence's first record in the outputs.
// Returns true when the assignment hit its loop bound (nothing is written then).
template <class Real>
__device__ __forceinline__ bool assign_and_chain(const int n, const int off, const double dummy, Real real, int32_t* out_succ,
                                                 int32_t* out_head, int32_t* out_pos, double* out_cost) {
    __shared__ double s_u[RL_CAP + 1], s_v[2 * RL_CAP + 1], s_minv[2 * RL_CAP + 1];
    __shared__ int s_p[2 * RL_CAP + 1], s_way[2 * RL_CAP + 1];
    __shared__ unsigned char s_used[2 * RL_CAP + 1];
    __shared__ double s_redv[RL_THREADS / 64];
    __shared__ int s_redj[RL_THREADS / 64];
    __shared__ int s_fail, s_rows;
    const int tid = threadIdx.x;
    const int m = 2 * n;
    for (int j = tid; j <= m; j += RL_THREADS) { s_v[j] = 0.0; s_p[j] = 0; s_way[j] = 0; }
    for (int i = tid; i <= n; i += RL_THREADS) s_u[i] = 0.0;
    if (tid == 0) { s_fail = 0; s_rows = 0; }
    __syncthreads();
    auto cost = [&](int i, int j) -> double {      // row i, column j, both from 0
        if (j >= n) return j - n == i ? dummy : RL_BIG;
        return real(i, j);
    };

    // 2. the assignment: row after row, a shortest augmenting path each
    bool fail = false;
    for (int i = 1; i <= n && !fail; ++i) {
        for (int j = 1 + tid; j <= m; j += RL_THREADS) { s_minv[j] = RL_INF; s_used[j] = 0; }
        if (tid == 0) s_p[0] = i;
        __syncthreads();
        int j0 = 0, rounds = 0;
        while (true) {
            const int i0 = s_p[j0];
            const double ui0 = s_u[i0];
            double best = RL_INF;
            int bj = 0;
            for (int j = 1 + tid; j <= m; j += RL_THREADS) {
                if (j == j0) { s_used[j] = 1; continue; }
                if (s_used[j]) continue;
                const double cur = cost(i0 - 1, j - 1) - ui0 - s_v[j];
                double mv = s_minv[j];
                if (cur < mv) { mv = cur; s_minv[j] = cur; s_way[j] = j0; }
                if (mv < best) { best = mv; bj = j; }
            }
            wave_min_col(best, bj);
            if ((tid & 63) == 0) { s_redv[tid >> 6] = best; s_redj[tid >> 6] = bj; }
            __syncthreads();
            double delta = s_redv[0];
            int j1 = s_redj[0];
#pragma unroll
            for (int w = 1; w < RL_THREADS / 64; ++w) {
                const double ov = s_redv[w];
                const int oj = s_redj[w];
                if (ov < delta || (ov == delta && oj < j1)) { delta = ov; j1 = oj; }
            }
            if (j1 == 0 || ++rounds > m + 1) { fail = true; break; }
            if (tid == 0) s_u[i] += delta;             // column 0 (p[0] = i) is always in the tree
            for (int j = 1 + tid; j <= m; j += RL_THREADS) {
                if (s_used[j]) { s_u[s_p[j]] += delta; s_v[j] -= delta; } else s_minv[j] -= delta;
            }
            j0 = j1;
            const bool free_col = s_p[j0] == 0;       // read before the barrier: lane 0 rewrites p right after it
            __syncthreads();
            if (free_col) break;
        }
        if (fail) break;
        if (tid == 0) {
            int links = 0;
            do {
                const int j1 = s_way[j0];
                s_p[j0] = s_p[j1];
                j0 = j1;
                if (++links > m + 1) { s_fail = 1; break; }
            } while (j0);
        }
        __syncthreads();
        fail = s_fail != 0;
    }

    // the links: row p[j] - 1 -> column j - 1 where that is a real column at an allowed cost.  s_minv's memory holds succ | pred now.
    int* s_succ = reinterpret_cast<int*>(s_minv);
    int* s_pred = s_succ + RL_CAP;
    __syncthreads();
    if (!fail) {
        int rows = 0;
        for (int j = 1 + tid; j <= m; j += RL_THREADS) rows += s_p[j] > 0;
        if (rows) atomicAdd(&s_rows, rows);
    }
    for (int k = tid; k < n; k += RL_THREADS) { s_succ[k] = -1; s_pred[k] = -1; }
    __syncthreads();
    if (!fail && s_rows != n) fail = true;
    if (fail) return true;
    for (int j = 1 + tid; j <= n; j += RL_THREADS) {
        const int r = s_p[j] - 1;
        if (r < 0 || r >= n) continue;
        const double c = cost(r, j - 1);
        if (c < RL_BIG) { s_succ[r] = j - 1; s_pred[j - 1] = r; out_cost[off + r] = c; }
    }
    __syncthreads();

    // 3. chain head and position: pointer jumping along the predecessors (a link goes forward in time, so there is no cycle; the
    // number of rounds is bounded by log2 n whatever the links are).  s_p / s_way hold the pointers and the distances now.
    int* s_ptr = s_p;
    int* s_dist = s_way;
    for (int k = tid; k < n; k += RL_THREADS) {
        const int pr = s_pred[k];
        s_ptr[k] = pr >= 0 ? pr : k;
        s_dist[k] = pr >= 0 ? 1 : 0;
        if (s_succ[k] < 0) out_cost[off + k] = 0.0;
    }
    __syncthreads();
    for (int span = 1; span < n; span <<= 1) {
        int np[RL_PER], nd[RL_PER];
#pragma unroll
        for (int e = 0; e < RL_PER; ++e) {
            const int k = tid + e * RL_THREADS;
            if (k < n) { const int q = s_ptr[k]; np[e] = s_ptr[q]; nd[e] = s_dist[k] + s_dist[q]; }
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < RL_PER; ++e) {
            const int k = tid + e * RL_THREADS;
            if (k < n) { s_ptr[k] = np[e]; s_dist[k] = nd[e]; }
        }
        __syncthreads();
    }
    for (int k = tid; k < n; k += RL_THREADS) {
        out_succ[off + k] = s_succ[k];
        out_head[off + k] = s_ptr[k];
        out_pos[off + k] = s_dist[k];
    }
    return false;
}

__global__ void __launch_bounds__(RL_THREADS)
relink_kernel(RelinkArgs A) {
    __shared__ double s_cost[RL_LDS_N * RL_LDS_N];

    const int s = blockIdx.x, tid = threadIdx.x;
    const int off = A.seq[(size_t)s * 4], n = A.seq[(size_t)s * 4 + 1], woff = A.seq[(size_t)s * 4 + 2];
    const bool in_lds = n <= RL_LDS_N;
    bool bad = off < 0 || n < 0 || n > RL_CAP || (long long)off + n > A.n_records;
    if (!bad && !in_lds) bad = !A.work || woff < 0 || (long long)woff + (long long)n * n > A.work_doubles;
    if (bad) {
        if (tid == 0) A.status[s] = 2;
        return;
    }
    if (n == 0) {
        if (tid == 0) A.status[s] = 0;
        return;
    }
    double* gcost = in_lds ? nullptr : A.work + woff;

    // 1. the real part of the matrix
    for (int q = tid; q < n * n; q += RL_THREADS) {
        const int i = q / n, j = q - i * n;
        const double c = link_cost_of(A, off + i, off + j);
        if (in_lds) s_cost[q] = c; else gcost[q] = c;
    }
    const bool fail = assign_and_chain(n, off, A.max_dist, [&](int i, int j) -> double {
        return in_lds ? s_cost[i * n + j] : gcost[(size_t)i * n + j];
    }, A.succ, A.head, A.pos, A.link_cost);
    if (tid == 0) A.status[s] = fail ? 1 : 0;
}

// ---- Re-identification by bone lengths (relinking.reidentify_sequences; include/mvmc.h: mvmc_reid_signature, mvmc_reid_link) ----
// SIGNATURE of a record, from the joints of ALL its poses.  Per pose and bone j = 1 .. 17: b_j = sqrt(dx dx + dy dy + dz dz) of joint j
// minus its parent, no contraction.  Ten sides (the values 0 - 6 and 8 - 10 of the skeleton's side map; 7 is the root): sides 0 - 6
// have a left and a right bone and the value (b_lo + b_hi) / 2 in joint order, sides 8, 9, 10 one bone; a pose gives a side a value
// only when all its bones are finite.  Per side with m values: med = the lower median (rank (m - 1) / 2 in ascending order), mad = the
// lower median of |x - med|, se = 1.4826 mad 1.2533 / sqrt(m) in that order; a side with m < min_poses is undefined (NaN, NaN).
// One workgroup per record.  The ten values of every pose stay in LDS up to RS_LDS_POSES poses, in the caller's workspace (rows
// 10 first .. 10 (first + poses) of it) beyond.  A selection is exact: the values are >= 0, so their bit patterns order as unsigned
// integers, and eight counting passes of eight bits each (integer counts per digit in LDS, a scan by one wave per side) fix the
// pattern of the wanted rank from the top byte down, for the ten sides at once.  Nothing depends on the order of the values.
constexpr int RS_THREADS = 256;
constexpr int RS_SIDES = 10;
constexpr int RS_LDS_POSES = MVMC_REID_LDS_POSES;
__constant__ int RS_PARENT[18] = {-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 9, 10, 8, 12, 13, 8, 15, 15};
__constant__ int RS_LO[RS_SIDES] = {1, 2, 3, 9, 10, 11, 16, 7, 8, 15};
__constant__ int RS_HI[RS_SIDES] = {4, 5, 6, 12, 13, 14, 17, -1, -1, -1};

struct ReidSigArgs {
    const double* joints;     // (n_poses, 18, 3)
    const int32_t* rec;       // (N, 2): first pose row, poses
    int n_poses, min_poses;
    double* sig;              // (N, 20): med (10), se (10)
    int32_t* cnt;             // (N, 10)
    double* ends;             // (N, 6): centroid of the first pose, of the last pose
    int32_t* status;          // (N)
    double* work;
    long long work_doubles;
};

__device__ inline double reid_bone(const double* P, int j) {
#pragma clang fp contract(off)
    const int p = RS_PARENT[j];
    const double dx = P[3 * j] - P[3 * p], dy = P[3 * j + 1] - P[3 * p + 1], dz = P[3 * j + 2] - P[3 * p + 2];
    return sqrt(dx * dx + dy * dy + dz * dz);
}

__global__ void __launch_bounds__(RS_THREADS)
reid_signature_kernel(ReidSigArgs A) {
    __shared__ double s_val[RS_SIDES * RS_LDS_POSES];
    __shared__ unsigned int s_hist[RS_SIDES * 256];
    __shared__ unsigned long long s_prefix[RS_SIDES];
    __shared__ int s_k[RS_SIDES], s_cnt[RS_SIDES];
    __shared__ double s_med[RS_SIDES];

    const int r = blockIdx.x, tid = threadIdx.x;
    const int first = A.rec[(size_t)r * 2], m = A.rec[(size_t)r * 2 + 1];
    const bool in_lds = m <= RS_LDS_POSES;
    bool bad = first < 0 || m < 1 || m > MVMC_REID_MAX_POSES || (long long)first + m > A.n_poses;
    if (!bad && !in_lds) bad = !A.work || (long long)RS_SIDES * ((long long)first + m) > A.work_doubles;
    if (bad) {
        if (tid == 0) A.status[r] = 2;
        return;
    }
    double* gval = in_lds ? nullptr : A.work + (size_t)RS_SIDES * first;
    const double* J = A.joints + (size_t)first * 54;
    const double nan = __builtin_nan("");

    for (int q = tid; q < RS_SIDES * 256; q += RS_THREADS) s_hist[q] = 0u;
    if (tid < RS_SIDES) s_cnt[tid] = 0;
    __syncthreads();

    // the ten values of every pose (NaN: the pose gives the side none); side sd of pose p at sd m + p
    for (int q = tid; q < RS_SIDES * m; q += RS_THREADS) {
#pragma clang fp contract(off)
        const int p = q / RS_SIDES, sd = q - p * RS_SIDES;
        const double* P = J + (size_t)p * 54;
        const double lo = reid_bone(P, RS_LO[sd]);
        double x = lo;
        bool ok = isfinite(lo);
        if (RS_HI[sd] >= 0) {
            const double hi = reid_bone(P, RS_HI[sd]);
            ok = ok && isfinite(hi);
            x = (lo + hi) / 2.0;
        }
        if (!ok) x = nan;
        if (in_lds) s_val[sd * m + p] = x; else gval[(size_t)sd * m + p] = x;
        if (ok) atomicAdd(&s_cnt[sd], 1);
    }
    if (tid < 6) {          // the centroids of the first and the last pose: the mean of the 18 joints, summed in joint order
        const double* P = J + (size_t)(tid < 3 ? 0 : m - 1) * 54;
        const int c = tid < 3 ? tid : tid - 3;
        double sum = 0.0;
        for (int k = 0; k < 18; ++k) sum = sum + P[3 * k + c];
        A.ends[(size_t)r * 6 + tid] = sum / 18.0;
    }
    __syncthreads();

    const int wave = tid >> 6, lane = tid & 63;
    double mad_of = nan;        // lanes 0 .. 9: the side's mad
    for (int mode = 0; mode < 2; ++mode) {      // 0: the lower median of x; 1: of |x - med|
        if (tid < RS_SIDES) { s_prefix[tid] = 0ull; s_k[tid] = (s_cnt[tid] - 1) / 2; }
        __syncthreads();
        for (int pass = 0; pass < 8; ++pass) {
            const int shift = 56 - 8 * pass;
            for (int sd = 0; sd < RS_SIDES; ++sd) {
                if (s_cnt[sd] == 0) continue;
                const unsigned long long prefix = s_prefix[sd];
                const double med = mode == 0 ? 0.0 : s_med[sd];
                for (int i = tid; i < m; i += RS_THREADS) {
                    const double x = in_lds ? s_val[sd * m + i] : gval[(size_t)sd * m + i];
                    if (!(x == x)) continue;
                    const unsigned long long key = (unsigned long long)__double_as_longlong(mode == 0 ? x : fabs(x - med));
                    if (pass == 0 || (key >> (shift + 8)) == prefix) atomicAdd(&s_hist[sd * 256 + (int)((key >> shift) & 255ull)], 1u);
                }
            }
            __syncthreads();
            for (int sd = wave; sd < RS_SIDES; sd += RS_THREADS / 64) {     // one wave per side: the digit that holds rank k
                unsigned int* h = s_hist + sd * 256 + 4 * lane;
                const unsigned int h0 = h[0], h1 = h[1], h2 = h[2], h3 = h[3];
                h[0] = 0u; h[1] = 0u; h[2] = 0u; h[3] = 0u;
                const int c = (int)(h0 + h1 + h2 + h3);
                int incl = c;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const int t = __shfl_up(incl, o);
                    if (lane >= o) incl += t;
                }
                const int k = s_k[sd], excl = incl - c;
                if (s_cnt[sd] > 0 && excl <= k && k < incl) {
                    int left = k - excl, b = 0;
                    if (left >= (int)h0) { left -= (int)h0; b = 1;
                        if (left >= (int)h1) { left -= (int)h1; b = 2;
                            if (left >= (int)h2) { left -= (int)h2; b = 3; } } }
                    s_prefix[sd] = (s_prefix[sd] << 8) | (unsigned long long)(4 * lane + b);
                    s_k[sd] = left;
                }
            }
            __syncthreads();
        }
        if (tid < RS_SIDES) {
            const double v = s_cnt[tid] > 0 ? __longlong_as_double((long long)s_prefix[tid]) : nan;
            if (mode == 0) s_med[tid] = v; else mad_of = v;
        }
        __syncthreads();
    }
    if (tid < RS_SIDES) {
#pragma clang fp contract(off)
        const int c = s_cnt[tid];
        const bool defined = c >= A.min_poses;
        A.sig[(size_t)r * 20 + tid] = defined ? s_med[tid] : nan;
        A.sig[(size_t)r * 20 + RS_SIDES + tid] = defined ? 1.4826 * mad_of * 1.2533 / sqrt((double)c) : nan;
        A.cnt[(size_t)r * RS_SIDES + tid] = c;
    }
    if (tid == 0) A.status[r] = 0;
}

// LINKS.  Per sequence the records are nodes in (first frame, track id) order.  z(A, B) = sqrt(mean over the sides defined in both of
// (l_A - l_B)^2 / (se_A^2 + se_B^2 + 2 floor^2)), summed in side order, undefined (NaN) with fewer than 5 common sides.  A -> B is a
// candidate when A != B, gap = B.first - A.last >= 1 (<= max_gap when one is given), z <= max_z, and the centroid of B's first pose
// lies within reach + speed gap of the centroid of A's last pose (a non-finite distance allows nothing).  VETO: two records overlap
// when Q.first <= R.last and R.first <= Q.last; the candidate is refused when some other record Q overlaps B but not A and z(A, B) >
// ratio z(A, Q), or overlaps A but not B and z(A, B) > ratio z(Q, B) (an undefined z vetoes nothing; a Q that overlaps both ends
// does not compete).  The n x 2n matrix holds z where allowed, RL_BIG elsewhere, max_z in a row's dummy column; the assignment and
// the chains are mvmc_relink's (assign_and_chain).  One 256-lane workgroup per sequence: the symmetric z matrix is kept (LDS up to
// RL_LDS_N records, where the allowed entries are marked in a bit mask and the matrix becomes the cost matrix in place; the
// workspace beyond, z and costs side by side), so the O(n^3) veto loop reads it instead of recomputing distances.
struct ReidLinkArgs {
    const double* sig;        // (N, 20)
    const double* ends;       // (N, 6)
    const int32_t* frames;    // (N, 2): first frame, last frame
    const int32_t* seq;       // (S, 4): first record, records, offset into work (doubles), 0
    int n_records, max_gap;   // max_gap 0: no bound
    double max_z, ratio, floor2, reach, speed;      // floor2 = 2 floor^2
    int32_t *succ, *head, *pos;
    double* link_cost;
    int32_t* status;
    double* work;
    long long work_doubles;
};

__device__ inline double reid_z(const double* sa, const double* sb, double floor2) {
#pragma clang fp contract(off)
    double sum = 0.0;
    int c = 0;
    for (int q = 0; q < RS_SIDES; ++q) {
        const double la = sa[q], lb = sb[q], ea = sa[RS_SIDES + q], eb = sb[RS_SIDES + q];
        if (!(la == la && lb == lb && ea == ea && eb == eb)) continue;
        const double d = la - lb;
        sum += (d * d) / ((ea * ea + eb * eb) + floor2);
        ++c;
    }
    return c >= 5 ? sqrt(sum / (double)c) : __builtin_nan("");
}

__device__ inline bool reid_overlap(const int32_t* fq, const int32_t* fr) { return fq[0] <= fr[1] && fr[0] <= fq[1]; }

// A -> B passes every condition but the veto (rows a, b of frames / ends; z = z(A, B))
__device__ inline bool reid_gate(const ReidLinkArgs& A, int a, int b, double z) {
#pragma clang fp contract(off)
    const long long gap = (long long)A.frames[(size_t)b * 2] - (long long)A.frames[(size_t)a * 2 + 1];
    if (a == b || gap < 1 || (A.max_gap > 0 && gap > A.max_gap)) return false;
    if (!(z <= A.max_z)) return false;
    const double* ea = A.ends + (size_t)a * 6 + 3;
    const double* eb = A.ends + (size_t)b * 6;
    const double dx = eb[0] - ea[0], dy = eb[1] - ea[1], dz = eb[2] - ea[2];
    const double d = sqrt(dx * dx + dy * dy + dz * dz);
    return isfinite(d) && d <= A.reach + A.speed * (double)gap;
}

__global__ void __launch_bounds__(RL_THREADS)
reid_link_kernel(ReidLinkArgs A) {
    __shared__ double s_cost[RL_LDS_N * RL_LDS_N];
    __shared__ unsigned long long s_mask[RL_LDS_N];

    const int s = blockIdx.x, tid = threadIdx.x;
    const int off = A.seq[(size_t)s * 4], n = A.seq[(size_t)s * 4 + 1], woff = A.seq[(size_t)s * 4 + 2];
    const bool in_lds = n <= RL_LDS_N;
    bool bad = off < 0 || n < 0 || n > RL_CAP || (long long)off + n > A.n_records;
    if (!bad && !in_lds) bad = !A.work || woff < 0 || (long long)woff + 2ll * n * n > A.work_doubles;
    if (bad) {
        if (tid == 0) A.status[s] = 2;
        return;
    }
    if (n == 0) {
        if (tid == 0) A.status[s] = 0;
        return;
    }
    double* gz = in_lds ? nullptr : A.work + woff;
    double* gcost = in_lds ? nullptr : gz + (size_t)n * n;
    auto z_at = [&](int i, int j) -> double { return in_lds ? s_cost[i * n + j] : gz[(size_t)i * n + j]; };

    // 1. the z matrix
    for (int q = tid; q < n * n; q += RL_THREADS) {
        const int i = q / n, j = q - i * n;
        const double z = reid_z(A.sig + (size_t)(off + i) * 20, A.sig + (size_t)(off + j) * 20, A.floor2);
        if (in_lds) s_cost[q] = z; else gz[q] = z;
    }
    if (tid < RL_LDS_N) s_mask[tid] = 0ull;
    __syncthreads();
    // the gates and the veto
    const int32_t* fr = A.frames + (size_t)off * 2;
    for (int q = tid; q < n * n; q += RL_THREADS) {
        const int i = q / n, j = q - i * n;
        const double z = z_at(i, j);
        bool ok = reid_gate(A, off + i, off + j, z);
        for (int k = 0; ok && k < n; ++k) {
            if (k == i || k == j) continue;
            const bool ovi = reid_overlap(fr + 2 * k, fr + 2 * i), ovj = reid_overlap(fr + 2 * k, fr + 2 * j);
            if (ovj && !ovi && z > A.ratio * z_at(i, k)) ok = false;
            if (ovi && !ovj && z > A.ratio * z_at(k, j)) ok = false;
        }
        if (in_lds) { if (ok) atomicOr(&s_mask[i], 1ull << j); }
        else gcost[q] = ok ? z : RL_BIG;
    }
    __syncthreads();
    if (in_lds)
        for (int q = tid; q < n * n; q += RL_THREADS) {
            const int i = q / n, j = q - i * n;
            if (!((s_mask[i] >> j) & 1ull)) s_cost[q] = RL_BIG;
        }
    const bool fail = assign_and_chain(n, off, A.max_z, [&](int i, int j) -> double {
        return in_lds ? s_cost[i * n + j] : gcost[(size_t)i * n + j];
    }, A.succ, A.head, A.pos, A.link_cost);
    if (tid == 0) A.status[s] = fail ? 1 : 0;
}

}  // namespace

extern "C" long long mvmc_reid_work_words(int n_records) {
    if (n_records < 0 || n_records > RL_CAP) return -1;
    return n_records <= RL_LDS_N ? 0 : 2ll * n_records * n_records;
}

extern "C" int mvmc_reid_signature(const double* joints, const int32_t* rec, int n_poses, int n_records, int min_poses, double* sig,
                                   int32_t* cnt, double* ends, int32_t* status, double* work, long long work_words,
                                   mvmcStream_t stream) {
    if (n_poses < 0 || n_records < 0 || min_poses < 1 || work_words < 0 || (work_words > 0 && !work)) return MVMC_ERR_ARG;
    if (n_records == 0) return MVMC_OK;
    if (!rec || !sig || !cnt || !ends || !status || (n_poses > 0 && !joints)) return MVMC_ERR_ARG;
    ReidSigArgs A;
    A.joints = joints; A.rec = rec; A.n_poses = n_poses; A.min_poses = min_poses;
    A.sig = sig; A.cnt = cnt; A.ends = ends; A.status = status; A.work = work; A.work_doubles = work_words;
    hipLaunchKernelGGL(reid_signature_kernel, dim3(n_records), dim3(RS_THREADS), 0, (hipStream_t)stream, A);
    MVMC_CHECK_LAUNCH();
    return MVMC_OK;
}

extern "C" int mvmc_reid_link(const double* sig, const double* ends, const int32_t* frames, const int32_t* seq, int n_records,
                              int n_seqs, int max_gap, double max_z, double ratio, double floor, double reach, double speed,
                              int32_t* succ, int32_t* head, int32_t* pos, double* link_cost, int32_t* status, double* work,
                              long long work_words, mvmcStream_t stream) {
    if (n_records < 0 || n_seqs < 0 || max_gap < 0 || work_words < 0 || (work_words > 0 && !work)) return MVMC_ERR_ARG;
    if (!(max_z >= 0.0 && max_z < RL_BIG) || !(ratio >= 0.0 && ratio <= 1.0) || !(floor >= 0.0 && floor < RL_BIG) ||
        !(reach >= 0.0 && reach < RL_BIG) || !(speed >= 0.0 && speed < RL_BIG))
        return MVMC_ERR_ARG;
    if (n_seqs == 0) return MVMC_OK;
    if (!seq || !status || (n_records > 0 && (!sig || !ends || !frames || !succ || !head || !pos || !link_cost))) return MVMC_ERR_ARG;
    ReidLinkArgs A;
    A.sig = sig; A.ends = ends; A.frames = frames; A.seq = seq; A.n_records = n_records; A.max_gap = max_gap;
    A.max_z = max_z; A.ratio = ratio; A.floor2 = 2.0 * (floor * floor); A.reach = reach; A.speed = speed;
    A.succ = succ; A.head = head; A.pos = pos; A.link_cost = link_cost; A.status = status; A.work = work; A.work_doubles = work_words;
    hipLaunchKernelGGL(reid_link_kernel, dim3(n_seqs), dim3(RL_THREADS), 0, (hipStream_t)stream, A);
    MVMC_CHECK_LAUNCH();
    return MVMC_OK;
}

extern "C" long long mvmc_relink_work_words(int n_records) {
    if (n_records < 0 || n_records > RL_CAP) return -1;
    return n_records <= RL_LDS_N ? 0 : (long long)n_records * n_records;
}

extern "C" int mvmc_relink(const double* rec, const int32_t* frames, const int32_t* seq, int n_records, int n_seqs, int max_gap,
                           double max_dist, double near_dist, double speed, int32_t* succ, int32_t* head, int32_t* pos,
                           double* link_cost, int32_t* status, double* work, long long work_words, mvmcStream_t stream) {
    if (n_records < 0 || n_seqs < 0 || max_gap < 1 || work_words < 0 || (work_words > 0 && !work)) return MVMC_ERR_ARG;
    if (!(max_dist >= 0.0 && max_dist < RL_BIG) || !(near_dist >= 0.0 && near_dist < RL_BIG) || !(speed >= 0.0 && speed < RL_BIG))
        return MVMC_ERR_ARG;
    if (n_seqs == 0) return MVMC_OK;
    if (!seq || !status || (n_records > 0 && (!rec || !frames || !succ || !head || !pos || !link_cost))) return MVMC_ERR_ARG;
    RelinkArgs A;
    A.rec = rec; A.frames = frames; A.seq = seq; A.n_records = n_records; A.max_gap = max_gap;
    A.max_dist = max_dist; A.near_dist = near_dist; A.speed = speed;
    A.succ = succ; A.head = head; A.pos = pos; A.link_cost = link_cost; A.status = status; A.work = work; A.work_doubles = work_words;
    hipLaunchKernelGGL(relink_kernel, dim3(n_seqs), dim3(RL_THREADS), 0, (hipStream_t)stream, A);
    MVMC_CHECK_LAUNCH();
    return MVMC_OK;
}
