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

__global__ void __launch_bounds__(RL_THREADS)
relink_kernel(RelinkArgs A) {
    __shared__ double s_cost[RL_LDS_N * RL_LDS_N];
    __shared__ double s_u[RL_CAP + 1], s_v[2 * RL_CAP + 1], s_minv[2 * RL_CAP + 1];
    __shared__ int s_p[2 * RL_CAP + 1], s_way[2 * RL_CAP + 1];
    __shared__ unsigned char s_used[2 * RL_CAP + 1];
    __shared__ double s_redv[RL_THREADS / 64];
    __shared__ int s_redj[RL_THREADS / 64];
    __shared__ int s_fail, s_rows;

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
    const int m = 2 * n;

    // 1. the real part of the matrix
    for (int q = tid; q < n * n; q += RL_THREADS) {
        const int i = q / n, j = q - i * n;
        const double c = link_cost_of(A, off + i, off + j);
        if (in_lds) s_cost[q] = c; else gcost[q] = c;
    }
    for (int j = tid; j <= m; j += RL_THREADS) { s_v[j] = 0.0; s_p[j] = 0; s_way[j] = 0; }
    for (int i = tid; i <= n; i += RL_THREADS) s_u[i] = 0.0;
    if (tid == 0) { s_fail = 0; s_rows = 0; }
    __syncthreads();
    const double max_dist = A.max_dist;
    auto cost = [&](int i, int j) -> double {      // row i, column j, both from 0
        if (j >= n) return j - n == i ? max_dist : RL_BIG;
        return in_lds ? s_cost[i * n + j] : gcost[(size_t)i * n + j];
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
    if (fail) {
        if (tid == 0) A.status[s] = 1;
        return;
    }
    for (int j = 1 + tid; j <= n; j += RL_THREADS) {
        const int r = s_p[j] - 1;
        if (r < 0 || r >= n) continue;
        const double c = cost(r, j - 1);
        if (c < RL_BIG) { s_succ[r] = j - 1; s_pred[j - 1] = r; A.link_cost[off + r] = c; }
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
        if (s_succ[k] < 0) A.link_cost[off + k] = 0.0;
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
        A.succ[off + k] = s_succ[k];
        A.head[off + k] = s_ptr[k];
        A.pos[off + k] = s_dist[k];
    }
    if (tid == 0) A.status[s] = 0;
}

}  // namespace

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
