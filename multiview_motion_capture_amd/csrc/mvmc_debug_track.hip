// Diagnostic entry points of the temporal layer (declared in include/mvmc.h under "diagnostics"): the forms of mvmc_track.hip's device
// functions that only the chain kernels call -- st_affinity_wave on a whole workgroup with a pose-pair block made ahead of it
// (st_pose_pairs, st_pose_pairs_lines + st_stage_keypoints), the 64-lane ballot form of assign_chain, the multi-lane commit_chain --
// on caller-supplied data, so that tests can compare them with the stand-alone kernels (mvmc_st_affinity, mvmc_track_assign,
// mvmc_track_commit) at inputs the chain kernels' own workloads never produce (tests/test_gpu_track_kernels.py).
#define MVMC_DEVICE_ONLY
#include "mvmc_common.h"
#include "mvmc_track.hip"
#undef MVMC_DEVICE_ONLY

namespace {

// LDS, in doubles: [ st_affinity_wave's part (NS*NS + 10 doubles + 2 NS ints), the line tables before it (2 * 4 * P * 85) | the
// frame's keypoints (N * 51) | the pose-pair block (N * N) ], the order of the chain kernel's BIG arena (mvmc_chain.hip: CH_KOFF_BIG)
__host__ __device__ inline int dbg_st_head_doubles(int NS, int P, int pair_form) {
    int a = NS * NS + 10 + NS, l = pair_form == 2 ? 2 * 4 * P * 85 : 0;
    a = a > l ? a : l;
    return (a + 1) & ~1;
}

template <int NT>
__global__ void __launch_bounds__(NT)
debug_st_affinity_wg_kernel(const double* __restrict__ kps17, const int32_t* __restrict__ counts, const int32_t* __restrict__ frame_idx,
                            const double* __restrict__ track_joints, const int32_t* __restrict__ n_tracks,
                            const double* __restrict__ Pm, const double* __restrict__ F2, int C, int P, int T, double min_score,
                            int pair_form, double* __restrict__ W, double* __restrict__ Dout, int32_t* __restrict__ group_counts) {
    extern __shared__ double sm[];
    const int b = blockIdx.x, f = frame_idx[b], N = C * P;
    double* kf = sm + dbg_st_head_doubles(T + N, P, pair_form);
    double* E = kf + N * 51;
    const double* Epre = nullptr;
    const double* kf_lds = nullptr;
    if (pair_form == 1) {            // the SMALL layout: the block from global keypoints, which the wave reads from there too
        st_pose_pairs(E, kps17, counts, f, F2, C, P, min_score);
        __syncthreads();
        Epre = E;
    } else if (pair_form == 2) {     // the BIG layout: keypoints staged in LDS, the block by line tables in the wave's own part
        st_stage_keypoints(kf, kps17, f, C, P);
        __syncthreads();
        st_pose_pairs_lines<NT>(E, sm, kf, counts, f, F2, C, P, min_score);
        Epre = E;
        kf_lds = kf;
    }
    st_affinity_wave<NT>(sm, kps17, counts, b, f, track_joints, n_tracks, Pm, F2, C, P, T, min_score, W, Dout, group_counts, Epre, N,
                         kf_lds);
}

__global__ void __launch_bounds__(64)
debug_assign_wave_kernel(const int32_t* __restrict__ labels_sp, const int32_t* __restrict__ ncl_sp, const int32_t* __restrict__ labels_st,
                         const int32_t* __restrict__ ncl_st, const int32_t* __restrict__ counts, const int32_t* __restrict__ frame_idx,
                         const int32_t* __restrict__ n_tracks, const double* __restrict__ track_params, int C, int P, int T, int K, int V,
                         int32_t* __restrict__ members, int32_t* __restrict__ n_members, uint8_t* __restrict__ cold,
                         double* __restrict__ init, int32_t* __restrict__ status, int32_t* __restrict__ n_new,
                         int32_t* __restrict__ overflow) {
    const int b = blockIdx.x;
    assign_chain(threadIdx.x, 64, b, frame_idx[b], labels_sp, ncl_sp, labels_st, ncl_st, counts, n_tracks, track_params, C, P, T, K, V,
                 members, cold, init, status, n_new, overflow ? overflow + b : nullptr, n_members);
}

__global__ void __launch_bounds__(64)
debug_commit_wave_kernel(const int32_t* __restrict__ status, const int32_t* __restrict__ n_new, const double* __restrict__ ik_params,
                         const double* __restrict__ ik_joints, int T, int K, int n_inits, double* __restrict__ track_params,
                         double* __restrict__ track_joints, int32_t* __restrict__ meta, int32_t* __restrict__ n_tracks,
                         int32_t* __restrict__ next_id, int32_t* __restrict__ n_dead, int32_t* __restrict__ slot_src,
                         int32_t* __restrict__ overflow) {
    const int b = blockIdx.x;
    commit_chain(threadIdx.x, 64, b, status, n_new, ik_params, ik_joints, T, K, n_inits, track_params, track_joints, meta, n_tracks,
                 next_id, n_dead, slot_src, overflow ? overflow + b : nullptr);
}

}  // namespace

extern "C" int mvmc_debug_st_affinity_wg(const double* kps17, const int32_t* counts, const int32_t* frame_idx,
                                         const double* track_joints, const int32_t* n_tracks, const double* Pmats, const double* F2,
                                         int n_chains, int n_views, int p_max, int t_max, double min_score, int nt_threads,
                                         int pair_form, double* W, double* D, int32_t* group_counts, mvmcStream_t stream) {
    if (!kps17 || !counts || !frame_idx || !track_joints || !n_tracks || !Pmats || !F2 || !W || !group_counts) return MVMC_ERR_ARG;
    if (n_views <= 0 || p_max <= 0 || t_max <= 0) return MVMC_ERR_ARG;
    if ((nt_threads != 256 && nt_threads != 512) || pair_form < 0 || pair_form > 2) return MVMC_ERR_ARG;
    const int N = n_views * p_max, NS = t_max + N;
    if (NS > MVMC_MAX_NODES) return MVMC_ERR_UNSUPPORTED;
    const size_t lds = ((size_t)dbg_st_head_doubles(NS, p_max, pair_form) + (size_t)N * 51 + (size_t)N * N) * sizeof(double);
    if (lds > 160 * 1024) return MVMC_ERR_UNSUPPORTED;
    if (n_chains <= 0) return n_chains == 0 ? MVMC_OK : MVMC_ERR_ARG;
    auto launch = [&](auto kernel, int nt) -> int {
        if (lds > 65536 && hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return MVMC_ERR_LAUNCH;
        hipLaunchKernelGGL(kernel, dim3(n_chains), dim3(nt), lds, (hipStream_t)stream, kps17, counts, frame_idx, track_joints, n_tracks,
                           Pmats, F2, n_views, p_max, t_max, min_score, pair_form, W, D, group_counts);
        return MVMC_OK;
    };
    const int rc = nt_threads == 256 ? launch(debug_st_affinity_wg_kernel<256>, 256) : launch(debug_st_affinity_wg_kernel<512>, 512);
    if (rc != MVMC_OK) return rc;
    MVMC_CHECK_LAUNCH();
    return MVMC_OK;
}

extern "C" int mvmc_debug_track_wave(int phase, const int32_t* labels_sp, const int32_t* ncl_sp, const int32_t* labels_st,
                                     const int32_t* ncl_st, const int32_t* counts, const int32_t* frame_idx, int32_t* n_tracks,
                                     double* track_params, int n_chains, int n_views, int p_max, int t_max, int k_max, int v_max,
                                     int32_t* members, int32_t* n_members, uint8_t* cold, double* init_params, int32_t* status,
                                     int32_t* n_new, const double* ik_params, const double* ik_joints, int n_inits,
                                     double* track_joints, int32_t* meta, int32_t* next_id, int32_t* n_dead, int32_t* slot_src,
                                     int32_t* overflow, mvmcStream_t stream) {
    if (phase != 0 && phase != 1) return MVMC_ERR_ARG;
    if (!n_tracks || !track_params || !status || !n_new || t_max <= 0 || k_max <= 0) return MVMC_ERR_ARG;
    if (t_max > 16) return MVMC_ERR_UNSUPPORTED;      // the ballot form's `1ull << nt`, the chain layouts' own bound
    if (phase == 0) {
        if (!labels_sp || !ncl_sp || !labels_st || !ncl_st || !counts || !frame_idx || !members || !cold || !init_params)
            return MVMC_ERR_ARG;
        if (n_views <= 0 || p_max <= 0 || v_max <= 0) return MVMC_ERR_ARG;
        if (n_views > 16 || n_views * p_max > 64) return MVMC_ERR_UNSUPPORTED;   // 16 + 64 nodes: the two ballot words
    } else if (!ik_params || !ik_joints || !track_joints || !meta || !next_id || !n_dead)
        return MVMC_ERR_ARG;
    if (n_chains <= 0) return n_chains == 0 ? MVMC_OK : MVMC_ERR_ARG;
    if (phase == 0)
        hipLaunchKernelGGL(debug_assign_wave_kernel, dim3(n_chains), dim3(64), 0, (hipStream_t)stream, labels_sp, ncl_sp, labels_st,
                           ncl_st, counts, frame_idx, n_tracks, track_params, n_views, p_max, t_max, k_max, v_max, members, n_members,
                           cold, init_params, status, n_new, overflow);
    else
        hipLaunchKernelGGL(debug_commit_wave_kernel, dim3(n_chains), dim3(64), 0, (hipStream_t)stream, status, n_new, ik_params,
                           ik_joints, t_max, k_max, n_inits, track_params, track_joints, meta, n_tracks, next_id, n_dead, slot_src,
                           overflow);
    MVMC_CHECK_LAUNCH();
    return MVMC_OK;
}
