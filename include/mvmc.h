/*
 * mvmc.h -- C ABI of the MI355X (gfx950) hot path of multi-view motion capture:
 * cross-view association -> multi-view DLT triangulation -> temporal IK.
 *
 * The reference (khanhha/multiview_motion_capture) is pure Python and has no
 * FFI of its own; the boundary it offers is a set of Python callables
 * (SURVEY.md section 8b).  Each entry point below is the batched device form
 * of one of those callables and cites the reference function it replaces
 * (file:line relative to the reference checkout).  The Python mirror in
 * multiview_motion_capture_amd/ binds them with ctypes and keeps the
 * reference's names and signatures.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the parameter name ends in
 *     `_host`; the caller owns all buffers, nothing is allocated or freed and
 *     nothing synchronises inside a call (safe for hipGraph capture);
 *   - `stream` is a hipStream_t (NULL = default stream);
 *   - return value: MVMC_OK or an MVMC_ERR_* code, never an exception;
 *   - tensors are dense row-major; shapes are written (d0,d1,...).
 *   - a "pose" is 17 COCO joints x (x, y, score) in float64; poses of a batch
 *     live in one array `kps17` of shape (F, C, P, 17, 3); pose index
 *     q = (f*C + c)*P + p, so the camera of pose q is (q / P) % C.
 */
#ifndef MVMC_H
#define MVMC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MVMC_ABI_VERSION 6

enum {
    MVMC_OK = 0,
    MVMC_ERR_ARG = 1,         /* bad shape / null pointer / unsupported size */
    MVMC_ERR_LAUNCH = 2,      /* hipLaunch / runtime error */
    MVMC_ERR_UNSUPPORTED = 3  /* size outside the compiled kernel variants */
};

enum { MVMC_F32 = 0, MVMC_F64 = 1 };

#define MVMC_N_COCO 17
#define MVMC_N_SKEL 18
#define MVMC_N_SIDE 11
#define MVMC_N_PARAM 68   /* root(3) + euler(18*3) + side bone lengths(11) */
#define MVMC_MAX_NODES 80 /* max graph nodes (2-D poses + tracklets) per frame: C8 P8 + 16 tracklets */

typedef void* mvmcStream_t; /* hipStream_t */

/* Skeleton constants (inverse_kinematics.py:94-117 Skeleton, :120-173 load_skeleton).
 * Host struct, passed by pointer and copied into the kernel arguments. */
typedef struct {
    double bone_dirs[MVMC_N_SKEL][3]; /* ref_bone_dirs */
    int32_t parents[MVMC_N_SKEL];     /* joint_parents (-1 for the root) */
    int32_t side_map[MVMC_N_SKEL];    /* ref_side_to_full_bone_lens_map */
    int32_t n_side;                   /* number of side lengths (11; 18 = identity map of the old pickle schema) */
    double ref_side_lens[MVMC_N_SKEL]; /* ref_side_bone_lens (first n_side entries): cold-start lengths */
} mvmcSkeleton;

int mvmc_abi_version(void);
const char* mvmc_status_string(int status);

/* Host helper: first `count` doubles of numpy.random.RandomState(0).rand()
 * (MT19937, init_genrand(0), 53-bit doubles).  match_als seeds its factor with
 * RandomState(0).rand(n, r) (mv_association.py:271) == table[i*r + j]. */
int mvmc_als_seed_table(double* out_host, int count);

/* IN-1 + IN-2: OpenPose-25 -> COCO-17 gather (pose_def.py:262-270,
 * motion_capture.py:980-983) and filter_bad_pose(0.01, 4, 5)
 * (motion_capture.py:1023-1043) with per-view compaction (order kept).
 *   kps        (F,C,P,J_in,3) f32|f64, J_in = 25 (gathered) or 17 (copied)
 *   counts_in  (F,C) people per view, or NULL = P everywhere
 *   kps17      (F,C,P,17,3) f64 out (slots >= counts_out are zero)
 *   counts_out (F,C) people kept per view */
int mvmc_ingest(const void* kps, int dtype, int n_frames, int n_views, int p_max, int n_joints_in,
                const int32_t* counts_in, double min_score, int min_valid, double min_bb_size,
                double* kps17, int32_t* counts_out, mvmcStream_t stream);

/* AS-1: calc_pairwise_f_mats (mv_math_util.py:267-285).  K (C,3,3), Rt (C,3,4) f64 -> F (C,C,3,3) f32. */
int mvmc_fmats(const double* K, const double* Rt, int n_views, float* F, mvmcStream_t stream);

/* AS-2 + AS-3: geometry_affinity (mv_math_util.py:320-351) with projected_distance (:288-317).
 * Graph nodes of frame f = its poses in (view, person) order; n_f = sum_c counts[f,c].
 *   D, S  (F,N,N) f32 out with N = C*P (only [0:n_f,0:n_f] is meaningful, rest 0); either may be NULL
 * Both are the reference's bit for bit: the float32 statistics in NumPy's pairwise order, and the sigmoid's exp as NumPy's float32 exp
 * (AVX2 / AVX-512F form: Cody-Waite reduction, P5 / Q2, fused steps -- not the correctly-rounded function; np_exp_f32 in csrc/mvmc_common.h). */
int mvmc_affinity(const double* kps17, const int32_t* counts, const float* Fmats, int n_frames, int n_views,
                  int p_max, float* D, float* S, mvmcStream_t stream);

/* AS-4 + AS-5 + AS-6: match_als (mv_association.py:222-318), transform_closure (:99-121) and the
 * cluster rule of parse_match_result (motion_capture.py:417-425).
 *   W            (F,N,N) f32|f64 affinity in compact node order (leading dimension N)
 *   group_counts (F,G) nodes per group (views; for match_spatial_time group 0 = tracklets)
 *   g_max        upper bound of any group's node count (rank <= min(n, 2*g_max) selects the kernel variant)
 *   seed_table   first seed_len doubles of RandomState(0).rand() (mvmc_als_seed_table)
 *   x_bin, match_mat  (F,N,N) u8 out, may be NULL
 *   labels       (F,N) i32 out: cluster ordinal of each node, -1 = in no cluster of >= 2 members
 *   n_clusters   (F) i32 out (kept columns); iters (F) i32 out (ALS iterations run) */
int mvmc_als_associate(const void* W, int w_dtype, const int32_t* group_counts, int n_frames, int n_groups,
                       int n_max, int g_max, const double* seed_table, int seed_len, uint8_t* x_bin, uint8_t* match_mat,
                       int32_t* labels, int32_t* n_clusters, int32_t* iters, mvmcStream_t stream);

/* AS-5 + AS-6 alone: transform_closure (mv_association.py:99-121) and the cluster rule of
 * parse_match_result (motion_capture.py:419-425) on a caller-supplied binary matrix.
 *   x_bin (F,N,N) u8, n_nodes (F) i32 -> match_mat (F,N,N) u8 (may be NULL), labels (F,N), n_clusters (F) */
int mvmc_closure_labels(const uint8_t* x_bin, const int32_t* n_nodes, int n_frames, int n_max, uint8_t* match_mat,
                        int32_t* labels, int32_t* n_clusters, mvmcStream_t stream);

/* match_svt (mv_association.py:321-411): ADMM with singular-value thresholding and the doubly-stochastic block projection
 * (myproj2dpam, :15-60); the matcher match_multiview_poses can select instead of match_als.  pSelect = 1 (the reference's default).
 *   S            (F,N,N) f32|f64 affinity in compact node order (leading dimension N <= 64); not modified (the reference zeroes
 *                the diagonal of its argument; the symmetrised, zero-diagonal copy lives on the device here)
 *   group_counts (F,G) nodes per group, G <= 16; g_max upper bound of any group's node count (<= 16)
 *   alpha, lambda, mu, tol, max_iter, dual_stochastic: the reference's keyword arguments (0.1, 50, 64, 5e-4, 20, 1)
 *   work         (F,3,N,N) f64 device workspace (Y and the two projection states)
 *   x_bin        (F,N,N) u8 out: (X + X^T) / 2 > 0.5;  x_out (F,N,N) f64 out or NULL: X itself
 *   iters        (F) i32 out: SVD-equivalent decompositions run (info['iter'] + 1 when the tolerance was met, else max_iter);
 *                -1 for a refused row: a negative count, a count above the launch's group width (8 when g_max <= 8, else 16),
 *                or counts that sum beyond N.  Such a row gets zero x_bin / x_out and leaves its work slice untouched
 * Arithmetic is float64 for either input type.  Follow with mvmc_closure_labels for match_mat / cluster labels. */
int mvmc_svt_associate(const void* S, int s_dtype, const int32_t* group_counts, int n_frames, int n_groups, int n_max,
                       int g_max, double alpha, double lambda, double mu, double tol, int max_iter, int dual_stochastic,
                       double* work, uint8_t* x_bin, double* x_out, int32_t* iters, mvmcStream_t stream);

/* Turns labels into member lists: members (F,K,V) pose index q (ascending node order, -1 padded),
 * n_members (F,K).  Clusters beyond K or members beyond V are dropped (n_members still counts them). */
int mvmc_cluster_members(const int32_t* labels, const int32_t* counts, int n_frames, int n_views, int p_max,
                         int k_max, int v_max, int32_t* members, int32_t* n_members, mvmcStream_t stream);

/* TR-1 + TR-2: triangulate_point_groups_from_multiple_views_linear(post_optimize=False)
 * (mv_math_util.py:152-187, :215-240).  One problem = one member list.
 *   kps     (n_poses,J,3) f64 (J = n_joints; 17 on the batched path, 18 with the synthetic mid-spine);
 *   Pmats (C,3,4) f64; members (B,V) pose indices (-1 = unused slot)
 *   out     (B,J,4) f64: x, y, z, mean score of the views used; problems with < 1 member give NaN */
int mvmc_dlt(const double* kps, const double* Pmats, const int32_t* members, int n_problems, int v_max,
             int n_views, int p_max, int n_joints, double min_score, double* out, mvmcStream_t stream);

/* IN-1/IN-2 + TR-1/TR-2 in ONE pass over the raw keypoints (BASELINE config 2, triangulation only): mvmc_ingest followed by mvmc_dlt
 * on the 17 COCO joints, without the 17-joint tensor ever going to memory (a wave per frame keeps it in LDS): 12 C P J bytes in and
 * 17 x 32 bytes per cluster out per frame instead of the two-kernel form's extra 2 x 408 C P bytes.  Same results bit for bit.
 *   kps, dtype, n_joints_in, counts_in, ingest_min_score, min_valid, min_bb_size: as mvmc_ingest
 *   members (F,K,V) i32: the clusters of every frame as pose indices in mvmc_ingest's OUTPUT numbering, (f C + c) P + slot, all of
 *           frame f (-1 = unused); out (F,K,17,4) f64 as mvmc_dlt; counts_out (F,C) i32 or NULL: people per view after the filter */
int mvmc_ingest_dlt(const void* kps, int dtype, int n_frames, int n_views, int p_max, int n_joints_in, const int32_t* counts_in,
                    double ingest_min_score, int min_valid, double min_bb_size, const double* Pmats, const int32_t* members,
                    int k_max, int v_max, double min_score, double* out, int32_t* counts_out, mvmcStream_t stream);

/* The same pass with float32 keypoints in AND float32 points out -- SURVEY 8(d)'s I/O for config 2: 12 C P J bytes read and
 * 16 P J bytes written per frame, each point ONE 16-byte store.  The arithmetic is mvmc_ingest_dlt's (float64; the reference
 * triangulates in float64, mv_math_util.py:152-187,215-240); out (F,K,17,4) f32 = that result rounded once at the store.
 * MVMC_ERR_UNSUPPORTED for shapes the pipelined kernel does not hold (k_max * 17 > 192, n_views * p_max > 128, p_max > 16, ...):
 * use mvmc_ingest_dlt there. */
int mvmc_ingest_dlt_f32(const float* kps, int n_frames, int n_views, int p_max, int n_joints_in, const int32_t* counts_in,
                        double ingest_min_score, int min_valid, double min_bb_size, const double* Pmats, const int32_t* members,
                        int k_max, int v_max, double min_score, float* out, int32_t* counts_out, mvmcStream_t stream);

/* TR-2, post_optimize=True (mv_math_util.py:189-210): scipy least_squares(max_nfev = 2) on the unsigned
 * residual |proj - obs| * score with eps = 1e-6, i.e. one trust-region trial step from the DLT points, kept
 * only if it lowers the cost.  pts (B,J,4) is the output of mvmc_dlt, updated in place (x, y, z only). */
int mvmc_triangulate_postopt(const double* kps, const double* Pmats, const int32_t* members, int n_problems,
                             int v_max, int n_views, int p_max, int n_joints, double* pts, mvmcStream_t stream);

/* FK-1 + FK-2: foward_kinematics (inverse_kinematics.py:176-199) with Quaternions.from_euler /
 * transforms (Quaternions.py:449-462, :335-366).
 *   params (B,3+54+n_side) f64 = root, euler(18,3), bone lengths
 *   joints (B,18,3) out; G (B,18,4,4) out or NULL */
int mvmc_fk(const mvmcSkeleton* skel_host, const double* params, int n_problems, double* joints, double* G,
            mvmcStream_t stream);

/* IK-1..IK-4: PoseSolver.solve (inverse_kinematics.py:351-433) = two trust-region-reflective
 * least-squares stages (solve_pose_reproj :202-238, solve_pose_bone_lens_reproj :241-277; SciPy
 * least_squares defaults, max_nfev evaluations each).
 *   members      (B,V) pose indices into kps17 (-1 = none; v_max = V <= 64, every member is used)
 *   init_params  (B,68) warm-start parameters, ignored where cold[b] != 0
 *   cold         (B) u8: 1 = cold start (root = midpoint of the post-optimised DLT hips, zero angles,
 *                reference lengths, max_nfev_cold),
 *                0 = warm (max_nfev_warm); NULL = all cold
 *   params_out   (B,68); joints_out (B,18,3); info_out (B,8) f64 =
 *                {cost1, nfev1, status1, cost2, nfev2, status2, njev1+njev2, number of trust-region models that
 *                took the eigensolver fallback (no clean split between range and null space)} or NULL
 *   scratch      (B, MVMC_IK_SCRATCH_DOUBLES) f64 device workspace: the Householder vectors of each trust-region model
 *                and the eigenvectors of the (rare) eigensolver fallback; contents undefined before and after */
#define MVMC_IK_SCRATCH_DOUBLES 7680
int mvmc_ik_solve(const mvmcSkeleton* skel_host, const double* kps17, const double* Pmats,
                  const int32_t* members, int n_problems, int v_max, int n_views, int p_max,
                  const double* init_params, const uint8_t* cold, int max_nfev_cold, int max_nfev_warm,
                  double* params_out, double* joints_out, double* info_out, double* scratch, mvmcStream_t stream);

/* ---- temporal layer: match_spatial_time + tracker, batched over independent chains (sub-sequences) ---- */

/* AS-8 helper: get_fundamental_matrix(P_i, P_j) (mv_math_util.py:57-77) for every view pair.
 * Pmats (C,3,4) f64 -> F2 (C,C,3,3) f64 with x_j^T F2[i][j] x_i = 0. */
int mvmc_fmats_from_projections(const double* Pmats, int n_views, double* F2, mvmcStream_t stream);

/* AS-7/8/9: node graph of match_spatial_time (motion_capture.py:651-756) for one frame of every chain.
 * Nodes of chain b = its n_tracks[b] live tracklets (last FK joints), then the 2-D poses of frame
 * frame_idx[b] by view.  2D-2D different views: calc_epipolar_error (mv_math_util.py:80-115, score product
 * > 0.1); 2D-3D: reprojection_error (motion_capture.py:403-414); same view / 3D-3D: NaN -> nanmax + 1;
 * S = 1/(1+exp(5 (D-15)/30)) clamped (S < 1e-3 -> 0).  Chains with n_tracks == 0 get an empty graph (they
 * take the match_spatial path).
 *   track_joints (B,T,18,3) f64; min_score = 0.1 in the reference (motion_capture.py:696,714,725);
 *   W (B,NS,NS) f64 out, NS = T + C*P; D (B,NS,NS) raw distances (NaN kept) out or NULL;
 *   group_counts (B,C+1) i32 out = {n_tracks, people per view} */
int mvmc_st_affinity(const double* kps17, const int32_t* counts, const int32_t* frame_idx,
                     const double* track_joints, const int32_t* n_tracks, const double* Pmats, const double* F2,
                     int n_chains, int n_views, int p_max, int t_max, double min_score, double* W, double* D,
                     int32_t* group_counts, mvmcStream_t stream);

/* TK-1, first half (motion_capture.py:763-808 and :618-626): cluster labels -> IK problems of the frame.
 * Chains without tracklets read labels_sp (B,C*P) (match_spatial, every member kept); the others read
 * labels_st (B,T+C*P) (tracklet-anchored clusters, one pose per view, first wins).
 *   members (B,T+K,V) pose indices; cold (B,T+K) u8; init_params (B,T+K,68);
 *   status (B,T) i32: 0 unmatched (dies), 1 one view (kept, not updated), 2 updated; n_new (B) new tracklets;
 *   overflow (B) i32 in/out or NULL: bit 0 is OR-ed in where a cluster (more than k_max new ones) or a member (more than v_max
 *   views) was dropped for lack of room -- the reference has no such caps; k_max >= C*P / 2 and v_max >= C*P rule both out */
int mvmc_track_assign(const int32_t* labels_sp, const int32_t* ncl_sp, const int32_t* labels_st,
                      const int32_t* ncl_st, const int32_t* counts, const int32_t* frame_idx,
                      const int32_t* n_tracks, const double* track_params, int n_chains, int n_views, int p_max,
                      int t_max, int k_max, int v_max, int32_t* members, uint8_t* cold, double* init_params,
                      int32_t* status, int32_t* n_new, int32_t* overflow, mvmcStream_t stream);

/* TK-1, second half (MvTracklet.update / mark_missed / __init__, motion_capture.py:352-391, :924-963):
 * applies the frame's IK results to the tracklet table (order kept, survivors first, new ones appended).
 *   meta (B,T,4) i32 = {id, state (1 tentative, 2 confirmed), hits, length}; n_inits = 3 in the reference;
 *   slot_src (B,T) i32 out or NULL: IK problem slot each table entry was solved in this frame (-1 = not solved);
 *   overflow (B) i32 in/out or NULL: bit 1 is OR-ed in where a new tracklet did not fit the table of t_max slots */
int mvmc_track_commit(const int32_t* status, const int32_t* n_new, const double* ik_params, const double* ik_joints,
                      int n_chains, int t_max, int k_max, int n_inits, double* track_params, double* track_joints,
                      int32_t* meta, int32_t* n_tracks, int32_t* next_id, int32_t* n_dead, int32_t* slot_src,
                      int32_t* overflow, mvmcStream_t stream);

/* ---- multi-GPU glue.  No counterpart in the reference: its tracker is one sequential pass
 * (motion_capture.py:1062-1116).  A sequence is cut into chains that cold-start; contiguous chain ranges go to the GPUs; one
 * all-gather of the packed messages below; then the identities are stitched across ALL chain boundaries on every rank. ---- */

/* Message of one shard, in 4-byte words (n_chains_cap = chains the message has room for, >= the shard's own):
 *   [0,8)   header i32 {n_chains, chain_len, t_max, rows written, rows wanted, row_cap, n_frames, 0}; rows wanted > row_cap = overflow
 *   ids     (n_chains_cap) i32: number of local identities of each chain (the tracker's next_id)
 *   bounds  (n_chains_cap, 2, t_max, MVMC_BOUND_WORDS): tracklet table of the chain's first / last frame:
 *           {local id i32 or -1, 18 x 3 joints f32 (NaN when empty), pad}
 *   rows    (row_cap, MVMC_ROW_WORDS): one row per LIVE tracklet and frame, in frame order:
 *           {frame, slot, id, state, hits, length} i32, 54 joints f32, 68 parameters f32
 *   local   the shard's OWN stitch, made before the gather so that no rank repeats another's work:
 *           [0,8) i32 {identities that start in this shard, pairs matched at its inner chain boundaries, error word (bit 0: a chain
 *                 with more than id_cap ids, bit 1: an assignment did not terminate), void word (bit i = void_words[i] != 0), 0 ...}
 *           lmatch (n_chains_cap, t_max) i32: slot of the previous chain's last frame matched to slot s of this chain's first (-1;
 *                 the shard's first chain: -1, its boundary belongs to the gathered pass).  A live tracklet with a non-finite joint
 *                 is left out of the assignment: it matches nobody (-1) and its identity starts anew; the others are assigned
 *                 optimally among themselves
 *           lgid   (n_chains_cap, id_cap) i32: shard-local identity of (chain, local id), numbered in chain order; -1 = no such id */
#define MVMC_BOUND_WORDS 56
#define MVMC_ROW_WORDS 128
long long mvmc_pack_message_words(int n_chains_cap, int t_max, int row_cap, int id_cap);   /* -1 on bad arguments */
long long mvmc_pack_work_words(int n_frames, int chain_len, int id_cap);                  /* words of mvmc_pack_tracks' workspace */

/* Packs mvmc_chain_run's per-frame outputs (out_params (F,t_tables,68), out_joints (F,t_tables,18,3), out_meta (F,t_tables,4),
 * out_n_tracks (F)) and next_id (n_chains) into `message` (mvmc_pack_message_words words), then stitches the shard's own chain
 * boundaries (chain b-1 | b: optimal assignment -- Kuhn-Munkres -- of the last frame's tracklets to the first frame's on the mean
 * joint distance, pairs farther than max_dist metres dropped; tracklets with a non-finite joint take no part) and numbers its
 * identities locally (the `local` section).  n_frames = 0 (an empty shard) writes the header and an empty local section only; the
 * table pointers may then be NULL.
 *   t_tables  slots per frame of the tables; t_max <= 16 slots of the message: the SAME on every rank (a rank whose repair tier
 *             widened its tables still packs t_max slots; every frame's live tracklets must fit: more are cut and show as an
 *             overflow of rows wanted in no header -- callers pass t_max >= the widest table any rank can have)
 *   void_words (n_void_words <= 32) u32 device words or NULL: non-zero words (mvmc_chain_run's flags[B .. B + 3): hand-over time-out,
 *             graph too large, capacity exceeded) are recorded in the message, and every rank's stitch reports them (info[2] bit 2):
 *             a void step is seen by all ranks without any of them reading device memory before the collective
 *   work      mvmc_pack_work_words i32 device workspace */
int mvmc_pack_tracks(const double* out_params, const double* out_joints, const int32_t* out_meta, const int32_t* out_n_tracks,
                     const int32_t* next_id, int n_frames, int chain_len, int t_tables, int t_max, int n_chains_cap, int row_cap,
                     int id_cap, double max_dist, const uint32_t* void_words, int n_void_words, int32_t* work, void* message,
                     mvmcStream_t stream);

/* Stitches the chains of `world` gathered messages (rank order = sequence order; message r at messages + r * message_words words).
 * The inner boundaries of every shard arrive stitched (the `local` sections); here only the world - 1 boundaries between shards are
 * matched (same rule), local identities become global ones (roots numbered in chain order), and the tables are written -- the result
 * of one pass over all chain boundaries, at a cost per rank that does not grow with the number of chains of the OTHER ranks beyond
 * writing their rows of the tables.
 *   gid    (n_chains_total_cap, id_cap) i32 out: global identity of (chain, local id), -1 where the chain has fewer identities
 *   match  (n_chains_total_cap, t_max) i32 out: slot of the previous chain's last frame matched to slot s of this chain's first, -1
 *   info   (4) i32 out: {chains, global identities, error word, pairs}; error word bit 0 = a message overflowed or a chain has more
 *          than id_cap ids, bit 1 = an assignment did not terminate (cannot happen: the costs are finite, a tracklet with a
 *          non-finite joint is left out of the assignment -- it matches nobody and starts a new identity), bit 2 = some shard's void word is set (its compute
 *          step was void).  Non-zero = the result is void
 *   work   mvmc_stitch_work_words i32 device workspace;  n_chains_total_cap >= world * n_chains_cap; id_cap as packed */
long long mvmc_stitch_work_words(int world, int t_max, int id_cap);
int mvmc_stitch_chains(const void* messages, long long message_words, int world, int n_chains_cap, int t_max, int row_cap,
                       int id_cap, double max_dist, int n_chains_total_cap, int32_t* gid, int32_t* match, int32_t* info,
                       int32_t* work, mvmcStream_t stream);

/* ---- diagnostics (used by the tests; not part of the hot path's call surface) ---- */

/* The IK kernel's symmetric eigensolver on caller-supplied matrices: A (B,n,n) symmetric PSD, g (B,n),
 * 3 <= n <= 50.  lam (B,n) ascending with the numerically-null cluster (lam <= 1e-13 lam_max) set to 0;
 * Vt (B,n,n) rows = eigenvectors (rows 0..k0-1 of the null cluster are zero); k0 (B) = size of the null
 * cluster; phase_cycles (B,5) or NULL = shader cycles of {tridiagonalisation, multisection, twisted
 * factorisation, re-orthogonalisation, back-transformation}.  g is unused (kept for ABI stability). */
int mvmc_debug_eigh(const double* A, const double* g, int n_problems, int n, double* lam, double* Vt, int32_t* k0,
                    double* phase_cycles, mvmcStream_t stream);

/* One trust-region step of the IK solver computed in the Krylov tridiagonal basis (no eigendecomposition), on a
 * caller-supplied least-squares model: J = B (n_problems,m,n row-major), residual image r (n_problems,m), so
 * g = B^T r and M = B^T B.  3 <= m,n <= 50.  step (n_problems,n); out4 (n_problems,4) = {alpha, predicted
 * reduction, |step| incl. absorber, size of the leading (range) block, or -1 where the IK kernel would fall back
 * to the eigensolver (then alpha = -1, step = 0)}.  phase_cycles (n_problems,4) or NULL = shader cycles of the
 * tridiagonalisation's {reflector + publish, matrix-vector + exchange, rank-2 update} phases and their total. */
int mvmc_debug_trstep(const double* B, const double* r, int n_problems, int m, int n, double Delta, double alpha0,
                      double* step, double* out4, double* phase_cycles, mvmcStream_t stream);

/* The forms of the temporal layer that only the chain kernels run, on caller-supplied data (tests/test_gpu_track_kernels.py compares
 * them with mvmc_st_affinity / mvmc_track_assign / mvmc_track_commit bit for bit).
 * mvmc_debug_st_affinity_wg: arguments and results of mvmc_st_affinity; one workgroup of nt_threads (256 or 512) per chain runs the
 *   graph builder with the 2-D / 2-D block taken from pair_form: 0 = computed in place (as mvmc_st_affinity does on one wave),
 *   1 = made ahead by one thread per ordered pose pair from the keypoints in global memory (the chain kernel's small layout),
 *   2 = made ahead by per-view-pair line tables from keypoints staged in LDS (its big layout).  MVMC_ERR_UNSUPPORTED where
 *   t_max + n_views p_max > MVMC_MAX_NODES or the workgroup would need more than 160 KB of LDS.
 * mvmc_debug_track_wave: one 64-lane wave per chain.  phase 0 = mvmc_track_assign's arguments and results by the ballot form of the
 *   assignment (n_members (B, t_max + k_max) i32 or NULL: with it the member count of every problem slot is written there and rows of
 *   `members` are valid in [0, count) only, no -1 padding); phase 1 = mvmc_track_commit's by the multi-lane commit.  Pointers that
 *   the phase does not use may be NULL.  MVMC_ERR_UNSUPPORTED where t_max > 16, n_views > 16 or n_views p_max > 64 (the chain
 *   layouts' bounds, which the ballot words assume). */
int mvmc_debug_st_affinity_wg(const double* kps17, const int32_t* counts, const int32_t* frame_idx, const double* track_joints,
                              const int32_t* n_tracks, const double* Pmats, const double* F2, int n_chains, int n_views, int p_max,
                              int t_max, double min_score, int nt_threads, int pair_form, double* W, double* D,
                              int32_t* group_counts, mvmcStream_t stream);
int mvmc_debug_track_wave(int phase, const int32_t* labels_sp, const int32_t* ncl_sp, const int32_t* labels_st,
                          const int32_t* ncl_st, const int32_t* counts, const int32_t* frame_idx, int32_t* n_tracks,
                          double* track_params, int n_chains, int n_views, int p_max, int t_max, int k_max, int v_max,
                          int32_t* members, int32_t* n_members, uint8_t* cold, double* init_params, int32_t* status, int32_t* n_new,
                          const double* ik_params, const double* ik_joints, int n_inits, double* track_joints, int32_t* meta,
                          int32_t* next_id, int32_t* n_dead, int32_t* slot_src, int32_t* overflow, mvmcStream_t stream);

/* ONE trust-region model and ONE trial step of the production IK solver from a caller-given iterate -- the unit in which the
 * reference's recorded iterates are compared (tests/golden/ik_trf_traces.npz: x_k, Delta_k, alpha_k of SciPy's trf_no_bounds,
 * trf.py:466-500, as called from inverse_kinematics.py:236,274).  The device functions are the solver's own.
 *   params (B,68): the point x_k (stage 0 optimises the first 57 and keeps params[57:] as lengths; stage 1 all 68)
 *   Delta, alpha0 (B): trust radius and the Levenberg-Marquardt parameter handed to the sub-problem (solve_lsq_trust_region's
 *                initial_alpha)
 *   out (B, MVMC_IK_STEP_OUT_DOUBLES) f64:
 *     [0] cost at x   [1] |g|_inf   [2] alpha   [3] predicted reduction   [4] |step| as the solver accounts for it (= Delta whenever
 *     the sub-problem is rank deficient: the share the reference spends on numerically-null directions is modelled, not taken)
 *     [5] cost at the trial point   [6] path: 0 stopped by the gradient test, 1 Krylov step, 2 eigenbasis fallback; + 4 where the
 *     Euler-space model was used instead of the reduced coordinates; -1 = fewer than two views   [7] rows of the leading block
 *     [8, 76) g = J^T f by parameter (0 where the column is structurally zero)   [80, 148) step   [160, 228) trial point
 *   scratch as mvmc_ik_solve. */
#define MVMC_IK_STEP_OUT_DOUBLES 240
int mvmc_debug_ik_model_step(const mvmcSkeleton* skel_host, const double* kps17, const double* Pmats, const int32_t* members,
                             int n_problems, int v_max, int n_views, int p_max, const double* params, int stage,
                             const double* Delta, const double* alpha0, double* out, double* scratch, mvmcStream_t stream);

/* The stages of PoseSolver.solve one at a time, and their 3-D-target variants:
 *   stage_mask 1 = solve_pose_reproj (x = root, euler; inverse_kinematics.py:202-238),
 *              2 = solve_pose_bone_lens_reproj (x = root, euler, side lengths; :241-277), 3 = both in sequence;
 *   targets3d  NULL: reprojection residual on kps17 / members as in mvmc_ik_solve;
 *              (B,18,4) f64 = x, y, z, weight per observation row (COCO-17 + mid-spine): solve_pose (:280-307) and
 *              solve_pose_bone_lens (:310-336), residual (joint - target) * weight; kps17, Pmats, members are unused.
 * Every problem starts from init_params (B,68) with max_nfev evaluations per stage (least_squares(max_nfev=n_max_iter)).
 * Outputs and scratch as in mvmc_ik_solve; info of a stage that was not run is 0. */
int mvmc_ik_solve_stages(const mvmcSkeleton* skel_host, const double* kps17, const double* Pmats,
                         const int32_t* members, const double* targets3d, int n_problems, int v_max, int n_views,
                         int p_max, const double* init_params, int stage_mask, int max_nfev,
                         double* params_out, double* joints_out, double* info_out, double* scratch,
                         mvmcStream_t stream);

/* TRF-faithful IK (diagnostic, never on the hot path): PoseSolver.solve (inverse_kinematics.py:380-433) with the reference's own
 * numerical method -- scipy.optimize.least_squares defaults as called at inverse_kinematics.py:236,274: 2-point finite-difference
 * Jacobians (step sqrt(eps) sign(x) max(1,|x|)), an SVD of J and solve_lsq_trust_region -- instead of the production solver's analytic
 * Jacobian and Krylov step; the cold start triangulates with post_optimize=True through the same least_squares restatement
 * (mv_math_util.py:189-210).  Used to measure the band in which independent implementations of the reference's algorithm land.
 * Arguments as mvmc_ik_solve, plus stage_mask (1 = solve_pose_reproj only, 2 = solve_pose_bone_lens_reproj only, 3 = both);
 *   work  (B, MVMC_IK_FD_WORK_DOUBLES) f64 device workspace.  v_max <= 8. */
#define MVMC_IK_FD_WORK_DOUBLES 40960
int mvmc_debug_ik_solve_fd(const mvmcSkeleton* skel_host, const double* kps17, const double* Pmats, const int32_t* members,
                           int n_problems, int v_max, int n_views, int p_max, const double* init_params, const uint8_t* cold,
                           int max_nfev_cold, int max_nfev_warm, int stage_mask, double* params_out, double* joints_out,
                           double* info_out, double* work, mvmcStream_t stream);

/* The whole temporal hot path of a shard in ONE launch: a persistent 256-thread workgroup per chain runs
 * graph (match_spatial where the chain has no tracklet, match_spatial_time otherwise) -> ALS -> assignment -> IK ->
 * commit for the chain_len frames of its chain -- MvTracker.update_4d (motion_capture.py:873-963) per chain, the
 * same device code as mvmc_affinity / mvmc_st_affinity / mvmc_als_associate / mvmc_track_assign / mvmc_ik_solve /
 * mvmc_track_commit issued frame by frame, and the same results.  Chain b owns frames [b chain_len, (b+1) chain_len).
 * All pointers are device memory owned by the caller (N = n_views p_max, NS = t_max + N, NP = t_max + k_max,
 * B = n_chains, F = B chain_len).  Two LDS layouts (MVMC_ERR_UNSUPPORTED outside them: use the per-stage entry points), both with
 * n_views <= 16, p_max <= 8, NP <= 64, v_max <= 64:
 *   small  N <= 40, NS <= 48, max(t_max, p_max) <= 8 (its association variants hold rank 16) (configs 1-4; 128 VGPRs, four
 *          workgroups per CU; launches of at most two workgroups per CU run the 256-VGPR build of the same kernel); every frame's
 *          actual graph must have <= 24 nodes without tracklets and <= 32 with them, and the frame <= 24 poses in clusters (the IK
 *          phase's view pool) -- checked on the device;
 *   big    N <= 64, NS <= 80, t_max <= 16 (config 5, C8 P8; one 512-thread workgroup per CU; also taken with force_big): graphs of
 *          up to 72 nodes and rank 16 on the fast association variant, up to 80 nodes and rank 32 (sixteen live tracklets) on the
 *          generic one inside the same workgroup: every graph of those sizes fits.
 * Capacities the reference does not have (motion_capture.py:417-446, :763-808 accept any cluster size and any number of clusters and
 * tracklets): with k_max >= N / 2 (a new tracklet needs two poses) and v_max >= min(N, 64) (clusters are disjoint sets of the
 * frame's poses; the view blocks of a frame's IK problems share one pool, so a cluster may be as large as the frame) neither a
 * cluster nor a member is ever dropped; what remains is t_max (tracklet slots, tied to the rank the association variants hold)
 * and the graph sizes above.  A chain that exceeds one of them is reported in its void word, flags[B + 4 + b], and its results are
 * void; tracker.repair_chains re-runs such chains through the per-stage entry points with wider tables. */
typedef struct mvmcChainBuffers {
    int32_t n_chains, chain_len, n_views, p_max, t_max, k_max, v_max, max_nfev_cold, max_nfev_warm, n_inits, seed_len;
    int32_t n_parts;            /* workgroups per chain: 1 = one persistent workgroup per chain; p > 1 (dividing chain_len) =
                                   p workgroups running consecutive frame ranges of the chain one after the other, so that
                                   the hardware dispatcher balances the load over the CUs */
    int32_t force_big;          /* != 0: the big layout even where the small one would do (tests) */
    int32_t hand_over;          /* how a chain's workgroups follow one another (n_parts > 1).  0 = by block index (part * n_chains +
                                   chain; a part waits for its chain's flag: relies on workgroups being dispatched in block order,
                                   bounded wait, loud time-out); 1 = ready queue (a workgroup draws a ticket when it starts and takes
                                   the chain that has been ready longest: no assumption about dispatch order); 2 = the mapping of 0
                                   indexed by a ticket drawn when the workgroup starts instead of by the block index (a part's
                                   predecessor holds a lower ticket, so it has started: no assumption about dispatch order, the speed
                                   of 0; what the Python layer uses).  Same results bit for bit */
    /* inputs */
    const double* kps17;        /* (F,C,P,17,3) after mvmc_ingest */
    const int32_t* counts;      /* (F,C) */
    const double* Pmats;        /* (C,3,4); mvmc_chain_run_rigs: (R,C,3,4), R = n_rigs */
    const float* Fmats;         /* (C,C,3,3) from mvmc_fmats; mvmc_chain_run_rigs: (R,C,C,3,3) */
    const double* F2;           /* (C,C,3,3) from mvmc_fmats_from_projections; mvmc_chain_run_rigs: (R,C,C,3,3) */
    const double* seed_table;   /* mvmc_als_seed_table, on the device */
    /* tracker state, in/out (zero-initialised for fresh chains) */
    double* params;             /* (B,T,68) */
    double* joints;             /* (B,T,18,3) */
    int32_t* meta;              /* (B,T,4) id, state, hits, length */
    int32_t* n_tracks;          /* (B) */
    int32_t* next_id;           /* (B) */
    int32_t* n_dead;            /* (B) */
    int32_t* slot_src;          /* (B,T) */
    /* workspaces, contents undefined before and after */
    float* S_sp;                /* (B,N,N) */
    double* W_st;               /* (B,NS,NS) */
    int32_t* group_counts;      /* (B,C+1) */
    int32_t* labels_sp;         /* (B,N) */
    int32_t* labels_st;         /* (B,NS) */
    int32_t* n_clusters_sp;     /* (B) */
    int32_t* n_clusters_st;     /* (B) */
    int32_t* iters_sp;          /* (B) */
    int32_t* iters_st;          /* (B) */
    int32_t* members;           /* (B,NP,V); row s holds n_members[s] entries, the rest of the row is undefined */
    int32_t* n_members;         /* (B,NP) */
    uint8_t* cold;              /* (B,NP) */
    double* init;               /* (B,NP,68) */
    int32_t* status;            /* (B,T) */
    int32_t* n_new;             /* (B) */
    double* ik_params;          /* (B,NP,68) */
    double* ik_joints;          /* (B,NP,18,3) */
    double* ik_info;            /* (B,NP,8) */
    double* ik_scratch;         /* (B,8,MVMC_IK_SCRATCH_DOUBLES) */
    /* per-frame outputs: the tracklet table after every frame */
    double* out_params;         /* (F,T,68) */
    double* out_joints;         /* (F,T,18,3) */
    int32_t* out_meta;          /* (F,T,4) */
    int32_t* out_n_tracks;      /* (F) */
    double* out_info;           /* (F,NP,8) IK info rows of the frame's problems, or NULL */
    int32_t* out_als_iters;     /* (F) ALS iterations of the frame's graph, or NULL */
    uint32_t* flags;            /* (B (n_parts + 1) + 8) u32, zeroed by the call: [0,B) hand-over flags of the chains; afterwards
                                   flags[B] != 0 = a workgroup timed out waiting for its predecessor, flags[B + 1] != 0 = a graph was
                                   too large for the kernel's ALS variant, flags[B + 2] != 0 = a capacity was exceeded in some chain
                                   (bit 0: a cluster, a member or a view block dropped, bit 1: more than t_max tracklets),
                                   flags[B + 4 + b] = the void word of chain b (bits 0, 1 as before, bit 2 = graph too large, bit 3 =
                                   internal: a meeting of two IK waves timed out, builds with -DMVMC_WITH_IK_PAIR only, bit 4 =
                                   mvmc_chain_run_rigs: the chain's rig index is outside [0, n_rigs) -- no calibration was read,
                                   its frames are empty tables, out_n_tracks = 0; also raised in flags[B + 2]): a
                                   non-zero word voids the chain's results (all chains' after a time-out); from 2 B + 4 on: the
                                   ticket counter (hand_over 1, 2), the ready queue's tail and ring (hand_over == 1) */
    double* out_phase_cycles;   /* (B,8) diagnostic: shader cycles of each chain by phase {graph, ALS, assignment, IK, commit,
                                   outputs, whole chain, 0}, or NULL */
} mvmcChainBuffers;
int mvmc_chain_run(const mvmcSkeleton* skel_host, const mvmcChainBuffers* buffers, mvmcStream_t stream);

/* mvmc_chain_run with a calibration per chain: buffers->Pmats, Fmats and F2 hold n_rigs rigs of n_views cameras each
 * ((R,C,3,4), (R,C,C,3,3), (R,C,C,3,3)), and chain b uses rig rig_of_chain[b] ((n_chains) i32 device, or NULL: rig 0 for every
 * chain).  A chain whose index lies outside [0, n_rigs) reads no calibration: bit 4 of its void word, empty tables.  n_rigs < 1, or
 * rig_of_chain == NULL with n_rigs != 1: MVMC_ERR_ARG.  mvmc_chain_run(s, b, st) is mvmc_chain_run_rigs(s, b, NULL, 1, st). */
int mvmc_chain_run_rigs(const mvmcSkeleton* skel_host, const mvmcChainBuffers* buffers, const int32_t* rig_of_chain, int n_rigs,
                        mvmcStream_t stream);

/* mvmc_chain_run_rigs with chains that sit the launch out: active ((n_chains) u8 device, or NULL: every chain runs).  A chain with
 * active[b] == 0 writes nothing -- not its state, not its out_* rows or out_phase_cycles row, not its void word, not flags[B + 1],
 * flags[B + 2] -- and its rig index is not read, so an out-of-range index raises no bit 4.  The per-frame driver of many live rigs
 * (multiview_motion_capture_amd/live.py) steps, in one launch of chain_len 1, the sessions that have a frame this tick.
 * active != NULL with n_parts > 1: MVMC_ERR_ARG (an idle chain's first part would never hand over to its successors).
 * mvmc_chain_run_rigs(s, b, r, n, st) is mvmc_chain_run_sessions(s, b, r, n, NULL, st). */
int mvmc_chain_run_sessions(const mvmcSkeleton* skel_host, const mvmcChainBuffers* buffers, const int32_t* rig_of_chain, int n_rigs,
                            const uint8_t* active, mvmcStream_t stream);

/* ---- body fit of finished tracklets (multiview_motion_capture_amd/body_fit.py).  No counterpart in the reference: its IK fits the
 * side lengths again on every frame (inverse_kinematics.py:380-433).  One side-length vector per identity, every frame's pose re-solved
 * against it.  A "problem" is one (identity, frame) pair of a tracklet record; problems of one launch may come from several sequences
 * (frames laid end to end in kps17, one rig of n_views cameras per sequence). ---- */

/* Observation selection.  Per (problem b, camera c): among the poses of frame frame_of[b] in camera c, the one with the smallest
 * reprojection_error (motion_capture.py:403-414; the 2D-3D distance of mvmc_st_affinity) to the problem's joints, if that distance is
 * finite and below max_dist (the affinity floor 15 + 30 ln(999) / 5 of the tracker's graph; ties between poses: the lower slot).
 * Then two problems of one frame that chose the same pose: the smaller distance keeps it (equal: the lower rank), the other takes
 * nothing in that camera.
 *   kps17 (F,C,P,17,3), counts (F,C) as mvmc_ingest writes them; Pmats (R,C,3,4), R = n_rigs
 *   frame_of, rig_of (B) i32; joints (B,18,3) f64: the record's FK joints
 *   order (B) i32: the problems sorted so that each frame's are contiguous; grp_lo, grp_hi (B) i32: the range of order[] that holds
 *   the problems of b's frame; rank (B) i32: the position of b's record in the caller's list (the tie-break)
 *   choice (B,C) i32 out: nearest pose index q = (f C + c) P + p before the conflicts, or -1; dist (B,C) f64 out (+inf: none)
 *   members (B,C) i32 out: the selected pose index or -1 (the members format of mvmc_ik_solve); n_views_out (B) i32 out */
int mvmc_body_observe(const double* kps17, const int32_t* counts, int n_frames, int n_views, int p_max, const double* Pmats,
                      int n_rigs, const int32_t* frame_of, const int32_t* rig_of, const double* joints, const int32_t* order,
                      const int32_t* grp_lo, const int32_t* grp_hi, const int32_t* rank, int n_problems, double min_score,
                      double max_dist, int32_t* choice, double* dist, int32_t* members, int32_t* n_views_out, mvmcStream_t stream);

/* Length step: Levenberg-Marquardt on the side lengths of every identity, all roots and angles fixed; ONE launch, one 64-lane
 * workgroup per identity.  Identity i owns problems [id_lo[i], id_lo[i+1]) (every one with >= 2 members).  The residual is the IK's
 * (16 observation rows per member, score-weighted, 1e-5 in the denominator), E = 1/2 sum r^2; H = J^T J, g = J^T r over the
 * identity's problems, summed per lane in problem order and across lanes in a fixed butterfly (no atomics: bit-identical from run to
 * run and whatever else the launch holds).  Each trial solves (H + mu diag(H)) d = -g on the free slots, mu starts at mu0, / 10 after
 * an accepted trial (E(l + d) < E(l)), x 10 after a rejected one; stop after max_iter trials, when |d|_inf < xtol, when the model's
 * predicted reduction is below ftol E, or when an accepted trial reduced E by less than ftol E.
 *   params (B,68) f64: root and angles of each problem (its lengths are not read); members (B,C) as from mvmc_body_observe
 *   lens (n_ids,11) f64 in/out; free_mask (n_ids) i32: bit s = slot s is free; fix_free 0: set from diag(H) > 0 at the start and
 *   written, 1: read
 *   info (n_ids, MVMC_BODY_INFO_DOUBLES) f64 out: {E at the start, E at the end, trials made, trials accepted, per trial 1 accepted /
 *   0 rejected, -1 after the last}; max_iter <= MVMC_BODY_INFO_DOUBLES - 4
 *   work (B, MVMC_BODY_WORK_DOUBLES) f64 device workspace */
#define MVMC_BODY_INFO_DOUBLES 16
#define MVMC_BODY_WORK_DOUBLES 270
int mvmc_body_lengths(const mvmcSkeleton* skel_host, const double* kps17, int n_views, int p_max, const double* Pmats,
                      const int32_t* rig_of, const int32_t* members, const double* params, const int32_t* id_lo, int n_ids,
                      double* lens, int32_t* free_mask, int fix_free, int max_iter, double mu0, double ftol, double xtol,
                      double* info, double* work, mvmcStream_t stream);

/* mvmc_ik_solve_stages (reprojection mode) with a calibration per problem: Pmats (R,C,3,4), R = n_rigs, and problem b uses rig
 * rig_of_problem[b] ((B) i32 device).  The same device code as mvmc_ik_solve_stages; a problem whose rig lies outside [0, n_rigs)
 * gets NaN outputs, as one with fewer than two views. */
int mvmc_ik_solve_stages_rigs(const mvmcSkeleton* skel_host, const double* kps17, const double* Pmats, int n_rigs,
                              const int32_t* rig_of_problem, const int32_t* members, int n_problems, int v_max, int n_views,
                              int p_max, const double* init_params, int stage_mask, int max_nfev, double* params_out,
                              double* joints_out, double* info_out, double* scratch, mvmcStream_t stream);

/* ---- trajectory smoothing of finished tracklets (multiview_motion_capture_amd/smoothing.py).  No counterpart in the reference, whose
 * only temporal element is the IK's warm start.  One Levenberg-Marquardt solve per identity over every frame from its first to its last:
 * E = 1/2 sum_t sum_v |r_tv(x_t)|^2 (the IK's stage-1 residual at frame t's lengths, the views members[t] selects)
 *   + 1/2 sum_t |Wv^1/2 (x_t - x_{t-1})|^2 + 1/2 sum_t |Wa^1/2 (x_{t+1} - 2 x_t + x_{t-1})|^2,
 * x_t = the MVMC_SMOOTH_K stage-1 parameters of frame t (root translation, then the Euler angles of the joints whose rotation moves an
 * observed joint); W diagonal: root_* on the translation, ang_* on the angles.  Every other column of a frame's 68 is held.  A frame
 * (row) of the launch belongs to identity id_of[f]; identity i owns the rows [id_lo[i], id_lo[i+1]), consecutive frames, >= 2 of them.
 * The host issues, with phase = 0, 1, ..., max_iter: mvmc_smooth_blocks (at x for phase 0, at x_trial after) then mvmc_smooth_step.
 * Every decision is taken on the device; a stopped identity is skipped by both.  Nothing is allocated or synchronised inside. ---- */
#define MVMC_SMOOTH_K 39
#define MVMC_SMOOTH_BLOCK_DOUBLES 820    /* per row and buffer: J^T J upper triangle (780), J^T r (39), E */
#define MVMC_SMOOTH_WORK_DOUBLES 3940    /* per row: the factor (780 + 2 x 1521), y / d, g, diag A (39 each) */
#define MVMC_SMOOTH_INFO_DOUBLES 32      /* per identity: E_data, E_prior at the start; E_data, E_prior now; trials, accepted, mu, stop
                                          * reason (0 running, 1 max_iter, 2 xtol, 3 predicted reduction below ftol E, 4 achieved
                                          * reduction below ftol E, 5 factorisation failed); per trial 1 accepted / 0 rejected, -1 after
                                          * the last.  max_iter <= MVMC_SMOOTH_INFO_DOUBLES - 8 */
#define MVMC_SMOOTH_MAX_VIEWS 64

/* The data blocks of one evaluation: one wave per row.  kps17 (F,C,P,17,3) as mvmc_ingest writes it; Pmats (R,C,3,4); rig_of (N) i32;
 * members (N,C) i32 pose indices or -1 (a row without any: zero blocks); x (N,68) f64 the point; id_of (N) i32; ctl (n_ids,4) i32 the
 * identities' control words ({stopped, buffer of the accepted point, 0, 0}; {0, 1, 0, 0} before phase 0).  blk (2,N,
 * MVMC_SMOOTH_BLOCK_DOUBLES) f64 out: the row's blocks go to buffer 1 - ctl[id][1]. */
int mvmc_smooth_blocks(const mvmcSkeleton* skel_host, const double* kps17, int n_views, int p_max, const double* Pmats,
                       const int32_t* rig_of, const int32_t* members, const double* x, const int32_t* id_of, const int32_t* ctl,
                       int n_frames, double* blk, mvmcStream_t stream);

/* One LM step per identity, one 256-lane workgroup each.  phase 0: E at x from the blocks, mu = mu0; phase > 0: the trial x_trial is
 * accepted when E(x_trial) < E(x) (x = x_trial, mu / 10; stop when the reduction is below ftol E), else mu x 10.  Then, unless
 * max_iter trials are made: (A + mu diag A) d = -grad E by a block-banded Cholesky (the factor in work (N, MVMC_SMOOTH_WORK_DOUBLES)),
 * stop when |d|_inf < xtol or the predicted reduction is below ftol E, else x_trial = x + d.  x, x_trial (N,68) f64 in/out; blk as
 * written by mvmc_smooth_blocks; id_lo (n_ids + 1) i32; ctl (n_ids,4) i32 in/out; info (n_ids, MVMC_SMOOTH_INFO_DOUBLES) f64 out. */
int mvmc_smooth_step(const mvmcSkeleton* skel_host, double* x, double* x_trial, const double* blk, const int32_t* id_lo, int n_ids,
                     int n_frames, double root_vel, double root_acc, double ang_vel, double ang_acc, double mu0, double ftol,
                     double xtol, int max_iter, int phase, int32_t* ctl, double* info, double* work, mvmcStream_t stream);

/* The per-frame covariance of the smoothed trajectory, one 256-lane workgroup per identity (csrc/mvmc_smooth_cov.hip).  At the final x
 * the Laplace / Gauss-Newton covariance of E is sigma^2 A^-1, A = the data blocks at x + the exact prior Hessian (the matrix
 * mvmc_smooth_step factors).  The launch factors A + mu diag A with the smoother's own sweep, then one backward recursion over the
 * factor (Takahashi's selected inverse) gives the diagonal blocks Sigma_tt of its inverse row by row.  mu >= 0 is a small damping: at
 * mu = 0 the matrix is singular for this skeleton (the Rz angles of the two knees are stage-1 columns but move no joint, and the
 * prior sees differences only), the joints' covariances do not depend on mu to first order.  From each Sigma_tt, while it is on the chip:
 *   jcov (N, 18, 6) f64 out: C_K = D_K Sigma_tt D_K^T of every skeleton joint K, D_K = d X_K / d x_t (3 x MVMC_SMOOTH_K); the six
 *        values (0,0) (0,1) (0,2) (1,1) (1,2) (2,2), m^2 per px^2 (unit variance: the host applies the noise scale);
 *   pvar (N, MVMC_SMOOTH_K) f64 out: the diagonal of Sigma_tt, m^2 or rad^2 per px^2;
 *   cinfo (n_ids, MVMC_SMOOTH_COV_INFO_DOUBLES) f64 out: {status, E_data at x, n_res = 2 x the (selected view, observed joint) pairs
 *        whose score is not zero, edof = sum_t tr(Sigma_tt J_t^T J_t), 0...}.  status 0: solved.  1: the factor has a pivot
 *        that is not positive and finite -- every jcov / pvar row of the identity is NaN (n_res, edof too), the recursion is not run.
 *        2: an identity of fewer than two rows, nothing solved, NaN rows.
 * x (N,68) f64 the final point; blk (N, MVMC_SMOOTH_BLOCK_DOUBLES) f64 the data blocks AT x (one buffer of mvmc_smooth_blocks' two);
 * id_lo, the weights, kps17, Pmats, rig_of and members as the two entries above take them (the rows' scores give n_res); work (N,
 * MVMC_SMOOTH_WORK_DOUBLES) f64 is overwritten with the factor.  Every sum runs in a fixed order inside the identity's own
 * workgroup: the same bits alone, in a batch and from run to run.  Nothing is allocated or synchronised inside. */
#define MVMC_SMOOTH_COV_INFO_DOUBLES 8
int mvmc_smooth_cov(const mvmcSkeleton* skel_host, const double* x, const double* blk, const int32_t* id_lo, int n_ids, int n_frames,
                    double root_vel, double root_acc, double ang_vel, double ang_acc, double mu, const double* kps17, int n_views,
                    int p_max, const double* Pmats, const int32_t* rig_of, const int32_t* members, double* work, double* jcov, double* pvar,
                    double* cinfo, mvmcStream_t stream);

/* ---- fixed-lag smoothing of live sessions (multiview_motion_capture_amd/live_smoothing.py).  The objective is the trajectory
 * smoother's above; the problem is a short sliding window per live identity (one tracklet of one session), and ONE launch does a whole
 * tick of every identity of every session: one 256-lane workgroup per item.  State that stays on the device between ticks, per
 * identity slot: rows (MVMC_SMOOTH_WIN_RING, 68) f64 and members (MVMC_SMOOTH_WIN_RING, C) i32, row r of the identity (r = frame -
 * first frame) at ring position r mod MVMC_SMOOTH_WIN_RING, and count (2) i32 = {rows, first frame}.  kps17 is the sessions' ring of
 * ingested keypoints, (F,C,P,17,3) as mvmc_ingest writes them, which the members index.
 * An item (MVMC_SMOOTH_WIN_ITEM_INTS i32): {slot, rig, d, is_data, reset, src, first_frame, work_row}.  The identity gets d new rows
 * (reset: it is new and gets exactly one): d - 1 missing rows, then row src of new_params (n_new,68) / new_members (n_new,C) when
 * is_data, else one more missing row; a missing row is a copy of the identity's last row and has no members.  Then, with n rows: the
 * last m = min(window, n) rows are free, the h = min(2, n - m) rows before them frozen history, and n_iter Levenberg-Marquardt trials
 * (mvmc_smooth_step's rules, mu from mu0) minimise the free rows' data terms + every velocity / acceleration term that touches a free
 * row over the free rows' MVMC_SMOOTH_K columns, warm from the rows' values; the free rows go back into the ring.  n < 2: no solve.
 *   info (n_items, MVMC_SMOOTH_WIN_INFO_DOUBLES) f64 out: E_data, E_prior at the start; E_data, E_prior at the end; trials, accepted,
 *   mu, stop reason (mvmc_smooth_step's; 6: the item was malformed and skipped; 0 with trials 0: nothing to solve); per trial 1 / 0,
 *   -1 after the last.  n_iter <= MVMC_SMOOTH_WIN_INFO_DOUBLES - 8.
 *   work: device workspace of at least mvmc_smooth_window_work_doubles(n_items, window) doubles; item i uses rows work_row ..
 *   work_row + window of its row part (work_row + window <= n_items * window).
 * Argument errors return before any HIP call; nothing is allocated or synchronised inside. ---- */
#define MVMC_SMOOTH_WIN_MAX 32
#define MVMC_SMOOTH_WIN_RING 66
#define MVMC_SMOOTH_WIN_ITEM_INTS 8
#define MVMC_SMOOTH_WIN_INFO_DOUBLES 16
long long mvmc_smooth_window_work_doubles(int n_items, int window);   /* -1: bad arguments */
int mvmc_smooth_window(const mvmcSkeleton* skel_host, const double* kps17, int n_views, int p_max, const double* Pmats, int n_rigs,
                       const int32_t* items, int n_items, const double* new_params, const int32_t* new_members, int n_new,
                       double* rows, int32_t* members, int32_t* count, int n_slots, int window, int n_iter, double root_vel,
                       double root_acc, double ang_vel, double ang_acc, double mu0, double ftol, double xtol, double* info,
                       double* work, long long work_doubles, mvmcStream_t stream);

/* The per-joint covariance of the rows a tick emits (csrc/mvmc_smooth_window_cov.hip; live_smoothing.py: covariance="joints"): ONE
 * launch after mvmc_smooth_window[_robust], one 256-lane workgroup per item, that only READS the state above (rows, members, count, the
 * keypoint ring, Pmats).  An item (MVMC_SMOOTH_COV_ITEM_INTS i32): {slot, rig, emit_row, work_row}; emit_row counts from the
 * identity's first row.  With n = count[slot] rows the window is the one mvmc_smooth_window solved: the last m = min(window, n) rows
 * free, the h = min(2, n - m) rows before them frozen.  A_w = the free rows' data blocks at their values (with a loss the weighted ones)
 * + the exact Hessian of every prior term that touches a free row, the history held fixed: the matrix the window's LM step factors.
 * The launch factors A_w + mu diag A_w with the smoothers' sweep (mu as mvmc_smooth_cov takes it: without history A_w alone is
 * singular, and at mu = 0 its last pivot is a rounding residue of either sign, so status 1 is not guaranteed there) and runs
 * mvmc_smooth_cov's backward recursion from the last free row down to the emitted one, e = emit_row - (n - m): Sigma_ee is the
 * covariance of the emitted row CONDITIONAL on the frozen history (and on the rig, the lengths and the view selection).  From it:
 *   jcov (n_items, 18, 6), pvar (n_items, MVMC_SMOOTH_K) f64 out: as mvmc_smooth_cov's, of the emitted row alone, unit variance;
 *   cinfo (n_items, MVMC_SMOOTH_COV_INFO_DOUBLES) f64 out: {status, E_data of the free rows, n_res, edof, m, e, 0, 0}.  full != 0: the
 *        recursion goes on down to free row 0 and n_res, edof = sum_t tr(Sigma_tt H_t) are those of all free rows (mvmc_smooth_cov's
 *        definitions); full == 0: it stops at row e, n_res and edof are NaN, jcov and pvar have the same bits.
 *        status 0: solved.  1: a pivot of the factor is not positive and finite, NaN outputs.  2: n < 2, nothing was solved, NaN.
 *        6: the item is malformed (slot or rig out of range, n < 1, emit_row not a free row, work_row < 0 or work_row + window >
 *        n_items * window), NaN outputs; it is never followed out of bounds and its neighbours are not touched.
 * loss, loss_px: MVMC_SMOOTH_LOSS_* and its scale under mvmc_smooth_window_robust's rule (MVMC_SMOOTH_LOSS_NONE: loss_px is not read).
 * work: at least mvmc_smooth_window_cov_work_doubles(n_items, window) doubles, overwritten.  Every sum runs in a fixed order inside the
 * item's own workgroup: the same bits alone, among other items and from run to run.  Argument errors return before any HIP call;
 * nothing is allocated or synchronised inside. */
#define MVMC_SMOOTH_COV_ITEM_INTS 4
long long mvmc_smooth_window_cov_work_doubles(int n_items, int window);   /* -1: bad arguments */
int mvmc_smooth_window_cov(const mvmcSkeleton* skel_host, const double* kps17, int n_views, int p_max, const double* Pmats, int n_rigs,
                           const int32_t* items, int n_items, const double* rows, const int32_t* members, const int32_t* count,
                           int n_slots, int window, double root_vel, double root_acc, double ang_vel, double ang_acc, double mu,
                           int full, int loss, double loss_px, double* work, long long work_doubles, double* jcov, double* pvar,
                           double* cinfo, mvmcStream_t stream);

/* ---- a robust loss on the smoothers' keypoint residuals (restated in tests/smooth_robust_np.py).  For one (selected view, observed
 * joint) pair of a row: score s, plain pixel residual (ru, rv) = proj(X_k) - obs, e^2 = ru^2 + rv^2, delta = loss_px > 0 (pixels),
 *   MVMC_SMOOTH_LOSS_HUBER   rho = 1/2 e^2, w = 1 for e <= delta; otherwise rho = delta (e - 1/2 delta), w = delta / e
 *   MVMC_SMOOTH_LOSS_CAUCHY  rho = 1/2 delta^2 log1p(e^2 / delta^2), w = 1 / (1 + e^2 / delta^2)
 * The score stays outside the loss: E_data = sum s^2 rho replaces 1/2 sum s^2 e^2 wherever a cost is read or written, and at every
 * linearisation the pair's contribution to the blocks is multiplied by w (iteratively reweighted, no second-order correction); a pair
 * with s = 0 contributes nothing.  The blocks keep their layout (J^T W J upper triangle, J^T W r, sum s^2 rho), so the step, the sweep
 * and the covariance entry read them as they are; the prior is not touched.  Every buffer and precondition is that of the entry
 * without _robust.  MVMC_SMOOTH_LOSS_NONE runs that entry's kernel (loss_px is not read); a loss outside these three, or with a loss a
 * loss_px that is not a finite number > 0: MVMC_ERR_ARG.
 * The weights entry, one wave per row, does FK and the projections only: w (N, C, 16) f64 out, the weight of camera c's member and
 * observed joint k (the IK's observation order) at x (N,68) -- 1 with MVMC_SMOOTH_LOSS_NONE -- and NaN where the camera has no member
 * in the row or the pair's score is 0. ---- */
#define MVMC_SMOOTH_LOSS_NONE 0
#define MVMC_SMOOTH_LOSS_HUBER 1
#define MVMC_SMOOTH_LOSS_CAUCHY 2
int mvmc_smooth_blocks_robust(const mvmcSkeleton* skel_host, const double* kps17, int n_views, int p_max, const double* Pmats,
                              const int32_t* rig_of, const int32_t* members, const double* x, const int32_t* id_of, const int32_t* ctl,
                              int n_frames, double* blk, int loss, double loss_px, mvmcStream_t stream);
int mvmc_smooth_obs_weights(const mvmcSkeleton* skel_host, const double* kps17, int n_views, int p_max, const double* Pmats,
                            const int32_t* rig_of, const int32_t* members, const double* x, int n_frames, int loss, double loss_px,
                            double* w, mvmcStream_t stream);
int mvmc_smooth_window_robust(const mvmcSkeleton* skel_host, const double* kps17, int n_views, int p_max, const double* Pmats, int n_rigs,
                              const int32_t* items, int n_items, const double* new_params, const int32_t* new_members, int n_new,
                              double* rows, int32_t* members, int32_t* count, int n_slots, int window, int n_iter, double root_vel,
                              double root_acc, double ang_vel, double ang_acc, double mu0, double ftol, double xtol, double* info,
                              double* work, long long work_doubles, int loss, double loss_px, mvmcStream_t stream);

/* ---- foot contacts of the trajectory smoother (smoothing.py: contacts=; restated in tests/smooth_contact_np.py).  Per identity and
 * foot f = 0 (skeleton joint MVMC_SMOOTH_FOOT_L), 1 (MVMC_SMOOTH_FOOT_R) a label c[t][f] per row; a run is a maximal stretch of
 * consecutive rows with c != 0 of one foot, and every run has one anchor a (metres).  The term
 *   E_contact = 1/2 contact_weight sum_{t, f: c != 0} |X_f(x_t) - a_run(t, f)|^2      (contact_weight in px^2 / m^2)
 * belongs to one row for fixed anchors: it joins that row's block alone, outside the robust loss, and the step, the sweep and the
 * covariance entry read the blocks as they are.  Over the anchors it is minimised in closed form: the mean of X_f over the run.
 * mvmc_smooth_blocks_contact is mvmc_smooth_blocks_robust with the term: cmask (N, 2) i32 and anchors (N, 2, 3) f64 per row (an anchor
 * is read only where the mask is not 0), contact_weight finite and >= 0.  A row whose mask is (0, 0) gets the blocks of
 * mvmc_smooth_blocks_robust bit for bit; a row with a mask but no selected view gets the term alone.
 * mvmc_smooth_contact_anchors, ONE launch, one workgroup of two waves per identity, one wave per foot (csrc/mvmc_smooth_contact.hip):
 * joints (N, 18, 3) f64 the FK joints of the rows, id_lo (n_ids + 1) i32.  detect != 0: the labels are made here -- row t of foot f is
 * a contact when its speed, |p[t+1] - p[t-1]| / 2 inside the identity and |p[t+1] - p[t]| at its first and |p[t] - p[t-1]| at its last
 * row (metres per frame), is < speed and, with use_ground != 0, ground[0..2] . p - ground[3] < height (ground: 4 doubles on the HOST,
 * the plane's normal and offset; not read otherwise); then the runs shorter than min_run rows are dropped.  detect == 0: cmask is read as given and not changed.  anchors out: the run's mean (summed in row order)
 * on every row of the run, NaN on every other row.  ctl (n_ids, 4) i32, mvmc_smooth_step's control words: ctl[id][0] is set to 0 (the
 * identity runs again) when either foot has a run, and is not touched otherwise.  An identity's numbers depend on nothing else in
 * the launch; there is no limit on the rows of an identity. ---- */
#define MVMC_SMOOTH_FOOT_L 3
#define MVMC_SMOOTH_FOOT_R 6
int mvmc_smooth_blocks_contact(const mvmcSkeleton* skel_host, const double* kps17, int n_views, int p_max, const double* Pmats,
                               const int32_t* rig_of, const int32_t* members, const double* x, const int32_t* id_of, const int32_t* ctl,
                               int n_frames, double* blk, int loss, double loss_px, const int32_t* cmask, const double* anchors,
                               double contact_weight, mvmcStream_t stream);
int mvmc_smooth_contact_anchors(const double* joints, const int32_t* id_lo, int n_ids, int n_frames, int detect, double speed,
                                int min_run, int use_ground, const double* ground, double height, int32_t* cmask, double* anchors,
                                int32_t* ctl, mvmcStream_t stream);

/* ---- a floor under the contacts of the trajectory smoother (smoothing.py: floor=; restated in tests/smooth_floor_np.py).  Per sequence
 * a unit floor normal n (T = I - n n^T projects into the floor), per identity ONE level h (metres along n) shared by all its runs and
 * both feet; over the labelled (row, foot) pairs L of the contacts above
 *   E_contact = 1/2 contact_weight sum_L |T (X_f(x_t) - a_run)|^2 + 1/2 floor_weight sum_L (n . X_f(x_t) - h)^2
 * h is minimised in closed form too: the mean of n . X_f over L.  The stored anchor of a row is the point T mean_run + n h on the
 * plane, so with c = X_f - a (n . c = n . X_f - h) the row's term is 1/2 wc |c|^2 + 1/2 (wf - wc)(n . c)^2.
 * mvmc_smooth_blocks_floor is mvmc_smooth_blocks_contact with normals (n_rigs, 3) f64, read through rig_of[row], and floor_weight
 * finite and >= 0 (else MVMC_ERR_ARG before any HIP call): the labelled row's W_K += wc I + (wf - wc) n n^T, t_K += wc c +
 * (wf - wc)(n . c) n, E += the term, in the lane of the contact term, with no LDS and no barrier more.  A row whose sequence has a NaN
 * normal, or whose mask is (0, 0), gets mvmc_smooth_blocks_contact's block bit for bit.
 * mvmc_smooth_floor_anchors, ONE launch after mvmc_smooth_contact_anchors (which still makes the labels and the run means), the same
 * two waves per identity: levels (n_ids) f64 out, h = the mean of n . ankle over L, summed in ONE fixed order -- the left foot's rows
 * ascending, then the right foot's --, n = normals[rig_of[the identity's first row]]; every labelled row's anchor a is replaced by
 * a - n (n . a - h).  An identity without a labelled row or with a NaN normal: level NaN, its anchors untouched.  cmask is read only.
 * An identity's numbers depend on nothing else in the launch; there is no limit on its rows. ---- */
int mvmc_smooth_blocks_floor(const mvmcSkeleton* skel_host, const double* kps17, int n_views, int p_max, const double* Pmats,
                             const int32_t* rig_of, const int32_t* members, const double* x, const int32_t* id_of, const int32_t* ctl,
                             int n_frames, double* blk, int loss, double loss_px, const int32_t* cmask, const double* anchors,
                             double contact_weight, const double* normals, double floor_weight, mvmcStream_t stream);
int mvmc_smooth_floor_anchors(const double* joints, const int32_t* id_lo, int n_ids, int n_frames, const int32_t* rig_of,
                              const double* normals, const int32_t* cmask, double* anchors, double* levels, mvmcStream_t stream);

/* ---- foot contacts of the live smoother (live_smoothing.py: contacts="auto"; restated in tests/live_smooth_contact_np.py).  Two more
 * state arrays stay on the device between ticks, per identity slot and ring position: contact (n_slots, MVMC_SMOOTH_WIN_RING, 2) i32,
 * the row's label per foot, and anchors (n_slots, MVMC_SMOOTH_WIN_RING, 2, 3) f64, NaN without a label.
 * mvmc_smooth_window_contact is mvmc_smooth_window_robust, still ONE launch per tick and one 256-lane workgroup per item, with:
 *   append   the new rows get label 0 and a NaN anchor (reset: the slot's whole rings are cleared);
 *   solve    every free row with a label adds 1/2 contact_weight |ankle_f(x_r) - anchor|^2 under its STORED label and anchor (the
 *            term of mvmc_smooth_blocks_contact, outside the loss); history rows carry no term.  info's E_data includes it;
 *   relabel  after the last trial, on the solved values: rows with index <= n - 1 - lag are frozen and keep label and anchor for good;
 *            the rows after them are labelled again by mvmc_smooth_contact_anchors' rule (speed < contact_speed, one-sided at the
 *            identity's first and newest row; with use_ground != 0 also ground[0..2] . p - ground[3] < contact_height, ground 4
 *            doubles on the HOST); then over the window's rows, history included: a run whose first visible row is frozen keeps that
 *            row's anchor on all its rows and is never dropped; a run without a frozen row is dropped when shorter than
 *            contact_min_frames, else its anchor is the mean of its rows' ankles, summed in row order.
 *   cinfo (n_items, MVMC_SMOOTH_LIVE_CONTACT_DOUBLES) f64 out: label L, R and anchor L (3), R (3) of the row n - 1 - lag (the row the
 *            tick emits: frozen from this tick on; 0 and NaN when there is none), E_contact at the start and at the end of the tick.
 * 0 <= lag < window, contact_min_frames >= 1, lag + 1 >= contact_min_frames, contact_weight finite >= 0, contact_speed finite (and
 * with use_ground a finite ground and contact_height), else MVMC_ERR_ARG before any HIP call; a malformed item is skipped with stop
 * reason 6.  mvmc_smooth_window_cov_contact is mvmc_smooth_window_cov whose free rows' blocks carry the term of the labels and anchors
 * as they stand in the two arrays (after the tick's launch: the relabelled ones); it only reads them. ---- */
#define MVMC_SMOOTH_LIVE_CONTACT_DOUBLES 10
int mvmc_smooth_window_contact(const mvmcSkeleton* skel_host, const double* kps17, int n_views, int p_max, const double* Pmats, int n_rigs,
                               const int32_t* items, int n_items, const double* new_params, const int32_t* new_members, int n_new,
                               double* rows, int32_t* members, int32_t* count, int n_slots, int window, int n_iter, double root_vel,
                               double root_acc, double ang_vel, double ang_acc, double mu0, double ftol, double xtol, double* info,
                               double* work, long long work_doubles, int loss, double loss_px, int32_t* contact, double* anchors,
                               int lag, double contact_weight, double contact_speed, int contact_min_frames, int use_ground,
                               const double* ground, double contact_height, double* cinfo, mvmcStream_t stream);
int mvmc_smooth_window_cov_contact(const mvmcSkeleton* skel_host, const double* kps17, int n_views, int p_max, const double* Pmats,
                                   int n_rigs, const int32_t* items, int n_items, const double* rows, const int32_t* members,
                                   const int32_t* count, int n_slots, int window, double root_vel, double root_acc, double ang_vel,
                                   double ang_acc, double mu, int full, int loss, double loss_px, double* work, long long work_doubles,
                                   double* jcov, double* pvar, double* cinfo, const int32_t* contact, const double* anchors,
                                   double contact_weight, mvmcStream_t stream);

/* ---- one skeleton per live identity, estimated as frames arrive (live_smoothing.py: lengths="auto"; csrc/mvmc_live_lengths.hip;
 * restated in tests/live_lengths_np.py, which is the definition).  The window launches above solve every row under its own columns
 * 57:68; these two launches, one before and one after the tick's window launch, decide what those columns hold.  Both take the
 * window launch's items (MVMC_SMOOTH_WIN_ITEM_INTS i32 each: slot, d, is_data, reset and src are read, rig by the update alone).
 * State per identity slot, lens_state (n_slots, MVMC_LIVE_LEN_STATE_DOUBLES) f64:
 *   [0, 66)    A = sum J^T J, the upper triangle, entry (s, t), s <= t, at s * 11 - s (s - 1) / 2 + (t - s)
 *   [66, 77)   b = sum J^T (J l_r - r)
 *   [77, 88)   l, the current skeleton             [88, 99)   l0, the lengths of the identity's first row (the prior's mean)
 *   99 next_row   100 contributed   101 committed (0 / 1)   102 committed_row (-1 before)        -- integers held as doubles
 * mvmc_live_lengths_apply, elementwise, one lane per (item, length): a reset item with data sets A = b = 0, l = l0 = row src of
 *   new_params, the counters to {0, 0, 0, -1}; another item with data gets new_params[src, 57:68] = l; items without data, malformed
 *   items (slot or src out of range) and rows of new_params no item names are untouched.
 * mvmc_live_lengths_update, after the window launch, one 64-lane workgroup per item, with n = count[slot] rows: for r = next_row ..
 *   n - 1 - lag ascending (d > 1: from n - d on, the rows from before a jump of the frame index are passed over for good -- the
 *   keypoint ring may have been overwritten at their position), unless the identity is committed: a row with >= 2 members contributes
 *   mvmc_body_lengths' residual r and Jacobian J in the lengths (16 observation rows per member, score-weighted, 1e-5 in the
 *   denominator), the pose at the row's values, linearised at the row's own lengths l_r: A += J^T J, b += J^T (J l_r - r), contributed
 *   += 1.  next_row = max(next_row, n - lag).  If a row contributed: (A + prior I) l = b + prior l0 by Cholesky; a pivot that is not
 *   positive and finite, or a length that is not finite, or not > 0 on a slot with curvature (A_ss > 0; slot 7 has none and a zero
 *   reference length, the prior alone holds it at l0), keeps the old l (status 1).  commit > 0 and contributed >= commit:
 *   committed = 1, committed_row = n - lag.  l goes into columns 57:68 of rows max(n - lag, 0) .. n - 1; no other row is written.
 *   The lanes share a row's (member, observation row) pairs; every sum runs in a fixed order with a fixed butterfly across the lanes
 *   and no atomics: an identity's bits depend on nothing else in the launch.
 *   linfo (n_items, MVMC_LIVE_LEN_INFO_DOUBLES) f64 out: {status (0; 1 the solve failed and l was kept; 6 malformed), rows contributed
 *   this tick, contributed, committed, committed_row, l (11), 1/2 sum r^2 of this tick's contributing rows}.  An item whose slot or rig
 *   is out of range, or whose rows to visit lie outside the ring (count < 1, next_row outside [0, n], n - next_row >
 *   MVMC_SMOOTH_WIN_RING), is malformed: status 6, the rest of its linfo NaN, nothing else written.
 * 0 <= lag < MVMC_SMOOTH_WIN_MAX, prior finite > 0, commit >= 0 (0: never), else MVMC_ERR_ARG; argument errors return before any HIP
 * call; nothing is allocated or synchronised inside. ---- */
#define MVMC_LIVE_LEN_STATE_DOUBLES 103
#define MVMC_LIVE_LEN_INFO_DOUBLES 17
int mvmc_live_lengths_apply(const int32_t* items, int n_items, double* new_params, int n_new, double* lens_state, int n_slots,
                            mvmcStream_t stream);
int mvmc_live_lengths_update(const mvmcSkeleton* skel_host, const double* kps17, int n_views, int p_max, const double* Pmats, int n_rigs,
                             const int32_t* items, int n_items, double* rows, const int32_t* members, const int32_t* count, int n_slots,
                             int lag, double prior, int commit, double* lens_state, double* linfo, mvmcStream_t stream);

/* ---- re-linking of the records of one person (multiview_motion_capture_amd/relinking.py).  No counterpart in the reference.  Per
 * sequence, its records in (first frame, track id) order are the nodes; record a may be followed by record b when 1 <= gap =
 * first(b) - last(a) <= max_gap, at the cost mean_k |last_joints(a)[k] + v gap - first_joints(b)[k]| (metres; v = the mean of a's end
 * velocity and b's start velocity, of the one that is defined, or zero), allowed when cost <= min(max_dist, near_dist + speed gap).
 * The links taken minimise sum cost + max_dist x (records without a successor): an optimal assignment (Kuhn-Munkres with potentials,
 * rows in record order, the first minimum wins) on the n x 2n matrix of the allowed costs and one dummy column per row.  ONE launch,
 * one 256-lane workgroup per sequence; at most MVMC_RELINK_MAX_RECORDS records per sequence.
 *   rec (N, MVMC_RELINK_REC_DOUBLES) f64 per record: the joints (18,3) of its last pose, of its first pose, then four joint centroids:
 *     of the last pose, of the pose k = min(4, poses - 1) before it, of the first pose, of the pose k after it
 *   frames (N,4) i32 per record: first frame, last frame, the frames between the two end centroids, between the two start centroids
 *     (0: the record has one pose and no velocity)
 *   seq (S,4) i32 per sequence: its first record, its records, the offset of its part of work (in 8-byte words), 0
 *   succ (N) i32 out: the record that follows (position within the sequence) or -1; head (N) i32 out: the first record of its chain;
 *   pos (N) i32 out: its position in the chain; link_cost (N) f64 out: the cost of the link to succ (0 without one)
 *   status (S) i32 out: 0 ok, 1 the assignment hit its loop bound (the sequence's outputs are not written), 2 the sequence's row of seq
 *     does not fit n_records / the capacity / work (nothing is read or written for it)
 *   work: a sequence of more than 64 records keeps its n x n costs there: mvmc_relink_work_words(n) 8-byte words each (-1: n outside
 *     the capacity), work_words in all; may be NULL when no sequence needs any.
 * Argument errors return before any HIP call; nothing is allocated, freed or synchronised inside. ---- */
#define MVMC_RELINK_MAX_RECORDS 512
#define MVMC_RELINK_REC_DOUBLES 120
long long mvmc_relink_work_words(int n_records);
int mvmc_relink(const double* rec, const int32_t* frames, const int32_t* seq, int n_records, int n_seqs, int max_gap, double max_dist,
                double near_dist, double speed, int32_t* succ, int32_t* head, int32_t* pos, double* link_cost, int32_t* status,
                double* work, long long work_words, mvmcStream_t stream);

/* ---- re-identification of a person after a long hole, by bone lengths (multiview_motion_capture_amd/relinking.py:
 * reidentify_sequences; restated in tests/reid_np.py).  No counterpart in the reference.  Two launches.
 * SIGNATURE of a record from the joints of ALL its poses, one 256-lane workgroup per record.  Per pose and bone j = 1 .. 17: b_j =
 * sqrt(dx dx + dy dy + dz dz) of joint j minus its parent (no contraction).  Ten sides: the values 0 - 6 and 8 - 10 of the skeleton's
 * side map (7 is the root and has no bone); sides 0 - 6 have a left and a right bone and the value (b_lo + b_hi) / 2 in joint order,
 * sides 8, 9, 10 one bone; a pose gives a side a value only when all its bones are finite.  Per side with m values: med = the lower
 * median (rank (m - 1) / 2 in ascending order), mad = the lower median of |x - med|, se = 1.4826 mad 1.2533 / sqrt(m) evaluated in
 * that order; a side with m < min_poses is undefined (med = se = NaN).  Both medians are exact selections (counting passes over the
 * bit patterns, integer counts only): the result does not depend on the order of the values.
 *   joints (n_poses,18,3) f64; rec (N,2) i32 per record: its first pose row, its poses (1 .. MVMC_REID_MAX_POSES)
 *   sig (N,20) f64 out: med (10), se (10); cnt (N,10) i32 out: the values per side; ends (N,6) f64 out: the joint centroid (the mean
 *   of the 18 joints, summed in joint order) of the first pose, of the last pose
 *   status (N) i32 out: 0 ok, 2 the row of rec does not fit n_poses / the capacity / work (nothing else is read or written for it)
 *   work: a record of more than MVMC_REID_LDS_POSES poses keeps its values in words 10 first .. 10 (first + poses) of it, so
 *     work_words >= 10 n_poses serves every record; records that use it must not share pose rows; may be NULL when none needs it.
 * LINKS, one 256-lane workgroup per sequence, nodes in (first frame, track id) order as in mvmc_relink.  z(A, B) = sqrt(mean over the
 * sides defined in both of (l_A - l_B)^2 / (se_A^2 + se_B^2 + 2 floor^2)), summed in side order; undefined with fewer than 5 common
 * sides.  A -> B is a candidate when A != B, gap = first(B) - last(A) >= 1 (and <= max_gap when max_gap > 0; 0 = no bound), z is
 * defined and <= max_z, and |first centroid of B - last centroid of A| <= reach + speed gap (a non-finite distance allows nothing).
 * Veto: records overlap when first(Q) <= last(R) and first(R) <= last(Q); the candidate is refused when another record Q overlaps B
 * but not A with z(A, B) > ratio z(A, Q), or overlaps A but not B with z(A, B) > ratio z(Q, B) (an undefined z vetoes nothing; a Q
 * that overlaps both ends vetoes nothing).  The links taken are an optimal assignment on the n x 2n matrix (z where allowed, max_z in
 * a row's dummy column), by mvmc_relink's own device code, as are the chains.
 *   sig, ends: the first launch's outputs; frames (N,2) i32: first frame, last frame; seq (S,4) i32 and succ, head, pos, link_cost (the
 *   z of the link taken), status: as for mvmc_relink
 *   work: a sequence of more than 64 records keeps its z and cost matrices there: mvmc_reid_work_words(n) 8-byte words each (-1: n
 *     outside the capacity MVMC_RELINK_MAX_RECORDS).
 * min_poses >= 1; max_z, floor, reach, speed finite, >= 0 and below 1e6; 0 <= ratio <= 1; max_gap >= 0; else MVMC_ERR_ARG.  Argument
 * errors return before any HIP call; nothing is allocated, freed or synchronised inside. ---- */
#define MVMC_REID_MAX_POSES 65536
#define MVMC_REID_LDS_POSES 512
long long mvmc_reid_work_words(int n_records);
int mvmc_reid_signature(const double* joints, const int32_t* rec, int n_poses, int n_records, int min_poses, double* sig, int32_t* cnt,
                        double* ends, int32_t* status, double* work, long long work_words, mvmcStream_t stream);
int mvmc_reid_link(const double* sig, const double* ends, const int32_t* frames, const int32_t* seq, int n_records, int n_seqs,
                   int max_gap, double max_z, double ratio, double floor, double reach, double speed, int32_t* succ, int32_t* head,
                   int32_t* pos, double* link_cost, int32_t* status, double* work, long long work_words, mvmcStream_t stream);

/* ---- refinement of every sequence's camera rig from its tracked people (multiview_motion_capture_amd/rig_refine.py; restated in
 * tests/rig_refine_np.py).  No counterpart in the reference.  A bundle adjustment: the unknowns are the points (one per record frame
 * and keypoint) and, per free camera, a rotation increment (R <- exp([w]x) R) and a translation increment; the residual is the plain
 * pixel reprojection K (R X + t), E = 1/2 sum r^2; Levenberg-Marquardt ((A + mu diag A) d = -g, mu / 10 accepted, x 10 rejected) with
 * the points eliminated by a Schur complement.  Sequences of one camera count share every launch; every sum has a fixed order (tiles
 * of MVMC_RIG_TILE points cut from the sequence's own points, tile parts added in tile order), no atomics.
 *   X, X_trial (N,3) f64; uv (N,C,2) f64, NaN = the camera does not observe the point.  PRECONDITION: every point of a running
 *     sequence has at least two observations among the cameras of the problem (a point without any has V = 0: its V* has no Cholesky
 *     factor and NaN goes into every sum of its tile); the caller's packing sees to that (rig_refine.py: pack_problems, min_views >= 2)
 *   tile (T,4) i32: sequence, first point, points (<= MVMC_RIG_TILE), 0;  seq (S,4) i32: first tile, tiles, first point, points
 *   slot (S,C) i32: the camera's position in the reduced system (0 .. n_free - 1, ascending with the camera) or -1 = held
 *   cams, cams_trial (S,C,MVMC_RIG_CAM_DOUBLES) f64: K (9), R (9), t (3), row-major
 *   ctl (S,4) i32 in/out: stop (0 = running, MVMC_RIG_STOP_*), trials made, trials accepted, 1 = the current reduced matrix is not
 *     positive definite.  A sequence whose stop is not 0 idles
 *   info (S,MVMC_RIG_INFO_DOUBLES) f64: E at the start, E now, mu, |c_ref - c_0| of the input, the camera part of d.g, of d^T diag(A) d,
 *     of |d|_inf, the last predicted reduction; [8, 8 + MAX_ITER) per trial 1 accepted / 0 rejected; [8 + MAX_ITER, ..) E at the start
 *     and after every trial
 *   part (T, mvmc_rig_part_doubles(C)) and part2 (T,4) f64 workspaces; red (S, mvmc_rig_red_doubles(C)) f64 out: the reduced matrix
 *     (M x M, M = 6 (C - 1), identity on unused slots), the reduced gradient (M), the camera step (M)
 * One trial = mvmc_rig_accumulate (tile parts at the current state and mu, on the matrix cores with variant = 1 or as FMAs with
 * variant = 0; then per sequence the sum, the Cholesky solve and the trial cameras) followed by mvmc_rig_step (the points' steps and
 * the trial cost per tile; then per sequence accept / reject, the gauge rescale about camera 0's centre that keeps |c_ref - c_0|, and
 * the stop rules).  Nothing is read back, allocated or synchronised inside.
 * mvmc_rig_start: per candidate point the DLT of mvmc_dlt over the views with score > min_score, with the point's own rig:
 *   obs (N,C,3) f64 u, v, score; rig_of (N) i32; Pmats (R,C,3,4) -> X0 (N,4) x, y, z, mean score; dist (N,C) reprojection distance
 *   (px) in the views used, NaN elsewhere. ---- */
#define MVMC_RIG_TILE 64
#define MVMC_RIG_MAX_CAMS 8
#define MVMC_RIG_MAX_ITER 24
#define MVMC_RIG_CAM_DOUBLES 21
#define MVMC_RIG_INFO_DOUBLES 64
#define MVMC_RIG_STOP_XTOL 1
#define MVMC_RIG_STOP_FTOL 2
#define MVMC_RIG_STOP_FEW_CAMERAS 3
#define MVMC_RIG_STOP_FEW_POINTS 4
#define MVMC_RIG_STOP_MAX_ITER 5
long long mvmc_rig_part_doubles(int n_views);   /* -1: n_views outside 2 .. MVMC_RIG_MAX_CAMS */
long long mvmc_rig_red_doubles(int n_views);
int mvmc_rig_start(const double* obs, const int32_t* rig_of, const double* Pmats, int n_points, int n_views, int n_rigs,
                   double min_score, double* X0, double* dist, mvmcStream_t stream);
int mvmc_rig_accumulate(const double* X, const double* uv, const int32_t* tile, const int32_t* seq, const int32_t* slot,
                        const double* cams, double* cams_trial, int32_t* ctl, double* info, int n_points, int n_tiles, int n_seqs,
                        int n_views, int max_iter, double mu0, int variant, double* part, double* red, mvmcStream_t stream);
int mvmc_rig_step(double* X, double* X_trial, const double* uv, const int32_t* tile, const int32_t* seq, const int32_t* slot,
                  double* cams, const double* cams_trial, int32_t* ctl, double* info, const double* red, int n_points, int n_tiles,
                  int n_seqs, int n_views, int max_iter, double ftol, double xtol, double* part2, mvmcStream_t stream);
/* The same two halves of a trial with a robust loss (restated in tests/rig_robust_np.py).  For an observation with plain residual
 * (ru, rv): s^2 = ru^2 + rv^2, delta = loss_px > 0,
 *   MVMC_RIG_LOSS_HUBER   rho = 1/2 s^2, w = 1 for s <= delta; otherwise rho = delta (s - 1/2 delta), w = delta / s
 *   MVMC_RIG_LOSS_CAUCHY  rho = 1/2 delta^2 log1p(s^2 / delta^2), w = 1 / (1 + s^2 / delta^2)
 * E = sum rho replaces 1/2 sum r^2 wherever a cost is read or written (info, the decision); at every linearisation the observation's
 * Jacobian rows and residual are multiplied by sqrt(w) (iteratively reweighted, no second-order correction), and the step and its
 * predicted reduction are those of the weighted model.  Every buffer, layout and precondition is that of the entries above; the
 * iteration converges linearly, so ftol and xtol are the caller's to choose.  MVMC_RIG_LOSS_NONE runs the code of the entries above
 * (loss_px is not read); a loss outside these three, or with a loss a loss_px that is not a finite number > 0: MVMC_ERR_ARG.
 * mvmc_rig_weights: w (N,C) f64 out, the weight of every observation at (X, cams) -- 1 with MVMC_RIG_LOSS_NONE -- and NaN where the
 * camera does not observe the point; rows of points outside every tile are not written. */
#define MVMC_RIG_LOSS_NONE 0
#define MVMC_RIG_LOSS_HUBER 1
#define MVMC_RIG_LOSS_CAUCHY 2
int mvmc_rig_accumulate_robust(const double* X, const double* uv, const int32_t* tile, const int32_t* seq, const int32_t* slot,
                               const double* cams, double* cams_trial, int32_t* ctl, double* info, int n_points, int n_tiles, int n_seqs,
                               int n_views, int max_iter, double mu0, int variant, double* part, double* red, int loss, double loss_px,
                               mvmcStream_t stream);
int mvmc_rig_step_robust(double* X, double* X_trial, const double* uv, const int32_t* tile, const int32_t* seq, const int32_t* slot,
                         double* cams, const double* cams_trial, int32_t* ctl, double* info, const double* red, int n_points,
                         int n_tiles, int n_seqs, int n_views, int max_iter, double ftol, double xtol, double* part2, int loss,
                         double loss_px, mvmcStream_t stream);
int mvmc_rig_weights(const double* X, const double* uv, const int32_t* tile, const double* cams, int n_points, int n_tiles, int n_seqs,
                     int n_views, int loss, double loss_px, double* w, mvmcStream_t stream);
/* The two halves of a trial with intrinsic unknowns (restated in tests/rig_intr_np.py).  A camera with islot >= 0 has n_intr more
 * unknowns: n_intr = 1 phi (K00, K01, K11 <- e^phi x themselves), n_intr = 3 also dcx, dcy (added to K02, K12).  Their rows of an
 * observation are d(u, v)/dphi = (u - cx, v - cy), d/dcx = (1, 0), d/dcy = (0, 1), times sqrt(w) with a loss.
 *   islot (S,C) i32: the camera's position among the sequence's cameras with free intrinsics (ascending with the camera) or -1 = K
 *     held.  Camera 0 has slot -1 (its pose is held) and may have islot >= 0; a camera whose observations left has both -1
 *   K0 (S,C,3) f64: fx, cx, cy of the input K, the centre of the prior
 *   focal_sigma (relative), centre_sigma (px): the prior E_prior = 1/2 sum (phi / focal_sigma)^2 + 1/2 sum (dcx^2 + dcy^2) /
 *     centre_sigma^2 over the cameras with islot >= 0, phi = log(K00 / fx0) accumulated over the call; +inf = no term.  They are
 *     scalars of the launch so that the entry can refuse them.  E_prior is part of every cost in info and of the decision, and of
 *     the diagonal and gradient of the intrinsic columns
 *   cams is updated in K as well on an accepted trial; cams_trial carries the trial K
 * Layout of the reduced system: one contiguous block per camera in camera order, its 6 pose columns if slot >= 0, then its n_intr
 * intrinsic columns if islot >= 0; M = 6 (C - 1) + n_intr C columns, identity on those past the sequence's own.  red (S,
 * mvmc_rig_red_doubles_intr) is that M x M matrix, the gradient (M), the step (M); part has mvmc_rig_part_doubles_intr per tile.
 * In |d|_inf the intrinsic steps count as phi and dc / fx.  The gauge rescale moves no intrinsic.  The stacked product runs on the
 * matrix cores: variant must be 1.  MVMC_RIG_LOSS_NONE is the plain cost plus prior.  n_intr outside {1, 3}, a sigma that is <= 0 or
 * NaN, variant != 1: MVMC_ERR_ARG, nothing launched.  Everything else is as in the entries above. */
long long mvmc_rig_part_doubles_intr(int n_views, int n_intr);   /* -1: n_views outside 2 .. MVMC_RIG_MAX_CAMS or n_intr not 1 or 3 */
long long mvmc_rig_red_doubles_intr(int n_views, int n_intr);
int mvmc_rig_accumulate_intr(const double* X, const double* uv, const int32_t* tile, const int32_t* seq, const int32_t* slot,
                             const double* cams, double* cams_trial, int32_t* ctl, double* info, int n_points, int n_tiles, int n_seqs,
                             int n_views, int max_iter, double mu0, int variant, double* part, double* red, int loss, double loss_px,
                             int n_intr, const int32_t* islot, const double* K0, double focal_sigma, double centre_sigma,
                             mvmcStream_t stream);
int mvmc_rig_step_intr(double* X, double* X_trial, const double* uv, const int32_t* tile, const int32_t* seq, const int32_t* slot,
                       double* cams, const double* cams_trial, int32_t* ctl, double* info, const double* red, int n_points, int n_tiles,
                       int n_seqs, int n_views, int max_iter, double ftol, double xtol, double* part2, int loss, double loss_px,
                       int n_intr, const int32_t* islot, const double* K0, double focal_sigma, double centre_sigma, mvmcStream_t stream);

/* ---- lens distortion at the door of the pipeline (multiview_motion_capture_amd/lens.py; restated in tests/lens_np.py).  No counterpart
 * in the reference, whose only projection is project_3d_points_to_image_plane_without_distortion (mv_math_util.py).  Every other entry
 * point reads keypoints as pinhole pixels of P = K Rt; mvmc_lens_undistort turns a detector's raw pixels into those, once, and
 * mvmc_lens_distort is the way back (drawing on the raw images).  One pass over the triples, float64 arithmetic, a float32 output is
 * the float64 result rounded once.
 *   kps_in, kps_out (F,C,n_points,3) f32|f64 triples (x, y, score), dtype as mvmc_ingest; n_points = P J for any J.  kps_out may be
 *     kps_in (each lane reads, then writes, its own triple)
 *   lens (R,C,MVMC_LENS_DOUBLES) f64, one row per (rig, camera): {model, fx, fy, cx, cy, skew, k[0..7], 0, 0}; a row whose model is
 *     neither MVMC_LENS_BROWN nor MVMC_LENS_FISHEYE is a pinhole row
 *   rig_of_frame (F) i32 or NULL = rig 0.  A frame whose index lies outside [0, R) reads no row: its triples come out (0,0,0) and
 *     its dropped row is -1
 *   dropped (F,C) i32 out, every element written once: scored keypoints of the view without a valid pre-image (undistort); distort
 *     writes 0 (it drops nothing) or -1
 * Normalised coordinates y = (v - cy) / fy, x = (u - cx - skew y) / fx; pixels u = fx x + skew y + cx, v = fy y + cy.
 * BROWN (OpenCV's order k1 k2 p1 p2 k3 k4 k5 k6): r2 = x^2 + y^2, rad = (1 + k1 r2 + k2 r2^2 + k3 r2^3) / (1 + k4 r2 + k5 r2^2 + k6 r2^3),
 *   x' = x rad + 2 p1 x y + p2 (r2 + 2 x^2), y' = y rad + p1 (r2 + 2 y^2) + 2 p2 x y.  The inverse is Newton's iteration in (x, y) with
 *   the analytic Jacobian from the distorted point: at most MVMC_LENS_MAX_ITER steps, converged when |dx| + |dy| <= 1e-13 (1 + |x| + |y|)
 *   (x, y after the step).
 * FISHEYE (cv2.fisheye, Kannala-Brandt k1..k4): theta = atan r, theta_d = theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8),
 *   scale theta_d / r (1 at r = 0).  The inverse is Newton's iteration in theta from theta_d, |d| <= 1e-13 (1 + |theta|), then
 *   r = tan theta.
 * Accept rule of the inverse, for a triple with score > 0: the iteration converged; the result is finite; at every iterate a step was
 *   taken from and at the answer the forward Jacobian's determinant (fisheye: d theta_d / d theta) is positive and Brown's rad is
 *   positive; fisheye: 0 <= theta < MVMC_LENS_FISHEYE_MAX_THETA.  A rejected triple is written (0,0,0) -- OpenPose's "not detected",
 *   which mvmc_ingest's score test ignores -- and counted.  A triple with score <= 0 and every triple of a pinhole row is copied bit
 *   for bit; scores always are.
 * Argument errors return MVMC_ERR_ARG before any HIP call; MVMC_ERR_UNSUPPORTED for more than 128 cameras. ---- */
#define MVMC_LENS_DOUBLES 16
#define MVMC_LENS_PINHOLE 0
#define MVMC_LENS_BROWN 1
#define MVMC_LENS_FISHEYE 2
#define MVMC_LENS_MAX_ITER 12
#define MVMC_LENS_FISHEYE_MAX_THETA 1.5
int mvmc_lens_undistort(const void* kps_in, int dtype, int n_frames, int n_views, int n_points, const double* lens,
                        const int32_t* rig_of_frame, int n_rigs, void* kps_out, int32_t* dropped, mvmcStream_t stream);
int mvmc_lens_distort(const void* kps_in, int dtype, int n_frames, int n_views, int n_points, const double* lens,
                      const int32_t* rig_of_frame, int n_rigs, void* kps_out, int32_t* dropped, mvmcStream_t stream);

/* ---- calibration of every sequence's rig from one person walking the volume (multiview_motion_capture_amd/rig_init.py; restated in
 * tests/rig_init_np.py).  No counterpart in the reference.  The relative pose of every camera pair from two-view geometry; the pose
 * graph, the bundle adjustment (mvmc_rig_*) and the metric scale follow on the host side.  Sequences of any frame and camera counts
 * share every launch; one wave per pair (or per pair and hypothesis), sums in a fixed order, no atomics: a pair's numbers depend on
 * nothing else in the launch.
 *   xn (n_rows,17,2) f64: the normalised coordinates K^-1 (u, v, 1) of the ONE pose of a (frame, view), NaN where the joint is not
 *     usable (no or several poses in the view, score too low); the row of (sequence s, frame f, view c) is seq[s][0] + f C_s + c
 *   seq (S,4) i32: first row, frames F_s, cameras C_s, 0;  pair (Q,4) i32: sequence, a, b (a != b), first frame slot: the pair owns
 *     the F_s frame slots from there of mom, cnt and usable, and 17 times as many correspondence slots (frame f, joint j at f 17 + j)
 *     of mask and points.  A pair row that does not fit n_rows / n_slots / its sequence is skipped.
 * mvmc_pair_moments -> norm (Q,MVMC_RIGINIT_NORM_DOUBLES) f64: centroid x, y and scale (mean distance -> sqrt 2) of side a, of side
 *   b, the number of correspondences, 0;  mom (n_slots,45) f64: per frame the upper triangle (row-major) of sum r r^T over its common
 *   joints in joint order, r = (ub ua, ub va, ub, vb ua, vb va, vb, ua, va, 1) in Hartley-normalised coordinates: the row of
 *   x_b^T E x_a = 0, E row-major;  cnt (n_slots) i32 the frame's common joints;  usable (n_slots) i32: the pair's frames with
 *   cnt >= 1 in frame order, then -1;  n_usable (Q) i32.
 * mvmc_pair_consensus: hypothesis h of a pair sums mom over the sample_frames frames usable[floor(u[h][k] n_usable)] (u (H,m) f64 in
 *   [0, 1), duplicates allowed, summed in k order), takes the eigenvector of the smallest eigenvalue (cyclic Jacobi, fixed sweeps),
 *   E = T_b^T Ehat T_a scaled to Frobenius norm 1 -> E (Q,H,9) f64, and count (Q,H) i32: the correspondences with Sampson distance
 *   < thr[q] (thr (Q) f64).  A pair with n_usable < sample_frames: E = 0, count = 0.
 * mvmc_pair_refit: the hypothesis with the largest count (ties: lowest index) is round 0; every round: the moment matrix over the
 *   inliers of the current E, its null vector, denormalised and projected onto the essential matrices (singular values 1, 1, 0);
 *   the refit round with the most inliers (ties: the earliest) -- round 0 when there is no refit round or the best one has fewer than
 *   9/10 of round 0's inliers (a collapsed refit) -- is decomposed: t = +-u2, first the sign that makes its largest component
 *   positive; R = U W V^T and U W^T V^T, the larger trace first; candidates (R0,t), (R0,-t), (R1,t), (R1,-t); the inliers are
 *   triangulated with mvmc_dlt's arithmetic for [I|0], [R|t]; the candidate with the most points in front of both cameras wins (ties:
 *   lowest index) -> pose (Q,MVMC_RIGINIT_POSE_DOUBLES) f64: R (9), t (3, unit), E (9), the hypothesis, the round, the inliers, the
 *   four votes, the candidate, 0 0 0;  round_count (Q,MVMC_RIGINIT_MAX_ROUNDS+1) i32, -1 for rounds not made;  mask (n_slots 17) i32;
 *   points (n_slots 17,3) f64 in camera a's frame, NaN where not an inlier.  A pair without a hypothesis with an inlier: all zero.
 * Argument errors return MVMC_ERR_ARG before any HIP call. ---- */
#define MVMC_RIGINIT_NORM_DOUBLES 8
#define MVMC_RIGINIT_POSE_DOUBLES 32
#define MVMC_RIGINIT_MAX_ROUNDS 8
#define MVMC_RIGINIT_MAX_SAMPLE 32
int mvmc_pair_moments(const double* xn, const int32_t* seq, const int32_t* pair, int n_seqs, int n_pairs, int n_rows, int n_slots,
                      double* norm, double* mom, int32_t* cnt, int32_t* usable, int32_t* n_usable, mvmcStream_t stream);
int mvmc_pair_consensus(const double* xn, const int32_t* seq, const int32_t* pair, int n_seqs, int n_pairs, int n_rows, int n_slots,
                        const double* norm, const double* mom, const int32_t* usable, const int32_t* n_usable, const double* u,
                        const double* thr, int n_hyp, int sample_frames, double* E, int32_t* count, mvmcStream_t stream);
int mvmc_pair_refit(const double* xn, const int32_t* seq, const int32_t* pair, int n_seqs, int n_pairs, int n_rows, int n_slots,
                    const double* norm, const double* E, const int32_t* count, const double* thr, int n_hyp, int refit_rounds,
                    double* pose, int32_t* round_count, int32_t* mask, double* points, mvmcStream_t stream);

/* ---- detections with exchanged left / right limbs (multiview_motion_capture_amd/exchanges.py; restated in tests/exchange_np.py).  No
 * counterpart in the reference.  Against the 3-D joints of finished records, every detection's arms, legs and face are tested for a
 * left / right exchange of their labels and the exchange is undone in the caller's keypoints.
 * Limb groups as COCO-17 pairs (left, right): arms (5,6) (7,8) (9,10), flag bit 0; legs (11,12) (13,14) (15,16), bit 1; face (3,4),
 * bit 2 -- the pairs among reprojection_error's 15 common joints (motion_capture.py:403-414), compared with the same BASIC_18 joints;
 * the eyes (1,2) follow the face, in BODY_25 input the feet (19,20,21) <-> (22,23,24) follow the legs.
 *
 * mvmc_exchange_observe: mvmc_body_observe's problems, arguments and conflict rule with an exchange-aware distance.  Per (problem b,
 * camera c) the problem's joints are projected once (1e-5 in the denominator).  For a pose of b's frame in camera c, a common keypoint
 * is valid when its score > min_score; a group's costs run over its pairs with BOTH keypoints valid, summed in the order above, left
 * keypoint before right: e0 the pixel distances under the labels as they are, e1 with each keypoint compared with the other side's
 * joint; n_g the keypoints counted.  d* = (the as-is distances of the valid keypoints outside such pairs -- pair order, then the nose
 * -- + min(e0, e1) of arms, legs, face in this order) / (valid common keypoints).  The pose with the smallest d* that is finite and
 * below max_dist is chosen (ties: the lower slot); then, as in mvmc_body_observe, of two problems of one frame that chose one pose
 * the smaller d* keeps it (equal: the lower rank), the other takes nothing.  Group g of the pose a problem keeps is exchanged iff
 * n_g >= 2 and e1 + margin_px n_g < e0 and e1 < ratio e0 (both strict; products and sums rounded one by one).
 *   kps17, counts, n_frames, n_views, p_max, Pmats, n_rigs, frame_of, rig_of, joints, order, grp_lo, grp_hi, rank, n_problems,
 *   min_score, max_dist: as mvmc_body_observe.  margin_px finite and >= 0, 0 < ratio <= 1: else MVMC_ERR_ARG
 *   members (B,C) i32 out: the kept pose index q = (f C + c) P + p, or -1; dist (B,C) f64 out: d* of the nearest pose BEFORE the
 *   conflicts (+inf: none); flags (B,C) u8 out: bit g = group g of the kept pose is exchanged (0 without one); cost (B,C,3,2) f64
 *   out: e0, e1 per group of the kept pose, NaN for a group without a fully valid pair and where no pose is kept
 * No workspace, no allocation, no synchronisation, no atomics: every sum runs inside one lane in a fixed order, so a problem's
 * outputs are the same bits alone, in a batch and from run to run. */
int mvmc_exchange_observe(const double* kps17, const int32_t* counts, int n_frames, int n_views, int p_max, const double* Pmats,
                          int n_rigs, const int32_t* frame_of, const int32_t* rig_of, const double* joints, const int32_t* order,
                          const int32_t* grp_lo, const int32_t* grp_hi, const int32_t* rank, int n_problems, double min_score,
                          double max_dist, double margin_px, double ratio, int32_t* members, double* dist, uint8_t* flags,
                          double* cost, mvmcStream_t stream);

/* mvmc_exchange_apply: the repaired copy of the caller's keypoints.  kps_in, kps_out (n_slots, n_joints, 3) f32|f64 (dtype as
 * mvmc_ingest; n_joints 17 or 25; n_slots = F C P pose slots, different buffers); slot_flags (n_slots) u8: bit g = exchange group g
 * of the slot.  One lane per (x, y, score) triple copies the triple that belongs under its name: its partner's where the slot's flag
 * names its group -- also in a pair of which only one keypoint was valid, and in the followers -- its own otherwise.  No arithmetic
 * and no conversion: every triple of the output is a triple of the input, bit for bit. */
int mvmc_exchange_apply(const void* kps_in, int dtype, long long n_slots, int n_joints, const uint8_t* slot_flags, void* kps_out,
                        mvmcStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MVMC_H */
