// Trajectory smoothing of finished tracklets (multiview_motion_capture_amd/smoothing.py; algorithm restated in tests/smooth_np.py): one
// Levenberg-Marquardt solve per identity over every frame from its first to its last, E = the IK's stage-1 data term of every frame with
// selected views + a diagonal velocity / acceleration prior on the 39 stage-1 parameters.  No counterpart in the reference, whose only
// temporal element is the IK's warm start.
//   blocks  ONE wave per (identity, frame): FK, the stage-1 residual and its analytic Jacobian (angular velocity x lever arm through the
//           projection), reduced per observed joint first (W_k = sum_v s^2 (du du^T + dv dv^T), t_k = sum_v s (du fu + dv fv)), then
//           J^T J = sum_k D_k^T W_k D_k and J^T r = sum_k D_k^T t_k with D_k = d X_k / d x (3 x 39): the upper triangle, J^T r and E_t of
//           the frame into one of two block buffers (the other holds the blocks of the accepted point); with a robust loss
//           (mvmc_smooth_blocks_robust) the blocks of the reweighted model, the same layout: J^T W J, J^T W r, sum s^2 rho; with foot
//           contacts (mvmc_smooth_blocks_contact) the labelled rows' 1/2 wc |X_ankle - a|^2 joins the ankle's W_k, t_k and E, the same
//           layout again (the labels and anchors come from csrc/mvmc_smooth_contact.hip between two rounds of the solve); with a floor
//           (mvmc_smooth_blocks_floor) that term weighs the part along the sequence's floor normal with a second weight;
//   step    ONE 256-lane workgroup per identity: the accept / reject decision on the last trial (E summed in a fixed order), then one
//           block-banded solve of (A + mu diag(A)) d = -g over all the identity's frames (mvmc_smooth_sweep.h, the sweep the live
//           smoother runs too; the factor goes to the caller's workspace), and the next trial point.
//   weights ONE wave per row, after the solve: FK and the projections alone, the loss's weight of every (camera, observed joint) pair.
// Every sum runs in a fixed order inside one identity's own lanes: an identity's numbers depend on nothing else in the launch.
#define MVMC_DEVICE_ONLY
#include "mvmc_common.h"
#include "mvmc_track.hip"
#include "mvmc_ik1.hip"
#undef MVMC_DEVICE_ONLY

namespace {

#include "mvmc_smooth_row.h"
#include "mvmc_smooth_sweep.h"

template <int LOSS>
__global__ void __launch_bounds__(64) smooth_blocks_kernel(Ik1Tables T, const double* __restrict__ kps17, const double* __restrict__ Pmats,
                                                           int C, int Pmax, const int32_t* __restrict__ rig_of,
                                                           const int32_t* __restrict__ members, const double* __restrict__ xe,
                                                           const int32_t* __restrict__ id_of, const int32_t* __restrict__ ctl,
                                                           int n_frames, double* __restrict__ blk, double loss_px) {
    __shared__ SmBlkLds L;
    const int f = blockIdx.x;
    const int id = uni((int)id_of[f]);
    if (uni((int)ctl[id * 4]) != 0) return;                      // stopped identity: nothing to evaluate
    const int buf = 1 - uni((int)ctl[id * 4 + 1]);               // the buffer that does not hold the accepted point's blocks
    sm_row_block<LOSS>(T, L, kps17, Pmats + (size_t)rig_of[f] * C * 12, C, Pmax, members + (size_t)f * C, xe + (size_t)f * 68,
                       blk + ((size_t)buf * n_frames + f) * SM_BLK, loss_px);
}

// The same launch with the foot-contact term of the rows that carry a label (include/mvmc.h: mvmc_smooth_blocks_contact): cmask (N,2),
// anchors (N,2,3), wc = contact_weight.  A kernel of its own, so that the launches without contacts keep theirs.
template <int LOSS>
__global__ void __launch_bounds__(64) smooth_blocks_contact_kernel(Ik1Tables T, const double* __restrict__ kps17,
                                                                   const double* __restrict__ Pmats, int C, int Pmax,
                                                                   const int32_t* __restrict__ rig_of, const int32_t* __restrict__ members,
                                                                   const double* __restrict__ xe, const int32_t* __restrict__ id_of,
                                                                   const int32_t* __restrict__ ctl, int n_frames, double* __restrict__ blk,
                                                                   double loss_px, const int32_t* __restrict__ cmask,
                                                                   const double* __restrict__ anchors, double wc) {
    __shared__ SmBlkLds L;
    const int f = blockIdx.x;
    const int id = uni((int)id_of[f]);
    if (uni((int)ctl[id * 4]) != 0) return;
    const int buf = 1 - uni((int)ctl[id * 4 + 1]);
    sm_row_block<LOSS, true>(T, L, kps17, Pmats + (size_t)rig_of[f] * C * 12, C, Pmax, members + (size_t)f * C, xe + (size_t)f * 68,
                             blk + ((size_t)buf * n_frames + f) * SM_BLK, loss_px, cmask + (size_t)f * 2, anchors + (size_t)f * 6, wc);
}

// The contact launch with a floor (include/mvmc.h: mvmc_smooth_blocks_floor): normals (n_rigs,3) the unit floor normal of every
// sequence, NaN where it has none, wf = floor_weight.  Again a kernel of its own: the launches without a floor keep theirs.
template <int LOSS>
__global__ void __launch_bounds__(64) smooth_blocks_floor_kernel(Ik1Tables T, const double* __restrict__ kps17,
                                                                 const double* __restrict__ Pmats, int C, int Pmax,
                                                                 const int32_t* __restrict__ rig_of, const int32_t* __restrict__ members,
                                                                 const double* __restrict__ xe, const int32_t* __restrict__ id_of,
                                                                 const int32_t* __restrict__ ctl, int n_frames, double* __restrict__ blk,
                                                                 double loss_px, const int32_t* __restrict__ cmask,
                                                                 const double* __restrict__ anchors, double wc,
                                                                 const double* __restrict__ normals, double wf) {
    __shared__ SmBlkLds L;
    const int f = blockIdx.x;
    const int id = uni((int)id_of[f]);
    if (uni((int)ctl[id * 4]) != 0) return;
    const int buf = 1 - uni((int)ctl[id * 4 + 1]);
    const int rig = uni((int)rig_of[f]);
    sm_row_block<LOSS, true, true>(T, L, kps17, Pmats + (size_t)rig * C * 12, C, Pmax, members + (size_t)f * C, xe + (size_t)f * 68,
                                   blk + ((size_t)buf * n_frames + f) * SM_BLK, loss_px, cmask + (size_t)f * 2, anchors + (size_t)f * 6,
                                   wc, normals + (size_t)rig * 3, wf);
}

// ---- weights ----
struct SmPosLds { double Rl[18 * 9], Rg[18 * 9], pos[18 * 3]; };

// One row per wave: w[f][c][k] = the loss's weight of camera c's member and observed joint k at x, NaN without a member or a score.
// Every slot of the row is written exactly once, by the lane that owns it.
template <int LOSS>
__global__ void __launch_bounds__(64) smooth_obs_weights_kernel(Ik1Tables T, const double* __restrict__ kps17,
                                                                const double* __restrict__ Pmats, int C, int Pmax,
                                                                const int32_t* __restrict__ rig_of, const int32_t* __restrict__ members,
                                                                const double* __restrict__ xe, double loss_px, double* __restrict__ wout) {
    __shared__ SmPosLds L;
    const int f = blockIdx.x, lane = threadIdx.x & 63;
    sm_row_fk<false>(T, L, xe + (size_t)f * 68);
    const double* Prig = Pmats + (size_t)rig_of[f] * C * 12;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    for (int i = lane; i < C * NOBS; i += 64) {
        const int c = i / NOBS, k = i - c * NOBS, m = members[(size_t)f * C + c];
        double wl = nan;
        if (m >= 0) {
            const int K = kIkSkel[k];
            double ob0, ob1, s, w, u, vv, rho;
            sm_pair(kps17 + (size_t)m * 51, Prig + (size_t)((m / Pmax) % C) * 12, kIkObs[k], L.pos[3 * K], L.pos[3 * K + 1],
                    L.pos[3 * K + 2], ob0, ob1, s, w, u, vv);
            const double ru = u - ob0, rv = vv - ob1;
            if (s != 0.0) sm_rho_w<LOSS>(ru * ru + rv * rv, loss_px, rho, wl);
        }
        wout[((size_t)f * C + c) * NOBS + k] = wl;
    }
}

// ---- step ----
__global__ void __launch_bounds__(SM_THREADS) smooth_step_kernel(Ik1Tables T, double* __restrict__ xall, double* __restrict__ xtall,
                                                                 const double* __restrict__ blk, const int32_t* __restrict__ id_lo,
                                                                 int n_frames, double root_vel, double root_acc, double ang_vel,
                                                                 double ang_acc, double mu0, double ftol, double xtol, int max_iter,
                                                                 int phase, int32_t* __restrict__ ctl, double* __restrict__ info,
                                                                 double* __restrict__ work) {
    __shared__ SmSweepLds L;
    const int tid = threadIdx.x, id = blockIdx.x;
    int32_t* cl = ctl + id * 4;
    if (uni((int)cl[0]) != 0) return;   // stopped: wave-uniform for the whole workgroup
    const int lo = id_lo[id], n = id_lo[id + 1] - lo;
    double* inf = info + (size_t)id * MVMC_SMOOTH_INFO_DOUBLES;
    double* x = xall + (size_t)lo * 68;
    double* xt = xtall + (size_t)lo * 68;
    double* wk = work + (size_t)lo * SM_WORK;
    sm_sweep_tables(L, T, root_vel, root_acc, ang_vel, ang_acc);
    int cur = uni((int)cl[1]);
    const double* bcur;
    double mu;
    int trials, n_acc;
    if (phase == 0) {   // the start: the blocks at x0 are in buffer 1 - cur
        cur = 1 - cur;
        bcur = blk + ((size_t)cur * n_frames + lo) * SM_BLK;
        const double Ed = sm_data_energy(L, bcur, SM_BLK, n), Ep = sm_prior_energy(L, x, n, 0);
        if (tid < MVMC_SMOOTH_INFO_DOUBLES) inf[tid] = tid < 8 ? 0.0 : -1.0;
        __syncthreads();
        if (tid == 0) { inf[0] = Ed; inf[1] = Ep; inf[2] = Ed; inf[3] = Ep; cl[1] = cur; }
        mu = mu0;
        trials = 0;
        n_acc = 0;
    } else {            // the decision on the trial whose blocks are in buffer 1 - cur
        const double* btr = blk + ((size_t)(1 - cur) * n_frames + lo) * SM_BLK;
        const double Etd = sm_data_energy(L, btr, SM_BLK, n), Etp = sm_prior_energy(L, xt, n, 0);
        const double Ed = inf[2], Ep = inf[3];
        const double E = Ed + Ep, Et = Etd + Etp;
        mu = inf[6];
        trials = (int)inf[4];
        n_acc = (int)inf[5];
        __syncthreads();
        const bool acc = Et < E;
        if (tid == 0) inf[8 + trials] = acc ? 1.0 : 0.0;
        ++trials;
        bool stop = false;
        if (acc) {
            for (int i = tid; i < n * 68; i += SM_THREADS) x[i] = xt[i];
            cur = 1 - cur;
            mu /= 10.0;
            ++n_acc;
            if (tid == 0) { inf[2] = Etd; inf[3] = Etp; cl[1] = cur; }
            if (E - Et < ftol * E) stop = true;
        } else {
            mu *= 10.0;
        }
        if (stop) {
            if (tid == 0) { inf[4] = trials; inf[5] = n_acc; inf[6] = mu; inf[7] = 4.0; cl[0] = 1; }
            return;
        }
        bcur = blk + ((size_t)cur * n_frames + lo) * SM_BLK;
    }
    if (trials >= max_iter) {
        if (tid == 0) { inf[4] = trials; inf[5] = n_acc; inf[6] = mu; inf[7] = 1.0; cl[0] = 1; }
        return;
    }
    const SmStep st = sm_sweep(L, bcur, SM_BLK, wk, SM_WORK, x, n, 0, n, mu);
    const double E = inf[2] + inf[3];
    const double pred = st.pred, dmax = st.dmax;
    const int fail = uni(st.fail);
    int why = 0;
    if (fail || !(dmax == dmax)) why = 5;
    else if (dmax < xtol) why = 2;
    else if (pred < ftol * E) why = 3;
    if (why) {
        if (tid == 0) { inf[4] = trials; inf[5] = n_acc; inf[6] = mu; inf[7] = why; cl[0] = 1; }
        return;
    }
    for (int i = tid; i < n * 68; i += SM_THREADS) xt[i] = x[i];
    __syncthreads();
    for (int i = tid; i < n * SK; i += SM_THREADS) {
        const int t = i / SK, q = i - t * SK;
        xt[(size_t)t * 68 + L.colx[q]] = x[(size_t)t * 68 + L.colx[q]] + wk[(size_t)t * SM_WORK + W_Y + q];
    }
    if (tid == 0) { inf[4] = trials; inf[5] = n_acc; inf[6] = mu; inf[7] = 0.0; }
}

}  // namespace

extern "C" int mvmc_smooth_blocks_robust(const mvmcSkeleton* skel_host, const double* kps17, int n_views, int p_max, const double* Pmats,
                                         const int32_t* rig_of, const int32_t* members, const double* x, const int32_t* id_of,
                                         const int32_t* ctl, int n_frames, double* blk, int loss, double loss_px, mvmcStream_t stream) {
    if (!skel_host || n_frames < 0 || n_views <= 0 || n_views > MVMC_SMOOTH_MAX_VIEWS || p_max <= 0) return MVMC_ERR_ARG;
    if (!sm_loss_ok(loss, loss_px)) return MVMC_ERR_ARG;
    if (n_frames == 0) return MVMC_OK;
    if (!kps17 || !Pmats || !rig_of || !members || !x || !id_of || !ctl || !blk) return MVMC_ERR_ARG;
    Ik1Tables T;
    if (!sm_tables(skel_host, &T)) return MVMC_ERR_UNSUPPORTED;
    auto kernel = loss == MVMC_SMOOTH_LOSS_HUBER    ? smooth_blocks_kernel<MVMC_SMOOTH_LOSS_HUBER>
                  : loss == MVMC_SMOOTH_LOSS_CAUCHY ? smooth_blocks_kernel<MVMC_SMOOTH_LOSS_CAUCHY>
                                                    : smooth_blocks_kernel<MVMC_SMOOTH_LOSS_NONE>;
    hipLaunchKernelGGL(kernel, dim3(n_frames), dim3(64), 0, (hipStream_t)stream, T, kps17, Pmats, n_views, p_max, rig_of, members, x,
                       id_of, ctl, n_frames, blk, loss_px);
    MVMC_CHECK_LAUNCH();
    return MVMC_OK;
}

extern "C" int mvmc_smooth_blocks_contact(const mvmcSkeleton* skel_host, const double* kps17, int n_views, int p_max, const double* Pmats,
                                          const int32_t* rig_of, const int32_t* members, const double* x, const int32_t* id_of,
                                          const int32_t* ctl, int n_frames, double* blk, int loss, double loss_px, const int32_t* cmask,
                                          const double* anchors, double contact_weight, mvmcStream_t stream) {
    if (!skel_host || n_frames < 0 || n_views <= 0 || n_views > MVMC_SMOOTH_MAX_VIEWS || p_max <= 0) return MVMC_ERR_ARG;
    if (!sm_loss_ok(loss, loss_px)) return MVMC_ERR_ARG;
    if (!(contact_weight >= 0.0 && contact_weight <= 1.7976931348623157e308)) return MVMC_ERR_ARG;   // (NaN fails both)
    if (n_frames == 0) return MVMC_OK;
    if (!kps17 || !Pmats || !rig_of || !members || !x || !id_of || !ctl || !blk || !cmask || !anchors) return MVMC_ERR_ARG;
    Ik1Tables T;
    if (!sm_tables(skel_host, &T)) return MVMC_ERR_UNSUPPORTED;
    auto kernel = loss == MVMC_SMOOTH_LOSS_HUBER    ? smooth_blocks_contact_kernel<MVMC_SMOOTH_LOSS_HUBER>
                  : loss == MVMC_SMOOTH_LOSS_CAUCHY ? smooth_blocks_contact_kernel<MVMC_SMOOTH_LOSS_CAUCHY>
                                                    : smooth_blocks_contact_kernel<MVMC_SMOOTH_LOSS_NONE>;
    hipLaunchKernelGGL(kernel, dim3(n_frames), dim3(64), 0, (hipStream_t)stream, T, kps17, Pmats, n_views, p_max, rig_of, members, x,
                       id_of, ctl, n_frames, blk, loss_px, cmask, anchors, contact_weight);
    MVMC_CHECK_LAUNCH();
    return MVMC_OK;
}

extern "C" int mvmc_smooth_blocks_floor(const mvmcSkeleton* skel_host, const double* kps17, int n_views, int p_max, const double* Pmats,
                                        const int32_t* rig_of, const int32_t* members, const double* x, const int32_t* id_of,
                                        const int32_t* ctl, int n_frames, double* blk, int loss, double loss_px, const int32_t* cmask,
                                        const double* anchors, double contact_weight, const double* normals, double floor_weight,
                                        mvmcStream_t stream) {
    if (!skel_host || n_frames < 0 || n_views <= 0 || n_views > MVMC_SMOOTH_MAX_VIEWS || p_max <= 0) return MVMC_ERR_ARG;
    if (!sm_loss_ok(loss, loss_px)) return MVMC_ERR_ARG;
    if (!(contact_weight >= 0.0 && contact_weight <= 1.7976931348623157e308)) return MVMC_ERR_ARG;   // (NaN fails both)
    if (!(floor_weight >= 0.0 && floor_weight <= 1.7976931348623157e308)) return MVMC_ERR_ARG;
    if (n_frames == 0) return MVMC_OK;
    if (!kps17 || !Pmats || !rig_of || !members || !x || !id_of || !ctl || !blk || !cmask || !anchors || !normals) return MVMC_ERR_ARG;
    Ik1Tables T;
    if (!sm_tables(skel_host, &T)) return MVMC_ERR_UNSUPPORTED;
    auto kernel = loss == MVMC_SMOOTH_LOSS_HUBER    ? smooth_blocks_floor_kernel<MVMC_SMOOTH_LOSS_HUBER>
                  : loss == MVMC_SMOOTH_LOSS_CAUCHY ? smooth_blocks_floor_kernel<MVMC_SMOOTH_LOSS_CAUCHY>
                                                    : smooth_blocks_floor_kernel<MVMC_SMOOTH_LOSS_NONE>;
    hipLaunchKernelGGL(kernel, dim3(n_frames), dim3(64), 0, (hipStream_t)stream, T, kps17, Pmats, n_views, p_max, rig_of, members, x,
                       id_of, ctl, n_frames, blk, loss_px, cmask, anchors, contact_weight, normals, floor_weight);
    MVMC_CHECK_LAUNCH();
    return MVMC_OK;
}

extern "C" int mvmc_smooth_blocks(const mvmcSkeleton* skel_host, const double* kps17, int n_views, int p_max, const double* Pmats,
                                  const int32_t* rig_of, const int32_t* members, const double* x, const int32_t* id_of, const int32_t* ctl,
                                  int n_frames, double* blk, mvmcStream_t stream) {
    return mvmc_smooth_blocks_robust(skel_host, kps17, n_views, p_max, Pmats, rig_of, members, x, id_of, ctl, n_frames, blk,
                                     MVMC_SMOOTH_LOSS_NONE, 0.0, stream);
}

extern "C" int mvmc_smooth_obs_weights(const mvmcSkeleton* skel_host, const double* kps17, int n_views, int p_max, const double* Pmats,
                                       const int32_t* rig_of, const int32_t* members, const double* x, int n_frames, int loss,
                                       double loss_px, double* w, mvmcStream_t stream) {
    if (!skel_host || n_frames < 0 || n_views <= 0 || n_views > MVMC_SMOOTH_MAX_VIEWS || p_max <= 0) return MVMC_ERR_ARG;
    if (!sm_loss_ok(loss, loss_px)) return MVMC_ERR_ARG;
    if (n_frames == 0) return MVMC_OK;
    if (!kps17 || !Pmats || !rig_of || !members || !x || !w) return MVMC_ERR_ARG;
    Ik1Tables T;
    if (!sm_tables(skel_host, &T)) return MVMC_ERR_UNSUPPORTED;
    auto kernel = loss == MVMC_SMOOTH_LOSS_HUBER    ? smooth_obs_weights_kernel<MVMC_SMOOTH_LOSS_HUBER>
                  : loss == MVMC_SMOOTH_LOSS_CAUCHY ? smooth_obs_weights_kernel<MVMC_SMOOTH_LOSS_CAUCHY>
                                                    : smooth_obs_weights_kernel<MVMC_SMOOTH_LOSS_NONE>;
    hipLaunchKernelGGL(kernel, dim3(n_frames), dim3(64), 0, (hipStream_t)stream, T, kps17, Pmats, n_views, p_max, rig_of, members, x,
                       loss_px, w);
    MVMC_CHECK_LAUNCH();
    return MVMC_OK;
}

extern "C" int mvmc_smooth_step(const mvmcSkeleton* skel_host, double* x, double* x_trial, const double* blk, const int32_t* id_lo,
                                int n_ids, int n_frames, double root_vel, double root_acc, double ang_vel, double ang_acc, double mu0,
                                double ftol, double xtol, int max_iter, int phase, int32_t* ctl, double* info, double* work,
                                mvmcStream_t stream) {
    if (!skel_host || n_ids < 0 || n_frames < 0 || phase < 0 || max_iter < 0 || max_iter > MVMC_SMOOTH_INFO_DOUBLES - 8) return MVMC_ERR_ARG;
    if (!(root_vel >= 0.0) || !(root_acc >= 0.0) || !(ang_vel >= 0.0) || !(ang_acc >= 0.0) || !(mu0 > 0.0)) return MVMC_ERR_ARG;
    if (n_ids == 0) return MVMC_OK;
    if (!x || !x_trial || !blk || !id_lo || !ctl || !info || !work) return MVMC_ERR_ARG;
    Ik1Tables T;
    if (!sm_tables(skel_host, &T)) return MVMC_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(smooth_step_kernel, dim3(n_ids), dim3(SM_THREADS), 0, (hipStream_t)stream, T, x, x_trial, blk, id_lo, n_frames,
                       root_vel, root_acc, ang_vel, ang_acc, mu0, ftol, xtol, max_iter, phase, ctl, info, work);
    MVMC_CHECK_LAUNCH();
    return MVMC_OK;
}
