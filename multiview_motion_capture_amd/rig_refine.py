"""Refine each sequence's camera rig from its own tracked people: an offline step between a first track and a re-track.

Every stage of the offline pipeline takes the rig as given.  refine_rigs() repairs a rig that is a little stale (a bumped tripod, a
calibration a day old) by a bundle adjustment over the keypoints of the people the tracker already follows:

  a. selection: sequences.select_views (mvmc_body_observe on the records' joints: per record frame and camera a pose slot or -1), every
     ``frame_step``-th frame of each record;
  b. points: one per (record, frame, keypoint of the 17 ingested) that at least ``min_views`` selected views see with score >
     ``min_score``; start = mvmc_dlt's arithmetic on the input rig (a NaN point is dropped); an observation farther than ``max_px``
     from its point's reprojection is dropped, once; a point left with fewer than ``min_views`` observations is dropped.  The set is
     then fixed;
  c. cameras: camera 0 is held; a camera with fewer than ``min_cam_obs`` observations is held too -- it is not moved at all, not even
     by the gauge rescale, so its observations leave the problem (points are checked against ``min_views`` once more; one pass).
     Fewer than two free cameras or fewer than 3 points: the input rig comes back with ``stop`` saying so;
  d. Levenberg-Marquardt with the body fit's rules on E = 1/2 sum r^2 (plain pixel reprojection, unweighted; by default the two
     gates are the only outlier handling); unknowns: every point, and per free camera a rotation increment (R <- exp([w]x) R) and a
     translation increment.  The points are eliminated by a Schur complement; the reduced camera system is solved by Cholesky.
     ``loss="huber" | "cauchy"`` (opt-in) puts a robust loss behind the two gates: with s the length of an observation's residual
     and delta = ``loss_px``, Huber has rho = 1/2 s^2, w = 1 for s <= delta and rho = delta (s - 1/2 delta), w = delta / s beyond;
     Cauchy has rho = 1/2 delta^2 log1p(s^2 / delta^2), w = 1 / (1 + s^2 / delta^2).  E = sum rho is then the cost of every rule, and
     at every linearisation the observation's Jacobian rows and residual are multiplied by sqrt(w) (iteratively reweighted, no
     second-order correction).  The reweighted iteration converges linearly: it makes more trials, and ``ftol`` around 1e-5 .. 1e-8
     stops it cleanly where the default 1e-12 runs to ``max_iter``;
  e. after every accepted trial the camera centres and points are scaled about camera 0's centre so that the distance from camera 0
     to the first free camera keeps its input length (an exact gauge move).

  f. ``intrinsics="focal" | "focal+centre"`` (opt-in) adds per camera a log-scale phi of the focal length (K[0,0], K[0,1], K[1,1] <-
     e^phi x themselves) and, with "focal+centre", additive dcx, dcy on the principal point, with a Gaussian prior about the input K
     (``focal_sigma`` relative, ``centre_sigma_px`` px; E_prior = 1/2 sum (phi / sigma_f)^2 + 1/2 sum (dcx^2 + dcy^2) / sigma_c^2,
     part of every cost the rules read).  Camera 0's pose stays held, its intrinsics are free; a camera held for too few observations
     keeps its K too; ``intrinsics_held`` names cameras whose K is trusted.  What the geometry allows (measured on rigs that fixate
     one point, tests/test_rig_intr_cpu.py): with the focal lengths alone the only null direction of the reduced matrix at three or
     more cameras is the scale gauge, at two cameras there is one more; with the principal points there are three more at any
     camera count.  So "focal+centre" without a finite ``centre_sigma_px``, and any mode on a two-camera sequence without a finite
     ``focal_sigma``, are refused with ValueError.  The price of a free focal length is its correlation with depth: the camera
     centres come out less sharp along the optical axes than with a known K.

It does not estimate distortion, a free aspect ratio or skew, shares no intrinsics between cameras or sequences, does no time
synchronisation and is no calibration from scratch: the input rig must be good enough for the tracker to produce records.

Device code: csrc/mvmc_rigfit.hip (include/mvmc.h: mvmc_rig_start, mvmc_rig_accumulate, mvmc_rig_step; with a loss
mvmc_rig_accumulate_robust, mvmc_rig_step_robust, mvmc_rig_weights; with intrinsics mvmc_rig_accumulate_intr, mvmc_rig_step_intr);
NumPy restatement: tests/rig_refine_np.py, with a loss tests/rig_robust_np.py, with intrinsics tests/rig_intr_np.py.  Sequences with the same number of cameras share every launch, each with its own rig; there is no host
synchronisation between the trials and one read-back per group.
"""
from __future__ import annotations

import time
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

from . import body_fit
from .body_fit import LM_FTOL, LM_MU0, LM_XTOL
from .common import Calib
from .sequences import SequenceInput, check_records, no_sequences, plan_groups, select_views, stack_group, stopwatch

TILE = 64            # include/mvmc.h: MVMC_RIG_TILE
MAX_CAMS = 8         # MVMC_RIG_MAX_CAMS
MAX_ITER_CAP = 24    # MVMC_RIG_MAX_ITER
STOP = {0: "running", 1: "xtol", 2: "ftol", 3: "few_cameras", 4: "few_points", 5: "max_iter"}   # MVMC_RIG_STOP_*
LOSS = {None: 0, "huber": 1, "cauchy": 2}    # MVMC_RIG_LOSS_*
LOSS_PX = 6.0        # three times a 2 px detector noise; a choice, not a tuned optimum
INTRINSICS = {None: 0, "focal": 1, "focal+centre": 3}    # unknowns per camera: n_intr of mvmc_rig_accumulate_intr


@dataclass
class RigRefinement:
    calibs: list                 # NEW [Calib] * C: K and img_wh_size kept, Rt / P / Kr_inv new
    rms_before: float            # px, over the observations of the problem (NaN without any)
    rms_after: float
    n_points: int
    n_obs: int
    obs_per_camera: np.ndarray   # (C,)
    held: np.ndarray             # (C,) bool: cameras not moved
    cost: np.ndarray             # E at the start and after every trial
    trials: list                 # 1 accepted / 0 rejected
    stop: str                    # "ftol", "xtol", "max_iter", "few_cameras", "few_points"
    moved: np.ndarray            # (C, 2): rotation angle (rad) and centre displacement (m)
    # filled only with a loss.  cost then holds the robust E = sum rho; rms_before and rms_after stay the PLAIN rms over the problem's
    # observations, comparable with a call without a loss
    loss: Optional[str] = None
    loss_px: Optional[float] = None
    downweighted: Optional[np.ndarray] = None   # (C,) share of the camera's observations with final w < 0.5 (NaN without any)
    weights: Optional[np.ndarray] = None        # (N, C) final w, NaN where not observed; only with return_weights=True
    # filled only with intrinsics.  calibs then carry K_after; cost includes the prior; rms_before / rms_after stay the plain rms
    intrinsics: Optional[str] = None
    K_before: Optional[np.ndarray] = None       # (C,3,3)
    K_after: Optional[np.ndarray] = None        # (C,3,3)
    k_moved: Optional[np.ndarray] = None        # (C,3): phi, dcx, dcy; zeros where the camera's K was held
    cost_prior: Optional[float] = None          # E_prior at K_after


def check_loss(who, loss, loss_px, ftol, xtol):
    """The checks of the robust-loss arguments, before any device work: ValueError."""
    if loss not in LOSS:
        raise ValueError(f'{who}: loss is None, "huber" or "cauchy"')
    if loss is not None and not (np.isfinite(float(loss_px)) and float(loss_px) > 0.0):
        raise ValueError(f"{who}: loss_px must be a finite number > 0")
    for name, v in (("ftol", ftol), ("xtol", xtol)):
        if v is not None and not (np.isfinite(float(v)) and float(v) >= 0.0):
            raise ValueError(f"{who}: {name} must be None or a finite number >= 0")


def check_intrinsics(who, intrinsics, focal_sigma, centre_sigma_px, intrinsics_held=(), n_cams=()):
    """The checks of the intrinsics arguments, before any device work: ValueError, or (n_intr, sigma_f, sigma_c) with +inf for no
    term.  n_cams: the camera counts of the sequences the two-camera refusal and intrinsics_held are checked against.  Both refusals
    come from null spaces of the reduced matrix (module docstring, f)."""
    if intrinsics not in INTRINSICS:
        raise ValueError(f'{who}: intrinsics is None, "focal" or "focal+centre"')
    sig = []
    for name, v in (("focal_sigma", focal_sigma), ("centre_sigma_px", centre_sigma_px)):
        sig.append(np.inf if v is None else float(v))
        if not sig[-1] > 0.0:
            raise ValueError(f"{who}: {name} must be None or a number > 0")
    held = [int(c) for c in intrinsics_held]
    if intrinsics is None:
        return 0, sig[0], sig[1]
    if intrinsics == "focal+centre" and not np.isfinite(sig[1]):
        raise ValueError(f'{who}: intrinsics="focal+centre" needs a finite centre_sigma_px (the principal points are not observable '
                         f"from the reprojections alone)")
    for C in n_cams:
        if C == 2 and not np.isfinite(sig[0]):
            raise ValueError(f"{who}: intrinsics on a two-camera sequence need a finite focal_sigma (two focal lengths are not "
                             f"observable from the reprojections alone)")
        if any(not 0 <= c < C for c in held):
            raise ValueError(f"{who}: intrinsics_held names a camera outside 0 .. {C - 1}")
    return INTRINSICS[intrinsics], sig[0], sig[1]


def intrinsic_slots(held, n_intr, intrinsics_held=()):
    """held (S,C) bool -> islot (S,C) i32: the camera's position among the sequence's cameras with free intrinsics, or -1.  Camera 0's
    are free; a camera held for too few observations (it left the problem) and the cameras of intrinsics_held keep their K."""
    free = np.full(held.shape, n_intr > 0)
    free[:, 1:] &= ~held[:, 1:]
    free[:, [int(c) for c in intrinsics_held]] = False
    return np.where(free, np.cumsum(free, axis=1) - 1, -1).astype(np.int32)


def check_refine(sequences, tracklets_per_sequence, max_iter, max_px, min_score, min_views, min_cam_obs, frame_step, loss=None,
                 loss_px=LOSS_PX, ftol=None, xtol=None, intrinsics=None, focal_sigma=None, centre_sigma_px=None, intrinsics_held=()):
    """The input checks of refine_rigs, before any device work: ValueError, or (shapes, per sequence the records' (frames, params,
    joints) arrays)."""
    check_loss("refine_rigs", loss, loss_px, ftol, xtol)
    check_intrinsics("refine_rigs", intrinsics, focal_sigma, centre_sigma_px)

    def own():
        if int(min_views) < 2:
            raise ValueError("refine_rigs: min_views >= 2 required (a point needs two views)")
        if int(frame_step) < 1:
            raise ValueError("refine_rigs: frame_step >= 1 required")
        if not 0 <= int(max_iter) <= MAX_ITER_CAP:
            raise ValueError(f"refine_rigs: 0 <= max_iter <= {MAX_ITER_CAP} required")
        if not (float(max_px) > 0.0 and float(min_score) >= 0.0 and int(min_cam_obs) >= 0):
            raise ValueError("refine_rigs: max_px > 0, min_score >= 0 and min_cam_obs >= 0 required")
    out = check_records(sequences, tracklets_per_sequence, "refine_rigs", own,
                        cameras=(2, MAX_CAMS, f"refine_rigs: sequence {{s}} has {{C}} cameras, 2 .. {MAX_CAMS} required"))
    check_intrinsics("refine_rigs", intrinsics, focal_sigma, centre_sigma_px, intrinsics_held, [len(q[2]) for q in sequences])
    return out


def _per_camera(seq_of, obs, n_seqs):
    """(S, C) observations per sequence and camera."""
    return np.stack([np.bincount(seq_of[obs[:, c]], minlength=n_seqs) for c in range(obs.shape[1])], axis=1)


def pack_problems(valid, dist, x_ok, seq_of, n_seqs, max_px, min_views, min_cam_obs):
    """Steps b - c on the candidates of a group.  valid (n,C) bool: the camera sees the candidate; dist (n,C) px at the start values;
    x_ok (n,) bool: the start value is finite; seq_of (n,) the candidate's sequence (position in the group).
    -> (obs (n,C) bool: the observations of the problem, held (S,C) bool, stop (S,) int: 0 or MVMC_RIG_STOP_FEW_*)."""
    valid = np.asarray(valid, bool)
    n, C = valid.shape
    with np.errstate(invalid="ignore"):
        obs = valid & (np.asarray(dist) <= max_px) & np.asarray(x_ok, bool)[:, None]
    obs &= (obs.sum(axis=1) >= min_views)[:, None]
    seq_of = np.asarray(seq_of, np.int64)
    held = _per_camera(seq_of, obs, n_seqs) < min_cam_obs
    held[:, 0] = True
    drop = held.copy()
    drop[:, 0] = False                       # camera 0 stays in the problem: it is the anchor
    obs &= ~drop[seq_of]
    obs &= (obs.sum(axis=1) >= min_views)[:, None]
    n_pts = np.bincount(seq_of[obs.any(axis=1)], minlength=n_seqs)
    stop = np.where((~held).sum(axis=1) < 2, 3, np.where(n_pts < 3, 4, 0)).astype(np.int32)
    return obs, held, stop


def tile_tables(n_points):
    """n_points (S,) points per sequence, stored sequence by sequence -> tile (T,4) i32 (sequence, first point, points, 0) and seq (S,4)
    i32 (first tile, tiles, first point, points): tiles of TILE points cut from each sequence's own points."""
    n_points = np.asarray(n_points, np.int64)
    p_lo = np.concatenate([[0], np.cumsum(n_points)])
    n_t = (n_points + TILE - 1) // TILE
    t_lo = np.concatenate([[0], np.cumsum(n_t)])
    tile = np.zeros((int(t_lo[-1]), 4), np.int32)
    for s in range(n_points.shape[0]):
        k = np.arange(n_t[s])
        tile[t_lo[s]:t_lo[s + 1], 0] = s
        tile[t_lo[s]:t_lo[s + 1], 1] = p_lo[s] + k * TILE
        tile[t_lo[s]:t_lo[s + 1], 2] = np.minimum(TILE, n_points[s] - k * TILE)
    seq = np.stack([t_lo[:-1], n_t, p_lo[:-1], n_points], axis=1).astype(np.int32)
    return tile, seq


def _moved(Rt_in, Rt_out):
    out = np.zeros((Rt_in.shape[0], 2))
    for c in range(Rt_in.shape[0]):
        D = Rt_out[c, :, :3] @ Rt_in[c, :, :3].T
        w = 0.5 * np.array([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
        out[c, 0] = np.arctan2(np.linalg.norm(w), (np.trace(D) - 1.0) / 2.0)     # (arccos of the trace alone loses half the digits near 0)
        out[c, 1] = np.linalg.norm(Rt_out[c, :, :3].T @ Rt_out[c, :, 3] - Rt_in[c, :, :3].T @ Rt_in[c, :, 3])
    return out


@dataclass
class GroupSolve:
    """solve_group's result for a group of S sequences: the host gates' arrays over the n candidates, the one read-back, and the
    device's start values and final points."""
    dist: np.ndarray             # (n, C) px at the start values, NaN where the camera does not see the candidate
    seq_of: np.ndarray           # (n,) the candidate's sequence
    obs: np.ndarray              # (n, C) bool: the observations of the problem
    held: np.ndarray             # (S, C) bool
    is_pt: np.ndarray            # (n,) bool: the candidate became a point
    n_pts: np.ndarray            # (S,)
    n_obs: np.ndarray            # (S, C)
    run: np.ndarray              # (S,) bool: the sequence was solved (the others stopped with few_cameras / few_points)
    cams_h: np.ndarray           # (S, C, 21): K, R, t after the trials
    info_h: np.ndarray           # (S, MVMC_RIG_INFO_DOUBLES)
    ctl_h: np.ndarray            # (S, 4)
    X0_d: object                 # (n, 4) device: the start values (None without candidates)
    X_d: object                  # device: the final points of dev_pt's candidates
    dev_pt: np.ndarray           # (n,) bool: is_pt of the solved sequences
    e_plain: Optional[np.ndarray] = None    # with a loss (S, 2): the plain 1/2 sum r^2 before and after
    w_h: Optional[np.ndarray] = None        # with a loss (points of dev_pt, C): the final weights
    islot: Optional[np.ndarray] = None      # with intrinsics (S, C): the camera's intrinsic block or -1
    K0: Optional[np.ndarray] = None         # with intrinsics (S, C, 3, 3): the input K
    sigma: tuple = (np.inf, np.inf)         # with intrinsics: the prior's focal_sigma, centre_sigma_px (+inf: no term)

    _host: Optional[tuple] = None           # points(): X_d and X0_d read back once, and each sequence's first row of X_d

    def points(self, r):
        """Sequence r's points (its candidates that are is_pt, in order; candidates are stored sequence by sequence): the final ones
        where it was solved, else the start values."""
        if self._host is None:
            x_lo = np.concatenate([[0], np.cumsum(np.bincount(self.seq_of[self.dev_pt], minlength=self.run.shape[0]))])
            self._host = (self.X_d.cpu().numpy(), self.X0_d.cpu().numpy()[:, :3] if self.X0_d is not None else np.zeros((0, 3)), x_lo)
        X, X0, x_lo = self._host
        return X[x_lo[r]:x_lo[r + 1]] if self.run[r] else X0[(self.seq_of == r) & self.is_pt]


def solve_group(obs_d, rig_c, Pm_d, Kin, Rtin, S, C, d, max_iter, max_px, min_score, min_views, min_cam_obs, variant, lap, loss=None,
                loss_px=LOSS_PX, ftol=None, xtol=None, intrinsics=None, focal_sigma=None, centre_sigma_px=None,
                intrinsics_held=()) -> GroupSolve:
    """Steps b - e on the candidates of a group of S sequences of C cameras: what refine_rigs does after its selection, and what
    rig_init.calibrate_rigs polishes with.  obs_d (n,C,3) f64 device: u, v, score per candidate and camera (None: no candidate);
    rig_c (n,) i32 device: the candidate's sequence; Pm_d (S,C,3,4) device; Kin (S,C,3,3), Rtin (S,C,3,4) host; lap: the caller's
    stopwatch (sequences.stopwatch), which gets "start" and "trials".  intrinsics: None runs the entries without intrinsic unknowns;
    "focal" / "focal+centre" the _intr entries (the problem is still packed on the input K)."""
    import torch

    from . import _cabi
    from . import device as dev
    T = dev.uploader(d)
    n_cand = 0 if obs_d is None else int(obs_d.shape[0])
    X0_d = None
    if n_cand:
        # the points and distances stay on the device; the host gates on the distances alone
        X0_d, dist_d = dev.rig_start(obs_d, rig_c, Pm_d, float(min_score))
        dist, seq_of = dist_d.cpu().numpy(), rig_c.cpu().numpy().astype(np.int64)
        x_ok = torch.isfinite(X0_d[:, :3]).all(dim=1).cpu().numpy()
    else:
        dist, seq_of, x_ok = np.zeros((0, C)), np.zeros((0,), np.int64), np.zeros((0,), bool)
    obs, held, stop0 = pack_problems(~np.isnan(dist), dist, x_ok, seq_of, S, float(max_px), int(min_views), int(min_cam_obs))
    is_pt = obs.any(axis=1)
    n_pts = np.bincount(seq_of[is_pt], minlength=S)
    n_obs = _per_camera(seq_of, obs, S)
    run = stop0 == 0
    dev_pt = is_pt & run[seq_of]                                            # points of the sequences that are solved
    tile, seq = tile_tables(np.where(run, n_pts, 0))
    slot = np.where(held, -1, np.cumsum(~held, axis=1) - 1).astype(np.int32)
    cams = np.concatenate([Kin.reshape(S, C, 9), Rtin[:, :, :, :3].reshape(S, C, 9), Rtin[:, :, :, 3]], axis=2)
    info = np.zeros((S, _cabi.RIG_INFO_DOUBLES))
    info[:, 8:8 + MAX_ITER_CAP] = -1.0
    ctl = np.zeros((S, 4), np.int32)
    ctl[:, 0] = stop0
    if n_cand:
        pt_d = T(dev_pt)
        X_d = X0_d[pt_d][:, :3].contiguous()
        uv_d = torch.where(T(obs[dev_pt])[:, :, None], obs_d[pt_d][:, :, :2], torch.full((), float("nan"), dtype=torch.float64, device=d))
        uv_d = uv_d.contiguous()
    else:
        X_d, uv_d = torch.zeros((0, 3), dtype=torch.float64, device=d), torch.zeros((0, C, 2), dtype=torch.float64, device=d)
    lap("start")
    Xt_d = X_d.clone()
    tile_d, seq_d, slot_d, cams_d, info_d, ctl_d = T(tile), T(seq), T(slot), T(cams), T(info), T(ctl)
    camt_d = cams_d.clone()
    n_intr, sig_f, sig_c = check_intrinsics("solve_group", intrinsics, focal_sigma, centre_sigma_px)
    part, part2, red = dev.rig_work(tile.shape[0], S, C, d)
    if n_intr:
        # the plain cost below keeps the work buffers of the entries without intrinsics; the trials get their own
        islot = intrinsic_slots(held, n_intr, intrinsics_held)
        islot_d, K0_d = T(islot), T(np.ascontiguousarray(Kin[:, :, [0, 0, 1], [0, 2, 2]]))
        part_i, _, red_i = dev.rig_work_intr(tile.shape[0], S, C, n_intr, d)
    ftol, xtol = LM_FTOL if ftol is None else float(ftol), LM_XTOL if xtol is None else float(xtol)
    code, px = LOSS[loss], 0.0 if loss is None else float(loss_px)      # MVMC_RIG_LOSS_NONE: the kernels of the entries without a loss
    extra = []

    def plain_cost():
        # 1/2 sum r^2 at (X, cams): an accumulate without a loss and without a trial on a control block of its own
        ctl2, info2 = T(ctl), T(info)
        dev.rig_accumulate(X_d, uv_d, tile_d, seq_d, slot_d, cams_d, camt_d.clone(), ctl2, info2, 0, LM_MU0, part, torch.zeros_like(red),
                           variant)
        return info2[:, 0]

    def accumulate():
        if n_intr:
            dev.rig_accumulate_intr(X_d, uv_d, tile_d, seq_d, slot_d, cams_d, camt_d, ctl_d, info_d, max_iter, LM_MU0, part_i, red_i, n_intr,
                                    islot_d, K0_d, sig_f, sig_c, variant, code, px)
        else:
            dev.rig_accumulate_robust(X_d, uv_d, tile_d, seq_d, slot_d, cams_d, camt_d, ctl_d, info_d, max_iter, LM_MU0, part, red, variant,
                                      code, px)

    def step():
        if n_intr:
            dev.rig_step_intr(X_d, Xt_d, uv_d, tile_d, seq_d, slot_d, cams_d, camt_d, ctl_d, info_d, red_i, max_iter, ftol, xtol, part2,
                              n_intr, islot_d, K0_d, sig_f, sig_c, code, px)
        else:
            dev.rig_step_robust(X_d, Xt_d, uv_d, tile_d, seq_d, slot_d, cams_d, camt_d, ctl_d, info_d, red, max_iter, ftol, xtol, part2,
                                code, px)

    if run.any():
        if code or n_intr:
            extra.append(plain_cost())
        for _ in range(max(int(max_iter), 1)):
            accumulate()
            if int(max_iter):
                step()
        if code or n_intr:
            extra += [plain_cost(), dev.rig_weights(X_d, uv_d, tile_d, cams_d, code, px).reshape(-1)]
    lap("trials")
    back = torch.cat([cams_d.reshape(-1), info_d.reshape(-1), ctl_d.reshape(-1).double()] + extra).cpu().numpy()   # the one read-back
    cams_h = back[:S * C * 21].reshape(S, C, 21)
    info_h = back[S * C * 21:S * C * 21 + info.size].reshape(S, -1)
    n_fix = S * C * 21 + info.size + 4 * S
    ctl_h = back[S * C * 21 + info.size:n_fix].reshape(S, 4).astype(np.int64)
    g = GroupSolve(dist, seq_of, obs, held, is_pt, n_pts, n_obs, run, cams_h, info_h, ctl_h, X0_d, X_d, dev_pt)
    if extra:
        g.e_plain, g.w_h = back[n_fix:n_fix + 2 * S].reshape(2, S).T, back[n_fix + 2 * S:].reshape(-1, C)
    if n_intr:
        g.islot, g.K0, g.sigma = islot, np.array(Kin, np.float64), (sig_f, sig_c)
    return g


def _intrinsic_record(g: GroupSolve, r: int, intrinsics):
    """The intrinsics' fields of sequence r: K_before, K_after, k_moved and cost_prior from the one read-back."""
    K0, K1 = g.K0[r], g.cams_h[r, :, :9].reshape(-1, 3, 3).copy()
    free, full = g.islot[r] >= 0, INTRINSICS[intrinsics] == 3
    dk = np.stack([np.log(K1[:, 0, 0] / K0[:, 0, 0]), K1[:, 0, 2] - K0[:, 0, 2], K1[:, 1, 2] - K0[:, 1, 2]], axis=1)
    dk = np.where(free[:, None], dk, 0.0) * np.array([1.0, full, full])
    e = 0.5 * float(np.sum((dk[:, 0] / g.sigma[0]) ** 2) + np.sum((dk[:, 1:] / g.sigma[1]) ** 2))
    return dict(intrinsics=intrinsics, K_before=K0.copy(), K_after=K1, k_moved=dk, cost_prior=e)


def decode(g: GroupSolve, r: int, cameras, Rtin, loss=None, loss_px=LOSS_PX, return_weights=False, intrinsics=None) -> RigRefinement:
    """Sequence r of a solved group as its RigRefinement.  cameras: per view (K, (w, h)); Rtin (C,3,4): the rig it started from."""
    C = g.held.shape[1]
    Rt_new = np.concatenate([g.cams_h[r, :, 9:18].reshape(C, 3, 3), g.cams_h[r, :, 18:21, None]], axis=2)
    n_o = int(g.n_obs[r].sum())
    if g.run[r]:
        n_t = int(g.ctl_h[r, 1])
        cost = g.info_h[r, 8 + MAX_ITER_CAP:8 + MAX_ITER_CAP + n_t + 1].copy()
        trials = [int(v) for v in g.info_h[r, 8:8 + n_t]]
        rb, ra = float(np.sqrt(2.0 * g.info_h[r, 0] / n_o)), float(np.sqrt(2.0 * g.info_h[r, 1] / n_o))
    else:
        dd = g.dist[(g.seq_of == r)[:, None] & g.obs]
        e0 = 0.5 * float(np.sum(dd * dd))
        cost, trials = (np.array([e0]) if n_o else np.zeros(0)), []
        rb = ra = float(np.sqrt(2.0 * e0 / n_o)) if n_o else float("nan")
    rob = {}
    if loss is not None:      # downweighted, weights, and for a solved sequence the PLAIN rms in place of the robust cost's
        rob = dict(loss=loss, loss_px=float(loss_px), downweighted=np.full(C, np.nan), weights=None)
        if g.run[r] and g.w_h is not None:
            lo = int(np.where(g.run, g.n_pts, 0)[:r].sum())
            w = g.w_h[lo:lo + int(g.n_pts[r])]
            with np.errstate(invalid="ignore", divide="ignore"):
                rob["downweighted"] = (w < 0.5).sum(axis=0) / (~np.isnan(w)).sum(axis=0)
            if return_weights:
                rob["weights"] = w.copy()
            rb, ra = (float(np.sqrt(2.0 * e / n_o)) for e in g.e_plain[r])
    Ks = [np.array(K, np.float64) for K, _ in cameras]
    if intrinsics is not None:
        rob.update(_intrinsic_record(g, r, intrinsics))
        Ks = [K.copy() for K in rob["K_after"]]
        if g.run[r] and g.e_plain is not None:           # the PLAIN rms in place of the cost's, which includes the prior
            rb, ra = (float(np.sqrt(2.0 * e / n_o)) for e in g.e_plain[r])
    calibs = [Calib.from_k_rt(Ks[k], Rt_new[k].copy(), wh) for k, (_, wh) in enumerate(cameras)]
    return RigRefinement(calibs=calibs, rms_before=rb, rms_after=ra, n_points=int(g.n_pts[r]), n_obs=n_o, obs_per_camera=g.n_obs[r].copy(),
                         held=g.held[r].copy(), cost=cost, trials=trials, stop=STOP[int(g.ctl_h[r, 0])], moved=_moved(Rtin, Rt_new), **rob)


def refine_rigs(sequences: Sequence[SequenceInput], tracklets_per_sequence: Sequence[list], max_iter: int = 10,
                max_px: float = body_fit.MAX_DIST, min_score: float = body_fit.MIN_SCORE, min_views: int = 2, min_cam_obs: int = 100,
                frame_step: int = 1, device="cuda:0", timings: Optional[dict] = None, variant: int = 1,
                problems: Optional[list] = None, loss: Optional[str] = None, loss_px: float = LOSS_PX, ftol: Optional[float] = None,
                xtol: Optional[float] = None, return_weights: bool = False, intrinsics: Optional[str] = None,
                focal_sigma: Optional[float] = None, centre_sigma_px: Optional[float] = None,
                intrinsics_held: Sequence[int] = ()) -> List[RigRefinement]:
    """Refine the rig of every sequence -- (kps (F_s,C,P_s,25|17,3), counts (F_s,C), one Calib per camera), the rows track_sequences
    takes -- from its MvTracklet records.  -> one RigRefinement per sequence; the inputs are not touched.
    timings: a dict that receives the seconds spent in {"select", "start", "trials", "records"} (synchronising between the parts).
    variant: 1 the tile products on the matrix cores, 0 as FMAs.  problems: a list that receives, per sequence, the packed problem
    (dict X0 (N,3), uv (N,C,2), cand (n,C,3), rows (N,): the candidates that became points) -- what the tests compare.
    loss: None (the plain least squares, the code path without these arguments), "huber" or "cauchy" at loss_px pixels, behind the
    two max_px gates; the records then carry loss, loss_px, downweighted and (return_weights=True) weights, their cost is the robust
    E, and rms_before / rms_after stay the plain rms.  ftol, xtol: the stop tolerances, None = the body fit's constants.
    intrinsics: None (K is taken as given, the code path without these arguments), "focal" (one log-scale per camera) or
    "focal+centre" (and the principal point), with a Gaussian prior about the input K of focal_sigma (relative) and centre_sigma_px
    (px), None = no term; intrinsics_held: cameras whose K is kept.  "focal+centre" without a finite centre_sigma_px, and intrinsics
    on a two-camera sequence without a finite focal_sigma, raise ValueError: those unknowns are not observable (module docstring, f).
    The records then carry intrinsics, K_before, K_after, k_moved and cost_prior, their calibs carry K_after, and cost includes the
    prior."""
    if no_sequences(sequences, tracklets_per_sequence, "refine_rigs"):
        return []
    shapes, recs = check_refine(sequences, tracklets_per_sequence, max_iter, max_px, min_score, min_views, min_cam_obs, frame_step, loss,
                                loss_px, ftol, xtol, intrinsics, focal_sigma, centre_sigma_px, intrinsics_held)
    import torch

    from . import device as dev
    d = torch.device(device)
    T = dev.uploader(d)
    lap, tm = stopwatch(timings, d, ("select", "start", "trials", "records"))
    out: List[Optional[RigRefinement]] = [None] * len(sequences)
    if problems is not None:
        problems[:] = [None] * len(sequences)
    for lay in plan_groups(shapes, 1):
        t0 = time.perf_counter()
        ids, S, C = lay.seq_ids, len(lay.seq_ids), lay.n_views
        grp = stack_group(lay, sequences)
        Kin = np.array([[np.asarray(c.K, np.float64).reshape(3, 3) for c in sequences[i][2]] for i in ids])
        Rtin = np.array([[np.asarray(c.Rt, np.float64).reshape(3, 4) for c in sequences[i][2]] for i in ids])
        obs_d = rig_c = Pm_d = None
        if any(recs[i] for i in ids):
            sel = select_views(grp, recs, d, float(max_px), float(min_score))
            n_of, k17, Pm_d = sel.n_of, sel.k17, sel.Pm_d
            take = np.concatenate([np.arange(0, n, int(frame_step)) + o for n, o in zip(n_of, sel.rec_lo[:-1])])
            mem = sel.members[T(take)].long()                                # (B, C)
            o17 = k17.reshape(-1, 17, 3)[mem.clamp(min=0)]                     # (B, C, 17, 3)
            o17[..., 2] = torch.where((mem >= 0)[:, :, None], o17[..., 2], torch.zeros((), dtype=o17.dtype, device=d))
            obs_all = o17.permute(0, 2, 1, 3).reshape(-1, C, 3)
            is_cand = ((obs_all[:, :, 2] > float(min_score)).sum(dim=1) >= int(min_views))
            obs_d = obs_all[is_cand].contiguous()
            rig_c = T(np.repeat(sel.rig_of[take], 17))[is_cand].contiguous()
            if not int(obs_d.shape[0]):
                obs_d = rig_c = Pm_d = None
        lap("select", t0)
        g = solve_group(obs_d, rig_c, Pm_d, Kin, Rtin, S, C, d, max_iter, max_px, min_score, min_views, min_cam_obs, variant, lap, loss,
                        loss_px, ftol, xtol, intrinsics, focal_sigma, centre_sigma_px, intrinsics_held)
        if problems is not None and obs_d is not None:
            cand, X0 = obs_d.cpu().numpy(), g.X0_d.cpu().numpy()
        for r, i in enumerate(ids):
            out[i] = decode(g, r, [(c.K, c.img_wh_size) for c in sequences[i][2]], Rtin[r], loss, loss_px, return_weights, intrinsics)
            if problems is not None and obs_d is not None:
                m = g.seq_of == r
                pr = g.is_pt[m]
                problems[i] = dict(cand=cand[m], rows=np.flatnonzero(pr), X0=X0[m][pr][:, :3],
                                   uv=np.where(g.obs[m][pr][:, :, None], cand[m][pr][:, :, :2], np.nan))
        lap("records")
    if timings is not None:
        timings.update(tm)
    return out


def refine_rig(tracklets: list, kps: np.ndarray, counts: np.ndarray, calibs: list, max_iter: int = 10, max_px: float = body_fit.MAX_DIST,
               min_score: float = body_fit.MIN_SCORE, min_views: int = 2, min_cam_obs: int = 100, frame_step: int = 1, device="cuda:0",
               timings: Optional[dict] = None, loss: Optional[str] = None, loss_px: float = LOSS_PX, ftol: Optional[float] = None,
               xtol: Optional[float] = None, return_weights: bool = False, intrinsics: Optional[str] = None,
               focal_sigma: Optional[float] = None, centre_sigma_px: Optional[float] = None,
               intrinsics_held: Sequence[int] = ()) -> RigRefinement:
    """refine_rigs for one sequence: records of kps (F,C,P,25|17,3), counts (F,C) and one Calib per camera -> RigRefinement."""
    return refine_rigs([(kps, counts, calibs)], [tracklets], max_iter=max_iter, max_px=max_px, min_score=min_score, min_views=min_views,
                       min_cam_obs=min_cam_obs, frame_step=frame_step, device=device, timings=timings, loss=loss, loss_px=loss_px,
                       ftol=ftol, xtol=xtol, return_weights=return_weights, intrinsics=intrinsics, focal_sigma=focal_sigma,
                       centre_sigma_px=centre_sigma_px, intrinsics_held=intrinsics_held)[0]
