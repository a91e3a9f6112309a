"""One skeleton per tracked person: an offline refinement of finished tracklet records.

The tracker's IK (PoseSolver.solve, inverse_kinematics.py:380-433) fits the 11 side bone lengths again on every frame, so a person's
limbs change length from frame to frame.  fit_sequences() gives every identity ONE side-length vector, shared by all of its frames, and
re-solves every frame's pose against it:

  a. selection (once): per (frame of the record, camera) the pose nearest to the record's joints -- the tracker's 2D-3D distance
     (reprojection_error, motion_capture.py:403-414, min score 0.1), below the affinity floor of its graph (15 + 30 ln(999) / 5 px);
     two records of one frame claiming one pose: the smaller distance keeps it (equal: the earlier record), the other takes nothing in
     that camera.  A frame left with fewer than 2 views is FROZEN: its angles are kept, it gets the identity's final lengths and its
     joints by FK, and it takes no part in b and c;
  b. l0 = per-slot median of the per-frame lengths (over the non-frozen frames; over all when every one is frozen);
  c. ``rounds`` rounds of
       length step: Levenberg-Marquardt on the lengths with every pose fixed (one workgroup per identity, one launch);
       pose step:   stage 1 of PoseSolver (solve_pose_reproj: root + angles), warm from the current pose, max_nfev evaluations.
     Both minimise the same E = 1/2 sum r^2 (the IK's residual over the identity's frames and selected views), so E does not increase.

Device code: csrc/mvmc_bodyfit.hip (include/mvmc.h: mvmc_body_observe, mvmc_body_lengths, mvmc_ik_solve_stages_rigs); NumPy
restatement: tests/body_fit_np.py.  Sequences with the same number of cameras share every launch (one per step), each with its own rig.
The input checks, the group stacking, step a and the record shells are sequences.py's (check_records, stack_group, select_views,
pose_tuples / new_record), shared with smoothing and rig_refine.
"""
from __future__ import annotations

import math
import time
from typing import List, Optional, Sequence

import numpy as np

from .sequences import (SequenceInput, check_records, new_record, no_sequences, plan_groups, pose_slot, pose_tuples, select_views,
                        stack_group, stopwatch)

MIN_SCORE = 0.1
MAX_DIST = 15.0 + 30.0 * math.log(999.0) / 5.0   # S = 1 / (1 + exp(5 (D - 15) / 30)) < 1e-3 is cut to 0 (mvmc_st_affinity)
LM_MU0 = 1e-3       # Marquardt's damping: (H + mu diag(H)) d = -g, mu dimensionless
LM_FTOL = 1e-12     # stop: predicted or achieved reduction below LM_FTOL E
LM_XTOL = 1e-10     # stop: |d|_inf below LM_XTOL m
MAX_ITER_CAP = 12   # include/mvmc.h: MVMC_BODY_INFO_DOUBLES - 4


def _check(sequences, tracklets_per_sequence, rounds, max_iter, max_nfev):
    def own():
        if int(rounds) < 0 or not 0 <= int(max_iter) <= MAX_ITER_CAP or int(max_nfev) < 1:
            raise ValueError(f"fit_sequences: rounds >= 0, 0 <= max_iter <= {MAX_ITER_CAP} and max_nfev >= 1 required")
    return check_records(sequences, tracklets_per_sequence, "fit_sequences", own)


def fit_sequences(sequences: Sequence[SequenceInput], tracklets_per_sequence: Sequence[list], rounds: int = 3, max_iter: int = 10,
                  max_nfev: int = 5, device="cuda:0", timings: Optional[dict] = None) -> List[list]:
    """Fit one skeleton per identity of every sequence -- (kps (F_s,C,P_s,25|17,3), counts (F_s,C), one Calib per camera), the rows
    track_sequences takes -- from its MvTracklet records (track_sequences, run_main_batched, MvTracker.update_4d, LivePool), whose
    frame_idxs index the sequence's kps.  Returns, per sequence, NEW records in the input order (the inputs are not touched): the same
    track_id, frame_idxs, state, hits and time_since_update; every pose's bone_lens is the record's ``bone_lens`` (11,); poses[k][2]
    holds the FK joints; ``fit_views`` (n,) the views used per frame (0: frozen); ``fit_cost`` (1 + 2 rounds,) the identity's E after
    round 0 and after every length and pose step; ``fit_select`` (n, C) the pose slot (ingest order) used per camera or -1;
    ``fit_trials`` per round the length step's trials (1 accepted, 0 rejected).
    Sequences with the same camera count share one launch per step: selection, then per round the length step and the pose step.
    timings: a dict that receives the seconds spent in {"select", "length", "pose", "records"} (synchronising between the parts)."""
    if no_sequences(sequences, tracklets_per_sequence, "fit_sequences"):
        return []
    shapes, recs = _check(sequences, tracklets_per_sequence, rounds, max_iter, max_nfev)
    import torch

    from . import device as dev
    d = torch.device(device)
    T = dev.uploader(d)
    lap, tm = stopwatch(timings, d, ("select", "length", "pose", "records"))
    out: List[list] = [[None] * len(r) for r in recs]
    for lay in plan_groups(shapes, 1):
        if not any(recs[i] for i in lay.seq_ids):
            continue
        t0 = time.perf_counter()
        sel = select_views(stack_group(lay, sequences), recs, d, MAX_DIST, MIN_SCORE, want_params=True)
        items, rec_lo, n_of, params, joints = sel.items, sel.rec_lo, sel.n_of, sel.params, sel.joints
        k17, Pm_d, rig_d, members = sel.k17, sel.Pm_d, sel.rig_d, sel.members
        nv = sel.n_views.cpu().numpy()
        t0 = lap("select", t0)
        live = nv >= 2
        # initial skeleton per identity, and the live problems of the identities that have any, identity by identity
        lens0 = np.empty((len(items), 11))
        for a in range(len(items)):
            sl = slice(rec_lo[a], rec_lo[a + 1])
            lv = live[sl]
            src = params[sl][lv] if lv.any() else params[sl]
            lens0[a] = np.median(src[:, 57:], axis=0)
            lens0[a, 7] = params[rec_lo[a], 57 + 7]
        owner = np.repeat(np.arange(len(items)), n_of)
        lp = np.flatnonzero(live)
        fitted = np.unique(owner[lp])                       # identities with at least one live problem
        id_slot = -np.ones(len(items), np.int64)
        id_slot[fitted] = np.arange(fitted.size)
        lens_fit = lens0.copy()
        costs = np.zeros((len(items), 1 + 2 * int(rounds)))
        trials = [[[] for _ in range(int(rounds))] for _ in items]
        par_live = params[lp].copy()
        jnt_live = None
        if lp.size:
            id_lo = np.concatenate([[0], np.cumsum(np.bincount(id_slot[owner[lp]], minlength=fitted.size))]).astype(np.int32)
            slot_of = torch.from_numpy(id_slot[owner[lp]]).to(d)
            mem_l, rig_l = members[T(lp)].contiguous(), rig_d[T(lp)].contiguous()
            par_d = T(par_live)
            lens_d = T(lens0[fitted])
            free_d = torch.zeros((fitted.size,), dtype=torch.int32, device=d)
            infos, pcosts = [], []
            for rd in range(max(int(rounds), 1)):
                t0 = time.perf_counter()
                infos.append(dev.body_lengths(k17, Pm_d, rig_l, mem_l, par_d, T(id_lo), lens_d, free_d, rd > 0,
                                              max_iter if rounds else 0, LM_MU0, LM_FTOL, LM_XTOL))
                t0 = lap("length", t0)
                if not rounds:
                    break
                init = par_d.clone()
                init[:, 57:] = lens_d[slot_of]
                par_d, jnt_d, info = dev.ik_solve_stages_rigs(init, 1, max_nfev, k17, Pm_d, rig_l, mem_l)
                pcosts.append(info[:, 0])
                lap("pose", t0)
            t0 = time.perf_counter()
            lens_fit[fitted] = lens_d.cpu().numpy()
            infos = [x.cpu().numpy() for x in infos]
            costs[fitted, 0] = infos[0][:, 0]
            for rd in range(int(rounds)):
                costs[fitted, 1 + 2 * rd] = infos[rd][:, 1]
                costs[fitted, 2 + 2 * rd] = np.add.reduceat(pcosts[rd].cpu().numpy(), id_lo[:-1])
                for s, a in enumerate(fitted):
                    n_t = int(infos[rd][s, 2])
                    trials[a][rd] = [int(v) for v in infos[rd][s, 4:4 + n_t]]
            if rounds:
                par_live = par_d.cpu().numpy()
                jnt_live = jnt_d.cpu().numpy()
        else:
            t0 = time.perf_counter()
        # every problem's final pose with its identity's lengths; joints: the pose step's where it ran, FK elsewhere
        params_out = params.copy()
        params_out[lp] = par_live
        params_out[:, 57:] = lens_fit[owner]
        need_fk = np.ones(params.shape[0], dtype=bool)
        joints_out = np.empty_like(joints)
        if jnt_live is not None:
            joints_out[lp] = jnt_live
            need_fk[lp] = False
        fk_rows = np.flatnonzero(need_fk)
        if fk_rows.size:
            joints_out[fk_rows] = dev.fk(T(params_out[fk_rows])).cpu().numpy()
        views_used = np.where(live, nv, 0)
        _records(out, items, recs, tracklets_per_sequence, rec_lo, params_out, joints_out, lens_fit, views_used,
                 pose_slot(members.cpu().numpy(), sel.Pg), costs, trials)
        lap("records", t0)
    if timings is not None:
        timings.update(tm)
    return out


def _records(out, items, recs, tracklets_per_sequence, rec_lo, params, joints, lens, views, sel, costs, trials):
    """New MvTracklet records from the fitted tables (one slice per record; the per-frame objects built from whole arrays)."""
    frames = np.concatenate([recs[i][j][0] for i, j in items])
    poses = pose_tuples(frames, params, joints)
    for a, (i, j) in enumerate(items):
        lo, hi = int(rec_lo[a]), int(rec_lo[a + 1])
        src = tracklets_per_sequence[i][j]
        t = new_record(src.track_id, poses[lo:hi], src)
        t.bone_lens = lens[a].copy()
        t.fit_views = views[lo:hi].astype(np.int32)
        t.fit_cost = costs[a].copy()
        t.fit_select = sel[lo:hi].astype(np.int32)
        t.fit_trials = trials[a]
        out[i][j] = t


def fit_tracklets(tracklets: list, kps: np.ndarray, counts: np.ndarray, calibs: list, rounds: int = 3, max_iter: int = 10,
                  max_nfev: int = 5, device="cuda:0", timings: Optional[dict] = None) -> list:
    """fit_sequences for one sequence: records of kps (F,C,P,25|17,3), counts (F,C) and one Calib per camera -> new records."""
    return fit_sequences([(kps, counts, calibs)], [tracklets], rounds=rounds, max_iter=max_iter, max_nfev=max_nfev, device=device,
                         timings=timings)[0]
