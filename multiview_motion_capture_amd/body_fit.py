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
"""
from __future__ import annotations

import math
import time
from typing import List, Optional, Sequence

import numpy as np

from .sequences import SequenceInput, check_sequences

MIN_SCORE = 0.1
MAX_DIST = 15.0 + 30.0 * math.log(999.0) / 5.0   # S = 1 / (1 + exp(5 (D - 15) / 30)) < 1e-3 is cut to 0 (mvmc_st_affinity)
LM_MU0 = 1e-3       # Marquardt's damping: (H + mu diag(H)) d = -g, mu dimensionless
LM_FTOL = 1e-12     # stop: predicted or achieved reduction below LM_FTOL E
LM_XTOL = 1e-10     # stop: |d|_inf below LM_XTOL m
MAX_ITER_CAP = 12   # include/mvmc.h: MVMC_BODY_INFO_DOUBLES - 4


def _record_arrays(rec, F: int, where: str):
    """(frames (n,), params (n,68), joints (n,18,3)) of one MvTracklet record; ValueError where it does not fit."""
    frames = np.asarray(rec.frame_idxs, dtype=np.int64)
    poses = rec.poses
    n = frames.shape[0]
    if n == 0 or len(poses) != n:
        raise ValueError(f"{where}: {n} frame indices and {len(poses)} poses")
    if frames.min() < 0 or frames.max() >= F:
        raise ValueError(f"{where}: frame {int(frames.max() if frames.max() >= F else frames.min())} outside the {F} frames of kps")
    if np.unique(frames).shape[0] != n:
        raise ValueError(f"{where}: a frame appears twice")
    try:
        root = np.array([np.asarray(p[1].root, np.float64).reshape(3) for p in poses])
        ang = np.array([np.asarray(p[1].euler_angles, np.float64).reshape(54) for p in poses])
        lens = np.array([np.asarray(p[1].bone_lens, np.float64).reshape(11) for p in poses])
        joints = np.array([np.asarray(p[2].keypoints, np.float64).reshape(18, 3) for p in poses])
    except (ValueError, AttributeError, TypeError) as e:
        raise ValueError(f"{where}: poses must be (frame, PoseShapeParam (3 + 18x3 + 11), BASIC_18 Pose): {e}") from None
    return frames, np.concatenate([root, ang, lens], axis=1), joints


def _check(sequences, tracklets_per_sequence, rounds, max_iter, max_nfev):
    if len(tracklets_per_sequence) != len(sequences):
        raise ValueError(f"fit_sequences: {len(tracklets_per_sequence)} record lists for {len(sequences)} sequences")
    if int(rounds) < 0 or not 0 <= int(max_iter) <= MAX_ITER_CAP or int(max_nfev) < 1:
        raise ValueError(f"fit_sequences: rounds >= 0, 0 <= max_iter <= {MAX_ITER_CAP} and max_nfev >= 1 required")
    shapes = check_sequences(sequences, "fit_sequences")
    recs = []
    for s, (tl, (F, _, _)) in enumerate(zip(tracklets_per_sequence, shapes)):
        recs.append([_record_arrays(t, F, f"sequence {s}, record {j}") for j, t in enumerate(tl)])
    return shapes, recs


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
    if len(sequences) == 0:
        if len(tracklets_per_sequence):
            raise ValueError("fit_sequences: records without sequences")
        return []
    shapes, recs = _check(sequences, tracklets_per_sequence, rounds, max_iter, max_nfev)
    import torch

    from . import device as dev
    d = torch.device(device)
    tm = {"select": 0.0, "length": 0.0, "pose": 0.0, "records": 0.0}

    def lap(k, t0):
        if timings is not None:
            torch.cuda.synchronize(d)
        t1 = time.perf_counter()
        tm[k] += t1 - t0
        return t1

    out: List[list] = [[None] * len(r) for r in recs]
    by_c = {}
    for i, (_, C, _) in enumerate(shapes):
        by_c.setdefault(C, []).append(i)
    for C, ids in by_c.items():
        items = [(i, j) for i in ids for j in range(len(recs[i]))]
        if not items:
            continue
        t0 = time.perf_counter()
        Pg = max(shapes[i][2] for i in ids)
        f_off = np.concatenate([[0], np.cumsum([shapes[i][0] for i in ids])]).astype(np.int64)
        ks = [np.asarray(sequences[i][0]) for i in ids]
        dt = np.float32 if all(k.dtype == np.float32 for k in ks) else np.float64
        kps = np.zeros((int(f_off[-1]), C, Pg, ks[0].shape[3], 3), dtype=dt)
        cnt = np.zeros((int(f_off[-1]), C), dtype=np.int32)
        for r, i in enumerate(ids):
            kps[f_off[r]:f_off[r + 1], :, :ks[r].shape[2]] = ks[r]
            cnt[f_off[r]:f_off[r + 1]] = np.asarray(sequences[i][1])
        Pm = np.array([[np.asarray(c.P, np.float64).reshape(3, 4) for c in sequences[i][2]] for i in ids])
        rig_of_seq = {i: r for r, i in enumerate(ids)}
        # problems in (sequence, record, frame) order
        fr = [recs[i][j][0] for i, j in items]
        n_of = np.array([f.shape[0] for f in fr], dtype=np.int64)
        rec_lo = np.concatenate([[0], np.cumsum(n_of)]).astype(np.int64)
        frame_of = np.concatenate([f + f_off[rig_of_seq[i]] for f, (i, _) in zip(fr, items)]).astype(np.int32)
        rig_of = np.repeat(np.array([rig_of_seq[i] for i, _ in items], dtype=np.int32), n_of)
        rank = np.repeat(np.array([j for _, j in items], dtype=np.int32), n_of)
        params = np.concatenate([recs[i][j][1] for i, j in items])
        joints = np.concatenate([recs[i][j][2] for i, j in items])
        order = np.argsort(frame_of, kind="stable").astype(np.int32)
        fs = frame_of[order]
        lo = np.searchsorted(fs, frame_of, side="left").astype(np.int32)
        hi = np.searchsorted(fs, frame_of, side="right").astype(np.int32)
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(d)
        k17, c17 = dev.ingest(T(kps), T(cnt))
        Pm_d = T(Pm)
        rig_d = T(rig_of)
        members, n_views, _, _ = dev.body_observe(k17, c17, Pm_d, T(frame_of), rig_d, T(joints), T(order), T(lo), T(hi), T(rank),
                                                  MAX_DIST, MIN_SCORE)
        nv = n_views.cpu().numpy()
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
        # selected pose slot per camera (ingest order) or -1
        mem_h = members.cpu().numpy().astype(np.int64)
        sel = np.where(mem_h >= 0, mem_h % Pg, -1)
        views_used = np.where(live, nv, 0)
        _records(out, items, recs, tracklets_per_sequence, rec_lo, params_out, joints_out, lens_fit, views_used, sel, costs, trials)
        lap("records", t0)
    if timings is not None:
        timings.update(tm)
    return out


def _records(out, items, recs, tracklets_per_sequence, rec_lo, params, joints, lens, views, sel, costs, trials):
    """New MvTracklet records from the fitted tables (one slice per record; the per-frame objects built from whole arrays)."""
    from .inverse_kinematics import PoseShapeParam
    from .motion_capture import MvTracklet
    from .pose_def import KpsFormat, Pose
    trans, ang = params[:, :3].copy(), params[:, 3:57].reshape(-1, 18, 3).copy()
    ones = np.ones((18, 1))
    for a, (i, j) in enumerate(items):
        src = tracklets_per_sequence[i][j]
        lo, hi = int(rec_lo[a]), int(rec_lo[a + 1])
        frm = recs[i][j][0].tolist()
        L = lens[a].copy()
        poses = [(frm[k], PoseShapeParam(trans[lo + k], ang[lo + k], L.copy()), Pose(KpsFormat.BASIC_18, joints[lo + k], ones.copy(), None))
                 for k in range(hi - lo)]
        t = MvTracklet(src.track_id, frm[0], poses[0][1], poses[0][2])
        t.frame_idxs = list(frm)
        t.poses = poses
        t.state = src.state
        t.hits = src.hits
        t.time_since_update = getattr(src, "time_since_update", 0)
        t.bone_lens = L
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
