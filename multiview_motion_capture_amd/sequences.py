"""Many recorded sequences, each with its own camera rig, through the batched temporal path in one launch per camera count.

track_sequences() cuts every sequence into chains of ``chain_len`` frames, lays the chains of all sequences with the same number of
cameras end to end, and runs them as ONE chain-kernel launch with a calibration per chain (tracker.run_chains_fused(..., rigs,
rig_of_chain): include/mvmc.h, mvmc_chain_run_rigs).  The repair tier and the chain-boundary stitch then run as on the benchmark's path,
the stitch per sequence over that sequence's own chains, so no identity crosses from one sequence into the next.  The stitched tables
become the reference's MvTracklet records.

These are the BATCHED semantics the benchmark measures, not frame-by-frame MvTracker.update_4d: every chain starts from match_spatial
and cold IK solves, and identities are carried across chain boundaries by the stitch.

The stages that run on finished records (body_fit, smoothing, rig_refine; parts of it live_smoothing, rig_init, relinking) share their
host front end and record writer here: check_records, stack_group, select_views (problem_tables, frame_buckets), stopwatch, and
pose_tuples / new_record / pose_slot.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import parallel
from .common import Calib

SequenceInput = Tuple[np.ndarray, np.ndarray, List[Calib]]   # kps25 (F,C,P,25,3) (or COCO-17 rows), counts (F,C), one Calib per camera


@dataclass
class GroupLayout:
    """Sequences of one camera count, laid out as the chains of one launch."""
    seq_ids: List[int]          # positions in the caller's list, in launch order; rig r of the launch = sequence seq_ids[r]
    n_views: int
    p_max: int                  # the group's largest P_s: every sequence is padded to it
    n_frames: List[int]         # real frames of each sequence
    chain_lo: List[int]         # first chain of each sequence
    n_chains: List[int]         # chains of each sequence (its frames padded to a multiple of chain_len)
    rig_of_chain: np.ndarray    # (B,) int32: the sequence's ordinal in the group

    @property
    def total_chains(self) -> int:
        return int(self.rig_of_chain.shape[0])


def check_sequences(sequences: Sequence[SequenceInput], who: str = "track_sequences") -> List[Tuple[int, int, int]]:
    """(F_s, C_s, P_s) of every sequence; raises ValueError on an empty list or inconsistent shapes.  Keypoint rows are OpenPose-25
    (what load_openpose_sequence returns) or COCO-17 (the per-frame pickles' poses), the same layout for every sequence.  A calibration
    with a lens model is refused (lens.require_pinhole, in ``who``'s name): the keypoints are read as pinhole pixels."""
    from .lens import require_pinhole
    if len(sequences) == 0:
        raise ValueError("track_sequences: no sequences")
    shapes, joints = [], set()
    for i, seq in enumerate(sequences):
        if len(seq) != 3:
            raise ValueError(f"sequence {i}: expected (kps25, counts, calibs)")
        kps, counts, calibs = seq
        kps, counts = np.asarray(kps), np.asarray(counts)
        if kps.ndim != 5 or kps.shape[3] not in (17, 25) or kps.shape[4] != 3:
            raise ValueError(f"sequence {i}: kps25 must be (F,C,P,25,3), got {kps.shape}")
        joints.add(kps.shape[3])
        F, C, P = kps.shape[:3]
        if counts.shape != (F, C):
            raise ValueError(f"sequence {i}: counts must be ({F},{C}), got {counts.shape}")
        if len(calibs) != C:
            raise ValueError(f"sequence {i}: {len(calibs)} calibrations for {C} cameras")
        require_pinhole(calibs, f"{who}: sequence {i}")
        if C < 1 or P < 1:
            raise ValueError(f"sequence {i}: no cameras or no person slots")
        if counts.size and (counts.min() < 0 or counts.max() > P):
            raise ValueError(f"sequence {i}: counts outside [0, {P}]")
        shapes.append((F, C, P))
    if len(joints) > 1:
        raise ValueError("track_sequences: OpenPose-25 and COCO-17 keypoints mixed")
    return shapes


def plan_groups(shapes: Sequence[Tuple[int, int, int]], chain_len: int) -> List[GroupLayout]:
    """Group sequences by camera count (groups in the order of their first sequence), pad each to whole chains, lay them end to end."""
    if chain_len < 1:
        raise ValueError("chain_len must be >= 1")
    by_c = {}
    for i, (_, C, _) in enumerate(shapes):
        by_c.setdefault(C, []).append(i)
    groups = []
    for C, ids in by_c.items():
        n_ch = [-(-shapes[i][0] // chain_len) for i in ids]
        lo = np.concatenate([[0], np.cumsum(n_ch)[:-1]]).astype(int).tolist()
        roc = np.repeat(np.arange(len(ids), dtype=np.int32), n_ch)
        groups.append(GroupLayout(seq_ids=list(ids), n_views=C, p_max=max(shapes[i][2] for i in ids),
                                  n_frames=[shapes[i][0] for i in ids], chain_lo=lo, n_chains=n_ch, rig_of_chain=roc))
    return groups


def pack_group(layout: GroupLayout, sequences: Sequence[SequenceInput], chain_len: int):
    """Host arrays of one launch: kps25 (B L, C, p_max, 25, 3) and counts (B L, C) i32, zero (= empty frames) where padded; the
    keypoints keep the sequences' joint layout and dtype (float32 if every sequence's is, float64 otherwise)."""
    F = layout.total_chains * chain_len
    ks = [np.asarray(sequences[i][0]) for i in layout.seq_ids]
    dt = np.float32 if all(k.dtype == np.float32 for k in ks) else np.float64
    kps = np.zeros((F, layout.n_views, layout.p_max, ks[0].shape[3], 3), dtype=dt)
    counts = np.zeros((F, layout.n_views), dtype=np.int32)
    for r, i in enumerate(layout.seq_ids):
        k, c = ks[r], np.asarray(sequences[i][1])
        f0, n = layout.chain_lo[r] * chain_len, layout.n_frames[r]
        kps[f0:f0 + n, :, :k.shape[2]] = k
        counts[f0:f0 + n] = c
    return kps, counts


# -- the record stages' shared front end (body_fit, smoothing, rig_refine; live_smoothing and rig_init take parts of it) --------------------
def no_sequences(sequences, tracklets_per_sequence, who: str) -> bool:
    """True for an empty call (the stage returns []); records without sequences: ValueError."""
    if len(sequences) == 0 and len(tracklets_per_sequence):
        raise ValueError(f"{who}: records without sequences")
    return len(sequences) == 0


def record_arrays(rec, F: int, where: str):
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


def check_records(sequences, tracklets_per_sequence, who: str, own_checks=None, cameras=None, increasing=False, finite=False):
    """The input checks every record stage shares, host only: ValueError, or (shapes, per sequence its records' record_arrays).  In
    this order: one record list per sequence; ``own_checks()`` (the stage's parameter checks); check_sequences; then sequence by
    sequence ``cameras`` = (lo, hi, message with {s} and {C}) and per record its arrays, ``increasing`` frames, ``finite`` parameters."""
    if len(tracklets_per_sequence) != len(sequences):
        raise ValueError(f"{who}: {len(tracklets_per_sequence)} record lists for {len(sequences)} sequences")
    if own_checks is not None:
        own_checks()
    shapes = check_sequences(sequences, who)
    recs = []
    for s, (tl, (F, C, _)) in enumerate(zip(tracklets_per_sequence, shapes)):
        if cameras is not None and not cameras[0] <= C <= cameras[1]:
            raise ValueError(cameras[2].format(s=s, C=C))
        rr = []
        for j, t in enumerate(tl):
            where = f"sequence {s}, record {j}"
            fr, par, jn = record_arrays(t, F, where)
            if increasing and np.any(np.diff(fr) <= 0):
                raise ValueError(f"{where}: frame indices must increase")
            if finite and not np.all(np.isfinite(par)):
                raise ValueError(f"{where}: parameters must be finite")
            rr.append((fr, par, jn))
        recs.append(rr)
    return shapes, recs


def stopwatch(timings: Optional[dict], device, keys):
    """-> (lap, tm).  tm: seconds per key, from 0.  lap(key, t0=None) adds the time since t0 (None: since the previous lap ended) to
    tm[key] and returns now; it synchronises ``device`` first only when the caller passed a ``timings`` dict."""
    import time

    import torch
    tm = {k: 0.0 for k in keys}
    last = [time.perf_counter()]

    def lap(k, t0=None):
        if timings is not None:
            torch.cuda.synchronize(device)
        t1 = time.perf_counter()
        tm[k] += t1 - (last[0] if t0 is None else t0)
        last[0] = t1
        return t1
    return lap, tm


@dataclass
class StackedGroup:
    """The sequences of one camera count, frames end to end: sequence seq_ids[r] owns rows f_off[r]:f_off[r + 1] and is rig r."""
    seq_ids: List[int]
    n_views: int
    Pg: int                     # person slots of every row (the group's largest P_s; the others zero)
    f_off: np.ndarray           # (S + 1,) i64
    kps: np.ndarray             # (f_off[-1], C, Pg, 25|17, 3): pack_group's dtype rule
    cnt: np.ndarray             # (f_off[-1], C) i32
    Pm: np.ndarray              # (S, C, 3, 4) f64


def stack_group(layout: GroupLayout, sequences: Sequence[SequenceInput]) -> StackedGroup:
    """One group of plan_groups(shapes, 1) -> its stacked host arrays (pack_group at a chain length of 1: a chain is a frame)."""
    kps, cnt = pack_group(layout, sequences, 1)
    Pm = np.array([[np.asarray(c.P, np.float64).reshape(3, 4) for c in sequences[i][2]] for i in layout.seq_ids])
    f_off = np.array(layout.chain_lo + [layout.total_chains], dtype=np.int64)
    return StackedGroup(list(layout.seq_ids), layout.n_views, layout.p_max, f_off, kps, cnt, Pm)


def frame_buckets(frame_of: np.ndarray):
    """frame_of (B,) i32 -> order, lo, hi (B,) i32: order[lo[b]:hi[b]] = the problems of b's frame, in input order (body_observe's
    tie rule looks through them)."""
    order = np.argsort(frame_of, kind="stable").astype(np.int32)
    fs = frame_of[order]
    lo, hi = (np.searchsorted(fs, frame_of, side=side).astype(np.int32) for side in ("left", "right"))
    return order, lo, hi


@dataclass
class Selection:
    """The selection problems of one group, one per (record, record frame) in (sequence, record, frame) order, and what
    mvmc_body_observe chose for them.  Record a = items[a] owns problems rec_lo[a]:rec_lo[a + 1]."""
    items: List[Tuple[int, int]]    # (sequence: position in the caller's list, record)
    n_of: np.ndarray                # (R,) i64 frames per record
    rec_lo: np.ndarray              # (R + 1,) i64
    frame_of: np.ndarray            # (B,) i32 stacked frame
    rig_of: np.ndarray              # (B,) i32 the sequence's ordinal in the group
    rank: np.ndarray                # (B,) i32 the record's position in its sequence's list: the earlier record wins a tie
    order: np.ndarray               # frame_buckets(frame_of)
    lo: np.ndarray
    hi: np.ndarray
    params: Optional[np.ndarray]    # (B,68) f64 host (None unless asked for)
    joints: np.ndarray              # (B,18,3) f64 host
    Pg: int
    f_off: np.ndarray
    # device side, filled by select_views
    k17: object = None              # (f_off[-1], C, Pg, 17, 3) ingested keypoints
    c17: object = None
    Pm_d: object = None
    rig_d: object = None            # rig_of
    members: object = None          # (B, C) i32: pose row of k17.reshape(-1, 17, 3) or -1
    n_views: object = None          # (B,) i32


def problem_tables(grp: StackedGroup, recs: Sequence[list], want_params: bool = False) -> Selection:
    """The host tables of a group's selection: recs[i] = check_records' arrays of sequence i's records (at least one in the group)."""
    rig_of_seq = {i: r for r, i in enumerate(grp.seq_ids)}
    items = [(i, j) for i in grp.seq_ids for j in range(len(recs[i]))]
    fr = [recs[i][j][0] for i, j in items]
    n_of = np.array([f.shape[0] for f in fr], dtype=np.int64)
    rec_lo = np.concatenate([[0], np.cumsum(n_of)]).astype(np.int64)
    frame_of = np.concatenate([f + grp.f_off[rig_of_seq[i]] for f, (i, _) in zip(fr, items)]).astype(np.int32)
    rig_of = np.repeat(np.array([rig_of_seq[i] for i, _ in items], dtype=np.int32), n_of)
    rank = np.repeat(np.array([j for _, j in items], dtype=np.int32), n_of)
    params = np.concatenate([recs[i][j][1] for i, j in items]) if want_params else None
    joints = np.concatenate([recs[i][j][2] for i, j in items])
    return Selection(items, n_of, rec_lo, frame_of, rig_of, rank, *frame_buckets(frame_of), params, joints, grp.Pg, grp.f_off)


def select_views(grp: StackedGroup, recs: Sequence[list], device, max_dist: float, min_score: float, want_params: bool = False) -> Selection:
    """Ingest the group's keypoints and select, per problem and camera, the pose nearest to the record's joints (body_fit's step a;
    include/mvmc.h: mvmc_body_observe).  No synchronisation: members and n_views stay on the device."""
    from . import device as dev
    T = dev.uploader(device)
    sel = problem_tables(grp, recs, want_params)
    sel.k17, sel.c17 = dev.ingest(T(grp.kps), T(grp.cnt))
    sel.Pm_d, sel.rig_d = T(grp.Pm), T(sel.rig_of)
    sel.members, sel.n_views, _, _ = dev.body_observe(sel.k17, sel.c17, sel.Pm_d, T(sel.frame_of), sel.rig_d, T(sel.joints), T(sel.order),
                                                      T(sel.lo), T(sel.hi), T(sel.rank), max_dist, min_score)
    return sel


def pose_slot(members: np.ndarray, Pg: int) -> np.ndarray:
    """members (.., C): rows of the ingested keypoints (frame, camera, slot) or -1 -> the pose slot in ingest order, or -1 (i32)."""
    mem = np.asarray(members).astype(np.int64)
    return np.where(mem >= 0, mem % Pg, -1).astype(np.int32)


def pose_tuples(frames, params: np.ndarray, joints: np.ndarray) -> list:
    """frames (n,), params (n,68), joints (n,18,3) -> an MvTracklet's poses [(frame, PoseShapeParam, BASIC_18 Pose)].  The poses' arrays
    are rows of copies made here: none aliases an input."""
    from .inverse_kinematics import PoseShapeParam
    from .pose_def import KpsFormat, Pose
    frm = np.asarray(frames).tolist()
    x = np.asarray(params)
    trans, ang, shape = x[:, :3].copy(), x[:, 3:57].reshape(-1, 18, 3).copy(), x[:, 57:].copy()
    jo = np.array(joints, copy=True).reshape(-1, 18, 3)
    ones = np.ones((18, 1))
    return [(frm[k], PoseShapeParam(trans[k], ang[k], shape[k]), Pose(KpsFormat.BASIC_18, jo[k], ones.copy(), None)) for k in range(len(frm))]


def new_record(track_id, poses: list, src=None, frame_idxs=None, state=None, hits=None, time_since_update=None):
    """An MvTracklet of ``poses``; state, hits and time_since_update (0 where it has none) from the record ``src`` unless given."""
    from .motion_capture import MvTracklet
    frame_idxs = [p[0] for p in poses] if frame_idxs is None else frame_idxs
    t = MvTracklet(track_id, frame_idxs[0], poses[0][1], poses[0][2])
    t.frame_idxs, t.poses = frame_idxs, poses
    t.state = src.state if state is None else state
    t.hits = src.hits if hits is None else hits
    t.time_since_update = getattr(src, "time_since_update", 0) if time_since_update is None else time_since_update
    return t


def tables_to_tracklets(meta: np.ndarray, n_tracks: np.ndarray, params: np.ndarray, joints: np.ndarray, gid: np.ndarray, chain_len: int,
                        n_real: int, frame_idx0: int = 0):
    """One sequence's stitched per-frame tables -> MvTracklet records, one per global identity, longest first.

    meta (F,T,4) {local id, state, hits, length}, n_tracks (F), params (F,T,68), joints (F,T,18,3): the tables of the sequence's chains
    (F = its chains x chain_len, padded frames included); gid (n_chains, id_cap): global identity of (chain, local id).  Rows of frames
    >= n_real (padding) are dropped; frame f is reported as frm_idx = frame_idx0 + f.

    MvTracker.update_4d's rule (motion_capture.py, update_4d) with the stitch's identities: a local tracklet of a chain is update_4d's
    tracklet id, so a frame's pose is appended to its global identity where that local tracklet first appears or where its ``hits``
    grew since its previous row; ``hits`` is then the number of frames appended (as in update_4d, where it counts them); ``state`` is
    the identity's state in its last row, Dead when that row lies before the sequence's last real frame; ``time_since_update`` counts
    the frames from its last appended frame to its last row (to the frame after it, for a dead one)."""
    from .motion_capture import TrackState
    L = int(chain_len)
    n_real = int(n_real)
    if n_real <= 0:
        return []
    T = meta.shape[1]
    n_t = np.asarray(n_tracks[:n_real]).astype(np.int64)
    f_idx, s_idx = np.nonzero(np.arange(T)[None, :] < n_t[:, None])       # live rows, in (frame, slot) order
    if f_idx.size == 0:
        return []
    local = meta[f_idx, s_idx, 0].astype(np.int64)
    chain = f_idx // L
    if local.min() < 0 or local.max() >= gid.shape[1]:
        raise ValueError("tables_to_tracklets: a local identity outside the stitch's id table")
    g = gid[chain, local].astype(np.int64)
    if g.min() < 0:
        raise ValueError("tables_to_tracklets: a live tracklet without a global identity")
    hits = meta[f_idx, s_idx, 2]
    # update_4d's rule per local tracklet: rows of one (chain, local id) in frame order, appended where first or where hits grew
    key = chain * gid.shape[1] + local
    order = np.lexsort((f_idx, key))
    k_o, h_o = key[order], hits[order]
    first = np.ones(order.size, dtype=bool)
    first[1:] = k_o[1:] != k_o[:-1]
    grew = np.zeros(order.size, dtype=bool)
    grew[1:] = h_o[1:] > h_o[:-1]
    take = np.zeros(f_idx.size, dtype=bool)
    take[order] = first | grew
    # per identity: appended rows in frame order, and its last row
    sel = np.nonzero(take)[0]
    sel = sel[np.lexsort((f_idx[sel], g[sel]))]
    ids, start, cnt = np.unique(g[sel], return_index=True, return_counts=True)
    last_any = np.lexsort((f_idx, g))
    ids_all, last_pos = np.unique(g[last_any][::-1], return_index=True)
    last_row = last_any[::-1][last_pos]                                   # (the last row of each identity, ids_all ascending)
    assert np.array_equal(ids, ids_all)
    fs, ss = f_idx[sel], s_idx[sel]
    poses = pose_tuples(frame_idx0 + fs, params[fs, ss], joints[fs, ss])
    last_f = f_idx[last_row]
    dead = last_f < n_real - 1
    state = np.where(dead, TrackState.Dead.value, meta[last_f, s_idx[last_row], 1])
    last_hit = fs[start + cnt - 1]
    since = last_f + dead.astype(np.int64) - last_hit
    out = []
    for j, tid in enumerate(ids.tolist()):
        a, n = int(start[j]), int(cnt[j])
        out.append(new_record(tid, poses[a:a + n], state=TrackState(int(state[j])), hits=n, time_since_update=int(since[j])))
    return sorted(out, key=lambda t: -len(t))


def track_sequences(sequences: Sequence[SequenceInput], chain_len: int = 16, t_max: Optional[int] = None,
                    max_dist: float = parallel.MAX_DIST, frame_idx0: int = 0, device="cuda:0", timings: Optional[dict] = None,
                    tables: Optional[list] = None, relink: bool = False, reidentify: bool = False):
    """Track every sequence -- (kps25 (F_s,C,P_s,25,3), counts (F_s,C), calibs: one Calib per camera), what
    motion_capture.load_openpose_sequence returns -- and return, per sequence, its MvTracklet records (longest first).

    Sequences with the same number of cameras share one chain-kernel launch, each with its own calibration (tracker.run_chains_fused
    with rigs / rig_of_chain); the chains the kernel's tables cannot hold go through tracker.repair_chains; identities are stitched
    across the chain boundaries of each sequence (parallel.pack_tracks / stitch_chains), never across two sequences.
    frame_idx0: the frm_idx of every sequence's first frame in the records.
    timings: a dict that receives the seconds spent in {"kernel", "repair_stitch", "convert"} (synchronising between the parts).
    tables: a list that receives, per sequence, its stitched tables as host arrays (padded frames included): dict(params, joints,
    meta, n_tracks, gid (its chains, parallel.ID_CAP), match, n_frames).
    relink: join the records of one person per sequence afterwards (relinking.relink_sequences with its defaults, max_dist as here;
    the tables stay the tracker's own).  Off by default: the records are then the stitch's, as before.
    reidentify: afterwards (after relink when both are asked for) join the records of one person across long holes by their bone
    lengths (relinking.reidentify_sequences with its defaults).  Off by default."""
    import time

    import torch

    from .device import uploader
    from .pipeline import HotPath
    from .tracker import check_chain_flags, repair_chains, run_chains_fused
    shapes = check_sequences(sequences)
    L = int(chain_len)
    d = torch.device(device)
    result: List[list] = [[] for _ in sequences]
    per_seq: List[Optional[dict]] = [None for _ in sequences]
    lap, tm = stopwatch(timings, d, ("kernel", "repair_stitch", "convert"))
    for lay in plan_groups(shapes, L):
        if lay.total_chains == 0:
            continue
        t0 = time.perf_counter()
        rigs = [HotPath(np.array([c.K for c in sequences[i][2]]), np.array([c.Rt for c in sequences[i][2]]), device=d)
                for i in lay.seq_ids]
        kps, counts = map(uploader(d), pack_group(lay, sequences, L))
        out = run_chains_fused(rigs[0], kps, counts, L, t_max=t_max, rigs=rigs, rig_of_chain=lay.rig_of_chain)
        t0 = lap("kernel", t0)
        repair_chains(rigs[0], kps, counts, out)
        check_chain_flags(out)
        T = out["params"].shape[1]
        stitched = []
        for r in range(len(lay.seq_ids)):
            lo, n = lay.chain_lo[r], lay.n_chains[r]
            if n == 0:
                stitched.append(None)
                continue
            f0, f1 = lo * L, (lo + n) * L
            view = {k: out[k][f0:f1] for k in ("params", "joints", "meta", "n_tracks")}
            row_cap = n * L * T
            msg = parallel.pack_tracks(view, out["next_id"][lo:lo + n].contiguous(), L, n, row_cap, max_dist=max_dist)
            stitched.append(parallel.stitch_chains(msg.view(1, -1), n, T, row_cap, max_dist))
        host = {k: out[k].cpu().numpy() for k in ("params", "joints", "meta", "n_tracks")}
        t0 = lap("repair_stitch", t0)
        for r, i in enumerate(lay.seq_ids):
            st = stitched[r]
            if st is None:
                continue
            parallel.check_stitch_info(st)
            f0, f1 = lay.chain_lo[r] * L, (lay.chain_lo[r] + lay.n_chains[r]) * L
            gid = st["gid"].cpu().numpy()
            result[i] = tables_to_tracklets(host["meta"][f0:f1], host["n_tracks"][f0:f1], host["params"][f0:f1], host["joints"][f0:f1],
                                            gid, L, lay.n_frames[r], frame_idx0)
            if tables is not None:
                per_seq[i] = dict({k: v[f0:f1] for k, v in host.items()}, gid=gid, match=st["match"].cpu().numpy(), n_frames=lay.n_frames[r])
        lap("convert", t0)
    if relink:
        from .relinking import relink_sequences
        t0 = time.perf_counter()
        result = relink_sequences(result, max_dist=max_dist, device=device)
        tm["relink"] = time.perf_counter() - t0
    if reidentify:
        from .relinking import reidentify_sequences
        t0 = time.perf_counter()
        result = reidentify_sequences(result, device=device)
        tm["reidentify"] = time.perf_counter() - t0
    if timings is not None:
        timings.update(tm)
    if tables is not None:
        tables.extend(per_seq)
    return result
