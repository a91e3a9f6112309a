"""Many recorded sequences, each with its own camera rig, through the batched temporal path in one launch per camera count.

track_sequences() cuts every sequence into chains of ``chain_len`` frames, lays the chains of all sequences with the same number of
cameras end to end, and runs them as ONE chain-kernel launch with a calibration per chain (tracker.run_chains_fused(..., rigs,
rig_of_chain): include/mvmc.h, mvmc_chain_run_rigs).  The repair tier and the chain-boundary stitch then run as on the benchmark's path,
the stitch per sequence over that sequence's own chains, so no identity crosses from one sequence into the next.  The stitched tables
become the reference's MvTracklet records.

These are the BATCHED semantics the benchmark measures, not frame-by-frame MvTracker.update_4d: every chain starts from match_spatial
and cold IK solves, and identities are carried across chain boundaries by the stitch.
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
    from .inverse_kinematics import PoseShapeParam
    from .motion_capture import MvTracklet, TrackState
    from .pose_def import KpsFormat, Pose
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
    x = params[fs, ss]
    trans, ang, shape = x[:, :3].copy(), x[:, 3:57].reshape(-1, 18, 3).copy(), x[:, 57:].copy()
    jo = joints[fs, ss].copy()
    frm = (frame_idx0 + fs).tolist()
    ones = np.ones((18, 1))
    poses = [(frm[k], PoseShapeParam(trans[k], ang[k], shape[k]), Pose(KpsFormat.BASIC_18, jo[k], ones.copy(), None))
             for k in range(sel.size)]
    last_f = f_idx[last_row]
    dead = last_f < n_real - 1
    state = np.where(dead, TrackState.Dead.value, meta[last_f, s_idx[last_row], 1])
    last_hit = fs[start + cnt - 1]
    since = last_f + dead.astype(np.int64) - last_hit
    out = []
    for j, tid in enumerate(ids.tolist()):
        a, n = int(start[j]), int(cnt[j])
        t = MvTracklet(tid, frm[a], poses[a][1], poses[a][2])
        t.frame_idxs = frm[a:a + n]
        t.poses = poses[a:a + n]
        t.hits = n
        t.state = TrackState(int(state[j]))
        t.time_since_update = int(since[j])
        out.append(t)
    return sorted(out, key=lambda t: -len(t))


def track_sequences(sequences: Sequence[SequenceInput], chain_len: int = 16, t_max: Optional[int] = None,
                    max_dist: float = parallel.MAX_DIST, frame_idx0: int = 0, device="cuda:0", timings: Optional[dict] = None,
                    tables: Optional[list] = None, relink: bool = False):
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
    the tables stay the tracker's own).  Off by default: the records are then the stitch's, as before."""
    import time

    import torch

    from .pipeline import HotPath
    from .tracker import check_chain_flags, repair_chains, run_chains_fused
    shapes = check_sequences(sequences)
    L = int(chain_len)
    d = torch.device(device)
    result: List[list] = [[] for _ in sequences]
    per_seq: List[Optional[dict]] = [None for _ in sequences]
    tm = {"kernel": 0.0, "repair_stitch": 0.0, "convert": 0.0}

    def lap(k, t0):
        if timings is not None:
            torch.cuda.synchronize(d)
        t1 = time.perf_counter()
        tm[k] += t1 - t0
        return t1

    for lay in plan_groups(shapes, L):
        if lay.total_chains == 0:
            continue
        t0 = time.perf_counter()
        rigs = [HotPath(np.array([c.K for c in sequences[i][2]]), np.array([c.Rt for c in sequences[i][2]]), device=d)
                for i in lay.seq_ids]
        kps_h, cnt_h = pack_group(lay, sequences, L)
        kps, counts = torch.from_numpy(kps_h).to(d), torch.from_numpy(cnt_h).to(d)
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
    if timings is not None:
        timings.update(tm)
    if tables is not None:
        tables.extend(per_seq)
    return result
