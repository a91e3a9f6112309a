"""Re-linking: the records of one person that the tracker split become one record per sequence (track -> RE-LINK -> fit -> smooth -> BVH).

The batched path starts every chain cold and stitches only the last frame of a chain to the first frame of the next; update_4d lets a
person who enters be born, lost and born again.  Either way one person can own several records.  relink_sequences() joins them from
the records alone (frames and the 18 x 3 joints of every appended pose; no keypoints, no calibration).  Per sequence:

  nodes   the records, in (first frame, track_id) order (so the result does not depend on the order of the caller's list);
  links   A may be followed by B when 1 <= gap = B.first_frame - A.last_frame <= max_gap (records that overlap in time are never
          joined), at the cost  mean over the 18 joints of | A.last_joints + v gap - B.first_joints |  (metres), where v is the mean of
          A's end velocity and B's start velocity: the displacement of the joint centroid over the last (first) min(4, poses - 1)
          appended poses divided by the FRAMES between them; of the one that is defined for a record of one pose; zero for two such;
  gate    a link is allowed when cost <= min(max_dist, near_dist + speed gap); a non-finite cost is not allowed;
  choice  the links taken minimise  sum cost + max_dist x (records left without a successor)  over all one-to-one choices among the
          allowed links: an optimal assignment (Kuhn-Munkres with potentials, rows in record order, the first minimum wins).

Chains of links become one record: the fragments' frames and poses concatenated, nothing changed or invented, so a joined record has a
hole where two fragments met; smoothing.smooth_sequences(fill_gaps=True) fills it.

Device code: csrc/mvmc_relink.hip (include/mvmc.h: mvmc_relink), one launch for all sequences of a call, one workgroup per sequence;
NumPy restatement: tests/relink_np.py.  The defaults: tools/relink_sweep.py (profiles/relink_sweep.json).
"""
from __future__ import annotations

import math
import time
from typing import List, Optional, Sequence

import numpy as np

from . import parallel

MAX_GAP = 16                      # frames: the chain length of the batched path (a person missed at a chain head is re-born inside it)
MAX_DIST = parallel.MAX_DIST      # metres: the stitch's own bound
NEAR_DIST, SPEED = 0.15, 0.03     # metres, metres per frame of gap: the gate grows with the gap
VEL_POSES = 4                     # poses the end / start velocity looks back / ahead
MAX_RECORDS = 512                 # include/mvmc.h: MVMC_RELINK_MAX_RECORDS (records of one sequence)
_REC = 120                        # include/mvmc.h: MVMC_RELINK_REC_DOUBLES
_LDS_N = 64                       # csrc/mvmc_relink.hip: sequences of more records keep their cost matrix in the workspace


def check_parameters(max_gap, max_dist, near_dist, speed) -> None:
    if isinstance(max_gap, bool) or int(max_gap) != max_gap or int(max_gap) < 1:
        raise ValueError("relink: max_gap must be an integer >= 1")
    if int(max_gap) >= 2 ** 30:
        raise ValueError("relink: max_gap too large")
    for name, x in (("max_dist", max_dist), ("near_dist", near_dist), ("speed", speed)):
        x = float(x)
        if not math.isfinite(x) or x < 0 or x >= 1e6:
            raise ValueError(f"relink: {name} must be finite, >= 0 and below 1e6")


def _joints(pose, where):
    try:
        j = np.asarray(pose[2].keypoints, dtype=np.float64)
    except (AttributeError, TypeError, IndexError, ValueError) as e:
        raise ValueError(f"{where}: poses must be (frame, PoseShapeParam, BASIC_18 Pose): {e}") from None
    if j.shape != (18, 3):
        raise ValueError(f"{where}: joints must be 18 x 3, got {j.shape}")
    return j


def pack_records(tracklets_per_sequence: Sequence[list]) -> dict:
    """The host arrays of one launch (include/mvmc.h: mvmc_relink), after every input check: rec (N,120) f64, frames (N,4) i32, seq
    (S,4) i32, work_words, and per sequence ``order``: position in the caller's list of node k (nodes in (first frame, track_id)
    order).  Only the four poses per record that the cost reads are touched."""
    orders, firsts, lasts, spans, ends = [], [], [], [], []
    for s, tl in enumerate(tracklets_per_sequence):
        n = len(tl)
        if n > MAX_RECORDS:
            raise ValueError(f"sequence {s}: {n} records, at most {MAX_RECORDS} per sequence")
        first, last, tid = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
        span = np.zeros((n, 2), np.int64)
        end = np.zeros((n, 4, 18, 3))
        for j, t in enumerate(tl):
            where = f"sequence {s}, record {j}"
            fr = np.asarray(t.frame_idxs, dtype=np.int64)
            m = fr.shape[0]
            if fr.ndim != 1 or m == 0 or len(t.poses) != m:
                raise ValueError(f"{where}: {fr.shape} frame indices and {len(t.poses)} poses")
            if np.any(np.diff(fr) <= 0):
                raise ValueError(f"{where}: frame indices must increase")
            if fr[0] < -2 ** 30 or fr[-1] >= 2 ** 30:
                raise ValueError(f"{where}: frame indices outside 32 bits")
            k = min(VEL_POSES, m - 1)
            first[j], last[j], tid[j] = fr[0], fr[-1], int(t.track_id)
            span[j] = fr[-1] - fr[-1 - k], fr[k] - fr[0]
            end[j, 0], end[j, 1] = _joints(t.poses[-1], where), _joints(t.poses[-1 - k], where)
            end[j, 2], end[j, 3] = _joints(t.poses[0], where), _joints(t.poses[k], where)
        order = np.lexsort((tid, first))
        orders.append(order)
        firsts.append(first[order]); lasts.append(last[order]); spans.append(span[order]); ends.append(end[order])
    counts = np.array([o.shape[0] for o in orders], dtype=np.int64)
    N, S = int(counts.sum()), len(orders)
    rec = np.zeros((N, _REC))
    frames = np.zeros((N, 4), np.int32)
    seq = np.zeros((S, 4), np.int32)
    if N:
        e = np.concatenate(ends)
        rec[:, :54] = e[:, 0].reshape(N, 54)
        rec[:, 54:108] = e[:, 2].reshape(N, 54)
        rec[:, 108:120] = e.mean(axis=2).reshape(N, 12)      # centroids: last, k back, first, k on
        frames[:, 0], frames[:, 1] = np.concatenate(firsts), np.concatenate(lasts)
        frames[:, 2:] = np.concatenate(spans)
    work = np.where(counts > _LDS_N, counts * counts, 0)
    if int(work.sum()) >= 2 ** 31:
        raise ValueError("relink: the cost matrices of one call exceed 2^31 words; pass fewer sequences per call")
    seq[:, 0] = np.concatenate([[0], np.cumsum(counts)[:-1]]) if S else 0
    seq[:, 1] = counts
    seq[:, 2] = np.concatenate([[0], np.cumsum(work)[:-1]]) if S else 0
    return dict(rec=rec, frames=frames, seq=seq, order=orders, work_words=int(work.sum()))


def solve_links(packed: dict, max_gap: int, max_dist: float, near_dist: float, speed: float, device="cuda:0") -> List[dict]:
    """ONE upload, one launch, one read-back: per sequence dict(succ, head, pos (n) i64, cost (n) f64) over its nodes."""
    import ctypes

    import torch

    from . import _cabi
    from .device import _stream
    rec, frames, seq = packed["rec"], packed["frames"], packed["seq"]
    N, S = rec.shape[0], seq.shape[0]
    if S == 0:
        return []
    d = torch.device(device)
    lib = _cabi.load()
    # the upload: rec | frames | seq as 8-byte words; the read-back: link_cost | succ, head, pos, status as 4-byte words
    n_fr, n_sq = 2 * N, 2 * S
    up = np.empty(N * _REC + n_fr + n_sq, dtype=np.float64)
    up[:N * _REC] = rec.reshape(-1)
    up_i = up.view(np.int32)
    up_i[2 * N * _REC:2 * (N * _REC + n_fr)] = frames.reshape(-1)
    up_i[2 * (N * _REC + n_fr):] = seq.reshape(-1)
    with torch.cuda.device(d):
        up_d = torch.from_numpy(up).to(d)
        out_d = torch.empty((N + (3 * N + S + 1) // 2,), dtype=torch.float64, device=d)
        work = torch.empty((max(1, packed["work_words"]),), dtype=torch.float64, device=d)
        b_up, b_out = up_d.data_ptr(), out_d.data_ptr()
        vp = ctypes.c_void_p
        o_i = b_out + 8 * N
        _cabi.check(lib.mvmc_relink(vp(b_up), vp(b_up + 8 * N * _REC), vp(b_up + 8 * (N * _REC + n_fr)), N, S, int(max_gap),
                                    float(max_dist), float(near_dist), float(speed), vp(o_i), vp(o_i + 4 * N), vp(o_i + 8 * N),
                                    vp(b_out), vp(o_i + 12 * N), vp(work.data_ptr()), ctypes.c_longlong(packed["work_words"]),
                                    _stream()), "mvmc_relink")
        out = out_d.cpu().numpy()
    cost = out[:N]
    ints = out[N:].view(np.int32)
    status = ints[3 * N:3 * N + S]
    if np.any(status == 2):
        raise RuntimeError("relink: a sequence's records do not fit the launch (status 2)")
    if np.any(status != 0):
        raise RuntimeError("relink: an assignment did not terminate (sequence %d)" % int(np.flatnonzero(status)[0]))
    res = []
    for s in range(S):
        a, n = int(seq[s, 0]), int(seq[s, 1])
        res.append(dict(succ=ints[a:a + n].astype(np.int64), head=ints[N + a:N + a + n].astype(np.int64),
                        pos=ints[2 * N + a:2 * N + a + n].astype(np.int64), cost=cost[a:a + n].copy()))
    return res


def merge_records(tracklets: list, order: np.ndarray, head: np.ndarray, pos: np.ndarray, cost: np.ndarray) -> list:
    """One sequence's records and its links (over the nodes: node k = tracklets[order[k]]) -> NEW MvTracklet records, longest first:
    track_id of the earliest fragment; frame_idxs / poses of the fragments in time order (the pose tuples themselves, unchanged);
    hits = the number of poses; state and time_since_update of the last fragment; ``relink_parts`` [(track_id, first frame, last
    frame) per fragment]; ``relink_costs`` [the cost of each link taken]."""
    from .sequences import new_record
    n = len(tracklets)
    if n == 0:
        return []
    by = np.lexsort((pos, head))                 # nodes chain after chain (heads ascending), each in time order
    starts = np.flatnonzero(np.r_[True, head[by][1:] != head[by][:-1]])
    bounds = np.r_[starts, n]
    out = []
    for a, b in zip(bounds[:-1], bounds[1:]):
        parts = [tracklets[order[k]] for k in by[a:b]]
        frames, poses = [], []
        for t in parts:
            frames += list(t.frame_idxs)
            poses += list(t.poses)
        t = new_record(parts[0].track_id, poses, parts[-1], frame_idxs=frames, hits=len(poses))
        t.relink_parts = [(p.track_id, int(p.frame_idxs[0]), int(p.frame_idxs[-1])) for p in parts]
        t.relink_costs = [float(cost[k]) for k in by[a:b - 1]]
        out.append(t)
    return sorted(out, key=lambda t: -len(t))


def relink_sequences(tracklets_per_sequence: Sequence[list], max_gap: int = MAX_GAP, max_dist: float = MAX_DIST,
                     near_dist: float = NEAR_DIST, speed: float = SPEED, device="cuda:0", timings: Optional[dict] = None,
                     links: Optional[list] = None) -> List[list]:
    """Join the records of one person, per sequence: MvTracklet records (track_sequences, run_main_batched, MvTracker.update_4d:
    tracker.tracklets + tracker.dead_tracklets) -> per sequence NEW records, longest first (merge_records; the inputs are not
    touched).  Attributes of later stages (bone_lens, fit_*, smooth_*) are not carried: re-link first, then fit.
    ValueError before any device work: frame indices that do not increase, max_gap < 1, non-finite or negative max_dist / near_dist /
    speed, joints that are not 18 x 3, more than MAX_RECORDS records in one sequence.
    timings: a dict that receives the seconds spent in {"pack", "launch" (upload, kernel, read-back), "records"}.
    links: a list that receives, per sequence, dict(order, succ, head, pos, cost) over its nodes (node k = input record order[k])."""
    t0 = time.perf_counter()
    check_parameters(max_gap, max_dist, near_dist, speed)
    packed = pack_records(tracklets_per_sequence)
    t1 = time.perf_counter()
    solved = solve_links(packed, max_gap, max_dist, near_dist, speed, device) if packed["rec"].shape[0] else \
        [dict(succ=np.zeros(0, np.int64), head=np.zeros(0, np.int64), pos=np.zeros(0, np.int64), cost=np.zeros(0))
         for _ in tracklets_per_sequence]
    t2 = time.perf_counter()
    out = [merge_records(list(tl), o, r["head"], r["pos"], r["cost"])
           for tl, o, r in zip(tracklets_per_sequence, packed["order"], solved)]
    if links is not None:
        links.extend(dict(r, order=o) for o, r in zip(packed["order"], solved))
    if timings is not None:
        timings.update(pack=t1 - t0, launch=t2 - t1, records=time.perf_counter() - t2)
    return out


def relink_tracklets(tracklets: list, max_gap: int = MAX_GAP, max_dist: float = MAX_DIST, near_dist: float = NEAR_DIST,
                     speed: float = SPEED, device="cuda:0", timings: Optional[dict] = None, links: Optional[list] = None) -> list:
    """relink_sequences for the records of one sequence."""
    return relink_sequences([tracklets], max_gap=max_gap, max_dist=max_dist, near_dist=near_dist, speed=speed, device=device,
                            timings=timings, links=links)[0]
