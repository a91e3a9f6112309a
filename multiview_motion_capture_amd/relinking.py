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

RE-IDENTIFICATION (track -> re-link -> RE-IDENTIFY -> fit -> smooth -> BVH; opt-in).  Re-linking follows motion across at most max_gap
frames; reidentify_sequences() joins the records of a person who was hidden for longer, or left and came back, from the bone lengths
that the 18 x 3 joints of every appended pose carry.  Per sequence, with the same nodes and the same choice:

  signature  from the joints of ALL poses of a record.  Per pose and bone j = 1 .. 17: b_j = sqrt(dx dx + dy dy + dz dz) of joint j
             minus joint SKEL_PARENTS[j].  Ten sides, the values 0 - 6 and 8 - 10 of SKEL_SIDE_MAP (7 is the root and has no bone):
             sides 0 - 6 have a left and a right bone and the value (b_lo + b_hi) / 2 in joint order, sides 8, 9, 10 one bone; a pose
             gives a side a value only when all its bones are finite.  Per side with m values: med = the lower median (rank
             (m - 1) // 2 in ascending order), mad = the lower median of |x - med|, se = 1.4826 mad 1.2533 / sqrt(m) in that order; a
             side with m < min_poses is undefined (NaN).  Both medians are exact selections: the order of the values does not matter;
  distance   z(A, B) = sqrt(mean over the sides defined in both of (l_A - l_B)^2 / (se_A^2 + se_B^2 + 2 floor^2)), summed in side
             order; undefined with fewer than 5 sides defined in both;
  candidate  A -> B when A != B, gap = B.first - A.last >= 1 (and <= max_gap when given), z defined and <= max_z, and |centroid of
             B's first pose - centroid of A's last pose| <= reach + speed gap (the mean of the 18 joints; a non-finite distance
             allows nothing).  reach and speed are physical bounds (1 m, 2 m/s at 25 frames/s), a choice, not tuned;
  veto       Q and R overlap when Q.first <= R.last and R.first <= Q.last: a record that overlaps another in time is certainly
             someone else.  A -> B is refused when another record Q overlaps B but not A and z(A, B) > ratio z(A, Q), or overlaps A
             but not B and z(A, B) > ratio z(Q, B).  An undefined z vetoes nothing; a Q that overlaps both ends does not compete for
             the link and vetoes nothing (a twin who is present throughout must not stop the other twin from coming back);
  choice     as above: the n x 2n matrix holds z where allowed and RL_BIG elsewhere, max_z in a row's dummy column; Kuhn-Munkres
             with potentials, rows in node order, the first minimum wins; then chains.

It joins no records that overlap in time, reads no appearance, and does nothing across sequences.  Two people whose skeletons agree
within the noise are not told apart (the veto refuses them), and a duplicate identity that overlaps the returning record vetoes
conservatively: such links are missed, never wrong.  A joined record keeps its hole; smooth_sequences(fill_gaps=True) would fill a long
one with invented motion, so pass fill_gaps=False for such records.
Device code: csrc/mvmc_relink.hip (mvmc_reid_signature: one workgroup per record, the only part that reads every pose; mvmc_reid_link:
one workgroup per sequence, the assignment and the chains are mvmc_relink's own instructions); NumPy restatement: tests/reid_np.py.
The defaults: tools/reid_sweep.py (profiles/reid_sweep.json).
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


def _frames(t, where):
    """A record's frame indices after the checks every pack makes."""
    fr = np.asarray(t.frame_idxs, dtype=np.int64)
    m = fr.shape[0] if fr.ndim == 1 else 0
    if fr.ndim != 1 or m == 0 or len(t.poses) != m:
        raise ValueError(f"{where}: {fr.shape} frame indices and {len(t.poses)} poses")
    if np.any(np.diff(fr) <= 0):
        raise ValueError(f"{where}: frame indices must increase")
    if fr[0] < -2 ** 30 or fr[-1] >= 2 ** 30:
        raise ValueError(f"{where}: frame indices outside 32 bits")
    return fr


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
            fr = _frames(t, where)
            m = fr.shape[0]
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
    out = []
    for t, parts, nodes in _joined(tracklets, order, head, pos):
        t.relink_parts = [(p.track_id, int(p.frame_idxs[0]), int(p.frame_idxs[-1])) for p in parts]
        t.relink_costs = [float(cost[k]) for k in nodes[:-1]]
        out.append(t)
    return sorted(out, key=lambda t: -len(t))


def _joined(tracklets: list, order: np.ndarray, head: np.ndarray, pos: np.ndarray):
    """Per chain of links, heads ascending: (the NEW record of the chain, its parts in time order, their nodes)."""
    from .sequences import new_record
    n = len(tracklets)
    if n == 0:
        return
    by = np.lexsort((pos, head))                 # nodes chain after chain (heads ascending), each in time order
    starts = np.flatnonzero(np.r_[True, head[by][1:] != head[by][:-1]])
    bounds = np.r_[starts, n]
    for a, b in zip(bounds[:-1], bounds[1:]):
        parts = [tracklets[order[k]] for k in by[a:b]]
        frames, poses = [], []
        for t in parts:
            frames += list(t.frame_idxs)
            poses += list(t.poses)
        yield new_record(parts[0].track_id, poses, parts[-1], frame_idxs=frames, hits=len(poses)), parts, by[a:b]


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


# ---- re-identification by bone lengths (the module docstring has the statement) ----
MAX_Z, RATIO, FLOOR, MIN_POSES = 2.0, 0.7, 0.004, 10     # tools/reid_sweep.py (profiles/reid_sweep.json); floor started at 0.002
REACH, REID_SPEED = 1.0, 0.08                            # metres, metres per frame of gap: 2 m/s at 25 frames/s; physical bounds, not tuned
MAX_POSES = 65536                                        # include/mvmc.h: MVMC_REID_MAX_POSES (poses of one record)
_LDS_POSES = 512                                         # include/mvmc.h: MVMC_REID_LDS_POSES


def check_reid_parameters(max_z, ratio, floor, min_poses, reach, speed, max_gap=None) -> None:
    for name, x in (("max_z", max_z), ("ratio", ratio), ("floor", floor), ("reach", reach), ("speed", speed)):
        x = float(x)
        if not math.isfinite(x) or x < 0 or x >= 1e6:
            raise ValueError(f"reidentify: {name} must be finite, >= 0 and below 1e6")
    if float(ratio) > 1:
        raise ValueError("reidentify: ratio must be <= 1")
    if isinstance(min_poses, bool) or int(min_poses) != min_poses or not 1 <= int(min_poses) < 2 ** 30:
        raise ValueError("reidentify: min_poses must be an integer >= 1")
    if max_gap is not None and (isinstance(max_gap, bool) or int(max_gap) != max_gap or not 1 <= int(max_gap) < 2 ** 30):
        raise ValueError("reidentify: max_gap must be None or an integer >= 1")


def pack_reid(tracklets_per_sequence: Sequence[list]) -> dict:
    """The host arrays of the two launches (include/mvmc.h: mvmc_reid_signature, mvmc_reid_link) after pack_records' input checks:
    joints (n_poses,18,3) f64 -- every pose of every record, read ONCE, records in node order --, rec (N,2) i32, frames (N,2) i32, seq
    (S,4) i32, the two workspaces' words, and per sequence ``order`` as in pack_records."""
    orders, blocks, recs, frs, counts = [], [], [], [], []
    row = 0
    for s, tl in enumerate(tracklets_per_sequence):
        n = len(tl)
        if n > MAX_RECORDS:
            raise ValueError(f"sequence {s}: {n} records, at most {MAX_RECORDS} per sequence")
        first, last, tid = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
        js = []
        for j, t in enumerate(tl):
            where = f"sequence {s}, record {j}"
            fr = _frames(t, where)
            if fr.shape[0] > MAX_POSES:
                raise ValueError(f"{where}: {fr.shape[0]} poses, at most {MAX_POSES} per record")
            try:
                J = np.array([p[2].keypoints for p in t.poses], dtype=np.float64)
            except (AttributeError, TypeError, IndexError, ValueError):
                J = None
            if J is None or J.shape != (fr.shape[0], 18, 3):
                J = np.array([_joints(p, where) for p in t.poses])
            first[j], last[j], tid[j] = fr[0], fr[-1], int(t.track_id)
            js.append(J)
        order = np.lexsort((tid, first))
        orders.append(order)
        counts.append(n)
        for k in order:
            recs.append((row, js[k].shape[0]))
            frs.append((first[k], last[k]))
            blocks.append(js[k])
            row += js[k].shape[0]
    if row >= 2 ** 31 // 54:
        raise ValueError("reidentify: too many poses in one call; pass fewer sequences per call")
    counts = np.array(counts, dtype=np.int64)
    N, S = int(counts.sum()), len(orders)
    joints = np.concatenate(blocks) if blocks else np.zeros((0, 18, 3))
    rec = np.array(recs, dtype=np.int32).reshape(N, 2)
    frames = np.array(frs, dtype=np.int32).reshape(N, 2)
    work = np.where(counts > _LDS_N, 2 * counts * counts, 0)
    if int(work.sum()) >= 2 ** 31:
        raise ValueError("reidentify: the matrices of one call exceed 2^31 words; pass fewer sequences per call")
    seq = np.zeros((S, 4), np.int32)
    seq[:, 0] = np.concatenate([[0], np.cumsum(counts)[:-1]]) if S else 0
    seq[:, 1] = counts
    seq[:, 2] = np.concatenate([[0], np.cumsum(work)[:-1]]) if S else 0
    sig_words = 10 * row if N and int(rec[:, 1].max()) > _LDS_POSES else 0
    return dict(joints=joints, rec=rec, frames=frames, seq=seq, order=orders, sig_work_words=sig_words, work_words=int(work.sum()))


def solve_reid(packed: dict, max_z: float, ratio: float, floor: float, min_poses: int, reach: float, speed: float,
               max_gap: Optional[int] = None, device="cuda:0", events: Optional[dict] = None) -> List[dict]:
    """ONE upload, two launches, one read-back on the current stream: per sequence dict(succ, head, pos (n) i64, cost (n) f64: the z
    of the link taken, sig (n,20), cnt (n,10), ends (n,6)) over its nodes.  events: a dict that receives the milliseconds of the parts
    {"upload_ms", "signature_ms", "link_ms" (the two launches by device events), "readback_ms"}; this synchronises between them."""
    import ctypes

    import torch

    from . import _cabi
    from .device import _stream
    joints, rec, frames, seq = packed["joints"], packed["rec"], packed["frames"], packed["seq"]
    n_poses, N, S = joints.shape[0], rec.shape[0], seq.shape[0]
    if S == 0:
        return []
    d = torch.device(device)
    lib = _cabi.load()
    # the upload: joints | rec, frames, seq as 4-byte words; the read-back: sig | ends | link_cost | cnt, record status, succ, head,
    # pos, sequence status as 4-byte words
    n_j = n_poses * 54
    up = np.empty(n_j + 2 * N + 2 * S, dtype=np.float64)
    up[:n_j] = joints.reshape(-1)
    up_i = up.view(np.int32)
    up_i[2 * n_j:2 * n_j + 2 * N] = rec.reshape(-1)
    up_i[2 * n_j + 2 * N:2 * n_j + 4 * N] = frames.reshape(-1)
    up_i[2 * n_j + 4 * N:] = seq.reshape(-1)
    with torch.cuda.device(d):
        t0 = time.perf_counter()
        up_d = torch.from_numpy(up).to(d)
        if events is not None:
            torch.cuda.synchronize()
            events["upload_ms"] = 1e3 * (time.perf_counter() - t0)
        out_d = torch.empty((27 * N + (14 * N + S + 1) // 2,), dtype=torch.float64, device=d)
        work_s = torch.empty((max(1, packed["sig_work_words"]),), dtype=torch.float64, device=d)
        work_l = torch.empty((max(1, packed["work_words"]),), dtype=torch.float64, device=d)
        vp = ctypes.c_void_p
        b_up, b_out = up_d.data_ptr(), out_d.data_ptr()
        p_rec = b_up + 8 * n_j
        p_sig, p_ends, p_cost, o_i = b_out, b_out + 8 * 20 * N, b_out + 8 * 26 * N, b_out + 8 * 27 * N
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)] if events is not None else None
        if ev:
            ev[0].record()
        if N:
            _cabi.check(lib.mvmc_reid_signature(vp(b_up), vp(p_rec), n_poses, N, int(min_poses), vp(p_sig), vp(o_i), vp(p_ends),
                                                vp(o_i + 40 * N), vp(work_s.data_ptr()), ctypes.c_longlong(packed["sig_work_words"]),
                                                _stream()), "mvmc_reid_signature")
        if ev:
            ev[1].record()
        _cabi.check(lib.mvmc_reid_link(vp(p_sig), vp(p_ends), vp(p_rec + 8 * N), vp(p_rec + 16 * N), N, S, int(max_gap or 0),
                                       float(max_z), float(ratio), float(floor), float(reach), float(speed), vp(o_i + 44 * N),
                                       vp(o_i + 48 * N), vp(o_i + 52 * N), vp(p_cost), vp(o_i + 56 * N), vp(work_l.data_ptr()),
                                       ctypes.c_longlong(packed["work_words"]), _stream()), "mvmc_reid_link")
        if ev:
            ev[2].record()
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = out_d.cpu().numpy()
        if ev:
            events.update(signature_ms=ev[0].elapsed_time(ev[1]), link_ms=ev[1].elapsed_time(ev[2]),
                          readback_ms=1e3 * (time.perf_counter() - t0))
    sig, ends, cost = out[:20 * N].reshape(N, 20), out[20 * N:26 * N].reshape(N, 6), out[26 * N:27 * N]
    ints = out[27 * N:].view(np.int32)
    cnt = ints[:10 * N].reshape(N, 10)
    if np.any(ints[10 * N:11 * N] != 0):
        raise RuntimeError("reidentify: a record's poses do not fit the launch (record status 2)")
    status = ints[14 * N:14 * N + S]
    if np.any(status == 2):
        raise RuntimeError("reidentify: a sequence's records do not fit the launch (status 2)")
    if np.any(status != 0):
        raise RuntimeError("reidentify: an assignment did not terminate (sequence %d)" % int(np.flatnonzero(status)[0]))
    res = []
    for s in range(S):
        a, n = int(seq[s, 0]), int(seq[s, 1])
        res.append(dict(succ=ints[11 * N + a:11 * N + a + n].astype(np.int64), head=ints[12 * N + a:12 * N + a + n].astype(np.int64),
                        pos=ints[13 * N + a:13 * N + a + n].astype(np.int64), cost=cost[a:a + n].copy(), sig=sig[a:a + n].copy(),
                        cnt=cnt[a:a + n].astype(np.int64), ends=ends[a:a + n].copy()))
    return res


def merge_reid_records(tracklets: list, order: np.ndarray, res: dict) -> list:
    """One sequence's records and its re-identification links -> NEW MvTracklet records, longest first, built as merge_records builds
    them.  ``reid_parts`` [(track_id, first frame, last frame) of every input record joined, in time order]; ``reid_costs`` [the z of
    each link taken]; ``reid_lengths`` / ``reid_sigma`` (10,) metres: the signature and its standard error (NaN: undefined side) -- of
    a joined record, those of its part with the most poses (the earliest among equals); ``relink_parts`` / ``relink_costs`` of the
    parts concatenated in time order when every part has them."""
    out = []
    for t, parts, nodes in _joined(tracklets, order, res["head"], res["pos"]):
        t.reid_parts = [(p.track_id, int(p.frame_idxs[0]), int(p.frame_idxs[-1])) for p in parts]
        t.reid_costs = [float(res["cost"][k]) for k in nodes[:-1]]
        k = nodes[int(np.argmax([len(p.poses) for p in parts]))]
        t.reid_lengths, t.reid_sigma = res["sig"][k, :10].copy(), res["sig"][k, 10:].copy()
        if all(hasattr(p, "relink_parts") and hasattr(p, "relink_costs") for p in parts):
            t.relink_parts = [x for p in parts for x in p.relink_parts]
            t.relink_costs = [x for p in parts for x in p.relink_costs]
        out.append(t)
    return sorted(out, key=lambda t: -len(t))


def reidentify_sequences(tracklets_per_sequence: Sequence[list], max_z: float = MAX_Z, ratio: float = RATIO, floor: float = FLOOR,
                         min_poses: int = MIN_POSES, reach: float = REACH, speed: float = REID_SPEED, max_gap: Optional[int] = None,
                         device="cuda:0", timings: Optional[dict] = None, links: Optional[list] = None) -> List[list]:
    """Join the records of one person across long holes by their bone lengths, per sequence (the module docstring has the statement):
    MvTracklet records, usually relink_sequences' -> per sequence NEW records, longest first (merge_reid_records; the inputs are not
    touched, the result does not depend on the order of the caller's lists).  Attributes of later stages are not carried.
    ValueError before any device work: what relink_sequences refuses, a record of more than MAX_POSES poses, max_z / ratio / floor /
    reach / speed non-finite or negative, ratio > 1, min_poses < 1, max_gap < 1.
    timings: a dict that receives the seconds spent in {"pack", "launch" (upload, two launches, read-back), "records"}.
    links: a list that receives, per sequence, dict(order, succ, head, pos, cost, sig, cnt, ends) over its nodes."""
    t0 = time.perf_counter()
    check_reid_parameters(max_z, ratio, floor, min_poses, reach, speed, max_gap)
    packed = pack_reid(tracklets_per_sequence)
    t1 = time.perf_counter()
    if packed["rec"].shape[0]:
        solved = solve_reid(packed, max_z, ratio, floor, min_poses, reach, speed, max_gap, device)
    else:
        solved = [dict(succ=np.zeros(0, np.int64), head=np.zeros(0, np.int64), pos=np.zeros(0, np.int64), cost=np.zeros(0),
                       sig=np.zeros((0, 20)), cnt=np.zeros((0, 10), np.int64), ends=np.zeros((0, 6))) for _ in tracklets_per_sequence]
    t2 = time.perf_counter()
    out = [merge_reid_records(list(tl), o, r) for tl, o, r in zip(tracklets_per_sequence, packed["order"], solved)]
    if links is not None:
        links.extend(dict(r, order=o) for o, r in zip(packed["order"], solved))
    if timings is not None:
        timings.update(pack=t1 - t0, launch=t2 - t1, records=time.perf_counter() - t2)
    return out


def reidentify_tracklets(tracklets: list, max_z: float = MAX_Z, ratio: float = RATIO, floor: float = FLOOR, min_poses: int = MIN_POSES,
                         reach: float = REACH, speed: float = REID_SPEED, max_gap: Optional[int] = None, device="cuda:0",
                         timings: Optional[dict] = None, links: Optional[list] = None) -> list:
    """reidentify_sequences for the records of one sequence."""
    return reidentify_sequences([tracklets], max_z=max_z, ratio=ratio, floor=floor, min_poses=min_poses, reach=reach, speed=speed,
                                max_gap=max_gap, device=device, timings=timings, links=links)[0]
