"""Detections with exchanged left / right limbs, repaired at the door: an offline stage on finished tracklet records.

A detector's typical failure is a detection whose arms, legs or face are labelled left for right.  Such a detection is not an outlier:
its keypoints are well measured and filed under the wrong names.  Once a 3-D pose of the person is known, the permutation can be
decided per (frame, camera, person, limb group) and undone in the keypoints, before any stage reads them -- where
lens.undistort_sequences fixes pixels.  repair_sequences() takes the sequences track_sequences takes and records of any stage (the
intended source: smoothing.smooth_sequences(loss="cauchy")) and returns the sequences with repaired keypoint arrays:

    track -> fit -> smooth(loss) -> REPAIR -> track again -> ...

The rule (restated in tests/exchange_np.py, which is its definition; include/mvmc.h: mvmc_exchange_observe, mvmc_exchange_apply):
  groups    as COCO-17 pairs: arms (5,6) (7,8) (9,10), legs (11,12) (13,14) (15,16), face (3,4): the pairs among reprojection_error's 15
            common joints.  The eyes (1,2) follow the face; in BODY_25 input every pair maps through OPENPOSE25_TO_COCO17 and the feet
            (19,20,21) <-> (22,23,24) follow the legs;
  costs     a problem is one (record, record frame); its joints are projected with the sequence's P.  For a pose of that frame in a
            camera, over the group's pairs with BOTH keypoints above min_score: e0 the sum of pixel distances under the labels as they
            are, e1 under the exchanged labels, n_g the keypoints counted;
  selection d* = (as-is distances of the valid keypoints outside such pairs + sum_g min(e0, e1)) / (valid common keypoints); per
            (problem, camera) the pose with the smallest finite d* < max_dist (ties: the lower slot), then mvmc_body_observe's conflict
            rule.  Where no group prefers the exchange this is body_fit's selection; a whole-body flip, whose as-is distance lies
            beyond max_dist, is selected here and repaired;
  decision  group g of the selected pose is exchanged iff n_g >= 2 and e1 + margin_px n_g < e0 and e1 < ratio e0 (both strict);
  apply     an exchanged group swaps the whole (x, y, score) triples of its pairs, the followers included; every other byte is copied.

What it is not: there is no temporal vote (every detection is decided on its own); it is as good as the records it is given (INTEGRATION.md
section C.10 has the measured recall per record source); it does nothing for LivePool / LiveSmoother; and a single keypoint put on its
neighbour is not an exchange -- that stays the robust loss's job.

Sequences with the same number of cameras share one launch sequence, each with its own rig.  The host front end is sequences.py's
(check_records, plan_groups, stack_group, problem_tables, stopwatch), as for body_fit and smoothing.
"""
from __future__ import annotations

import math
import time
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .body_fit import MAX_DIST, MIN_SCORE
from .sequences import SequenceInput, check_records, no_sequences, plan_groups, problem_tables, stack_group, stopwatch

MARGIN_PX = 4.0     # the exchange must win by this many pixels per keypoint counted ...
RATIO = 0.7         # ... and cost less than this share of the labels as they are
ARMS, LEGS, FACE = 1, 2, 4      # the flag bits
GROUPS = ("arms", "legs", "face")

OPENPOSE25_TO_COCO17 = (0, 16, 15, 18, 17, 5, 2, 6, 3, 7, 4, 12, 9, 13, 10, 14, 11)
_PAIRS17 = {ARMS: ((5, 6), (7, 8), (9, 10)), LEGS: ((11, 12), (13, 14), (15, 16)), FACE: ((1, 2), (3, 4))}
_FEET25 = ((19, 22), (20, 23), (21, 24))
# mvmc_ingest's filter_bad_pose (motion_capture.py:1023-1043), which decides the pose slots the selection sees
_INGEST_MIN_SCORE, _INGEST_MIN_VALID, _INGEST_MIN_BB = 0.01, 4, 5.0


def group_pairs(n_joints: int) -> dict:
    """flag bit -> the (left, right) keypoint rows an exchange of that group swaps, for COCO-17 or BODY_25 rows."""
    if n_joints == 17:
        return {b: tuple(p) for b, p in _PAIRS17.items()}
    if n_joints != 25:
        raise ValueError(f"group_pairs: 17 or 25 keypoint rows, got {n_joints}")
    m = OPENPOSE25_TO_COCO17
    out = {b: tuple((m[l], m[r]) for l, r in p) for b, p in _PAIRS17.items()}
    out[LEGS] = out[LEGS] + _FEET25
    return out


def apply_flags(kps: np.ndarray, flags: np.ndarray) -> np.ndarray:
    """The repaired copy of kps (..., 25|17, 3) on the host: flags (...) u8, bit 0 arms, 1 legs, 2 face -- what mvmc_exchange_apply
    writes, bit for bit (a pure permutation of every pose's triples)."""
    kps = np.asarray(kps)
    flags = np.asarray(flags)
    if kps.ndim < 2 or kps.shape[-1] != 3 or flags.shape != kps.shape[:-2]:
        raise ValueError(f"apply_flags: kps (...,25|17,3) and flags (...), got {kps.shape} and {flags.shape}")
    out = kps.copy()
    for bit, pairs in group_pairs(kps.shape[-2]).items():
        hit = (flags & bit) != 0
        if not hit.any():
            continue
        for l, r in pairs:
            out[..., l, :][hit] = kps[..., r, :][hit]
            out[..., r, :][hit] = kps[..., l, :][hit]
    return out


def ingest_slots(kps: np.ndarray, counts: np.ndarray) -> np.ndarray:
    """kps (F,C,P,25|17,3), counts (F,C) -> (F,C,P) i32: the caller's slot behind every slot of the ingested keypoints (mvmc_ingest
    drops the poses filter_bad_pose refuses and closes the gaps, order kept), -1 where the ingested view has no pose."""
    k = np.asarray(kps)
    rows = list(OPENPOSE25_TO_COCO17) if k.shape[3] == 25 else slice(None)
    F, C, P = k.shape[:3]
    with np.errstate(invalid="ignore"):
        # (the kernel's tests run in float64; minima and maxima are exact in the array's own dtype, so only they are widened)
        valid = k[..., rows, 2].astype(np.float64) > _INGEST_MIN_SCORE
        size = []
        for a in (0, 1):
            x = np.where(valid, k[..., rows, a], np.nan)
            lo = np.fmin.reduce(x, axis=-1, initial=np.inf).astype(np.float64)
            hi = np.fmax.reduce(x, axis=-1, initial=-np.inf).astype(np.float64)
            size.append(hi - lo)
        keep = (valid.sum(-1) >= _INGEST_MIN_VALID) & ~((size[0] < _INGEST_MIN_BB) | (size[1] < _INGEST_MIN_BB))
    keep &= np.arange(P)[None, None, :] < np.asarray(counts)[:, :, None]
    dest = np.cumsum(keep, axis=-1) - 1
    out = -np.ones((F, C, P), dtype=np.int32)
    f, c, p = np.nonzero(keep)
    out[f, c, dest[f, c, p]] = p
    return out


def _check(sequences, tracklets_per_sequence, margin_px, ratio, max_dist, min_score):
    def number(v, name):
        if isinstance(v, (bool, np.bool_, str)) or not np.isscalar(v) or not np.isreal(v):
            raise ValueError(f"repair_sequences: {name} must be a number, got {v!r}")
        return float(v)

    def own():
        m, r = number(margin_px, "margin_px"), number(ratio, "ratio")
        if not (math.isfinite(m) and m >= 0.0):
            raise ValueError(f"repair_sequences: margin_px must be finite and >= 0, got {margin_px}")
        if not 0.0 < r <= 1.0:
            raise ValueError(f"repair_sequences: ratio must lie in (0, 1], got {ratio}")
        if math.isnan(number(max_dist, "max_dist")) or math.isnan(number(min_score, "min_score")):
            raise ValueError("repair_sequences: max_dist and min_score must not be NaN")
    return check_records(sequences, tracklets_per_sequence, "repair_sequences", own)


def _empty_report(F: int, C: int, P: int) -> dict:
    return dict(flags=np.zeros((F, C, P), np.uint8), record=-np.ones((F, C, P), np.int32), cost=np.full((F, C, P, 3, 2), np.nan),
                exchanged={g: 0 for g in GROUPS})


def repair_sequences(sequences: Sequence[SequenceInput], tracklets_per_sequence: Sequence[list], margin_px: float = MARGIN_PX,
                     ratio: float = RATIO, max_dist: float = MAX_DIST, min_score: float = MIN_SCORE, device="cuda:0",
                     timings: Optional[dict] = None) -> Tuple[List[SequenceInput], List[dict]]:
    """Undo the left / right exchanges of every sequence's detections -- (kps (F_s,C,P_s,25|17,3), counts (F_s,C), one Calib per
    camera), the rows track_sequences takes -- against its records (of the tracker, body_fit or smoothing: only frame_idxs and the
    18 x 3 joints are read).  Returns (repaired, report): the same tuples with NEW keypoint arrays of the same shape, dtype and keypoint
    format (the inputs are not touched; counts and calibs are the same objects), and per sequence a dict of, in the caller's pose slots,
      flags (F,C,P) u8     bit 0 arms, bit 1 legs, bit 2 face exchanged (and undone in the result);
      record (F,C,P) i32   the record (position in the sequence's list) that selected the slot, or -1;
      cost (F,C,P,3,2) f64 the as-is and the exchanged cost of each group in pixels, NaN where undecided;
      exchanged            {"arms", "legs", "face"} -> the number of exchanges.
    timings: a dict that receives the seconds spent in {"pack", "observe", "report", "apply", "read_back"} (synchronising between the
    parts): stacking, upload and ingest; the selection launches; their tables read back and scattered to the pose slots; the apply
    launch; the repaired keypoints read back."""
    if no_sequences(sequences, tracklets_per_sequence, "repair_sequences"):
        return [], []
    shapes, recs = _check(sequences, tracklets_per_sequence, margin_px, ratio, max_dist, min_score)
    import torch

    from . import device as dev
    d = torch.device(device)
    T = dev.uploader(d)
    lap, tm = stopwatch(timings, d, ("pack", "observe", "report", "apply", "read_back"))
    repaired: List[Optional[tuple]] = [None] * len(sequences)
    report = [_empty_report(*s) for s in shapes]
    for lay in plan_groups(shapes, 1):
        if lay.total_chains == 0 or not any(recs[i] for i in lay.seq_ids):
            continue
        t0 = time.perf_counter()
        grp = stack_group(lay, sequences)
        sel = problem_tables(grp, recs)
        kps_d = T(grp.kps)
        k17, c17 = dev.ingest(kps_d, T(grp.cnt))
        args = (k17, c17, T(grp.Pm), T(sel.frame_of), T(sel.rig_of), T(sel.joints), T(sel.order), T(sel.lo), T(sel.hi), T(sel.rank))
        t0 = lap("pack", t0)
        mem_d, _, fl_d, cost_d = dev.exchange_observe(*args, max_dist, min_score, margin_px, ratio)
        t0 = lap("observe", t0)
        mem, fl, cost = mem_d.cpu().numpy().astype(np.int64), fl_d.cpu().numpy(), cost_d.cpu().numpy()
        C, Pg = grp.n_views, grp.Pg
        src_of = ingest_slots(grp.kps, grp.cnt)
        b, c = np.nonzero(mem >= 0)
        q = mem[b, c]
        f, k = q // (C * Pg), q % Pg
        p = src_of[f, c, k]
        if p.size and p.min() < 0:
            raise RuntimeError("repair_sequences: a selected pose has no slot in the caller's keypoints")
        slot_flags = np.zeros((grp.kps.shape[0], C, Pg), np.uint8)
        slot_flags[f, c, p] = fl[b, c]
        for r, i in enumerate(lay.seq_ids):
            m = sel.rig_of[b] == r
            fs = f[m] - int(grp.f_off[r])
            rep = report[i]
            rep["flags"][fs, c[m], p[m]] = fl[b[m], c[m]]
            rep["record"][fs, c[m], p[m]] = sel.rank[b[m]]
            rep["cost"][fs, c[m], p[m]] = cost[b[m], c[m]]
            rep["exchanged"] = {g: int(np.count_nonzero(rep["flags"] & (1 << n))) for n, g in enumerate(GROUPS)}
        t0 = lap("report", t0)
        out_d = dev.exchange_apply(kps_d, T(slot_flags))
        t0 = lap("apply", t0)
        out = out_d.cpu().numpy()
        for r, i in enumerate(lay.seq_ids):
            src = np.asarray(sequences[i][0])
            part = out[int(grp.f_off[r]):int(grp.f_off[r + 1]), :, :src.shape[2]]
            repaired[i] = (part.astype(src.dtype, copy=True), sequences[i][1], sequences[i][2])
        lap("read_back", t0)
    for i, seq in enumerate(sequences):
        if repaired[i] is None:           # no frames, or no record in the sequence's whole group: nothing to decide
            repaired[i] = (np.array(seq[0], copy=True), seq[1], seq[2])
    if timings is not None:
        timings.update(tm)
    return repaired, report


def repair_tracklets(tracklets: list, kps: np.ndarray, counts: np.ndarray, calibs: list, margin_px: float = MARGIN_PX,
                     ratio: float = RATIO, max_dist: float = MAX_DIST, min_score: float = MIN_SCORE, device="cuda:0",
                     timings: Optional[dict] = None):
    """repair_sequences for one sequence: records of kps (F,C,P,25|17,3), counts (F,C) and one Calib per camera -> ((kps, counts,
    calibs) repaired, its report)."""
    rep, info = repair_sequences([(kps, counts, calibs)], [tracklets], margin_px=margin_px, ratio=ratio, max_dist=max_dist,
                                 min_score=min_score, device=device, timings=timings)
    return rep[0], info[0]
