"""Calibrate each rig's extrinsics from one person walking the capture volume: the first step for cameras that only have intrinsics.

Every other stage takes the rig as given, and rig_refine.refine_rigs needs a rig good enough to track with.  calibrate_rigs() needs
no target: ONE person walks through the volume alone, so the same joint seen by two views is a correspondence without any
association.  The walk must COVER the volume: a person who wanders 0.2 m around one spot is near-degenerate for the two-view fit
(errors of several degrees); four or five places a few metres apart are enough.

  1. observations: a view contributes a frame only where counts[f, c] == 1 (frames with several people are ignored); its 17 ingested
     joints with score > ``min_score`` in normalised coordinates K^-1 (u, v, 1), skew included;
  2. mvmc_pair_moments: per camera pair the Hartley normalisation and per frame the moment matrix of its epipolar rows;
  3. mvmc_pair_consensus (the hot path): ``hypotheses`` essential matrices per pair, each from the moments of ``sample_frames`` whole
     frames (a minimal sample of 8 single joints fails at 2 px noise) named by a host table of np.random.default_rng(seed), each
     scored by the correspondences within ``inlier_px`` (Sampson);
  4. mvmc_pair_refit: the best hypothesis, ``refit_rounds`` refits over its inliers (the refit with the most inliers is kept; the
     hypothesis itself only when the refits lost more than a tenth of its inliers), the (R, t) that puts the triangulated inliers
     in front of both cameras, and those points;
  5. pose graph (host): Prim's maximum spanning tree from camera 0 over the pairs with >= ``min_pair_inliers`` inliers; the scale of
     every edge after the first from the median ratio of the depths two edges give the same points; composition;
  6. polish: rig_refine's bundle adjustment (camera 0 held) on the walk's own points, a (frame, joint) that >= 2 views see; by
     default plain least squares behind the ``polish_px`` gate, with ``polish_loss="huber" | "cauchy"`` rig_refine's robust loss at
     ``polish_loss_px`` pixels, which keeps detections with exchanged limbs that pass the gate from pulling on the rig; with
     ``polish_intrinsics="focal" | "focal+centre"`` rig_refine's intrinsic unknowns with their prior (``polish_focal_sigma``,
     ``polish_centre_sigma_px``) for a K that is only nominal -- the pair stage keeps the nominal K, and with two cameras the polish
     is skipped as without it, so no intrinsic is estimated there;
  7. metric scale from ``baseline=(i, j, metres)`` or, without one, from the limb lengths of the default skeleton -- an average-adult
     assumption good to about +-10 %, stated and not measured; ``world="floor"`` turns the result upright: +z the mean direction hips
     -> shoulders, z = 0 at the median of the lower ankle, x camera 0's optical axis along the floor, the origin below camera 0.

It estimates no intrinsics and no distortion (a Calib with a lens is refused: undistort first), uses no frames with several people, is
no live-session path and does no time synchronisation.  Device code: csrc/mvmc_riginit.hip (include/mvmc.h: mvmc_pair_moments,
mvmc_pair_consensus, mvmc_pair_refit) and rig_refine's kernels; NumPy restatement: tests/rig_init_np.py.  Sequences of any frame
and camera counts share the three pair launches; sequences of one camera count share the polish.
"""
from __future__ import annotations

import time
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

from . import body_fit
from .common import Calib
from .rig_refine import LOSS_PX, MAX_CAMS, MAX_ITER_CAP, RigRefinement, check_intrinsics, check_loss, decode, solve_group
from .sequences import stopwatch

MAX_SAMPLE, MAX_ROUNDS = 32, 8            # include/mvmc.h: MVMC_RIGINIT_MAX_SAMPLE, MVMC_RIGINIT_MAX_ROUNDS
MIN_COMMON = 10                           # points two edges must share for a scale
LIMBS = ((5, 7), (7, 9), (6, 8), (8, 10), (11, 13), (13, 15), (12, 14), (14, 16))     # COCO-17: arms, then legs
WORLDS = ("camera0", "floor")


def limb_lengths() -> np.ndarray:
    """Lengths of LIMBS in the default skeleton (device.skeleton_arrays: upper arm, forearm, thigh, shin)."""
    from .device import skeleton_arrays
    side = skeleton_arrays()[1]
    return np.array([side[4], side[5], side[4], side[5], side[1], side[2], side[1], side[2]])


@dataclass
class RigCalibration:
    calibs: Optional[list]           # NEW [Calib] * C (Calib.from_k_rt), None when the rig could not be calibrated
    stop: str                        # "ok" | "few_frames" | "disconnected"
    tree: list                       # the spanning tree's edges (from, to), in the order Prim added them
    pair_inliers: np.ndarray         # (C, C)
    rms_px: float                    # reprojection rms after the polish
    scale_source: Optional[str]      # "baseline" | "limbs"
    polish: Optional[RigRefinement]  # the bundle adjustment's record (camera 0 = [I|0], first tree edge of length 1)
    points: Optional[np.ndarray]     # (F,17,3) the walker's joints in the final world, NaN where there is none


def _cameras(cams, who):
    """Per view (K (3,3), (w, h)) of a Calib (its Rt is ignored) or a (K, (w, h)) pair."""
    from .lens import require_pinhole
    out = []
    for c, cam in enumerate(cams):
        if isinstance(cam, Calib):
            require_pinhole([cam], who)
            K, wh = cam.K, cam.img_wh_size
        else:
            try:
                K, wh = cam
            except (TypeError, ValueError):
                raise ValueError(f"{who}: camera {c} is neither a Calib nor (K, (w, h))")
        K = np.asarray(K, np.float64)
        if K.shape != (3, 3) or not np.isfinite(K).all() or K[0, 0] <= 0 or K[1, 1] <= 0:
            raise ValueError(f"{who}: camera {c}: K must be a finite 3 x 3 matrix with positive focal lengths")
        out.append((K, tuple(wh)))
    return out


def check_calibrate(sequences, hypotheses, sample_frames, inlier_px, min_score, min_pair_inliers, refit_rounds, polish_iter, polish_px,
                    baseline, world, polish_loss=None, polish_loss_px=LOSS_PX, polish_ftol=None, polish_intrinsics=None,
                    polish_focal_sigma=None, polish_centre_sigma_px=None):
    """The input checks of calibrate_rigs, before any device work: ValueError, or (per sequence (F, C, P), cameras, baselines)."""
    check_loss("calibrate_rigs", polish_loss, polish_loss_px, polish_ftol, None)
    check_intrinsics("calibrate_rigs", polish_intrinsics, polish_focal_sigma, polish_centre_sigma_px)
    if len(sequences) == 0:
        raise ValueError("calibrate_rigs: no sequences")
    if not 1 <= int(hypotheses) <= 65535:
        raise ValueError("calibrate_rigs: 1 <= hypotheses <= 65535 required")
    if not 1 <= int(sample_frames) <= MAX_SAMPLE:
        raise ValueError(f"calibrate_rigs: 1 <= sample_frames <= {MAX_SAMPLE} required")
    if not 0 <= int(refit_rounds) <= MAX_ROUNDS:
        raise ValueError(f"calibrate_rigs: 0 <= refit_rounds <= {MAX_ROUNDS} required")
    if not 0 <= int(polish_iter) <= MAX_ITER_CAP:
        raise ValueError(f"calibrate_rigs: 0 <= polish_iter <= {MAX_ITER_CAP} required")
    if not (float(inlier_px) > 0.0 and float(polish_px) > 0.0 and float(min_score) >= 0.0 and int(min_pair_inliers) >= 8):
        raise ValueError("calibrate_rigs: inlier_px > 0, polish_px > 0, min_score >= 0 and min_pair_inliers >= 8 required")
    if world not in WORLDS:
        raise ValueError(f"calibrate_rigs: world is one of {WORLDS}")
    bases = list(baseline) if isinstance(baseline, list) else [baseline] * len(sequences)
    if len(bases) != len(sequences):
        raise ValueError(f"calibrate_rigs: {len(bases)} baselines for {len(sequences)} sequences")
    shapes, cams, joints = [], [], set()
    for s, seq in enumerate(sequences):
        if len(seq) != 3:
            raise ValueError(f"calibrate_rigs: sequence {s}: expected (kps25, counts, cameras)")
        kps, counts = np.asarray(seq[0]), np.asarray(seq[1])
        if kps.ndim != 5 or kps.shape[3] not in (17, 25) or kps.shape[4] != 3:
            raise ValueError(f"calibrate_rigs: sequence {s}: kps25 must be (F,C,P,25|17,3), got {kps.shape}")
        F, C, P = kps.shape[:3]
        joints.add(kps.shape[3])
        if counts.shape != (F, C):
            raise ValueError(f"calibrate_rigs: sequence {s}: counts must be ({F},{C}), got {counts.shape}")
        if F < 1 or P < 1 or not 2 <= C <= MAX_CAMS:
            raise ValueError(f"calibrate_rigs: sequence {s}: at least one frame and person slot and 2 .. {MAX_CAMS} cameras required")
        if counts.size and (counts.min() < 0 or counts.max() > P):
            raise ValueError(f"calibrate_rigs: sequence {s}: counts outside [0, {P}]")
        if len(seq[2]) != C:
            raise ValueError(f"calibrate_rigs: sequence {s}: {len(seq[2])} cameras for {C} views")
        cams.append(_cameras(seq[2], f"calibrate_rigs: sequence {s}"))
        b = bases[s]
        if b is not None:
            if len(b) != 3 or int(b[0]) == int(b[1]) or not (0 <= int(b[0]) < C and 0 <= int(b[1]) < C) or not float(b[2]) > 0.0:
                raise ValueError(f"calibrate_rigs: sequence {s}: baseline is (i, j, metres) with two different cameras and metres > 0")
        shapes.append((F, C, P))
    if len(joints) > 1:
        raise ValueError("calibrate_rigs: OpenPose-25 and COCO-17 keypoints mixed")
    return shapes, cams, bases


def observations(k17, counts, K, min_score):
    """Stage 1.  k17 (F,C,P,17,3) ingested, counts (F,C), K (C,3,3) -> xn (F,C,17,2) normalised coordinates, NaN where not usable;
    px (F,C,17,3) the same keypoints as pixels u, v, score (score 0 where not usable)."""
    k = np.asarray(k17, np.float64)[:, :, 0]
    ok = (np.asarray(counts)[:, :, None] == 1) & (k[..., 2] > min_score)
    y = (k[..., 1] - K[None, :, 1, 2, None]) / K[None, :, 1, 1, None]
    x = (k[..., 0] - K[None, :, 0, 2, None] - K[None, :, 0, 1, None] * y) / K[None, :, 0, 0, None]
    return np.where(ok[..., None], np.stack([x, y], axis=-1), np.nan), np.where(ok[..., None], k, 0.0)


def pair_tables(shapes):
    """shapes [(F, C, ..)] -> seq (S,4) i32 (first row, F, C, 0), pair (Q,4) i32 (sequence, a, b, first frame slot) for every a < b,
    sequence by sequence, rows, slots."""
    seq, pair, row, slot = [], [], 0, 0
    for s, sh in enumerate(shapes):
        F, C = int(sh[0]), int(sh[1])
        seq.append((row, F, C, 0))
        row += F * C
        for a in range(C):
            for b in range(a + 1, C):
                pair.append((s, a, b, slot))
                slot += F
    if row >= 2 ** 31 // 34 or slot >= 2 ** 31 // 51:
        raise ValueError("calibrate_rigs: too many frames for one call (32-bit offsets); calibrate the sequences in several calls")
    return np.array(seq, np.int32).reshape(-1, 4), np.array(pair, np.int32).reshape(-1, 4), row, slot


def _edge(fits, a, b):
    """Pose of camera b relative to camera a (X_b = R X_a + t) and the pair's points in a's frame, whichever way the pair was fitted."""
    if a < b:
        f = fits[a, b]
        return f["R"], f["t"], f["pts"]
    f = fits[b, a]
    return f["R"].T, -f["R"].T @ f["t"], f["pts"] @ f["R"].T + f["t"]


def pose_graph(C, fits, min_pair_inliers, min_common=MIN_COMMON):
    """Stage 5.  fits {(a, b): dict(n_inl, R, t, pts (F 17, 3))} for a < b -> (stop, tree, Rt (C,3,4) or None): camera 0 = [I|0], the
    first edge of length 1.  An edge after the first takes its scale from the first placed edge at its placed camera: the median
    ratio of the depths the two give their common points there; fewer than ``min_common`` of them: the next best edge is tried."""
    W = np.zeros((C, C), np.int64)
    for (a, b), f in fits.items():
        W[a, b] = W[b, a] = f["n_inl"]
    Rt = np.zeros((C, 3, 4))
    Rt[0, :, :3] = np.eye(3)
    placed, ref, tree = [0], {}, []
    while len(placed) < C:
        cands = sorted((-W[a, b], min(a, b), max(a, b), a, b) for a in placed for b in range(C)
                       if b not in placed and W[a, b] >= min_pair_inliers)
        for _, _, _, a, b in cands:
            R, t, pts = _edge(fits, a, b)
            s = 1.0
            if tree:
                a0, b0, s0 = ref[a]
                p0 = _edge(fits, a0, b0)[2] if a0 == a else _edge(fits, b0, a0)[2]
                both = ~np.isnan(pts[:, 2]) & ~np.isnan(p0[:, 2])
                if both.sum() < min_common:
                    continue
                s = s0 * float(np.median(p0[both, 2] / pts[both, 2]))
            Rt[b, :, :3] = R @ Rt[a, :, :3]
            Rt[b, :, 3] = R @ Rt[a, :, 3] + s * t
            ref.setdefault(a, (a, b, s))
            ref[b] = (a, b, s)
            placed.append(b)
            tree.append((a, b))
            break
        else:
            return "disconnected", tree, None
    return "ok", tree, Rt


def finish(Rt, X, baseline=None, world="camera0"):
    """Stage 7.  Rt (C,3,4) with camera 0 = [I|0]; X (F,17,3) in camera 0's frame, NaN where there is no point -> (Rt, X, source)."""
    Rt, X = np.array(Rt, np.float64), np.array(X, np.float64)
    if baseline is not None:
        c = -np.einsum("cji,cj->ci", Rt[:, :, :3], Rt[:, :, 3])
        s, src = float(baseline[2]) / np.linalg.norm(c[int(baseline[0])] - c[int(baseline[1])]), "baseline"
    else:
        L = np.stack([np.linalg.norm(X[:, a] - X[:, b], axis=1) for a, b in LIMBS], axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            q = limb_lengths()[None] / L
        q = q[np.isfinite(q)]
        s, src = (float(np.median(q)) if q.size else 1.0), "limbs"
    Rt[:, :, 3] *= s
    X = X * s
    if world == "floor":
        up = 0.5 * (X[:, 5] + X[:, 6]) - 0.5 * (X[:, 11] + X[:, 12])
        up = up[~np.isnan(up).any(axis=1)]
        ank = None
        if up.shape[0]:
            z = up.mean(axis=0)
            z /= np.linalg.norm(z)
            ank = np.minimum(X[:, 15] @ z, X[:, 16] @ z)
            ank = ank[~np.isnan(ank)]
        if ank is None or not ank.size or abs(z[2]) > 1.0 - 1e-9:
            raise ValueError("calibrate_rigs: world='floor' needs frames with both shoulders and hips, frames with both ankles, and "
                             "a camera 0 that does not look straight up or down")
        x = np.array([0.0, 0.0, 1.0]) - z[2] * z
        x /= np.linalg.norm(x)
        Q = np.stack([x, np.cross(z, x), z])
        o = np.array([0.0, 0.0, -float(np.median(ank))])
        Rn = Rt[:, :, :3] @ Q.T
        Rt = np.concatenate([Rn, (Rt[:, :, 3] - Rn @ o)[:, :, None]], axis=2)
        X = X @ Q.T + o
    return Rt, X, src


def calibrate_rigs(sequences: Sequence[tuple], hypotheses: int = 128, sample_frames: int = 8, inlier_px: float = 6.0,
                   min_score: float = body_fit.MIN_SCORE, min_pair_inliers: int = 100, refit_rounds: int = 3, polish_iter: int = 10,
                   polish_px: float = body_fit.MAX_DIST, baseline=None, world: str = "camera0", seed: int = 0, device="cuda:0",
                   timings: Optional[dict] = None, detail: Optional[list] = None, polish_loss: Optional[str] = None,
                   polish_loss_px: float = LOSS_PX, polish_ftol: Optional[float] = None, polish_intrinsics: Optional[str] = None,
                   polish_focal_sigma: Optional[float] = None, polish_centre_sigma_px: Optional[float] = None) -> List[RigCalibration]:
    """Calibrate the rig of every sequence -- (kps25 (F_s,C_s,P_s,25|17,3), counts (F_s,C_s), cameras: per view a Calib, whose Rt is
    ignored, or (K, (w, h))) -- from the one person who walks through it.  -> one RigCalibration per sequence; a rig that cannot be
    calibrated comes back with ``stop`` saying why and calibs None.  baseline: (i, j, metres) for every sequence, or a list with one
    such tuple or None per sequence.  timings: a dict that receives the seconds spent in {"observe", "pairs", "graph", "polish"}
    (synchronising between the parts).  detail: a list that receives per sequence what the kernels returned for its pairs -- what the
    tests compare.  polish_loss: None (plain least squares, the code path without these arguments), "huber" or "cauchy" at
    polish_loss_px pixels (rig_refine's loss); polish_ftol: the polish's ftol, None = the body fit's constant.  With a loss the polish
    makes more trials (it converges linearly) and ``polish`` carries the loss's fields; rms_px stays the plain rms.
    polish_intrinsics: None (K as given), "focal" or "focal+centre": rig_refine's intrinsic unknowns in the polish, with the prior
    polish_focal_sigma (relative) and polish_centre_sigma_px (px) about the given K ("focal+centre" needs the latter); the calibs then
    carry the polished K and ``polish`` the intrinsics' fields.  The pair stage always works on the given K."""
    shapes, cams, bases = check_calibrate(sequences, hypotheses, sample_frames, inlier_px, min_score, min_pair_inliers, refit_rounds,
                                          polish_iter, polish_px, baseline, world, polish_loss, polish_loss_px, polish_ftol,
                                          polish_intrinsics, polish_focal_sigma, polish_centre_sigma_px)
    import torch

    from . import device as dev
    d = torch.device(device)
    T = dev.uploader(d)
    lap, tm = stopwatch(timings, d, ("observe", "pairs", "graph", "polish", "start", "trials"))
    t0 = time.perf_counter()
    S = len(sequences)
    Ks = [np.array([k for k, _ in cm]) for cm in cams]
    # stage 1: the ingest of every sequence (one launch per keypoint layout), the observations on the host
    groups = {}
    arrays = []
    for s, seq in enumerate(sequences):
        k = np.asarray(seq[0])
        if k.dtype not in (np.float32, np.float64):
            k = k.astype(np.float64)
        arrays.append(k)
        groups.setdefault(tuple(k.shape[1:4]) + (k.dtype.str,), []).append(s)
    xn, px = [None] * S, [None] * S
    for ids in groups.values():
        k17, c17 = dev.ingest(T(np.concatenate([arrays[s] for s in ids], axis=0)),
                            T(np.concatenate([np.asarray(sequences[s][1]).astype(np.int32) for s in ids], axis=0)))
        k17, c17 = k17.cpu().numpy(), c17.cpu().numpy()
        lo = 0
        for s in ids:
            F = shapes[s][0]
            one = np.where(np.asarray(sequences[s][1]) == 1, c17[lo:lo + F], 0)       # one pose given, and the ingest kept it
            xn[s], px[s] = observations(k17[lo:lo + F], one, Ks[s], float(min_score))
            lo += F
    t0 = lap("observe", t0)
    # stages 2 - 4: every pair of every sequence in three launches
    seq_t, pair_t, n_rows, n_slots = pair_tables(shapes)
    fbar = np.array([0.25 * (Ks[s][a, 0, 0] + Ks[s][a, 1, 1] + Ks[s][b, 0, 0] + Ks[s][b, 1, 1]) for s, a, b, _ in pair_t])
    thr = (float(inlier_px) / fbar) ** 2
    u = np.random.default_rng(seed).random((int(hypotheses), int(sample_frames)))
    xn_d = T(np.concatenate([x.reshape(-1, 17, 2) for x in xn], axis=0))
    seq_d, pair_d, thr_d = T(seq_t), T(pair_t), T(thr)
    norm_d, mom_d, cnt_d, usable_d, nus_d = dev.pair_moments(xn_d, seq_d, pair_d, n_slots)
    E_d, count_d = dev.pair_consensus(xn_d, seq_d, pair_d, norm_d, mom_d, usable_d, nus_d, T(u), thr_d)
    pose_d, rounds_d, mask_d, pts_d = dev.pair_refit(xn_d, seq_d, pair_d, n_slots, norm_d, E_d, count_d, thr_d, int(refit_rounds))
    pose, pts, n_usable = pose_d.cpu().numpy(), pts_d.cpu().numpy(), nus_d.cpu().numpy()
    t0 = lap("pairs", t0)
    if detail is not None:
        keep = dict(norm=norm_d, mom=mom_d, cnt=cnt_d, usable=usable_d, E=E_d, count=count_d, rounds=rounds_d, mask=mask_d)
        keep = {k: v.cpu().numpy() for k, v in keep.items()}
        detail[:] = [dict(pairs=[], u=u, xn=xn[s], px=px[s]) for s in range(S)]
    # stage 5: the pose graph of every sequence
    out: List[Optional[RigCalibration]] = [None] * S
    fits = [dict() for _ in range(S)]
    few = np.ones(S, bool)
    for q, (s, a, b, slot) in enumerate(pair_t):
        F = shapes[s][0]
        fits[s][int(a), int(b)] = dict(n_inl=int(pose[q, 23]), R=pose[q, :9].reshape(3, 3), t=pose[q, 9:12],
                                       pts=pts[slot * 17:(slot + F) * 17])
        few[s] &= n_usable[q] < int(sample_frames)
        if detail is not None:
            detail[s]["pairs"].append(dict(a=int(a), b=int(b), thr=thr[q], n_usable=int(n_usable[q]), pose=pose[q],
                                           pts=pts[slot * 17:(slot + F) * 17], mask=keep["mask"][slot * 17:(slot + F) * 17],
                                           norm=keep["norm"][q], mom=keep["mom"][slot:slot + F], cnt=keep["cnt"][slot:slot + F],
                                           usable=keep["usable"][slot:slot + F], E=keep["E"][q], count=keep["count"][q],
                                           rounds=keep["rounds"][q]))
    Rt_tree = [None] * S
    for s in range(S):
        C = shapes[s][1]
        W = np.zeros((C, C), np.int64)
        for (a, b), f in fits[s].items():
            W[a, b] = W[b, a] = f["n_inl"]
        stop, tree = "few_frames", []
        if not few[s]:
            stop, tree, Rt_tree[s] = pose_graph(C, fits[s], int(min_pair_inliers))
        out[s] = RigCalibration(calibs=None, stop=stop, tree=tree, pair_inliers=W, rms_px=float("nan"), scale_source=None, polish=None,
                                points=None)
    t0 = lap("graph", t0)
    # stage 6: the bundle adjustment, the sequences of one camera count in one group; stage 7 on its result
    by_c = {}
    for s in range(S):
        if out[s].stop == "ok":
            by_c.setdefault(shapes[s][1], []).append(s)
    for C, ids in by_c.items():
        n = len(ids)
        cand = [np.ascontiguousarray(px[s].transpose(0, 2, 1, 3)).reshape(-1, C, 3) for s in ids]      # (F 17, C, 3), (frame, joint) order
        is_c = [(c[:, :, 2] > float(min_score)).sum(axis=1) >= 2 for c in cand]
        obs = np.concatenate([c[m] for c, m in zip(cand, is_c)], axis=0)
        rig_c = np.repeat(np.arange(n, dtype=np.int32), [int(m.sum()) for m in is_c])
        Kin = np.array([Ks[s] for s in ids])
        Rtin = np.array([Rt_tree[s] for s in ids])
        any_c = obs.shape[0] > 0
        g = solve_group(T(obs) if any_c else None, T(rig_c) if any_c else None, T(np.einsum("scij,scjk->scik", Kin, Rtin)) if any_c else None,
                        Kin, Rtin, n, C, d, int(polish_iter), float(polish_px), float(min_score), 2, int(min_pair_inliers), 1, lap,
                        polish_loss, polish_loss_px, polish_ftol, None, polish_intrinsics, polish_focal_sigma, polish_centre_sigma_px)
        for r, s in enumerate(ids):
            pol = decode(g, r, cams[s], Rtin[r], polish_loss, polish_loss_px, intrinsics=polish_intrinsics)
            Rt_new = np.array([c.Rt for c in pol.calibs])
            wh = [w for _, w in cams[s]]
            X = np.full((cand[r].shape[0], 3), np.nan)
            X[np.flatnonzero(is_c[r])[g.is_pt[g.seq_of == r]]] = g.points(r)
            Rt_fin, X_fin, src = finish(Rt_new, X.reshape(-1, 17, 3), bases[s], world)
            K_fin = Ks[s] if pol.K_after is None else pol.K_after
            out[s].calibs = [Calib.from_k_rt(K_fin[c].copy(), Rt_fin[c], wh[c]) for c in range(C)]
            out[s].rms_px, out[s].scale_source, out[s].polish, out[s].points = pol.rms_after, src, pol, X_fin
        lap("polish")
    if timings is not None:
        tm["polish"] += tm.pop("start") + tm.pop("trials")
        timings.update(tm)
    return out


def calibrate_rig(kps: np.ndarray, counts: np.ndarray, cameras: list, **kw) -> RigCalibration:
    """calibrate_rigs for one sequence: kps (F,C,P,25|17,3), counts (F,C), per view a Calib or (K, (w, h)) -> RigCalibration."""
    return calibrate_rigs([(kps, counts, cameras)], **kw)[0]
