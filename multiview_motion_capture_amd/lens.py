"""Cameras with lens distortion: the door of the pipeline, and the way out.

Every stage of this package -- tracking, re-linking, rig refinement, body fit, the smoothers, BVH export -- reads a keypoint as a pixel
of the ideal pinhole camera P = K Rt, as the reference does (its only projection is
project_3d_points_to_image_plane_without_distortion).  A 2-D detector runs on the raw images of a real lens.  This module undistorts
its keypoints ONCE, before anything else sees them (one launch of mvmc_lens_undistort, include/mvmc.h), and hands on pinhole
calibrations; everything downstream stays as it is.  project_raw is the way back: 3-D joints onto the raw images.

A camera's model is ``Calib.lens`` (None = pinhole): Brown-Conrady with OpenCV's coefficients (cv2.calibrateCamera) or Kannala-Brandt
(cv2.fisheye.calibrate).  Every entry point that takes calibrations refuses one whose ``lens`` is set (require_pinhole), so a distorted
rig cannot be fed in silently wrong.  INTEGRATION.md section C.8; tests/lens_np.py restates the arithmetic in NumPy.

    seqs, report = lens.undistort_sequences(seqs)          # recorded: SequenceInput list in, the same with pinhole pixels out
    tracklets = track_sequences(seqs)
    bank = lens.LensBank(n_views, capacity); rid = bank.add(calibs); sid = pool.open_session(lens.pinhole(calibs))
    pool.update_4d_arrays(sids, frm_idxs, bank.undistort_arrays(rids, kps25), counts)      # live: one launch per tick
    uv, ok = lens.project_raw(joints3d, calibs)            # the way out
"""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .common import Calib, FrameData

PINHOLE, BROWN, FISHEYE = 0, 1, 2          # MVMC_LENS_* of include/mvmc.h
LENS_DOUBLES = 16
_MODEL_NAMES = {"brown": BROWN, "fisheye": FISHEYE}


@dataclass(frozen=True)
class Lens:
    """A distortion model and its eight coefficients: Brown (k1, k2, p1, p2, k3, k4, k5, k6), OpenCV's order; fisheye (k1 .. k4, 0 ..)."""
    model: int
    k: Tuple[float, ...]

    def __post_init__(self):
        if self.model not in (BROWN, FISHEYE):
            raise ValueError(f"Lens: model {self.model!r} is neither BROWN ({BROWN}) nor FISHEYE ({FISHEYE})")
        k = tuple(float(v) for v in self.k)
        if len(k) != 8 or not all(np.isfinite(k)):
            raise ValueError(f"Lens: eight finite coefficients expected, got {self.k!r}")
        object.__setattr__(self, "k", k)

    @classmethod
    def brown(cls, k1, k2, p1, p2, k3=0.0, k4=0.0, k5=0.0, k6=0.0) -> "Lens":
        return cls(BROWN, (k1, k2, p1, p2, k3, k4, k5, k6))

    @classmethod
    def fisheye(cls, k1, k2, k3, k4) -> "Lens":
        return cls(FISHEYE, (k1, k2, k3, k4, 0.0, 0.0, 0.0, 0.0))

    @classmethod
    def from_opencv(cls, dist_coeffs, fisheye: bool = False) -> "Lens":
        """cv2.calibrateCamera's distCoeffs (4, 5 or 8 values: k1 k2 p1 p2 [k3 [k4 k5 k6]]) or cv2.fisheye.calibrate's D (4 values).
        The thin-prism and tilt terms (12 and 14 values) have no model here."""
        d = [float(v) for v in np.asarray(dist_coeffs, np.float64).ravel()]
        if fisheye:
            if len(d) != 4:
                raise ValueError(f"Lens.from_opencv: a fisheye model has 4 coefficients, got {len(d)}")
            return cls.fisheye(*d)
        if len(d) not in (4, 5, 8):
            raise ValueError(f"Lens.from_opencv: 4, 5 or 8 distortion coefficients expected, got {len(d)}")
        return cls.brown(*d)


def require_pinhole(calibs, who: str) -> None:
    """Raises ValueError if a calibration carries a lens model: ``who`` reads pixels as pinhole pixels."""
    for c, cal in enumerate(calibs):
        if getattr(cal, "lens", None) is not None:
            raise ValueError(f"{who}: camera {c} has a lens model and this stage reads pinhole pixels; undistort first: "
                             "lens.undistort_sequences / LensBank")


def pinhole(calibs) -> List[Calib]:
    """Copies of the calibrations without their lens models: what the stages after undistortion take."""
    return [dataclasses.replace(c, lens=None) for c in calibs]


def lens_row(calib: Calib) -> np.ndarray:
    """One row of the device table: {model, fx, fy, cx, cy, skew, k[0..7], 0, 0}."""
    K = np.asarray(calib.K, np.float64).reshape(3, 3)
    row = np.zeros(LENS_DOUBLES)
    row[1:6] = K[0, 0], K[1, 1], K[0, 2], K[1, 2], K[0, 1]
    ln = getattr(calib, "lens", None)
    if ln is not None:
        if K[0, 0] == 0.0 or K[1, 1] == 0.0:
            raise ValueError("lens_table: a camera with a lens model has a zero focal length")
        row[0] = ln.model
        row[6:14] = ln.k
    return row


def lens_table(rigs_of_calibs) -> np.ndarray:
    """(R, C, 16) float64 table of mvmc_lens_undistort / mvmc_lens_distort: one rig per list of calibrations, all of one camera count."""
    rigs = [list(r) for r in rigs_of_calibs]
    if not rigs or not rigs[0] or any(len(r) != len(rigs[0]) for r in rigs):
        raise ValueError("lens_table: at least one rig, and the same number of cameras (>= 1) in every rig")
    return np.array([[lens_row(c) for c in r] for r in rigs])


def _table(rigs) -> np.ndarray:
    if isinstance(rigs, np.ndarray):
        t = np.ascontiguousarray(rigs, dtype=np.float64)
        if t.ndim != 3 or t.shape[2] != LENS_DOUBLES:
            raise ValueError(f"lens table: expected (R,C,{LENS_DOUBLES}), got {t.shape}")
        return t
    rigs = list(rigs)
    if rigs and isinstance(rigs[0], Calib):
        rigs = [rigs]
    return lens_table(rigs)


def _run(inverse: bool, kps, rigs, rig_of_frame, device):
    import torch

    from . import device as dev
    k = np.ascontiguousarray(kps)
    if k.dtype not in (np.float32, np.float64):
        k = k.astype(np.float64)
    d = torch.device(device)
    fn = dev.lens_undistort if inverse else dev.lens_distort
    out, dropped = fn(torch.from_numpy(k).to(d), torch.from_numpy(_table(rigs)).to(d),
                      None if rig_of_frame is None else np.asarray(rig_of_frame))
    return out.cpu().numpy(), dropped.cpu().numpy()


def undistort_keypoints(kps, rigs, rig_of_frame=None, device="cuda:0"):
    """kps (F,C,...,3) raw triples (x, y, score), float32 or float64 -> (pinhole triples of the same dtype, dropped (F,C)).  rigs: the
    calibrations of one rig, a list of rigs, or a lens_table; rig_of_frame (F,) picks each frame's rig (None: rig 0).  A keypoint
    without a valid pre-image comes out (0,0,0) and is counted; score <= 0 and pinhole cameras are copied bit for bit."""
    return _run(True, kps, rigs, rig_of_frame, device)


def distort_keypoints(kps, rigs, rig_of_frame=None, device="cuda:0"):
    """The forward model: pinhole triples -> raw triples; arguments as undistort_keypoints; nothing is dropped."""
    return _run(False, kps, rigs, rig_of_frame, device)


def undistort_sequences(sequences, max_dropped: float = 0.02, device="cuda:0"):
    """track_sequences' input with real lenses -> (the same tuples with pinhole-pixel keypoints, in their dtype, and pinhole(calibs);
    report).  One launch per distinct keypoint shape (C, P, J) and dtype; each sequence is a rig of the launch.
    report[i] = {"dropped": (C,) scored keypoints of each camera without a valid pre-image (now (0,0,0)), "scored": (C,) keypoints with
    score > 0}.  A camera that loses more than ``max_dropped`` of its scored keypoints raises ValueError: coefficients of the wrong model
    or in the wrong units do that, a good calibration does not."""
    seqs = list(sequences)
    if not seqs:
        raise ValueError("undistort_sequences: no sequences")
    groups: Dict[tuple, List[int]] = {}
    arrays = []
    for i, seq in enumerate(seqs):
        if len(seq) != 3:
            raise ValueError(f"sequence {i}: expected (kps25, counts, calibs)")
        k = np.asarray(seq[0])
        if k.dtype not in (np.float32, np.float64):
            k = k.astype(np.float64)
        if k.ndim != 5 or k.shape[4] != 3:
            raise ValueError(f"sequence {i}: kps25 must be (F,C,P,J,3), got {k.shape}")
        if len(seq[2]) != k.shape[1]:
            raise ValueError(f"sequence {i}: {len(seq[2])} calibrations for {k.shape[1]} cameras")
        arrays.append(k)
        groups.setdefault(tuple(k.shape[1:4]) + (k.dtype.str,), []).append(i)
    out: List[Optional[tuple]] = [None] * len(seqs)
    report: List[Optional[dict]] = [None] * len(seqs)
    for ids in groups.values():
        n = [arrays[i].shape[0] for i in ids]
        rig_of_frame = np.repeat(np.arange(len(ids), dtype=np.int32), n)
        und, drp = undistort_keypoints(np.concatenate([arrays[i] for i in ids], 0), [seqs[i][2] for i in ids], rig_of_frame, device)
        lo = 0
        for r, i in enumerate(ids):
            hi = lo + n[r]
            dropped = drp[lo:hi].sum(0, dtype=np.int64)
            scored = (arrays[i][..., 2] > 0).sum(axis=(0, 2, 3), dtype=np.int64)
            for c in range(len(dropped)):
                if dropped[c] > max_dropped * scored[c]:
                    raise ValueError(f"undistort_sequences: sequence {i}, camera {c}: {int(dropped[c])} of {int(scored[c])} scored "
                                     f"keypoints have no pre-image under its lens model (more than {max_dropped:.1%}); are the "
                                     "coefficients those of this model, in OpenCV's order?")
            out[i] = (und[lo:hi], seqs[i][1], pinhole(seqs[i][2]))
            report[i] = {"dropped": dropped, "scored": scored}
            lo = hi
    return out, report


def _pack_frames(frames_per_rig: Sequence[List[FrameData]]):
    """Poses of FrameData lists -> (S, C, P, J, 3) float64 triples, zero padded."""
    C = len(frames_per_rig[0])
    P, J = 1, None
    for fr in frames_per_rig:
        if len(fr) != C:
            raise ValueError(f"undistort: {len(fr)} views in a frame, {C} in the first")
        for f in fr:
            P = max(P, len(f.poses))
            for pose in f.poses.values():
                j = int(np.asarray(pose.keypoints).shape[0])
                if J not in (None, j):
                    raise ValueError("undistort: poses of different joint counts in one call")
                J = j
    k = np.zeros((len(frames_per_rig), C, P, J or 1, 3))
    for s, fr in enumerate(frames_per_rig):
        for c, f in enumerate(fr):
            for p, pose in enumerate(f.poses.values()):
                k[s, c, p, :, :2] = pose.keypoints
                k[s, c, p, :, 2] = np.asarray(pose.keypoints_score).ravel()
    return k


def _unpack_frames(k: np.ndarray, frames_per_rig) -> List[List[FrameData]]:
    from .pose_def import Pose
    out = []
    for s, fr in enumerate(frames_per_rig):
        cal = pinhole([f.calib for f in fr])
        out.append([FrameData(f.frame_idx, {pid: Pose(pose.pose_type, k[s, c, p, :, :2].copy(), k[s, c, p, :, 2:3].copy(), pose.box)
                                            for p, (pid, pose) in enumerate(f.poses.items())}, cal[c], f.view_id)
                    for c, f in enumerate(fr)])
    return out


def undistort_frame_data(d_frames: List[FrameData], device="cuda:0") -> List[FrameData]:
    """One frame of MvTracker.update_4d's input (a FrameData per view, each with its Calib and lens) -> new FrameData with pinhole
    pixels and pinhole calibrations; one launch.  A keypoint without a pre-image gets (0, 0) and score 0."""
    k = _pack_frames([d_frames])
    und, _ = undistort_keypoints(k, [[f.calib for f in d_frames]], None, device)
    return _unpack_frames(und, [d_frames])[0]


class LensBank:
    """The lens tables of up to ``capacity`` live rigs of ``n_views`` cameras, on the device: one launch undistorts one tick of many
    sessions.  ``add`` returns the rig's id; open the LivePool / LiveSmoother session with pinhole(calibs)."""

    def __init__(self, n_views: int, capacity: int, device="cuda:0"):
        import torch
        if int(n_views) < 1 or int(capacity) < 1:
            raise ValueError("LensBank: n_views >= 1 and capacity >= 1 required")
        self.C, self.capacity, self.device = int(n_views), int(capacity), torch.device(device)
        self._table = torch.zeros((self.capacity, self.C, LENS_DOUBLES), dtype=torch.float64, device=self.device)
        self._open: Dict[int, bool] = {}
        self._free = list(range(self.capacity))
        self.last_dropped = None       # (S, C) int32 device tensor of the last tick

    def add(self, calibs) -> int:
        if len(calibs) != self.C:
            raise ValueError(f"LensBank.add: {len(calibs)} cameras, the bank's rigs have {self.C}")
        if not self._free:
            raise ValueError(f"LensBank.add: all {self.capacity} slots are taken")
        import torch
        rows = torch.from_numpy(lens_table([calibs])[0])
        rid = self._free.pop(0)
        self._table[rid] = rows.to(self.device)
        self._open[rid] = True
        return rid

    def remove(self, rid: int) -> None:
        if rid not in self._open:
            raise ValueError(f"LensBank.remove: no rig {rid}")
        del self._open[rid]
        self._table[rid].zero_()
        self._free.append(rid)
        self._free.sort()

    def _rids(self, rids, what: str) -> np.ndarray:
        rids = [int(r) for r in rids]
        for r in rids:
            if r not in self._open:
                raise ValueError(f"{what}: no rig {r}")
        return np.asarray(rids, dtype=np.int32)

    def undistort_arrays(self, rids: Sequence[int], kps25):
        """One tick: kps25[i] ((C,P,J,3) raw triples, a NumPy array or a tensor, float32 or float64) is a frame of rig rids[i] -> the
        pinhole triples as a tensor on the bank's device, what LivePool.update_4d_arrays and LiveSmoother.update_4d_arrays take.  One
        launch, nothing is read back; ``last_dropped`` keeps the (S,C) counts on the device."""
        import torch

        from . import device as dev
        rig = self._rids(rids, "undistort_arrays")
        k = torch.as_tensor(kps25)
        if k.dim() != 5 or k.shape[0] != len(rig) or k.shape[1] != self.C or k.shape[4] != 3:
            raise ValueError(f"undistort_arrays: expected ({len(rig)},{self.C},P,J,3), got {tuple(k.shape)}")
        if k.dtype not in (torch.float32, torch.float64):
            k = k.to(torch.float64)
        k = k.to(self.device).contiguous()
        if len(rig) == 0:
            return k
        out, self.last_dropped = dev.lens_undistort(k, self._table, rig)
        return out

    def undistort_frames(self, frames: Dict[int, List[FrameData]]) -> Dict[int, List[FrameData]]:
        """One tick from FrameData: {rid: the frame's FrameData per view} -> the same with pinhole pixels and pinhole calibrations
        (LivePool.update_4d's input); one launch for all sessions."""
        items = list(frames.items())
        if not items:
            return {}
        for _, fr in items:
            if len(fr) != self.C:
                raise ValueError(f"undistort_frames: a frame of {len(fr)} views, the bank's rigs have {self.C}")
        k = _pack_frames([fr for _, fr in items])
        und = self.undistort_arrays([rid for rid, _ in items], k).cpu().numpy()
        return {rid: fr for (rid, _), fr in zip(items, _unpack_frames(und, [fr for _, fr in items]))}


def project_raw(joints3d, calibs, device="cuda:0"):
    """The way out: joints3d (N,J,3) world points -> (uv (N,C,J,2) pixels on the RAW images of ``calibs``, ok (N,C,J) bool).  The
    pinhole projection K (R X + t) followed by the forward lens model (mvmc_lens_distort).  ok is False, and uv NaN, for a point that
    is not in front of the camera.  Use it to draw tracked, fitted or smoothed joints on the raw images, or to measure reprojection
    against the raw detections."""
    X = np.asarray(joints3d, np.float64)
    if X.ndim != 3 or X.shape[2] != 3:
        raise ValueError(f"project_raw: joints3d must be (N,J,3), got {X.shape}")
    calibs = list(calibs)
    K = np.array([np.asarray(c.K, np.float64).reshape(3, 3) for c in calibs])
    Rt = np.array([np.asarray(c.Rt, np.float64).reshape(3, 4) for c in calibs])
    cam = np.einsum('cij,nkj->ncki', Rt[:, :, :3], X) + Rt[None, :, None, :, 3]
    with np.errstate(invalid="ignore", divide="ignore"):
        ok = np.isfinite(cam).all(-1) & (cam[..., 2] > 0)
        z = np.where(ok, cam[..., 2], 1.0)
        pix = np.einsum('cij,nckj->ncki', K, cam / z[..., None])
    tri = np.zeros(ok.shape + (3,))
    tri[..., :2] = np.where(ok[..., None], pix[..., :2], 0.0)
    tri[..., 2] = ok
    raw, _ = distort_keypoints(tri, [calibs], None, device)
    uv = np.where(ok[..., None], raw[..., :2], np.nan)
    return uv, ok
