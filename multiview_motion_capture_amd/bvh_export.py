"""BVH export of a fitted tracklet record (body_fit.fit_sequences / fit_tracklets).

HIERARCHY: the BASIC_18 tree of inverse_kinematics.load_skeleton(), OFFSET = bone direction x full bone length from the record's
side lengths.  The root carries Xposition Yposition Zposition Xrotation Yrotation Zrotation, every other joint Xrotation Yrotation
Zrotation: the FK's local rotation R = Rx Ry Rz (inverse_kinematics.py:176-199), in degrees.  Leaves are JOINTs with a zero End Site
(Nose has two leaf children, so a leaf cannot be an End Site of its parent).  MOTION: one line per frame from the record's first frame
to its last; a frame where the identity was not updated repeats the previous one.  World frame and metres, no axis conversion.

A BVH file has one skeleton: a record whose frames do not share one length vector is refused.
"""
from __future__ import annotations

from typing import Optional

import numpy as np


def _children(parents):
    ch = [[] for _ in parents]
    for j, p in enumerate(parents):
        if p >= 0:
            ch[p].append(j)
    return ch


def bvh_text(tracklet, frame_time: float = 1.0 / 30.0, skeleton=None) -> str:
    """The BVH file of one record as a string (see save_bvh)."""
    from .inverse_kinematics import load_skeleton
    from .pose_def import KpsFormat, get_kps_order
    sk = skeleton if skeleton is not None else load_skeleton()
    poses = tracklet.poses
    if len(poses) == 0:
        raise ValueError("save_bvh: empty record")
    lens = np.array([np.asarray(p[1].bone_lens, np.float64).ravel() for p in poses])
    if not np.all(lens == lens[0]):
        raise ValueError("save_bvh: the record's frames do not share one bone-length vector (fit it with body_fit first)")
    parents = [int(p) for p in sk.joint_parents]
    names = [k.name for k in get_kps_order(KpsFormat.BASIC_18)]
    full = np.asarray(sk.to_full_bone_lens(lens[0]), np.float64)
    offsets = np.asarray(sk.ref_bone_dirs, np.float64) * full[:, None]
    offsets[0] = 0.0
    ch = _children(parents)
    order, lines = [], ["HIERARCHY"]

    def emit(j, depth):
        ind = "\t" * depth
        order.append(j)
        lines.append(f"{ind}{'ROOT' if parents[j] < 0 else 'JOINT'} {names[j]}")
        lines.append(ind + "{")
        lines.append(f"{ind}\tOFFSET {offsets[j, 0]:.9f} {offsets[j, 1]:.9f} {offsets[j, 2]:.9f}")
        if parents[j] < 0:
            lines.append(f"{ind}\tCHANNELS 6 Xposition Yposition Zposition Xrotation Yrotation Zrotation")
        else:
            lines.append(f"{ind}\tCHANNELS 3 Xrotation Yrotation Zrotation")
        if ch[j]:
            for c in ch[j]:
                emit(c, depth + 1)
        else:
            lines.extend([f"{ind}\tEnd Site", ind + "\t{", f"{ind}\t\tOFFSET 0.000000000 0.000000000 0.000000000", ind + "\t}"])
        lines.append(ind + "}")

    emit(parents.index(-1), 0)
    frames = [int(f) for f in tracklet.frame_idxs]
    if any(b <= a for a, b in zip(frames, frames[1:])):
        raise ValueError("save_bvh: frame indices must increase")
    rows = np.array([np.concatenate([np.asarray(p[1].root, np.float64).ravel(),
                                     np.degrees(np.asarray(p[1].euler_angles, np.float64).reshape(18, 3)[order].ravel())])
                     for p in poses])
    # frames first..last; a gap repeats the previous updated frame
    src = np.searchsorted(np.array(frames), np.arange(frames[0], frames[-1] + 1), side="right") - 1
    lines += ["MOTION", f"Frames: {src.size}", f"Frame Time: {frame_time:.8f}"]
    lines += [" ".join(f"{v:.9f}" for v in rows[k]) for k in src]
    return "\n".join(lines) + "\n"


def save_bvh(path: str, tracklet, frame_time: float = 1.0 / 30.0, skeleton: Optional[object] = None) -> None:
    """Write one record (same bone lengths on every frame: body_fit's output) as a BVH file."""
    text = bvh_text(tracklet, frame_time, skeleton)
    with open(path, "w") as f:
        f.write(text)
