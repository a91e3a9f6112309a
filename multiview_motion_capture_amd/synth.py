"""Synthetic multi-view keypoint generator (the reference has none).

Cameras on a ring of radius 4 m at height 1.5-2.5 m looking at the scene centre, Shelf-like
intrinsics (f = 1080 px, 1032 x 776); P people with roots uniform in a 4 x 4 m area, the 18-joint
skeleton of inverse_kinematics.py:120-173 posed with N(0, 0.3 rad) angles that follow a smooth
random walk (0.02 rad, 2 cm per frame); joints projected into every view, OpenPose-25 layout,
N(0, 2 px) pixel noise, scores U(0.5, 1), 5 % of the joints dropped to (0, 0, 0) the way OpenPose
reports misses; the person order is shuffled independently per view and frame so that association
is not trivial.  numpy.random.default_rng(seed) makes every configuration reproducible.
"""
from __future__ import annotations

import numpy as np

from .device import SKEL_PARENTS, SKEL_SIDE_MAP, skeleton_arrays

# skeleton joint of each COCO keypoint (eyes are synthesised between nose and ear)
_COCO_FROM_SKEL = {0: 15, 3: 16, 4: 17, 5: 9, 6: 12, 7: 10, 8: 13, 9: 11, 10: 14, 11: 1, 12: 4, 13: 2, 14: 5,
                   15: 3, 16: 6}
# OpenPose-25 row of each COCO-17 joint (pose_def.py:111-137)
_OP25_OF_COCO = [0, 16, 15, 18, 17, 5, 2, 6, 3, 7, 4, 12, 9, 13, 10, 14, 11]


def make_cameras(n_views: int, rng: np.random.Generator):
    """-> K (C,3,3), Rt (C,3,4), P (C,3,4) float64."""
    K = np.array([[1080.0, 0, 516.0], [0, 1080.0, 388.0], [0, 0, 1.0]])
    Ks, Rts = [], []
    target = np.array([0.0, 0.0, 1.0])
    for c in range(n_views):
        th = 2 * np.pi * (c + rng.uniform(-0.15, 0.15)) / n_views
        pos = np.array([4.0 * np.cos(th), 4.0 * np.sin(th), rng.uniform(1.5, 2.5)])
        fwd = target - pos
        fwd /= np.linalg.norm(fwd)
        right = np.cross(fwd, np.array([0.0, 0.0, 1.0]))
        right /= np.linalg.norm(right)
        down = np.cross(fwd, right)
        R = np.stack([right, down, fwd])
        Rts.append(np.concatenate([R, (-R @ pos)[:, None]], axis=1))
        Ks.append(K.copy())
    Ks, Rts = np.array(Ks), np.array(Rts)
    return Ks, Rts, Ks @ Rts


def _rot(axis: int, a: np.ndarray) -> np.ndarray:
    c, s = np.cos(a), np.sin(a)
    R = np.zeros(a.shape + (3, 3))
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R[..., axis, axis] = 1.0
    R[..., i, i] = c
    R[..., j, j] = c
    R[..., i, j] = -s
    R[..., j, i] = s
    return R


def batched_fk(root: np.ndarray, euler: np.ndarray, side_lens: np.ndarray) -> np.ndarray:
    """Vectorised FK (R = Rx Ry Rz, parents precede children): root (...,3), euler (...,18,3) -> (...,18,3)."""
    dirs, _ = skeleton_arrays()
    off = dirs * side_lens[..., SKEL_SIDE_MAP, None] if side_lens.ndim > 1 else dirs * side_lens[SKEL_SIDE_MAP, None]
    R = _rot(0, euler[..., 0]) @ _rot(1, euler[..., 1]) @ _rot(2, euler[..., 2])
    Rg = [None] * 18
    pos = [None] * 18
    Rg[0], pos[0] = R[..., 0, :, :], root
    for j in range(1, 18):
        p = SKEL_PARENTS[j]
        pos[j] = pos[p] + np.einsum('...ij,...j->...i', Rg[p], np.broadcast_to(off[..., j, :], pos[p].shape))
        Rg[j] = Rg[p] @ R[..., j, :, :]
    return np.stack(pos, axis=-2)


def scene_walk(n_frames: int, n_people: int, seed: int, segment: int = 0, kappa: float = 4.5e-3):
    """One smooth, BOUNDED walk of the scene's people, cut into consecutive segments of ``n_frames`` frames:
    -> root (n_frames, P, 3), angles (n_frames, P, 18, 3) of segment ``segment``.  Every person wanders around a home position and a
    home pose (drawn from ``seed``): the increments of generate()'s random walk (2 cm and 0.02 rad per frame) with a pull of ``kappa``
    per frame towards home, started in its stationary state, so that a sequence of any length stays in front of the cameras (a plain
    random walk drifts by 9 m over the 200 k frames of BASELINE config 5).  With kappa = 4.5e-3 the wander has a standard deviation of
    0.21 rad / 0.21 m around a home pose of 0.21 rad: joint angles of 0.30 rad in all -- the distribution generate() draws at its chain
    heads, so the poses the solver sees are those of the chain-restart workload of rounds 1 - 5.  Segment s draws its increments from
    its own stream (seed, 3, s) and starts where segment s - 1 ends, so the segments of one seed (and one segment length) tile ONE
    scene whoever generates them: rank r of a sharded run generates segment r, replaying the cheap increments of the segments before
    it for its start state."""
    from scipy.signal import lfilter
    rng0 = np.random.default_rng([seed, 3])
    home_root = np.concatenate([rng0.uniform(-2, 2, size=(n_people, 2)), rng0.uniform(0.95, 1.1, size=(n_people, 1))], -1)
    home_ang = rng0.normal(0, 0.3 / np.sqrt(2.0), size=(n_people, 18, 3))
    sd = np.concatenate([0.02 * np.array([1, 1, 0.1]), np.full(54, 0.02)])                    # per-frame increments
    y0 = rng0.normal(0, 1.0, size=(n_people, 57)) * sd / np.sqrt(1.0 - (1.0 - kappa) ** 2)    # the stationary state
    a = [1.0, -(1.0 - kappa)]
    zi = ((1.0 - kappa) * y0).reshape(1, n_people * 57)
    y = None
    for s in range(segment + 1):
        rng = np.random.default_rng([seed, 3, s])
        d = (rng.normal(0, 1.0, size=(n_frames, n_people, 57)) * sd).reshape(n_frames, n_people * 57)
        y, zi = lfilter([1.0], a, d, axis=0, zi=zi)      # x_t = (1 - kappa) x_{t-1} + d_t, carried across the segments
    y = y.reshape(n_frames, n_people, 57)
    return home_root[None] + y[..., :3], home_ang[None] + y[..., 3:].reshape(n_frames, n_people, 18, 3)


def _rotvec_mat(w: np.ndarray) -> np.ndarray:
    """Rotation vectors (...,3) -> matrices (...,3,3) (Rodrigues)."""
    th = np.linalg.norm(w, axis=-1)[..., None, None]
    k = w / np.where(th[..., 0] > 0, th[..., 0], 1.0)
    Kx = np.zeros(w.shape[:-1] + (3, 3))
    Kx[..., 0, 1], Kx[..., 0, 2], Kx[..., 1, 2] = -k[..., 2], k[..., 1], -k[..., 0]
    Kx[..., 1, 0], Kx[..., 2, 0], Kx[..., 2, 1] = k[..., 2], -k[..., 1], k[..., 0]
    return np.eye(3) + np.sin(th) * Kx + (1.0 - np.cos(th)) * (Kx @ Kx)


def _floor_tilt(ang: np.ndarray, lens: np.ndarray, stance: int, normal: np.ndarray) -> np.ndarray:
    """planted_walk's angles (F,P,18,3) with the root rotated so that at every change of the stance foot both ankles are at the same
    height along ``normal`` (unit): at change frame t_c, d = right ankle - left ankle (root-relative), the least rotation that makes
    d perpendicular to the normal (axis d x n, angle -asin(n . d / |d|)); the rotation vectors interpolated linearly between the
    change frames, constant before the first and after the last; R_root <- Q R_root, back to Rx Ry Rz Euler angles, unwrapped."""
    from .smoothing import unwrap_euler
    F, P = ang.shape[:2]
    tc = np.arange(int(stance), F, int(stance))
    if tc.size == 0:
        return ang
    rel = batched_fk(np.zeros((tc.size, P, 3)), ang[tc], np.broadcast_to(lens, (tc.size, P, 11)))[:, :, [3, 6]]
    d = rel[:, :, 1] - rel[:, :, 0]
    axis = np.cross(d, normal)
    axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
    rv_c = axis * -np.arcsin((d @ normal) / np.linalg.norm(d, axis=-1))[..., None]        # (n_changes, P, 3)
    rv = np.empty((F, P, 3))
    for p in range(P):
        for e in range(3):
            rv[:, p, e] = np.interp(np.arange(F), tc, rv_c[:, p, e])
    R0 = _rot(0, ang[:, :, 0, 0]) @ _rot(1, ang[:, :, 0, 1]) @ _rot(2, ang[:, :, 0, 2])
    R = _rotvec_mat(rv) @ R0
    out = ang.copy()
    out[:, :, 0, 0] = np.arctan2(-R[..., 1, 2], R[..., 2, 2])
    out[:, :, 0, 1] = np.arcsin(np.clip(R[..., 0, 2], -1.0, 1.0))
    out[:, :, 0, 2] = np.arctan2(-R[..., 0, 1], R[..., 0, 0])
    for p in range(P):
        out[:, p] = unwrap_euler(out[:, p])
    return out


def planted_walk(n_frames: int, n_people: int, seed: int, stance: int = 8, side_lens=None, start=None, floor_normal=None):
    """A walk with planted feet, the ground truth for foot skate: -> root (n_frames, P, 3), angles (n_frames, P, 18, 3), contact
    (n_frames, P, 2) bool (columns: left ankle = skeleton joint 3, right ankle = joint 6).  The angles are scene_walk(seed)'s
    (segment 0: the mean-reverting walk around a home pose); the root is not drawn but PLACED, frame by frame, where the stance
    ankle stays exactly where it is.  The stance foot changes every ``stance`` frames: on the frame of the change the root still
    follows the old stance ankle, the other ankle's position on that frame becomes the new anchor, and both feet are labelled (a
    double support); from the next frame on the root follows the new one.  So one foot is down on every frame, and an ankle does
    not move between two consecutive frames on which it is labelled (to the rounding of one FK: ~1e-16 m).  Everybody starts on
    the left foot, at ``start`` (P, 3) (default: scene_walk's first roots).  side_lens (11,) or (P, 11): the bone lengths the FK is
    taken with (default: the skeleton's reference lengths).  Nothing puts the anchors on a common floor: the swing ankle is
    wherever the angles put it when its turn comes.
    floor_normal (3,) (default None: the output above, bit for bit): a walk on ONE floor.  The whole body is tilted about the root
    (the root joint's angles alone change) so that at every change of the stance foot both ankles are at the same height along the
    normal (_floor_tilt): every anchor of one person then lies on one plane with that normal (to ~1e-15 m), each person on a level
    of their own, and the planted ankles stay where they are as before.  The poses are random, so the tilts are large (up to ~85
    degrees: these people walk bent over, sideways or on their backs) and the swing ankle may dip several centimetres under the
    stance level: a ground truth for the geometry of contacts, not a gait."""
    if int(stance) != stance or stance < 2:
        raise ValueError("planted_walk: stance must be an integer >= 2")
    root_s, ang = scene_walk(n_frames, n_people, seed)
    lens = np.asarray(skeleton_arrays()[1] if side_lens is None else side_lens, np.float64) * np.ones((n_people, 11))
    if floor_normal is not None:
        n = np.array(floor_normal, np.float64)
        if n.shape != (3,) or not np.all(np.isfinite(n)) or not np.linalg.norm(n) > 0:
            raise ValueError("planted_walk: floor_normal must be a finite non-zero (3,) vector")
        ang = _floor_tilt(ang, lens, int(stance), n / np.linalg.norm(n))
    rel = batched_fk(np.zeros((n_frames, n_people, 3)), ang, np.broadcast_to(lens, (n_frames, n_people, 11)))[:, :, [3, 6]]
    root = np.empty((n_frames, n_people, 3))
    contact = np.zeros((n_frames, n_people, 2), dtype=bool)
    foot = 0
    anchor = (root_s[0] if start is None else np.asarray(start, np.float64) * np.ones((n_people, 3))) + rel[0, :, foot]
    for t in range(n_frames):
        root[t] = anchor - rel[t, :, foot]
        contact[t, :, foot] = True
        if t > 0 and t % int(stance) == 0:      # the change: the other ankle, where it is now, carries on
            foot = 1 - foot
            anchor = root[t] + rel[t, :, foot]
            contact[t, :, foot] = True
    return root, ang, contact


def generate(n_frames: int, n_views: int, n_people: int, seed: int, chain_len: int = 0, dtype=np.float32,
             drop=0.05, pix_sigma=2.0, shuffle=True, frame_seed=None, occlusion=0.0, spurious=0.0, walk=None, segment: int = 0,
             floor_normal=None):
    """-> dict(kps25 (F,C,P,25,3), counts (F,C) int32, K, Rt, P, gt_joints (F,P,18,3), gt_order (F,C,P)); walk="planted":
    gt_contact (F,P,2) bool too.

    occlusion: probability that a person is missed entirely by a view in a frame (the view's list gets shorter: ragged counts,
    tracklets seen by one view or none, deaths and re-births); spurious: probability that such a freed slot holds a false
    detection instead (a random pose of plausible size that matches nobody) -- CONDITIONAL on the slot being freed, so a view's
    list is shorter with probability occlusion * (1 - spurious) per person and spurious = 1 turns every occlusion into a ghost
    (round 2 divided by ``occlusion`` here, which made every freed slot a ghost whenever spurious >= occlusion: no ragged counts).
    gt_order is -1 for slots that hold no real person.
    Both default to 0, which leaves the output of earlier versions bit for bit unchanged.

    chain_len > 0 restarts the random walk every chain_len frames (independent sub-sequences).
    Cameras depend on ``seed`` only; ``frame_seed`` (default: seed) drives people, noise and shuffles,
    so ranks can share one calibration and still own different frame shards.

    walk="scene": ONE scene for any number of shards -- the people follow scene_walk(seed) (a smooth bounded walk, no restarts; chain_len
    is ignored), bone lengths come from ``seed``, and this call returns segment ``segment`` of it (frames [segment n_frames,
    (segment + 1) n_frames)); noise, scores, drops and shuffles of a segment come from (seed, 1, segment).  The same seed on every rank
    with segment = rank cuts one sequence into contiguous shards: what the tracklet stitch has identities to carry across.
    walk="planted": the scene walk's angles, bone lengths and noise streams with the roots of planted_walk(seed) -- one foot of
    every person is planted on every frame, the stance foot changes every 8 frames --, and gt_contact (F,P,2) in the output: the
    ground truth of foot skate (segment 0 only).  floor_normal (3,) (walk="planted" only; default None: the output without the argument
    bit for bit): planted_walk's walk on one floor, every person's footholds on one plane with that normal.
    walk=None (default): the random walk above, bit for bit the output of earlier versions."""
    K, Rt, Pm = make_cameras(n_views, np.random.default_rng(seed))
    F, C, Pn = n_frames, n_views, n_people
    if floor_normal is not None and walk != "planted":
        raise ValueError("generate: floor_normal belongs to walk='planted'")
    _, side = skeleton_arrays()
    if walk == "scene":
        root, ang = scene_walk(F, Pn, seed, segment)
        lens = side * np.random.default_rng([seed, 4]).uniform(0.9, 1.1, size=(Pn, 1)) * np.ones((Pn, 11))
        frame_seed = [seed, 5, int(segment)]
        rng = np.random.default_rng(frame_seed + [1])
    elif walk == "planted":
        if segment != 0:
            raise ValueError("generate: walk='planted' has one segment")
        lens = side * np.random.default_rng([seed, 4]).uniform(0.9, 1.1, size=(Pn, 1)) * np.ones((Pn, 11))
        root, ang, gt_contact = planted_walk(F, Pn, seed, side_lens=lens, floor_normal=floor_normal)
        frame_seed = [seed, 5, 0]
        rng = np.random.default_rng(frame_seed + [1])
    elif walk is not None:
        raise ValueError("generate: walk is None (random walk, restarted every chain_len frames), 'scene' or 'planted'")
    else:
        rng = np.random.default_rng([seed if frame_seed is None else frame_seed, 1])
        L = chain_len if chain_len > 0 else F
        n_chain = (F + L - 1) // L
        root0 = np.concatenate([rng.uniform(-2, 2, size=(n_chain, Pn, 2)), rng.uniform(0.95, 1.1, size=(n_chain, Pn, 1))], -1)
        ang0 = rng.normal(0, 0.3, size=(n_chain, Pn, 18, 3))
        d_root = rng.normal(0, 0.02, size=(n_chain, L, Pn, 3)) * np.array([1, 1, 0.1])
        d_ang = rng.normal(0, 0.02, size=(n_chain, L, Pn, 18, 3))
        d_root[:, 0] = 0
        d_ang[:, 0] = 0
        root = (root0[:, None] + np.cumsum(d_root, axis=1)).reshape(n_chain * L, Pn, 3)[:F]
        ang = (ang0[:, None] + np.cumsum(d_ang, axis=1)).reshape(n_chain * L, Pn, 18, 3)[:F]
        lens = side * rng.uniform(0.9, 1.1, size=(Pn, 1)) * np.ones((Pn, 11))
    joints = batched_fk(root, ang, np.broadcast_to(lens, (F, Pn, 11)))  # (F,P,18,3)

    # 3-D points of the OpenPose-25 layout
    X = np.zeros((F, Pn, 25, 3))
    have = np.zeros(25, dtype=bool)
    for coco, sk in _COCO_FROM_SKEL.items():
        X[:, :, _OP25_OF_COCO[coco]] = joints[:, :, sk]
        have[_OP25_OF_COCO[coco]] = True
    nose, lear, rear = joints[:, :, 15], joints[:, :, 16], joints[:, :, 17]
    X[:, :, 16] = 0.6 * nose + 0.4 * lear  # L_Eye
    X[:, :, 15] = 0.6 * nose + 0.4 * rear  # R_Eye
    X[:, :, 1] = joints[:, :, 8]           # Neck
    X[:, :, 8] = joints[:, :, 0]           # Mid_Hip
    for op, ankle, dx in ((19, 3, 0.12), (20, 3, 0.10), (21, 3, -0.05), (22, 6, 0.12), (23, 6, 0.10), (24, 6, -0.05)):
        X[:, :, op] = joints[:, :, ankle] + np.array([0.0, dx, -0.05])
    # project: (F,C,P,25)
    h = np.einsum('cik,fpjk->fcpji', Pm[:, :, :3], X) + Pm[None, :, None, None, :, 3]
    uv = h[..., :2] / h[..., 2:3]
    uv = uv + rng.normal(0, pix_sigma, size=uv.shape)
    score = rng.uniform(0.5, 1.0, size=uv.shape[:-1])
    miss = rng.uniform(size=score.shape) < drop
    kps = np.concatenate([uv, score[..., None]], axis=-1)
    kps[miss] = 0.0
    order = np.broadcast_to(np.arange(Pn), (F, C, Pn)).copy()
    if shuffle:
        order = rng.permuted(order, axis=-1)
        kps = np.take_along_axis(kps, order[..., None, None], axis=2)
    counts = np.full((F, C), Pn, dtype=np.int32)
    if occlusion > 0.0 or spurious > 0.0:
        rng2 = np.random.default_rng((frame_seed + [2]) if isinstance(frame_seed, list) else [seed if frame_seed is None else frame_seed, 2])
        gone = rng2.uniform(size=(F, C, Pn)) < occlusion
        ghost = gone & (rng2.uniform(size=(F, C, Pn)) < spurious)
        centre = rng2.uniform([100.0, 100.0], [900.0, 650.0], size=(F, C, Pn, 1, 2))
        fake = np.concatenate([centre + rng2.normal(0, 60.0, size=(F, C, Pn, 25, 2)), rng2.uniform(0.3, 0.9, size=(F, C, Pn, 25, 1))], axis=-1)
        kps = np.where(ghost[..., None, None], fake, kps)
        order = np.where(gone, -1, order)
        keep = ~gone | ghost
        # compact every view's list (kept slots first, their order preserved), zero the rest
        idx = np.argsort(~keep, axis=-1, kind="stable")
        kps = np.take_along_axis(kps, idx[..., None, None], axis=2)
        order = np.take_along_axis(order, idx, axis=2)
        counts = keep.sum(axis=-1).astype(np.int32)
        kps[np.arange(Pn)[None, None, :] >= counts[..., None]] = 0.0
        order = np.where(np.arange(Pn)[None, None, :] >= counts[..., None], -1, order)
    out = dict(kps25=np.ascontiguousarray(kps.astype(dtype)), counts=counts, K=K, Rt=Rt, P=Pm,
               gt_joints=joints, gt_order=order.astype(np.int32))
    if walk == "planted":
        out["gt_contact"] = gt_contact
    return out
