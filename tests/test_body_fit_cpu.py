"""CPU: the body fit's NumPy restatement (tests/body_fit_np.py) on noise-free synthetic observations, its selection rule on hand-built
cases, the BVH writer's round trip, and body_fit's input checks (before any device call)."""
import numpy as np
import pytest

import body_fit_np as bf
import oracle_np as o


def _cameras(n=4, dist=5.0, f=1000.0):
    Ps = []
    for k in range(n):
        a = 2 * np.pi * k / n
        c = np.array([dist * np.cos(a), dist * np.sin(a), 1.5])
        z = -c * np.array([1, 1, 0]) / np.linalg.norm(c[:2])
        x = np.cross(z, [0, 0, 1.0])
        x /= np.linalg.norm(x)
        y = np.cross(z, x)
        R = np.stack([x, y, z])
        K = np.array([[f, 0, 500], [0, f, 400], [0, 0, 1.0]])
        Ps.append(K @ np.concatenate([R, -R @ c[:, None]], axis=1))
    return np.array(Ps)


def _coco(joints, P, drop):
    """COCO-17 rows of FK joints seen by P (noise-free), scores 1 except the eyes and one of the mid-spine's four joints."""
    k = np.zeros((17, 3))
    h = joints[o.REPROJ_SKEL_IDX] @ P[:, :3].T + P[:, 3]
    k[o.REPROJ_COCO_IDX, :2] = h[:, :2] / (1e-5 + h[:, 2:3])
    k[o.REPROJ_COCO_IDX, 2] = 1.0
    k[drop, 2] = 0.0          # -> the guessed mid-spine observation has weight 0 (it is not a joint of the skeleton)
    return k


def _scene(n_frames=12, seed=0, frozen_frame=None):
    rng = np.random.default_rng(seed)
    Ps = _cameras()
    _, ref = o.skeleton_constants()
    true = ref * rng.uniform(0.9, 1.1, 11)
    true[7] = 0.0
    views, params, joints = [], [], []
    for f in range(n_frames):
        root = np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), 1.0])
        ang = rng.normal(0, 0.25, (18, 3))
        J = o.forward_kinematics(root, ang, true)[0]
        row = []
        for c in range(4):
            seen = frozen_frame is None or f != frozen_frame or c == 0
            row.append(_coco(J, Ps[c], [5, 6, 11, 12][c])[None] if seen else np.zeros((0, 17, 3)))
        views.append(row)
        pert = true * (1 + rng.uniform(-0.15, 0.15, 11))
        params.append(np.concatenate([root, ang.ravel(), pert]))
        joints.append(o.forward_kinematics(root, ang, pert)[0])
    rec = dict(frames=np.arange(n_frames), params=np.array(params), joints=np.array(joints))
    return views, Ps, rec, true


def test_oracle_recovers_one_constant_skeleton_and_e_never_increases():
    views, Ps, rec, true = _scene(12, seed=3, frozen_frame=5)
    res = bf.fit([views], [Ps], [[rec]], rounds=3)[0][0]
    free = res["free"]
    assert free.sum() == 10 and not free[7]                     # slot 7 (Mid_Hip) is structurally unobservable
    err = np.abs(res["lens"] - true)[free]
    print("\nlength error on the free slots:", err.max(), "cost trace:", res["cost"])
    assert err.max() <= 1e-6
    c = res["cost"]
    assert np.all(np.diff(c) <= 1e-12 * c[0]), c               # E after round 0, then after every length / pose step
    assert res["lens"][7] == rec["params"][0, 57 + 7]
    # the frozen frame: one view -> its angles kept, the final lengths, joints by FK
    assert res["views"][5] == 0 and np.all(res["views"][np.arange(12) != 5] == 4)
    assert np.array_equal(res["params"][5, :57], rec["params"][5, :57])
    assert np.array_equal(res["params"][5, 57:], res["lens"])
    J = o.forward_kinematics(res["params"][5, :3], res["params"][5, 3:57], res["lens"])[0]
    assert np.array_equal(res["joints"][5], J)
    # every frame shares the one length vector
    assert np.all(res["params"][:, 57:] == res["lens"])


def test_oracle_l0_is_the_median_and_negative_lengths_pass_through():
    views, Ps, rec, _ = _scene(7, seed=4)
    rec["params"][:, 57 + 5] = -np.abs(rec["params"][:, 57 + 5])
    res = bf.fit([views], [Ps], [[rec]], rounds=0)[0][0]
    assert np.array_equal(res["lens"][:7], np.median(rec["params"][:, 57:64], axis=0)[:7])
    assert res["lens"][5] < 0 and len(res["cost"]) == 1


def _one_view(J, P, shift=0.0):
    k = _coco(J, P, 1)
    k[:, 0] += shift
    return k


def test_selection_gate_conflict_tie_and_fewer_than_two_views():
    Ps = _cameras()
    _, ref = o.skeleton_constants()
    JA = o.forward_kinematics(np.array([0.0, 0, 1]), np.zeros((18, 3)), ref)[0]
    JB = o.forward_kinematics(np.array([0.3, 0, 1]), np.zeros((18, 3)), ref)[0]
    # frame 0: camera 0 sees A exactly and B shifted by 70 px (beyond the 56.44 px floor); cameras 1-3 see A exactly
    v0 = [np.array([_one_view(JA, Ps[0]), _one_view(JB, Ps[0], 70.0)])] + [np.array([_one_view(JA, Ps[c])]) for c in (1, 2, 3)]
    # gate: B's only pose in camera 0 is beyond the floor, and in cameras 1-3 it loses A's pose to record A (smaller distance)
    sel, dist, nv = bf.select([(0, 0, 0, JA), (0, 0, 1, JB)], [[v0]], [Ps])
    assert sel[0].tolist() == [0, 0, 0, 0] and nv[0] == 4
    assert sel[1].tolist() == [-1, -1, -1, -1] and nv[1] == 0
    d_gate = bf.reproj_dist(JB, v0[0][1], Ps[0])
    assert d_gate > bf.D_MAX and d_gate < 80
    # the conflict: the loser takes nothing in that camera, not its second choice
    v1 = [np.array([_one_view(JA, Ps[c]), _one_view(JA, Ps[c], 30.0)]) for c in range(4)]
    JA2 = JA + np.array([0.01, 0, 0])
    sel, dist, nv = bf.select([(0, 0, 0, JA2), (0, 0, 1, JA)], [[v1]], [Ps])
    assert sel[1].tolist() == [0, 0, 0, 0] and sel[0].tolist() == [-1] * 4 and nv.tolist() == [0, 4]
    # a tie goes to the earlier record in the caller's list, whatever the problem order
    sel, _, nv = bf.select([(0, 0, 1, JA), (0, 0, 0, JA)], [[v1]], [Ps])
    assert sel[1].tolist() == [0, 0, 0, 0] and sel[0].tolist() == [-1] * 4
    # two sequences never compete, even on the same frame number
    sel, _, nv = bf.select([(0, 0, 0, JA), (1, 0, 0, JA)], [[v1], [v1]], [Ps, Ps])
    assert nv.tolist() == [4, 4]
    # fewer than two views: frozen in the fit
    views, Ps2, rec, _ = _scene(3, seed=5, frozen_frame=1)
    res = bf.fit([views], [Ps2], [[rec]], rounds=1)[0][0]
    assert res["views"].tolist() == [4, 0, 4]


class _P:
    def __init__(self, root, euler, lens):
        self.root, self.euler_angles, self.bone_lens = root, euler, lens


class _Pose:
    def __init__(self, j):
        self.keypoints = j


class _Rec:
    def __init__(self, frames, params, joints, tid=0):
        self.track_id, self.frame_idxs = tid, list(frames)
        self.poses = [(f, _P(p[:3], p[3:57].reshape(18, 3), p[57:]), _Pose(j)) for f, p, j in zip(frames, params, joints)]
        self.state, self.hits, self.time_since_update = 2, len(frames), 0


def _parse_bvh(text):
    """A small BVH reader: (names, parents, offsets, channel counts, motion rows)."""
    tok = text.split()
    names, parents, offsets, nch, stack = [], [], [], [], []
    i = 1
    last = None
    while tok[i] != "MOTION":
        t = tok[i]
        if t in ("ROOT", "JOINT"):
            names.append(tok[i + 1])
            parents.append(stack[-1] if stack else -1)
            last = len(names) - 1
            i += 2
        elif t == "End":
            last = None
            i += 2
        elif t == "{":
            stack.append(last)
            i += 1
        elif t == "}":
            stack.pop()
            i += 1
        elif t == "OFFSET":
            if last is not None:
                offsets.append([float(x) for x in tok[i + 1:i + 4]])
            i += 4
        elif t == "CHANNELS":
            n = int(tok[i + 1])
            nch.append((n, tok[i + 2:i + 2 + n]))
            i += 2 + n
        else:
            raise AssertionError(t)
    n_frames = int(tok[i + 2])
    ft = float(tok[i + 5])
    vals = np.array([float(x) for x in tok[i + 6:]]).reshape(n_frames, -1)
    return names, parents, np.array(offsets), nch, vals, ft


def _rot(axis, deg):
    a = np.radians(deg)
    c, s = np.cos(a), np.sin(a)
    return {"X": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "Y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]),
            "Z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])}[axis]


def _bvh_fk(names, parents, offsets, nch, row):
    pos, G, at = {}, {}, 0
    for j in range(len(names)):
        n, chans = nch[j]
        v = row[at:at + n]
        at += n
        R = np.eye(3)
        t = np.zeros(3)
        for c, x in zip(chans, v):
            if c.endswith("position"):
                t["XYZ".index(c[0])] = x
            else:
                R = R @ _rot(c[0], x)
        p = parents[j]
        if p < 0:
            G[j], pos[j] = R, t + offsets[j]
        else:
            G[j], pos[j] = G[p] @ R, pos[p] + G[p] @ offsets[j]
    return pos


def test_save_bvh_round_trip_gaps_and_refusal(tmp_path):
    from multiview_motion_capture_amd.bvh_export import save_bvh
    from multiview_motion_capture_amd.pose_def import KpsFormat, get_kps_order
    rng = np.random.default_rng(7)
    _, ref = o.skeleton_constants()
    lens = ref * 1.05
    frames = [10, 11, 13, 16]
    params = np.array([np.concatenate([rng.normal(0, 1, 3), rng.normal(0, 0.6, 54), lens]) for _ in frames])
    joints = np.array([o.forward_kinematics(p[:3], p[3:57], lens)[0] for p in params])
    path = tmp_path / "t.bvh"
    save_bvh(str(path), _Rec(frames, params, joints), frame_time=1 / 25)
    names, parents, offsets, nch, vals, ft = _parse_bvh(path.read_text())
    order = [[k.name for k in get_kps_order(KpsFormat.BASIC_18)].index(nm) for nm in names]
    assert sorted(order) == list(range(18)) and abs(ft - 0.04) < 1e-9
    assert nch[0][1] == ["Xposition", "Yposition", "Zposition", "Xrotation", "Yrotation", "Zrotation"]
    assert all(c[1] == ["Xrotation", "Yrotation", "Zrotation"] for c in nch[1:])
    assert [order[p] if p >= 0 else -1 for p in parents] == [int(o.SKEL_PARENTS[j]) for j in order]
    assert vals.shape[0] == 7                                   # frames 10 .. 16
    src = [0, 1, 1, 2, 2, 2, 3]                                 # gaps repeat the previous updated frame
    worst = 0.0
    for r, k in enumerate(src):
        pos = _bvh_fk(names, parents, offsets, nch, vals[r])
        worst = max(worst, max(np.abs(pos[i] - joints[k][order[i]]).max() for i in range(18)))
    print("\nBVH round trip: worst joint difference", worst)
    assert worst <= 1e-6
    assert np.array_equal(vals[2], vals[1]) and np.array_equal(vals[4], vals[3])
    params[2, 57 + 3] *= 1.01
    with pytest.raises(ValueError):
        save_bvh(str(tmp_path / "u.bvh"), _Rec(frames, params, joints))


def test_body_fit_input_checks_run_before_any_device_call(monkeypatch):
    from multiview_motion_capture_amd import body_fit, device as dev
    from multiview_motion_capture_amd.common import Calib

    def boom(*a, **k):
        raise AssertionError("device called")
    for name in ("ingest", "body_observe", "body_lengths", "ik_solve_stages_rigs", "fk"):
        monkeypatch.setattr(dev, name, boom)
    Ps = _cameras()
    cal = [Calib.from_k_rt(np.eye(3), np.concatenate([np.eye(3), np.zeros((3, 1))], 1)) for _ in range(4)]
    kps = np.zeros((5, 4, 2, 25, 3))
    cnt = np.zeros((5, 4), np.int32)
    _, ref = o.skeleton_constants()
    p = np.concatenate([np.zeros(57), ref])
    good = _Rec([0, 1], [p, p], np.zeros((2, 18, 3)))
    with pytest.raises(ValueError, match="outside"):
        body_fit.fit_tracklets([_Rec([0, 5], [p, p], np.zeros((2, 18, 3)))], kps, cnt, cal)
    with pytest.raises(ValueError, match="calibrations"):
        body_fit.fit_tracklets([good], kps, cnt, cal[:3])
    with pytest.raises(ValueError):
        body_fit.fit_tracklets([good], kps[:, :, :, :20], cnt, cal)
    with pytest.raises(ValueError):
        body_fit.fit_tracklets([good], kps, cnt[:4], cal)
    with pytest.raises(ValueError, match="record lists"):
        body_fit.fit_sequences([(kps, cnt, cal)], [[good], []])
    with pytest.raises(ValueError):
        body_fit.fit_tracklets([good], kps, cnt, cal, rounds=-1)
    with pytest.raises(ValueError):
        body_fit.fit_tracklets([good], kps, cnt, cal, max_iter=99)
    with pytest.raises(ValueError, match="twice"):
        body_fit.fit_tracklets([_Rec([1, 1], [p, p], np.zeros((2, 18, 3)))], kps, cnt, cal)
    bad = _Rec([0, 1], [p[:60], p[:60]], np.zeros((2, 18, 3)))
    with pytest.raises(ValueError, match="PoseShapeParam"):
        body_fit.fit_tracklets([bad], kps, cnt, cal)
    assert body_fit.fit_sequences([], []) == []
