"""Inputs shared by the re-linking tests (tests/test_relink_cpu.py, tests/test_gpu_relink.py): ground-truth tracks cut into pieces, the
Shelf oracle tracker's records, and MvTracklet records from (track_id, frames, joints) rows."""
import numpy as np

from conftest import load_golden

PARAMS = dict(max_gap=16, max_dist=0.5, near_dist=0.15, speed=0.03)     # the parameters every gate is stated with
CUT_CASES = [(C, P, seed) for (C, P) in ((5, 4), (8, 8)) for seed in (20270501, 20270502, 20270503, 20270504)]


def fragments(gt, seed, n_cuts, g_max, sigma):
    """gt (F,P,18,3) -> [(person, frames, joints)]: N(0, sigma) noise on every joint, every person's track cut at n_cuts frames drawn
    without replacement from 20 .. F - 21, each cut followed by a hole of 1 .. g_max frames, pieces shorter than 3 frames dropped, the
    pieces shuffled."""
    F, P = gt.shape[:2]
    rng = np.random.default_rng([seed, 77])
    noisy = gt + rng.normal(0, sigma, size=gt.shape)
    recs = []
    for p in range(P):
        cuts = np.sort(rng.choice(np.arange(20, F - 20), size=n_cuts, replace=False))
        gaps = rng.integers(1, g_max + 1, size=n_cuts)
        lo = 0
        for c, g in zip(cuts, gaps):
            if c - lo < 3:
                continue
            recs.append((p, np.arange(lo, c), noisy[lo:c, p]))
            lo = c + g - 1 + 1
        recs.append((p, np.arange(lo, F), noisy[lo:F, p]))
    order = rng.permutation(len(recs))
    return [recs[i] for i in order]


def cut_case(C, P, seed, n_frames=300, n_cuts=3):
    """(people of the pieces, records (track_id = position in the list, frames, joints)) of one cut ground-truth case."""
    from multiview_motion_capture_amd import synth
    gt = synth.generate(n_frames, C, P, seed, walk="scene")["gt_joints"]
    pieces = fragments(gt, seed, n_cuts, 16, 0.01)
    return [p for p, _, _ in pieces], [(i, f, j) for i, (_, f, j) in enumerate(pieces)]


def true_links(people, recs, max_gap=16):
    """{(A, B)}: B is the next piece of A's person and the hole between them is <= max_gap."""
    true = set()
    for i, (_, fa, _) in enumerate(recs):
        nxt = [(fb[0], j) for j, (_, fb, _) in enumerate(recs) if people[j] == people[i] and fb[0] > fa[-1]]
        if nxt:
            f0, j = min(nxt)
            if f0 - fa[-1] <= max_gap:
                true.add((i, j))
    return true


def shelf_oracle_records():
    """The noise-free oracle tracker's Shelf records [(tracker id, frames, joints)], ids ascending: a pose per row where hits grew."""
    z = load_golden("shelf_clean_oracle_tracker.npz")
    meta, nt, J = z["meta"], z["n_tracks"], z["joints"]
    rows = {}
    for f in range(meta.shape[0]):
        for s in range(nt[f]):
            i, h = int(meta[f, s, 0]), int(meta[f, s, 2])
            r = rows.setdefault(i, {"f": [], "j": [], "h": -1})
            if h > r["h"]:
                r["f"].append(f)
                r["j"].append(J[f, s])
                r["h"] = h
    return [(i, np.array(r["f"]), np.array(r["j"])) for i, r in sorted(rows.items())]


def make_tracklets(recs, state=None):
    """(track_id, frames, joints) rows -> MvTracklet records (zero pose parameters: re-linking reads the joints alone)."""
    from multiview_motion_capture_amd.inverse_kinematics import PoseShapeParam
    from multiview_motion_capture_amd.motion_capture import MvTracklet, TrackState
    from multiview_motion_capture_amd.pose_def import KpsFormat, Pose
    out = []
    for tid, frames, joints in recs:
        poses = [(int(f), PoseShapeParam(np.zeros(3), np.zeros((18, 3)), np.zeros(11)),
                  Pose(KpsFormat.BASIC_18, np.array(j, np.float64), np.ones((18, 1)), None)) for f, j in zip(frames, joints)]
        t = MvTracklet(int(tid), poses[0][0], poses[0][1], poses[0][2])
        t.frame_idxs = [p[0] for p in poses]
        t.poses = poses
        t.hits = len(poses)
        t.state = state or TrackState.Confirmed
        out.append(t)
    return out


def label_poses(frames, joints, gt_joints, frame_idx0=0, within=0.2):
    """Per pose of a record the ground-truth person nearest to it (mean joint distance) when that person is within ``within`` metres,
    else -1.  frames (n,), joints (n,18,3), gt_joints (F,P,18,3); frame f of the record is row f - frame_idx0 of gt_joints."""
    d = np.linalg.norm(np.asarray(joints)[:, None] - gt_joints[np.asarray(frames) - frame_idx0], axis=-1).mean(-1)     # (n, P)
    who = d.argmin(axis=1)
    return np.where(d[np.arange(d.shape[0]), who] <= within, who, -1)


def identity_shares(labelled, n_people):
    """labelled: per record (frames, labels).  Per person: (tracked frames, poses of the person in the person's longest record) --
    the share of the tracked frames that lie in the longest record is their ratio."""
    out = []
    for p in range(n_people):
        tracked = set()
        longest = 0
        for frames, labels in labelled:
            mine = np.asarray(frames)[np.asarray(labels) == p]
            tracked |= set(mine.tolist())
            longest = max(longest, int(mine.size))
        out.append((len(tracked), longest))
    return out
