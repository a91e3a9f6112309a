"""Inputs shared by the re-identification tests (tests/test_reid_cpu.py, tests/test_gpu_reid.py) and tools (tools/reid_sweep.py,
tools/reid_probe.py): hand-built records whose bone lengths are exact binary fractions, so that every signature and z can be worked by
hand, and ground-truth scene walks cut into pieces with long holes."""
import numpy as np

from reid_np import PARENTS, SIDE_MAP, SIDES

PARAMS = dict(max_z=2.0, ratio=0.7, floor=0.002, min_poses=10, reach=1.0, speed=0.08, max_gap=None)    # every hand-built case's


def defaults():
    """The defaults of relinking.reidentify_sequences, as keywords of reid_np.reidentify."""
    from multiview_motion_capture_amd import relinking as r
    return dict(max_z=r.MAX_Z, ratio=r.RATIO, floor=r.FLOOR, min_poses=r.MIN_POSES, reach=r.REACH, speed=r.REID_SPEED, max_gap=None)


# Seeds other than the sweep's (tools/reid_sweep.py: 202806xx), picked among 20280701 .. 20280708 so that the restatement takes no link
# between two people at the defaults at sigma = 1 cm and 2 cm.  Not every seed does: (8, 8, 20280702) takes ONE wrong link at 2 cm with
# the veto on (none at 1 cm).  Without the veto (8,8) 20280701, 20280704, 20280707 and (5,4) 20280708 take wrong links.
CUT_CASES = [(5, 4, s) for s in (20280701, 20280702, 20280703, 20280708)] + [(8, 8, s) for s in (20280701, 20280703, 20280704, 20280707)]
SIGMAS = (0.01, 0.02)
BASE = np.array([32, 56, 52, 20, 36, 32, 12, 28, 36, 16]) / 128.0     # metres, the ten sides in SIDES order: exact in binary
SIDE_INDEX = {k: q for q, k in enumerate(SIDES)}


def skeleton(lengths, origin=(0.0, 0.0, 0.0), right=None):
    """(18,3): joint j = its parent + its bone along axis j % 3; bone j has the length of its side (``right`` (10,): the lengths of the
    right-hand bones -- the second bone in joint order -- where they differ).  With lengths and an origin that are multiples of 1/128
    every coordinate is exact, so b_j is the length itself."""
    J = np.zeros((18, 3))
    J[0] = origin
    seen = set()
    for j in range(1, 18):
        q = SIDE_INDEX[int(SIDE_MAP[j])]
        length = lengths[q] if (right is None or q not in seen) else right[q]
        seen.add(q)
        J[j] = J[PARENTS[j]]
        J[j, j % 3] += length
    return J


def record(tid, first, n, lengths, origin=(0.0, 0.0, 0.0), nan_joints=(), right=None):
    """(track_id, frames first .. first + n - 1, joints): n copies of one skeleton; joints ``nan_joints`` are NaN in every pose but
    the first and the last (a record end with a NaN joint has no centroid and links to nothing)."""
    J = np.repeat(skeleton(np.asarray(lengths, np.float64), origin, right)[None], n, axis=0)
    for j in nan_joints:
        J[1:-1, j] = np.nan
    return (tid, np.arange(first, first + n), J)


def z_of(delta, floor=PARAMS["floor"]):
    """z of two records without spread (se = 0) whose ten sides all differ by delta: |delta| / (floor sqrt 2)."""
    return abs(delta) / (floor * np.sqrt(2.0))


DB = 1.0 / 2048      # all ten sides longer by this: z = 0.1726 at the floor of 2 mm
DQ = 1.0 / 32768     # z = 0.0108
DX = 1.0 / 16        # z = 22.1
FAR = (64.0, 0.0, 0.0)


def link_cases():
    """name -> (records, {(track id of A, track id of B)} the links to be taken, params).  Every decision stays a factor 10 clear of
    its threshold in z (z = 0 or 0.17 against max_z = 2, and against ratio x 0.0108 = 0.0076 in the veto; 22 against max_z), or
    0.1 m clear of the reach."""
    P = PARAMS
    c = {}
    # Q (id 2) matches the other end far better (z = 0.0108) than B matches A (z = 0.1726); it is too far away to be linked itself
    c["veto by a record that overlaps B"] = ([record(0, 0, 20, BASE), record(1, 60, 20, BASE + DB), record(2, 50, 40, BASE + DQ, FAR)],
                                             set(), P)
    c["veto by a record that overlaps A"] = ([record(0, 0, 20, BASE + DB), record(1, 60, 20, BASE), record(2, 5, 30, BASE + DQ, FAR)],
                                             set(), P)
    c["no veto by a record that overlaps both ends"] = ([record(0, 0, 20, BASE), record(1, 60, 20, BASE + DB),
                                                         record(2, 0, 100, BASE + DQ, FAR)], {(0, 1)}, P)
    c["a chain of three"] = ([record(5, 0, 20, BASE), record(3, 50, 20, BASE), record(4, 120, 20, BASE)], {(5, 3), (3, 4)}, P)
    c["a tie goes to the lowest column"] = ([record(0, 0, 20, BASE), record(2, 40, 20, BASE), record(1, 40, 20, BASE, (0.5, 0.0, 0.0))],
                                            {(0, 1)}, P)
    c["gap 0"] = ([record(0, 0, 20, BASE), record(1, 19, 20, BASE)], set(), P)
    c["gap 1"] = ([record(0, 0, 20, BASE), record(1, 20, 20, BASE)], {(0, 1)}, P)
    c["gap at max_gap"] = ([record(0, 0, 20, BASE), record(1, 49, 20, BASE)], {(0, 1)}, dict(P, max_gap=30))
    c["gap over max_gap"] = ([record(0, 0, 20, BASE), record(1, 50, 20, BASE)], set(), dict(P, max_gap=30))
    c["within reach"] = ([record(0, 0, 20, BASE), record(1, 29, 20, BASE, (1.6875, 0.0, 0.0))], {(0, 1)}, P)       # 1.8 m at gap 10
    c["out of reach"] = ([record(0, 0, 20, BASE), record(1, 29, 20, BASE, (1.90625, 0.0, 0.0))], set(), P)
    c["z a tenth of max_z"] = ([record(0, 0, 20, BASE), record(1, 40, 20, BASE + DB)], {(0, 1)}, P)
    c["z ten times max_z"] = ([record(0, 0, 20, BASE), record(1, 40, 20, BASE + DX)], set(), P)
    # (two values are fewer than min_poses) joint 8 NaN removes the sides of bones 8, 9, 12, 15 (sides 9, 3, 10); joints 3 and 11 (leaves) sides 2 and 5; joint 16 side 6
    c["five common sides"] = ([record(0, 0, 20, BASE), record(1, 40, 20, BASE, nan_joints=(8, 3, 11))], {(0, 1)}, P)
    c["four common sides"] = ([record(0, 0, 20, BASE), record(1, 40, 20, BASE, nan_joints=(8, 3, 11, 16))], set(), P)
    c["nine poses"] = ([record(0, 0, 9, BASE), record(1, 40, 20, BASE)], set(), P)
    c["ten poses"] = ([record(0, 0, 10, BASE), record(1, 40, 20, BASE)], {(0, 1)}, P)
    return c


def taken(recs, res):
    """The links of a result (order, succ over the nodes) as {(track id of A, track id of B)}."""
    o = res["order"]
    return {(int(recs[o[i]][0]), int(recs[o[j]][0])) for i, j in enumerate(res["succ"]) if j >= 0}


def long_hole_fragments(gt, seed, sigma, n_cuts=2, g_min=20, g_max=80):
    """relink_cases.fragments' scheme with long holes: gt (F,P,18,3) -> [(person, frames, joints)]: N(0, sigma) noise on every joint,
    every person's track cut at n_cuts frames drawn without replacement from 40 .. F - 41, each cut followed by a hole of g_min ..
    g_max frames, pieces shorter than 3 frames dropped, the pieces shuffled."""
    F, P = gt.shape[:2]
    rng = np.random.default_rng([seed, 78])
    noisy = gt + rng.normal(0, sigma, size=gt.shape)
    recs = []
    for p in range(P):
        cuts = np.sort(rng.choice(np.arange(40, F - 40), size=n_cuts, replace=False))
        gaps = rng.integers(g_min, g_max + 1, size=n_cuts)
        lo = 0
        for c, g in zip(cuts, gaps):
            if c - lo >= 3:
                recs.append((p, np.arange(lo, c), noisy[lo:c, p]))
            lo = max(lo, c + g)
        if F - lo >= 3:
            recs.append((p, np.arange(lo, F), noisy[lo:F, p]))
    order = rng.permutation(len(recs))
    return [recs[i] for i in order]


_GT = {}


def scene_gt(C, P, seed, n_frames=400):
    """The ground-truth joints (F,P,18,3) of one scene walk (computed once per process)."""
    from multiview_motion_capture_amd import synth
    key = (C, P, seed, n_frames)
    if key not in _GT:
        _GT[key] = synth.generate(n_frames, C, P, seed, walk="scene")["gt_joints"]
    return _GT[key]


def cut_case(C, P, seed, sigma, n_frames=400, same_lengths=None):
    """(people of the pieces, records (track_id = position in the list, frames, joints)) of one cut scene walk.  same_lengths = (p, q):
    person q gets person p's skeleton -- q's joints are rebuilt from q's own bone directions with p's bone lengths."""
    gt = scene_gt(C, P, seed, n_frames)
    if same_lengths is not None:
        gt = gt.copy()
        p, q = same_lengths
        b_p = np.linalg.norm(gt[:, p, 1:] - gt[:, p, PARENTS[1:]], axis=-1).mean(axis=0)     # (17,)
        new = gt[:, q].copy()
        for j in range(1, 18):
            d = gt[:, q, j] - gt[:, q, PARENTS[j]]
            new[:, j] = new[:, PARENTS[j]] + d / np.linalg.norm(d, axis=-1, keepdims=True) * b_p[j - 1]
        gt[:, q] = new
    pieces = long_hole_fragments(gt, seed, sigma)
    return [p for p, _, _ in pieces], [(i, f, j) for i, (_, f, j) in enumerate(pieces)]


def true_links(people, recs):
    """{(A, B)} positions in recs: B is the next piece of A's person."""
    from relink_cases import true_links as tl
    return tl(people, recs, max_gap=10 ** 9)


def hide_people(g, hidden):
    """A copy of synth.generate's dict with people's detections removed in EVERY view: hidden = [(person, first frame, frames)].  Each
    view's list is compacted (the kept slots first, their order preserved) and its count lowered, through gt_order."""
    kps, order, counts = g["kps25"].copy(), g["gt_order"].copy(), g["counts"].copy()
    Pn = order.shape[2]
    for person, f0, n in hidden:
        for f in range(f0, f0 + n):
            for c in range(order.shape[1]):
                keep = (order[f, c] != person) & (np.arange(Pn) < counts[f, c])
                idx = np.argsort(~keep, kind="stable")
                kps[f, c], order[f, c] = kps[f, c, idx], order[f, c, idx]
                counts[f, c] = int(keep.sum())
                kps[f, c, counts[f, c]:] = 0.0
                order[f, c, counts[f, c]:] = -1
    return dict(g, kps25=kps, gt_order=order, counts=counts)


def random_sequence(n_records, seed, poses=12, people=5):
    """n_records records of ``poses`` poses each of ``people`` skeletons (BASE scaled by 0.9 .. 1.1) with 3 mm of noise on every joint,
    a NaN joint here and there, starting at random frames of 0 .. 40 n_records / people within a metre of each other: many overlap,
    many do not.  track_id = position in the list."""
    rng = np.random.default_rng([seed, 79])
    scale = rng.uniform(0.9, 1.1, size=people)
    recs = []
    for i in range(n_records):
        p = int(rng.integers(people))
        first = int(rng.integers(0, 40 * n_records // people + 1))
        J = np.repeat(skeleton(BASE * scale[p], rng.uniform(-0.5, 0.5, size=3))[None], poses, axis=0)
        J = J + rng.normal(0, 0.003, size=J.shape)
        if rng.uniform() < 0.3:
            J[int(rng.integers(1, poses - 1)), int(rng.integers(18))] = np.nan
        recs.append((i, np.arange(first, first + poses), J))
    return recs
