"""Hand-built cases of the exchange repair (tests/exchange_np.py is the rule; test_exchange_cpu.py gates the restatement on them,
test_gpu_exchange.py the device).  Two people in a T-pose, a couple of metres apart, seen by two or three cameras five metres away
that look at them from the front and from 35 degrees to either side: in every view left and right are tens of pixels apart, so the
truth is unambiguous.  The clean keypoints ARE the projections of the joints (the eyes, the neck, the mid hip and the feet, which the
rule never reads, are put beside them); a case then exchanges limbs, zeroes scores or moves single keypoints, and carries what the
repair has to report:

  seqs      [(kps (F,C,P,25|17,3), counts (F,C) i32, P (C,3,4), K (C,3,3), Rt (C,3,4))]
  records   per sequence [dict(frames (n,), joints (n,18,3))]
  params    dict(margin_px, ratio) the case runs at (the defaults unless it says otherwise)
  flags     per sequence (F,C,P) u8 the truth; record: per sequence (F,C,P) i32 the truth (-1: nobody selects the slot)
  nan_cost  [(sequence, frame, camera, slot, group)] selected slots whose group must come out undecided (NaN costs)

At most 8 problems per case."""
import numpy as np

import oracle_np as o

ARMS, LEGS, FACE = 1, 2, 4
FOCAL, CENTRE, DIST = 1000.0, 500.0, 5.0


def rest_joints():
    """BASIC_18 rest pose (T-pose, z up, the left side at +x), the pelvis one metre above the floor."""
    J = np.zeros((18, 3))
    for j in range(1, 18):
        J[j] = J[o.SKEL_PARENTS[j]] + o._SKEL_OFFSETS[j]
    return J + np.array([0.0, 0.0, 1.0])


def camera(azimuth_deg, height=1.2):
    """K, Rt of a camera DIST metres from the origin at this azimuth (0: straight in front, on the -y side), looking at (0, 0, 1)."""
    a = np.deg2rad(azimuth_deg)
    eye = np.array([DIST * np.sin(a), -DIST * np.cos(a), height])
    z = np.array([0.0, 0.0, 1.0]) - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, np.array([0.0, 0.0, 1.0]))
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.array([x, y, z])
    K = np.array([[FOCAL, 0.0, CENTRE], [0.0, FOCAL, CENTRE], [0.0, 0.0, 1.0]])
    return K, np.concatenate([R, (-R @ eye)[:, None]], axis=1)


def project(J, P):
    h = J @ P[:, :3].T + P[:, 3]
    return h[:, :2] / (1e-5 + h[:, 2:3])


def clean_pose(J, P, n_joints):
    """The detection of joints J (18,3) in camera P: (17|25, 3), every score 0.9."""
    uv = project(J, P)
    k17 = np.zeros((17, 3))
    k17[o.REPROJ_COCO_IDX, :2] = uv[o.REPROJ_SKEL_IDX]
    k17[1, :2] = 0.5 * (k17[0, :2] + k17[3, :2])          # the eyes between the nose and the ears
    k17[2, :2] = 0.5 * (k17[0, :2] + k17[4, :2])
    k17[:, 2] = 0.9
    if n_joints == 17:
        return k17
    k25 = np.zeros((25, 3))
    k25[o.OPENPOSE25_TO_COCO17] = k17
    k25[1, :2] = 0.5 * (k17[5, :2] + k17[6, :2])          # neck, mid hip
    k25[8, :2] = 0.5 * (k17[11, :2] + k17[12, :2])
    for n, d in enumerate(((6.0, 4.0), (9.0, 3.0), (-3.0, 5.0))):   # big toe, small toe, heel beside each ankle
        k25[19 + n, :2] = k17[15, :2] + np.array(d)
        k25[22 + n, :2] = k17[16, :2] + np.array([-d[0], d[1]])
    k25[[1, 8] + list(range(19, 25)), 2] = 0.8
    return k25


def people(n_frames):
    """joints (F, 2, 18, 3): person 0 walks along x, person 1 stands 1.3 m to the side with the arms a little lower."""
    J0 = rest_joints()
    J1 = rest_joints() + np.array([1.3, 0.4, 0.0])
    J1[[10, 11], 2] -= 0.15
    J1[[13, 14], 2] -= 0.25
    out = np.zeros((n_frames, 2, 18, 3))
    for f in range(n_frames):
        out[f, 0] = J0 + np.array([-0.6 + 0.05 * f, 0.02 * f, 0.0])
        out[f, 1] = J1
    return out


def scene(n_frames=2, azimuths=(0.0, 35.0, -35.0), n_joints=17, dtype=np.float64, n_slots=2, holes=None):
    """A clean sequence and one record per person.  Camera 1 lists the people in reverse order.  holes: {person: frames left out}."""
    cams = [camera(a) for a in azimuths]
    K, Rt = np.array([c[0] for c in cams]), np.array([c[1] for c in cams])
    P = np.array([k @ rt for k, rt in cams])
    J = people(n_frames)
    C = len(azimuths)
    kps = np.zeros((n_frames, C, n_slots, n_joints, 3), dtype)
    slot = np.zeros((C, 2), int)
    for c in range(C):
        slot[c] = (1, 0) if c == 1 else (0, 1)
        for f in range(n_frames):
            for p in range(2):
                kps[f, c, slot[c, p]] = clean_pose(J[f, p], P[c], n_joints)
    counts = np.full((n_frames, C), 2, np.int32)
    records = []
    for p in range(2):
        fr = np.array([f for f in range(n_frames) if f not in (holes or {}).get(p, ())])
        records.append(dict(frames=fr, joints=J[fr, p].copy()))
    truth_record = -np.ones((n_frames, C, n_slots), np.int32)
    for p in range(2):
        for f in records[p]["frames"]:
            truth_record[f, np.arange(C), slot[:, p]] = p
    return dict(kps=kps, counts=counts, P=P, K=K, Rt=Rt, J=J, slot=slot, records=records, record=truth_record,
                flags=np.zeros((n_frames, C, n_slots), np.uint8))


def rows_of(n_joints, bits):
    """(left, right) rows a detector that exchanges these groups swaps -- written out here, not taken from the code under test."""
    r17 = {ARMS: [(5, 6), (7, 8), (9, 10)], LEGS: [(11, 12), (13, 14), (15, 16)], FACE: [(1, 2), (3, 4)]}
    r25 = {ARMS: [(5, 2), (6, 3), (7, 4)], LEGS: [(12, 9), (13, 10), (14, 11), (19, 22), (20, 23), (21, 24)], FACE: [(16, 15), (18, 17)]}
    tab = r17 if n_joints == 17 else r25
    return [p for b in (ARMS, LEGS, FACE) if bits & b for p in tab[b]]


def exchange(sc, f, c, person, bits):
    """Exchange the groups ``bits`` of a person's detection in (frame, camera), and expect the repair to say so."""
    p = sc["slot"][c, person]
    k = sc["kps"][f, c, p]
    for l, r in rows_of(k.shape[0], bits):
        k[[l, r]] = k[[r, l]]
    sc["flags"][f, c, p] |= bits


def row(sc, coco):
    """The array row of a COCO-17 keypoint in the scene's format."""
    return coco if sc["kps"].shape[3] == 17 else int(o.OPENPOSE25_TO_COCO17[coco])


def case(name, scs, params=None, nan_cost=()):
    scs = scs if isinstance(scs, list) else [scs]
    assert sum(len(r["frames"]) for s in scs for r in s["records"]) <= 8, name
    return dict(name=name, seqs=[(s["kps"], s["counts"], s["P"], s["K"], s["Rt"]) for s in scs], records=[s["records"] for s in scs],
                params=dict(dict(margin_px=4.0, ratio=0.7), **(params or {})), flags=[s["flags"] for s in scs],
                record=[s["record"] for s in scs], nan_cost=list(nan_cost), J=[s["J"] for s in scs])


def _ears(sc, f, c, person):
    """(slot, row of the left ear, row of the right ear, pL, pR, D): the projected ears of a person and their distance in pixels."""
    uv = project(sc["J"][f, person], sc["P"][c])
    pL, pR = uv[16], uv[17]
    return sc["slot"][c, person], row(sc, 3), row(sc, 4), pL, pR, float(np.linalg.norm(pL - pR))


def _threshold(which, side):
    """The face of person 0 in (frame 0, camera 0) with the keypoint filed as the left ear ON the right ear's projection and the one
    filed as the right ear s pixels beyond the left ear's, away from the right: e1 = s, e0 = 2 D + s, n = 2.  The margin inequality
    reads margin < D, the ratio's s (1 - ratio) < 2 ratio D; at s = D: ratio > 1/3.  side +1: just inside (exchanged), -1: just outside."""
    sc = scene(2, n_joints=17, dtype=np.float64)
    p, l, r, pL, pR, D = _ears(sc, 0, 0, 0)
    away = (pL - pR) / D
    k = sc["kps"][0, 0, p]
    k[l, :2] = pR
    k[r, :2] = pL + D * away
    eps = 1e-6 * side
    params = dict(margin_px=D * (1.0 - eps), ratio=1.0) if which == "margin" else dict(margin_px=0.0, ratio=(1.0 + eps) / 3.0)
    if side > 0:
        sc["flags"][0, 0, p] = FACE
    return case(f"{which} {'inside' if side > 0 else 'outside'}", sc, params)


def all_cases():
    out = []
    # nothing exchanged (BODY_25, float32)
    out.append(case("clean body25 f32", scene(2, n_joints=25, dtype=np.float32)))
    # arms, legs or face exchanged in one camera each
    sc = scene(2, n_joints=17, dtype=np.float64)
    exchange(sc, 0, 0, 0, ARMS)
    exchange(sc, 0, 1, 1, LEGS)
    exchange(sc, 1, 2, 0, FACE)
    out.append(case("single groups coco17 f64", sc))
    sc = scene(2, n_joints=25, dtype=np.float64)
    exchange(sc, 1, 0, 1, ARMS)
    exchange(sc, 0, 2, 0, LEGS)
    exchange(sc, 1, 1, 0, FACE)
    exchange(sc, 0, 1, 1, ARMS | LEGS)
    out.append(case("single groups body25 f64", sc))
    # a whole-body flip: its as-is distance lies beyond max_dist (the CPU test asserts it)
    sc = scene(2, n_joints=17, dtype=np.float32)
    exchange(sc, 0, 1, 0, ARMS | LEGS | FACE)
    exchange(sc, 1, 0, 1, ARMS | LEGS | FACE)
    out.append(case("whole body flip coco17 f32", sc))
    # one keypoint of a pair at score 0: the pair is not counted, its triples are swapped all the same
    sc = scene(2, n_joints=25, dtype=np.float32)
    exchange(sc, 0, 0, 0, ARMS)
    sc["kps"][0, 0, sc["slot"][0, 0], row(sc, 7)] = 0.0
    sc["kps"][1, 2, sc["slot"][2, 1], row(sc, 14)] = 0.0
    out.append(case("one of a pair unseen body25 f32", sc))
    # a group without a fully valid pair: undecided
    sc = scene(2, n_joints=17, dtype=np.float64)
    p = sc["slot"][1, 0]
    sc["kps"][0, 1, p][[11, 13, 15], 2] = 0.0
    exchange(sc, 0, 1, 0, ARMS)
    out.append(case("legs undecided coco17 f64", sc, nan_cost=[(0, 0, 1, p, 1)]))
    # an exact tie: both ears on one representable point, margin 0 and ratio 1 -> e0 == e1 bit for bit, left alone
    sc = scene(2, n_joints=17, dtype=np.float32)
    p, l, r, pL, pR, D = _ears(sc, 0, 0, 0)
    sc["kps"][0, 0, p][[l, r], :2] = np.round(0.5 * (pL + pR))
    out.append(case("exact tie coco17 f32", sc, dict(margin_px=0.0, ratio=1.0)))
    # e1 just under and just over each inequality
    out += [_threshold(w, s) for w in ("margin", "ratio") for s in (+1, -1)]
    # two records competing for one pose: on distance (the nearer keeps it in every camera) ...
    sc = scene(2, n_joints=17, dtype=np.float64)
    exchange(sc, 0, 0, 0, LEGS)
    sc["records"][1] = dict(frames=sc["records"][0]["frames"].copy(), joints=sc["records"][0]["joints"] + np.array([0.02, 0.0, 0.01]))
    sc["record"][sc["record"] == 1] = -1
    out.append(case("two records, the nearer wins", sc))
    # ... and on rank: the same joints twice, the earlier record keeps the pose; record 2 follows person 1
    sc = scene(2, n_joints=25, dtype=np.float64)
    exchange(sc, 1, 1, 0, ARMS)
    exchange(sc, 1, 2, 1, LEGS)
    sc["records"] = [sc["records"][0], dict(frames=sc["records"][0]["frames"].copy(), joints=sc["records"][0]["joints"].copy()),
                     sc["records"][1]]
    sc["record"][sc["record"] == 1] = 2
    out.append(case("two records, the earlier wins", sc))
    # a camera without detections
    sc = scene(2, n_joints=17, dtype=np.float32)
    exchange(sc, 0, 0, 1, ARMS)
    exchange(sc, 1, 2, 0, FACE)
    sc["counts"][:, 1] = 0
    sc["record"][:, 1] = -1
    out.append(case("a camera with count 0", sc))
    # a non-finite keypoint: the pose is nobody's candidate
    sc = scene(2, n_joints=17, dtype=np.float64)
    exchange(sc, 0, 2, 0, ARMS)
    p = sc["slot"][0, 1]
    sc["kps"][1, 0, p, 8, 0] = np.nan
    sc["record"][1, 0, p] = -1
    exchange(sc, 1, 1, 1, LEGS)
    out.append(case("a non-finite keypoint", sc))
    # two sequences of three cameras with different rigs and person slots in one call, and one of two cameras beside them
    a = scene(2, azimuths=(0.0, 35.0, -35.0), n_joints=25, dtype=np.float32)
    b = scene(1, azimuths=(10.0, -25.0, 40.0), n_joints=25, dtype=np.float32, n_slots=3)
    c = scene(1, azimuths=(-15.0, 30.0), n_joints=25, dtype=np.float32)
    exchange(a, 1, 0, 0, ARMS)
    exchange(b, 0, 1, 1, LEGS | FACE)
    exchange(b, 0, 2, 0, ARMS)
    exchange(c, 0, 1, 0, ARMS | LEGS | FACE)
    out.append(case("three sequences, two camera counts", [a, b, c]))
    # a record with a hole in its frames
    sc = scene(4, n_joints=17, dtype=np.float64, holes={0: (1,), 1: (0, 2)})
    exchange(sc, 0, 0, 0, ARMS)
    exchange(sc, 1, 1, 0, LEGS)        # person 0 has no record frame here: nobody selects the pose, it stays exchanged
    sc["flags"][1, 1, sc["slot"][1, 0]] = 0
    exchange(sc, 3, 2, 1, FACE)
    exchange(sc, 2, 0, 0, LEGS)
    out.append(case("records with holes", sc))
    return out


ARMS25, LEGS25 = ((2, 5), (3, 6), (4, 7)), ((9, 12), (10, 13), (11, 14))      # tools/smooth_robust_probe.py's BODY_25 pairs


def draw_exchanges(kps25, seed):
    """tools/smooth_robust_probe.py's exchanges (its first three draws): 20 % of the slots, the arms OR the legs.
    -> (copy with the exchanges, (F,C,P) u8 flag bits drawn)."""
    rng = np.random.default_rng(seed)
    k = np.array(kps25, copy=True)
    F, C, P = k.shape[:3]
    swap = rng.random((F, C, P)) < 0.2
    arms = rng.random((F, C, P)) < 0.5
    for pairs, which in ((ARMS25, swap & arms), (LEGS25, swap & ~arms)):
        for a, b in pairs:
            ka, kb = k[..., a, :].copy(), k[..., b, :].copy()
            k[..., a, :] = np.where(which[..., None], kb, ka)
            k[..., b, :] = np.where(which[..., None], ka, kb)
    return k, ((swap & arms) * 1 + (swap & ~arms) * 2).astype(np.uint8)


class _Param:
    def __init__(self):
        self.root, self.euler_angles, self.bone_lens = np.zeros(3), np.zeros((18, 3)), np.ones(11)


class _Pose:
    def __init__(self, j):
        self.keypoints = j


class Record:
    """What the record stages read of an MvTracklet: frame_idxs and poses [(frame, parameters, BASIC_18 pose)]."""
    def __init__(self, frames, joints, track_id=0):
        self.track_id, self.frame_idxs = track_id, [int(f) for f in frames]
        self.poses = [(int(f), _Param(), _Pose(np.array(j, copy=True))) for f, j in zip(frames, joints)]

    def __len__(self):
        return len(self.frame_idxs)


def as_records(records):
    """A case's records (or any per-sequence lists of dict(frames, joints)) as objects the package's stages take."""
    return [[Record(r["frames"], r["joints"], j) for j, r in enumerate(rl)] for rl in records]
