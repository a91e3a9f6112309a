"""NumPy restatement of the re-identification step (multiview_motion_capture_amd/relinking.py: reidentify_sequences;
csrc/mvmc_relink.hip: mvmc_reid_signature, mvmc_reid_link), written from the statement of the problem, not from the kernels.

A record is (track_id, frames (n,) increasing, joints (n,18,3)).

SIGNATURE of a record, from the joints of ALL its poses:
  * per pose and bone j = 1 .. 17: b_j = sqrt(dx dx + dy dy + dz dz) of joint j minus joint PARENTS[j];
  * ten sides, the values 0 - 6 and 8 - 10 of SIDE_MAP (7 is the root and has no bone): sides 0 - 6 have a left and a right bone and
    the value (b_lo + b_hi) / 2 in joint order, sides 8, 9, 10 one bone; a pose gives a side a value only when all its bones are finite;
  * per side with m values: med = the lower median (rank (m - 1) // 2 in ascending order), mad = the lower median of |x - med|,
    se = 1.4826 mad 1.2533 / sqrt(m) evaluated in that order; a side with m < min_poses is undefined (NaN).
DISTANCE  z(A, B) = sqrt(mean over the sides defined in both of (l_A - l_B)^2 / (se_A^2 + se_B^2 + 2 floor^2)), summed in side order;
undefined (NaN) with fewer than 5 sides defined in both.
CANDIDATE A -> B: A != B; gap = B.first - A.last >= 1 (and <= max_gap when given); z defined and <= max_z; |centroid of B's first pose
- centroid of A's last pose| <= reach + speed gap (the centroid is the mean of the 18 joints; a non-finite distance allows nothing).
VETO: Q and R overlap when Q.first <= R.last and R.first <= Q.last.  A -> B is refused when another record Q overlaps B but not A and
z(A, B) > ratio z(A, Q), or overlaps A but not B and z(A, B) > ratio z(Q, B); an undefined z vetoes nothing, and neither does a Q that
overlaps both ends.
CHOICE as in relink_np: the n x 2n matrix holds z where allowed and BIG elsewhere, the dummy column of a row holds max_z; Kuhn-Munkres
with potentials, rows in node order ((first frame, track id)), the first minimum wins.
"""
import numpy as np

import relink_np as rn

BIG = rn.BIG
PARENTS = np.array([-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 9, 10, 8, 12, 13, 8, 15, 15])      # device.SKEL_PARENTS
SIDE_MAP = np.array([7, 0, 1, 2, 0, 1, 2, 8, 9, 3, 4, 5, 3, 4, 5, 10, 6, 6])          # device.SKEL_SIDE_MAP
SIDES = (0, 1, 2, 3, 4, 5, 6, 8, 9, 10)
SIDE_BONES = [[j for j in range(1, 18) if SIDE_MAP[j] == k] for k in SIDES]           # joint order
MIN_COMMON = 5


def bone_lengths(joints):
    """(m,18,3) -> (m,18): column j is b_j (column 0 NaN: the root has no bone)."""
    J = np.asarray(joints, np.float64).reshape(-1, 18, 3)
    b = np.full(J.shape[:2], np.nan)
    with np.errstate(invalid="ignore", over="ignore"):
        d = J[:, 1:] - J[:, PARENTS[1:]]
        b[:, 1:] = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])
    return b


def side_values(joints):
    """(m,18,3) -> (m,10): the value every pose gives every side, NaN where it gives none."""
    b = bone_lengths(joints)
    out = np.full((b.shape[0], len(SIDES)), np.nan)
    for q, bones in enumerate(SIDE_BONES):
        ok = np.all(np.isfinite(b[:, bones]), axis=1)
        with np.errstate(invalid="ignore", over="ignore"):
            x = (b[:, bones[0]] + b[:, bones[1]]) / 2.0 if len(bones) == 2 else b[:, bones[0]]
        out[ok, q] = x[ok]
    return out


def lower_median(x):
    """The value of rank (m - 1) // 2 in ascending order."""
    return np.sort(np.asarray(x, np.float64))[(len(x) - 1) // 2]


def signature(joints, min_poses):
    """(med (10,), se (10,), cnt (10,)) of one record."""
    vals = side_values(joints)
    med, se, cnt = np.full(10, np.nan), np.full(10, np.nan), np.zeros(10, np.int64)
    for q in range(10):
        x = vals[:, q]
        x = x[~np.isnan(x)]
        m = cnt[q] = x.size
        if m < min_poses or m == 0:
            continue
        med[q] = lower_median(x)
        with np.errstate(invalid="ignore"):
            mad = lower_median(np.abs(x - med[q]))
        se[q] = 1.4826 * mad * 1.2533 / np.sqrt(float(m))
    return med, se, cnt


def end_centroids(joints):
    """(6,): the centroid of the first pose, of the last pose."""
    return np.concatenate([rn.centroid(np.asarray(joints[0], np.float64)), rn.centroid(np.asarray(joints[-1], np.float64))])


def distance(a, b, floor):
    """z of two signatures (med, se); NaN when undefined."""
    f2 = 2.0 * (floor * floor)
    total, c = 0.0, 0
    for q in range(10):
        la, lb, ea, eb = a[0][q], b[0][q], a[1][q], b[1][q]
        if np.isnan(la) or np.isnan(lb) or np.isnan(ea) or np.isnan(eb):
            continue
        d = la - lb
        with np.errstate(divide="ignore", invalid="ignore"):
            total = total + (d * d) / ((ea * ea + eb * eb) + f2)
        c += 1
    return float(np.sqrt(total / float(c))) if c >= MIN_COMMON else float("nan")


def overlap(fq, fr):
    return fq[0] <= fr[1] and fr[0] <= fq[1]


def reidentify(recs, max_z, ratio, floor, min_poses, reach, speed, max_gap=None, veto=True):
    """recs: [(track_id, frames, joints)] of one sequence -> dict(order (position in recs of node k), succ, head, pos, cost (the z of
    the link taken) over the nodes, matrix, z (n,n), sig (n,20), cnt (n,10), ends (n,6)).  veto=False leaves the veto out (for the
    test that shows what it does)."""
    order = rn.node_order(recs)
    nodes = [recs[i] for i in order]
    n = len(nodes)
    sigs = [signature(r[2], min_poses) for r in nodes]
    ends = np.array([end_centroids(r[2]) for r in nodes]).reshape(n, 6)
    fr = [(int(r[1][0]), int(r[1][-1])) for r in nodes]
    Z = np.full((n, n), np.nan)
    for i in range(n):
        for j in range(n):
            Z[i, j] = distance(sigs[i], sigs[j], floor)
    a = np.full((n, 2 * n), BIG)
    for i in range(n):
        a[i, n + i] = max_z
        for j in range(n):
            gap = fr[j][0] - fr[i][1]
            if i == j or gap < 1 or (max_gap is not None and gap > max_gap):
                continue
            z = Z[i, j]
            if not z <= max_z:
                continue
            d = ends[j, :3] - ends[i, 3:]
            dist = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
            if not (np.isfinite(dist) and dist <= reach + speed * float(gap)):
                continue
            ok = True
            for q in range(n if veto else 0):
                if q == i or q == j:
                    continue
                ovi, ovj = overlap(fr[q], fr[i]), overlap(fr[q], fr[j])
                if ovj and not ovi and z > ratio * Z[i, q]:
                    ok = False
                if ovi and not ovj and z > ratio * Z[q, j]:
                    ok = False
            if ok:
                a[i, j] = z
    sig = np.array([np.concatenate(s[:2]) for s in sigs]).reshape(n, 20)
    cnt = np.array([s[2] for s in sigs], np.int64).reshape(n, 10)
    if n == 0:
        e = np.zeros(0, np.int64)
        return dict(order=e, succ=e, head=e, pos=e, cost=np.zeros(0), matrix=a, z=Z, sig=sig, cnt=cnt, ends=ends)
    col_of = rn.assign_rows(a)
    succ, head, pos, cost = rn.links_from_assignment(a, col_of)
    return dict(order=np.asarray(order, np.int64), succ=succ, head=head, pos=pos, cost=cost, matrix=a, z=Z, sig=sig, cnt=cnt, ends=ends)


record_links = rn.record_links
records_of = rn.records_of
