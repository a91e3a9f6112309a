"""NumPy restatement of the exchange repair (multiview_motion_capture_amd/exchanges.py, csrc/mvmc_exchange.hip): detections whose arms,
legs or face are labelled left for right, decided against the 3-D joints of finished records and undone in the keypoints.  This file is
the definition of the rule; the device is gated against it.  Plain loops, one pose at a time.

Data model (host side, no MvTracklet objects):
  views    per sequence, per frame, per camera: (n, 17, 3) COCO-17 poses in ingest order (body_fit_np.ingest_np);
  Ps       per sequence (C, 3, 4);
  problems list of (seq, frame, rec, joints (18,3)) in (sequence, record, frame) order; rec = the record's position in its sequence's
           list (the conflict rule's rank).

Rule:
  groups   COCO-17 pairs (left, right): arms (5,6) (7,8) (9,10); legs (11,12) (13,14) (15,16); face (3,4) -- the pairs among
           reprojection_error's 15 common joints (oracle_np.REPROJ_SKEL_IDX / REPROJ_COCO_IDX), each keypoint compared with its BASIC_18
           joint.  The eyes (1,2) follow the face; BODY_25 rows map through OPENPOSE25_TO_COCO17 and the feet (19,20,21) <-> (22,23,24)
           follow the legs;
  costs    the problem's joints projected with P (1e-5 in the denominator).  A common keypoint is valid when its score > min_score.  Over
           the group's pairs with BOTH keypoints valid, in the order above, left keypoint before right: e0 = sum of pixel distances under
           the labels as they are, e1 = the same with every keypoint compared with the OTHER side's joint, n_g = keypoints counted;
  d*       (as-is distances of the valid keypoints outside such pairs, in pair order and then the nose, + min(e0, e1) of arms, legs,
           face in this order) / (valid common keypoints); NaN without a valid keypoint;
  select   per (problem, camera) the pose with the smallest finite d* < max_dist (ties: the lower slot); two problems of one frame that
           chose one pose: the smaller d* keeps it, on equal d* the lower rec, the other takes nothing (body_fit_np.select's rule);
  decide   group g of the pose a problem keeps is exchanged iff n_g >= 2 and e1 + margin_px n_g < e0 and e1 < ratio e0 (both strict);
  apply    an exchanged group swaps the whole (x, y, score) triples of its pairs -- also of a pair with one valid keypoint, and the
           followers; every other byte is copied.
"""
import numpy as np

import oracle_np as o

MIN_SCORE = 0.1
D_MAX = 15.0 + 30.0 * np.log(999.0) / 5.0
MARGIN_PX = 4.0
RATIO = 0.7

PAIRS = ((5, 6), (7, 8), (9, 10), (11, 12), (13, 14), (15, 16), (3, 4))       # summation order
GROUP_OF_PAIR = (0, 0, 0, 1, 1, 1, 2)                                       # 0 arms, 1 legs, 2 face (the flag's bit)
NOSE = 0
SKEL_OF_COCO = {int(c): int(s) for s, c in zip(o.REPROJ_SKEL_IDX, o.REPROJ_COCO_IDX)}
FOLLOWERS17 = {2: ((1, 2),)}                                                # the eyes follow the face
FEET25 = ((19, 22), (20, 23), (21, 24))                                     # and the feet the legs


def project(joints, P):
    """(18,3), (3,4) -> (18,2) pixels, as reprojection_error projects."""
    uv = np.zeros((18, 2))
    for j in range(18):
        h = P[:, :3] @ joints[j] + P[:, 3]
        uv[j, 0] = h[0] / (1e-5 + h[2])
        uv[j, 1] = h[1] / (1e-5 + h[2])
    return uv


def _px(p, k):
    du, dv = p[0] - k[0], p[1] - k[1]
    return np.sqrt(du * du + dv * dv)


def pose_costs(uv, kp17, min_score=MIN_SCORE):
    """uv (18,2) projected joints, kp17 (17,3) -> (d*, e0 (3,), e1 (3,), n (3,))."""
    single, cnt = 0.0, 0
    e0, e1, n = np.zeros(3), np.zeros(3), np.zeros(3, int)
    with np.errstate(invalid="ignore", over="ignore"):
        for (l, r), g in zip(PAIRS, GROUP_OF_PAIR):
            pl, pr = uv[SKEL_OF_COCO[l]], uv[SKEL_OF_COCO[r]]
            vl, vr = kp17[l, 2] > min_score, kp17[r, 2] > min_score
            if vl and vr:
                e0[g] += _px(pl, kp17[l])
                e0[g] += _px(pr, kp17[r])
                e1[g] += _px(pr, kp17[l])
                e1[g] += _px(pl, kp17[r])
                n[g] += 2
            elif vl:
                single += _px(pl, kp17[l])
            elif vr:
                single += _px(pr, kp17[r])
            cnt += int(vl) + int(vr)
        if kp17[NOSE, 2] > min_score:
            single += _px(uv[SKEL_OF_COCO[NOSE]], kp17[NOSE])
            cnt += 1
        if cnt == 0:
            return np.nan, e0, e1, n
        total = single
        for g in range(3):
            total += e1[g] if e1[g] < e0[g] else e0[g]
        return total / cnt, e0, e1, n


def decide(e0, e1, n, margin_px=MARGIN_PX, ratio=RATIO):
    """-> (flags, cost (3,2)): the decision on one kept pose."""
    fl, cost = 0, np.full((3, 2), np.nan)
    for g in range(3):
        if n[g] == 0:
            continue
        cost[g] = e0[g], e1[g]
        if n[g] >= 2 and e1[g] + margin_px * n[g] < e0[g] and e1[g] < ratio * e0[g]:
            fl |= 1 << g
    return fl, cost


def observe(problems, views, Ps, margin_px=MARGIN_PX, ratio=RATIO, max_dist=D_MAX, min_score=MIN_SCORE):
    """-> sel (B,C) slot in the camera's pose list or -1 (after the conflicts), dist (B,C) d* of the nearest pose before the conflicts
    (inf: none), flags (B,C) u8, cost (B,C,3,2) (NaN: undecided or nothing kept)."""
    B = len(problems)
    C = max((Ps[s].shape[0] for s, _, _, _ in problems), default=0)
    choice = -np.ones((B, C), np.int64)
    dist = np.full((B, C), np.inf)
    terms = {}
    for b, (s, f, _, J) in enumerate(problems):
        for c in range(Ps[s].shape[0]):
            uv = project(J, Ps[s][c])
            for p, q in enumerate(views[s][f][c]):
                d, e0, e1, n = pose_costs(uv, q, min_score)
                if np.isfinite(d) and d < max_dist and d < dist[b, c]:
                    choice[b, c], dist[b, c] = p, d
                    terms[b, c] = (e0, e1, n)
    sel = choice.copy()
    for b, (s, f, r, _) in enumerate(problems):
        for c in range(C):
            if choice[b, c] < 0:
                continue
            for b2, (s2, f2, r2, _) in enumerate(problems):
                if b2 == b or s2 != s or f2 != f or choice[b2, c] != choice[b, c]:
                    continue
                if dist[b2, c] < dist[b, c] or (dist[b2, c] == dist[b, c] and r2 < r):
                    sel[b, c] = -1
    flags = np.zeros((B, C), np.uint8)
    cost = np.full((B, C, 3, 2), np.nan)
    for b in range(B):
        for c in range(C):
            if sel[b, c] >= 0:
                flags[b, c], cost[b, c] = decide(*terms[b, c], margin_px, ratio)
    return sel, dist, flags, cost


def swap_rows(n_joints, flag):
    """The (left, right) rows an exchange with these flag bits swaps in a pose of n_joints rows."""
    rows = []
    for (l, r), g in zip(PAIRS, GROUP_OF_PAIR):
        if flag >> g & 1:
            rows.append((l, r))
    for g, pairs in FOLLOWERS17.items():
        if flag >> g & 1:
            rows += list(pairs)
    if n_joints == 25:
        rows = [(int(o.OPENPOSE25_TO_COCO17[l]), int(o.OPENPOSE25_TO_COCO17[r])) for l, r in rows]
        if flag >> 1 & 1:
            rows += list(FEET25)
    return rows


def apply(kps, flags):
    """kps (F,C,P,25|17,3), flags (F,C,P) -> the repaired copy."""
    out = np.array(kps, copy=True)
    F, C, P = flags.shape
    for f in range(F):
        for c in range(C):
            for p in range(P):
                for l, r in swap_rows(kps.shape[3], int(flags[f, c, p])):
                    out[f, c, p, l] = kps[f, c, p, r]
                    out[f, c, p, r] = kps[f, c, p, l]
    return out


def ingest_slots(kps, counts):
    """-> slots[f][c] = the caller's slots of the poses mvmc_ingest keeps, in order."""
    out = []
    for f in range(kps.shape[0]):
        row = []
        for c in range(kps.shape[1]):
            good = []
            for p in range(int(counts[f, c])):
                q = np.asarray(kps[f, c, p], np.float64)
                if o.pose_is_good(o.openpose25_to_coco17(q) if q.shape[0] == 25 else q):
                    good.append(p)
            row.append(good)
        out.append(row)
    return out


def repair(seqs, records, margin_px=MARGIN_PX, ratio=RATIO, max_dist=D_MAX, min_score=MIN_SCORE):
    """seqs: list of (kps (F,C,P,25|17,3), counts (F,C), P (C,3,4)); records: per sequence a list of dict(frames (n,), joints (n,18,3)).
    -> (per sequence dict(kps repaired, flags (F,C,P) u8, record (F,C,P) i32, cost (F,C,P,3,2)) in the caller's slots, the problems,
    and observe()'s raw outputs)."""
    import body_fit_np as bf
    views = [bf.ingest_np(k, n) for k, n, _ in seqs]
    slots = [ingest_slots(k, n) for k, n, _ in seqs]
    Ps = [np.asarray(P, np.float64) for _, _, P in seqs]
    problems = [(s, int(f), r, np.asarray(rec["joints"][i], np.float64)) for s, rl in enumerate(records) for r, rec in enumerate(rl)
                for i, f in enumerate(rec["frames"])]
    sel, dist, flags, cost = observe(problems, views, Ps, margin_px, ratio, max_dist, min_score)
    out = []
    for k, n, _ in seqs:
        F, C, P = k.shape[:3]
        out.append(dict(flags=np.zeros((F, C, P), np.uint8), record=-np.ones((F, C, P), np.int32), cost=np.full((F, C, P, 3, 2), np.nan)))
    for b, (s, f, r, _) in enumerate(problems):
        for c in range(Ps[s].shape[0]):
            if sel[b, c] >= 0:
                p = slots[s][f][c][sel[b, c]]
                out[s]["flags"][f, c, p], out[s]["record"][f, c, p], out[s]["cost"][f, c, p] = flags[b, c], r, cost[b, c]
    for s, (k, _, _) in enumerate(seqs):
        out[s]["kps"] = apply(np.asarray(k), out[s]["flags"])
    return out, problems, (sel, dist, flags, cost)
