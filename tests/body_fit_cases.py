"""Hand-built cases of the body-fit kernels (csrc/mvmc_bodyfit.hip), shared by tests/test_body_fit_cases_cpu.py (the cases are what they
claim to be: the restatement alone) and tests/test_gpu_body_fit_kernels.py (the device against the restatement, kernel by kernel).
Builders only, and check_coverage().  Every case is the device's own padded tables, written by hand: nothing here goes through ingest.

  selection  SELECT_CASES: dict(kps17 (F,C,P,17,3), counts (F,C), Pm (R,C,3,4), frame_of, rig_of, rank (B,), joints (B,18,3));
  lengths    LENGTH_CASES: length_case(name) = the launch's tables and, per identity, the restatement's arguments;
  pose       pose_case(): the problems of a two-rig length scene, started off their optimum.
"""
import functools

import numpy as np

import body_fit_np as bf
import oracle_np as o
from test_body_fit_cpu import _cameras, _coco
from test_smooth_cpu import _fk, _walk

MARGIN = 1e-6          # every decision of every case is at least this far (relative) from its threshold
SEL_MARGIN = 1e-6      # px: two distances that a selection compares differ by at least this, or are bit-equal by construction


# ---- selection --------------------------------------------------------------------------------------------------------------------
def _people():
    _, ref = o.skeleton_constants()
    JA = o.forward_kinematics(np.array([0.0, 0, 1]), np.zeros((18, 3)), ref)[0]
    return JA, JA + np.array([0.007, 0.007, 0]), JA + np.array([0.07, 0.07, 0])      # A, A a hair off, B (14 .. 20 px from A)


def _pose(J, P, shift=0.0, score=1.0):
    k = _coco(J, P, 1)
    k[:, 0] += shift
    k[:, 2] *= score
    return k


def _sel(kps17, counts, Pm, problems, **kw):
    f, r, k, J = zip(*problems) if problems else ((), (), (), ())
    return dict(kps17=np.ascontiguousarray(kps17, np.float64), counts=np.asarray(counts, np.int32), Pm=np.asarray(Pm, np.float64),
                frame_of=np.array(f, np.int32), rig_of=np.array(r, np.int32), rank=np.array(k, np.int32),
                joints=np.array(J, np.float64).reshape(-1, 18, 3), **kw)


def _equal_poses():
    """Frame 0: the same pose in slots 0 and 2 of every camera (the lower slot wins).  Frame 1: the nearer pose in the higher slot."""
    Ps, (JA, _, _) = _cameras(), _people()
    kps = np.zeros((2, 4, 4, 17, 3))
    for c in range(4):
        kps[0, c, :3] = [_pose(JA, Ps[c]), _pose(JA, Ps[c], 70.0), _pose(JA, Ps[c])]
        kps[1, c, :3] = [_pose(JA, Ps[c], 3.0), _pose(JA, Ps[c], 70.0), _pose(JA, Ps[c])]
    return _sel(kps, np.full((2, 4), 3), Ps[None], [(0, 0, 0, JA), (1, 0, 0, JA)], slots=[[0] * 4, [2] * 4])


def _strict_bound():
    """Camera 0 holds a pose 20 px off (the tests launch again with max_dist at, and one ulp above, its distance), camera 1 the CPU
    test's 70 px pose beyond D_MAX."""
    Ps, (JA, _, _) = _cameras(), _people()
    kps = np.zeros((1, 4, 4, 17, 3))
    for c, s in enumerate((20.0, 70.0, 0.0, 0.0)):
        kps[0, c, 0] = _pose(JA, Ps[c], s)
    return _sel(kps, np.ones((1, 4)), Ps[None], [(0, 0, 0, JA)], slots=[[0, -1, 0, 0]])


def _unscored():
    """Poses without a joint above min_score (NaN distance) before, after and instead of a scored one; 0.1 is not above 0.1."""
    Ps, (JA, _, _) = _cameras(), _people()
    kps = np.zeros((1, 4, 4, 17, 3))
    kps[0, 0, :2] = [_pose(JA, Ps[0], 0.0, bf.MIN_SCORE), _pose(JA, Ps[0], 2.0)]
    kps[0, 1, 0] = _pose(JA, Ps[1], 0.0, 0.05)
    kps[0, 2, :2] = [_pose(JA, Ps[2], 2.0), _pose(JA, Ps[2], 0.0, 0.0)]
    kps[0, 3, 0] = _pose(JA, Ps[3])
    return _sel(kps, [[2, 1, 2, 1]], Ps[None], [(0, 0, 0, JA)], slots=[[1, -1, 0, 0]])


def _beyond_counts():
    """counts 0 and -2 over a perfect pose, a perfect pose one slot beyond counts = 1, and counts = p_max + 3 on the frame's last camera:
    the three slots behind it are the next frame's, which hold the perfect pose as that camera sees it (it would win if read)."""
    Ps, (JA, _, _) = _cameras(), _people()
    kps = np.zeros((2, 4, 2, 17, 3))
    kps[0, 0, 0] = _pose(JA, Ps[0])
    kps[0, 1, 0] = _pose(JA, Ps[1])
    kps[0, 2] = [_pose(JA, Ps[2], 5.0), _pose(JA, Ps[2])]
    kps[0, 3] = [_pose(JA, Ps[3], 5.0), _pose(JA, Ps[3], 8.0)]
    kps[1, :2] = _pose(JA, Ps[3])
    return _sel(kps, [[0, -2, 1, 5], [2, 2, 0, 0]], Ps[None], [(0, 0, 0, JA)], slots=[[-1, -1, 0, 0]])


def _out_of_range():
    """frame_of -1 and n_frames, rig_of -1 and n_rigs, between in-range problems of two rigs (one of which loses a conflict)."""
    Pm, (JA, JA2, _) = np.array([_cameras(), _cameras(dist=6.0)]), _people()
    kps = np.zeros((2, 4, 2, 17, 3))
    for c in range(4):
        kps[0, c, 0], kps[1, c, 0] = _pose(JA, Pm[0, c]), _pose(JA, Pm[1, c])
    probs = [(0, 0, 0, JA), (-1, 0, 1, JA), (2, 0, 2, JA), (0, -1, 3, JA), (0, 2, 4, JA), (1, 1, 0, JA), (0, 0, 5, JA2)]
    return _sel(kps, np.ones((2, 4)), Pm, probs, slots=[[0] * 4] + [[-1] * 4] * 4 + [[0] * 4, [-1] * 4], out=[1, 2, 3, 4])


def _two_rigs():
    """Two sequences of 2 frames laid end to end (rows 0-1: rig 0, rows 2-3: rig 1), both with records on their frame 0; the slots of A
    and B are swapped between them.  Nobody competes across the sequences, and each row is read through its own rig's cameras."""
    Pm, (JA, _, JB) = np.array([_cameras(), _cameras(dist=6.0)[[1, 2, 3, 0]]]), _people()
    JA, JB = JA + np.array([0.5, 0.2, 0]), JB + np.array([0.5, 0.2, 0])         # (off the rings' axis: every camera sees them differently)
    kps = np.zeros((4, 4, 2, 17, 3))
    for c in range(4):
        kps[0, c] = [_pose(JA, Pm[0, c]), _pose(JB, Pm[0, c])]
        kps[2, c] = [_pose(JB, Pm[1, c]), _pose(JA, Pm[1, c])]
    cnt = np.zeros((4, 4))
    cnt[[0, 2]] = 2
    return _sel(kps, cnt, Pm, [(0, 0, 0, JA), (0, 0, 1, JB), (2, 1, 0, JA), (2, 1, 1, JB)], slots=[[0] * 4, [1] * 4, [1] * 4, [0] * 4])


def _conflicts():
    """Row 0: the CPU test's v1 scene, two records claim pose 0 and the loser does not get its second choice (slot 1, 30 px).  Row 1:
    three records claim pose 0, two of them with identical joints, ranks (2, 0, 1) in problem order: rank 1 wins, not the farther rank 0.
    Row 2: A and B each lose a camera that holds only the other's pose and win the other three."""
    Ps, (JA, JA2, JB) = _cameras(), _people()
    kps = np.zeros((3, 4, 2, 17, 3))
    for c in range(4):
        kps[0, c] = kps[1, c] = [_pose(JA, Ps[c]), _pose(JA, Ps[c], 30.0)]
    kps[2, 0, 0], kps[2, 1, 0] = _pose(JA, Ps[0]), _pose(JB, Ps[1])
    kps[2, 2] = [_pose(JA, Ps[2]), _pose(JB, Ps[2])]
    kps[2, 3] = [_pose(JB, Ps[3]), _pose(JA, Ps[3])]
    probs = [(0, 0, 0, JA2), (0, 0, 1, JA), (1, 0, 2, JA), (1, 0, 0, JA2), (1, 0, 1, JA), (2, 0, 0, JA), (2, 0, 1, JB)]
    slots = [[-1] * 4, [0] * 4, [-1] * 4, [-1] * 4, [0] * 4, [0, -1, 0, 1], [-1, 0, 1, 0]]
    return _sel(kps, [[2] * 4, [2] * 4, [1, 1, 2, 2]], Ps[None], probs, slots=slots)


def _many():
    """67 records on 6 frames x 4 cameras x 4 slots (268 pairs: two blocks of the distance kernel, the second ragged): four people, the
    records a few centimetres off them, about eleven to a frame, so a pose has up to eleven claimants; ranks shuffled against the problem
    order."""
    rng = np.random.default_rng(5)
    Ps, (JA, _, _) = _cameras(), _people()
    people = [JA + np.array([0.35 * np.cos(a), 0.35 * np.sin(a), 0.0]) for a in (0.3, 1.9, 3.4, 5.0)]
    kps = np.zeros((6, 4, 4, 17, 3))
    cnt = rng.integers(2, 5, (6, 4))
    for f in range(6):
        for c in range(4):
            for p, q in enumerate(rng.permutation(4)):
                kps[f, c, p] = _pose(people[q], Ps[c])
                kps[f, c, p, :, :2] += rng.normal(0, 1.0, (17, 2))
    rank = rng.permutation(67)
    probs = [(b % 6, 0, int(rank[b]), people[b % 4] + rng.normal(0, 0.02, 3)) for b in range(67)]
    return _sel(kps, cnt, Ps[None], probs)


SELECT_CASES = dict(equal_poses=_equal_poses, strict_bound=_strict_bound, unscored=_unscored, beyond_counts=_beyond_counts,
                    out_of_range=_out_of_range, two_rigs=_two_rigs, conflicts=_conflicts, many=_many)


@functools.lru_cache(maxsize=None)
def select_case(name):
    """-> the case's tables (read-only).  slots (where given): the pose slot every (problem, camera) must end with, written by hand."""
    return SELECT_CASES[name]()


def select_reference(c, max_dist=bf.D_MAX):
    """(choice, dist, members, n_views) of the restatement on a case's tables."""
    return bf.select_padded(c["kps17"], c["counts"], c["Pm"], c["frame_of"], c["rig_of"], c["rank"], c["joints"], max_dist)


def permuted(c, perm):
    """The case with its problems in the order perm (problem i of the result is problem perm[i] of c)."""
    out = dict(c)
    for k in ("frame_of", "rig_of", "rank", "joints"):
        out[k] = np.ascontiguousarray(c[k][perm])
    if "slots" in c:
        out["slots"] = [c["slots"][i] for i in perm]
    return out


def permutations(n):
    """The problem orders the order-independence checks use: reversed, and one shuffle."""
    return [np.arange(n)[::-1].copy(), np.random.default_rng(n).permutation(n)]


def select_features(c, max_dist=bf.D_MAX):
    """What the restatement met on a case: slot ties, record ties, the largest group of claimants, NaN candidates, clamped counts, and the
    smallest gap (px) between two distances it compared that are not bit-equal (the case's margin)."""
    F, C, P = c["kps17"].shape[:3]
    R = c["Pm"].shape[0]
    choice, dist, members, nv = select_reference(c, max_dist)
    ft = dict(slot_ties=0, record_ties=0, claimants=0, nan=0, gap=np.inf, lost=0, both=0)
    ft["count_over"] = int((c["counts"] > P).sum())
    ft["count_under"] = int((c["counts"] <= 0).sum())
    ft["frame_out"] = sorted(set(int(f) for f in c["frame_of"] if not 0 <= f < F))
    ft["rig_out"] = sorted(set(int(r) for r in c["rig_of"] if not 0 <= r < R))

    def gaps(ds):
        ds = np.sort(np.asarray(ds))
        g = np.diff(ds)
        return int((g == 0).sum()), float(g[g > 0].min()) if (g > 0).any() else np.inf
    for b in range(len(c["frame_of"])):
        f, r = int(c["frame_of"][b]), int(c["rig_of"][b])
        if not (0 <= f < F and 0 <= r < R):
            continue
        for cam in range(C):
            ds = np.array([bf.reproj_dist(c["joints"][b], c["kps17"][f, cam, p], c["Pm"][r, cam])
                           for p in range(min(max(int(c["counts"][f, cam]), 0), P))])
            ft["nan"] += int(np.isnan(ds).sum())
            ds = ds[np.isfinite(ds)]
            ties, gap = gaps(np.concatenate([ds, [max_dist]]))
            ft["slot_ties"] += int(ties > 0 and dist[b, cam] == np.sort(ds)[0] and (ds == dist[b, cam]).sum() > 1)
            ft["gap"] = min(ft["gap"], gap)
            if choice[b, cam] >= 0:
                rivals = [b2 for b2 in range(len(c["frame_of"])) if c["frame_of"][b2] == f and choice[b2, cam] == choice[b, cam]]
                ties, gap = gaps(dist[rivals, cam])
                ft["claimants"] = max(ft["claimants"], len(rivals))
                ft["record_ties"] += int((dist[rivals, cam] == dist[b, cam]).sum() > 1 and dist[b, cam] == dist[rivals, cam].min())
                ft["gap"] = min(ft["gap"], gap)
        lost = (choice[b] >= 0) & (members[b] < 0)
        ft["lost"] += int(lost.sum())
        ft["both"] += int(lost.any() and (members[b] >= 0).any())
    return ft


# ---- length step ------------------------------------------------------------------------------------------------------------------
def length_scene(counts, seed, rigs=1, zero=(), drop_one=False, start=1.0, noise=2.0):
    """Identities with counts[i] problems on frames 0 .. counts[i] - 1 of one table (F = the largest count, 4 cameras, max(2, identities)
    pose slots): identity i is on rig i % rigs and its pose of frame k sits in slot (i + k) % P; the other slots hold decoys.  A walk
    (test_smooth_cpu._walk) under the identity's true lengths, seen with ``noise`` px on every keypoint and scores drawn in [0.3, 1];
    every problem's root and angles 0.01 off the truth; odd problems lack one camera, every fifth another one.
    zero: COCO joints whose score is 0 in every view; drop_one: the left shoulder's score is 0 in camera 0 (mid-spine weight 0).
    -> dict(kps17, Pm, rig_of, members, params, id_lo, lens0, ids: per identity dict(params, obs, prs, lens0))."""
    rng = np.random.default_rng([seed, 101])
    n_ids = len(counts)
    F, C, P = max(max(counts), 1), 4, max(2, n_ids)
    Pm = np.array([_cameras(4, dist=5.0 + r) for r in range(rigs)])
    kps = np.concatenate([rng.uniform(0, 1000, (F, C, P, 17, 2)), rng.uniform(0.3, 1.0, (F, C, P, 17, 1))], axis=-1)
    _, ref = o.skeleton_constants()
    rig_of, members, params, lens0, ids = [], [], [], [], []
    for i, n in enumerate(counts):
        true = ref * rng.uniform(0.9, 1.1, 11)
        l0 = true * (1 + rng.uniform(-0.05, 0.05, 11)) * start
        l0[7] = 0.123
        lens0.append(l0)
        walk = _walk(max(n, 1), 1000 * seed + i)[:n]
        walk[:, 57:] = true
        x = walk.copy()
        x[:, :57] += rng.normal(0, 0.01, (n, 57))
        obs, prs = [], []
        for k in range(n):
            J = _fk(walk[k])
            slot, r = (i + k) % P, i % rigs
            for c in range(C):
                q = _coco(J, Pm[r, c], 1)
                q[:, :2] += rng.normal(0, noise, (17, 2))
                q[o.REPROJ_COCO_IDX, 2] = rng.uniform(0.3, 1.0, len(o.REPROJ_COCO_IDX))
                q[list(zero), 2] = 0.0
                if drop_one and c == 0:
                    q[o.COCO_L_SHOULDER, 2] = 0.0
                kps[k, c, slot] = q
            sel = np.full(C, slot)
            if k % 2 == 1:
                sel[(i + k) % C] = -1
            if k % 5 == 4:
                sel[(i + k + 2) % C] = -1
            members.append([(k * C + c) * P + sel[c] if sel[c] >= 0 else -1 for c in range(C)])
            rig_of.append(r)
            ob, pr = bf.observations(sel, [kps[k, c] for c in range(C)], Pm[r])
            obs.append(ob)
            prs.append(pr)
        params.append(x)
        ids.append(dict(params=x, obs=obs, prs=prs, lens0=l0))
    return dict(kps17=kps, Pm=Pm, rig_of=np.array(rig_of, np.int32), members=np.array(members, np.int32).reshape(-1, C),
                params=np.concatenate(params).reshape(-1, 68), id_lo=np.concatenate([[0], np.cumsum(counts)]).astype(np.int32),
                lens0=np.array(lens0), ids=ids)


HELD = {"held_2": ((15, 16), (2,)), "held_12": ((13, 14, 15, 16), (1, 2)), "held_5": ((9, 10), (5,)), "held_610": ((0, 1, 2, 3, 4), (6, 10))}
# name -> (arguments of length_scene, arguments of the step).  The tolerances are part of the case: each is chosen so that the case's
# stop rule and every decision before it are clear of their thresholds (test_body_fit_cases_cpu.py: test_length_case_margins).
LENGTH_CASES = {
    "n1":        (dict(counts=(1,), seed=1), dict(mu0=1.0)),
    "n2":        (dict(counts=(2,), seed=2), dict(mu0=1.0)),
    "n63":       (dict(counts=(63,), seed=3), dict(mu0=1.0)),
    "n64":       (dict(counts=(64,), seed=4), dict(mu0=1.0)),
    "n65":       (dict(counts=(65,), seed=5), dict(mu0=1.0)),
    "n70":       (dict(counts=(70,), seed=6), dict(mu0=1.0)),
    "empty_mid": (dict(counts=(5, 0, 6), seed=7), {}),                       # an identity without problems between two others
    "it0":       (dict(counts=(6,), seed=8), dict(max_iter=0)),              # E0 alone: bf_eval's residual
    "it1":       (dict(counts=(6,), seed=8), dict(max_iter=1)),              # one step: H and g through lens + d; stops at max_iter
    "far6":      (dict(counts=(65,), seed=5, start=6.0), dict(max_iter=12)),   # rejected trials, the cap of 12
    "far8":      (dict(counts=(65,), seed=5, start=8.0), dict(max_iter=12)),
    "stop_xtol": (dict(counts=(6,), seed=9), dict(xtol=1e-4)),
    "stop_pred": (dict(counts=(6,), seed=9), dict(max_iter=12)),
    "stop_ftol": (dict(counts=(65,), seed=5, start=6.0), dict(max_iter=12, ftol=3e-2)),   # far6, stopped at its eighth trial
    "midhip":    (dict(counts=(6,), seed=10, drop_one=True), {}),
    "two_rigs":  (dict(counts=(6, 5), seed=11, rigs=2), {}),
    "three":     (dict(counts=(6, 5, 4), seed=12, rigs=2), {}),              # the bit-identity launches are cut from this one
    **{k: (dict(counts=(6,), seed=13, zero=z), {}) for k, (z, _) in HELD.items()},
}
FAR = ("far6", "far8", "stop_ftol")      # the far starts: lengths of metres, E of 1e9 and more
STEP_DEFAULTS = dict(max_iter=10, mu0=bf.LM_MU0, ftol=1e-6, xtol=bf.LM_XTOL)
MAX_ITER_CAP = 12      # include/mvmc.h: MVMC_BODY_INFO_DOUBLES - 4


def step_args(name):
    return {**STEP_DEFAULTS, **LENGTH_CASES[name][1]}


@functools.lru_cache(maxsize=None)
def length_case(name):
    """-> length_scene's dict of the case.  Shared between the tests: read-only."""
    return length_scene(**LENGTH_CASES[name][0])


def expected_info(E0, E, trace):
    """The device's info row (include/mvmc.h: mvmc_body_lengths) of a restated step."""
    row = -np.ones(4 + MAX_ITER_CAP)
    row[:4] = E0, E, len(trace), sum(trace)
    row[4:4 + len(trace)] = trace
    return row


def solve_identity(idn, free=None, reverse=False, **step):
    """The restatement on one identity of a scene -> dict(lens, free (11,) bool, mask, info (16,), log).  An identity without problems
    keeps its lengths (free 0, info {0, 0, 0, 0, -1 ..}); reverse: the (problem, view) pairs summed in the opposite order."""
    if len(idn["obs"]) == 0:
        return dict(lens=idn["lens0"].copy(), free=np.zeros(11, bool), mask=0, info=expected_info(0.0, 0.0, []), log=[])
    par, obs, prs = idn["params"], idn["obs"], idn["prs"]
    if reverse:
        par, obs, prs = par[::-1], [x[::-1] for x in obs[::-1]], [x[::-1] for x in prs[::-1]]
    log = []
    lens, fr, info = bf.length_step(par, obs, prs, idn["lens0"], free, log=log, **step)
    return dict(lens=lens, free=fr, mask=int(sum(1 << s for s in range(11) if fr[s])), info=expected_info(info["E0"], info["E"], info["trace"]),
                log=log)


@functools.lru_cache(maxsize=None)
def length_reference(name):
    """Per identity of the case: solve_identity's dict.  Computed once; read-only."""
    return [solve_identity(idn, **step_args(name)) for idn in length_case(name)["ids"]]


def stop_reason(ref, max_iter):
    """Why a restated step ended: "none" (no trial to make), "xtol", "pred", "ftol" or "max_iter"."""
    if not ref["log"]:
        return "none"
    last = ref["log"][-1]["stop"]
    assert last is not None or ref["info"][2] == max_iter
    return last or "max_iter"


def length_margin(name, free=None):
    """The smallest relative margin of any decision of the case (bf.length_margins over its identities), and which one it was."""
    a = step_args(name)
    worst = (np.inf, None)
    refs = length_reference(name) if free is None else [solve_identity(idn, free=free, **a) for idn in length_case(name)["ids"]]
    for i, ref in enumerate(refs):
        for k, v in bf.length_margins(ref["log"], a["ftol"], a["xtol"]).items():
            worst = min(worst, (float(v), f"identity {i}: {k}"), key=lambda t: t[0])
    return worst


def cut(c, ids):
    """A launch of the scene's identities ``ids`` in that order (their problems moved, the keypoint table as it is)."""
    rows = [np.arange(c["id_lo"][i], c["id_lo"][i + 1]) for i in ids]
    at = np.concatenate(rows).astype(int)
    return dict(kps17=c["kps17"], Pm=c["Pm"], rig_of=c["rig_of"][at], members=c["members"][at], params=c["params"][at],
                id_lo=np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32), lens0=c["lens0"][list(ids)],
                ids=[c["ids"][i] for i in ids])


FIX_FREE_CASE, FIX_FREE_MASK = "stop_pred", 0b00000110011        # slots 0, 1, 4, 5: fewer than diag(H) > 0 gives on that scene


def mask_bits(mask):
    return np.array([(mask >> s) & 1 for s in range(11)], bool)


# ---- pose step --------------------------------------------------------------------------------------------------------------------
POSE_NFEV = 5


@functools.lru_cache(maxsize=None)
def pose_case():
    """Twelve problems of two rigs (the "pose" scene: two identities of 6 frames), in alternating rig order, each started from its
    perturbed pose under its identity's starting lengths -> dict(kps17, Pm, rig_of, members, init (B,68), obs, prs)."""
    c = length_scene(counts=(6, 6), seed=21, rigs=2)
    at = np.arange(12).reshape(2, 6).T.ravel()
    init = c["params"].copy()
    obs, prs = [], []
    for i, idn in enumerate(c["ids"]):
        init[c["id_lo"][i]:c["id_lo"][i + 1], 57:] = idn["lens0"]
        obs += idn["obs"]
        prs += idn["prs"]
    return dict(kps17=c["kps17"], Pm=c["Pm"], rig_of=np.ascontiguousarray(c["rig_of"][at]), members=np.ascontiguousarray(c["members"][at]),
                init=np.ascontiguousarray(init[at]), obs=[obs[i] for i in at], prs=[prs[i] for i in at])


@functools.lru_cache(maxsize=None)
def pose_reference():
    """Per problem of pose_case(): (params (68,), cost, joints (18,3), margin) of bf.pose_step at POSE_NFEV evaluations."""
    c = pose_case()
    out = []
    for b in range(len(c["init"])):
        tr = []
        p, cost = bf.pose_step(c["init"][b], c["obs"][b], c["prs"][b], c["init"][b, 57:], POSE_NFEV, trace=tr)
        out.append((p, cost, _fk(p), bf.pose_margin(tr)))
    return out


# ---- coverage ---------------------------------------------------------------------------------------------------------------------
def check_coverage():
    """Asserts, on the restatement alone, that the case set reaches every branch it is for.  -> dict of what was found (printed by the
    CPU test), so that a later edit of the cases cannot lose a branch unnoticed."""
    rep = {}
    ft = {name: select_features(select_case(name)) for name in SELECT_CASES}
    rep["selection"] = {k: {a: v for a, v in f.items() if v not in (0, [], np.inf)} for k, f in ft.items()}
    assert ft["equal_poses"]["slot_ties"] >= 4                                   # a tie between slots
    assert ft["conflicts"]["record_ties"] >= 4                                   # a tie between records
    assert ft["conflicts"]["claimants"] == 3 and ft["many"]["claimants"] >= 3    # a three-way conflict, and larger groups
    assert ft["conflicts"]["both"] >= 2                                          # loses one camera, wins another
    assert ft["unscored"]["nan"] >= 3                                            # a NaN candidate
    assert ft["beyond_counts"]["count_over"] >= 1 and ft["beyond_counts"]["count_under"] >= 2      # a clamped count
    assert ft["out_of_range"]["frame_out"] == [-1, 2] and ft["out_of_range"]["rig_out"] == [-1, 2]   # each out-of-range kind
    for name, f in ft.items():
        assert f["gap"] >= SEL_MARGIN, (name, f["gap"])
    c = select_case("conflicts")
    assert c["rank"][2:5].tolist() == [2, 0, 1]                                  # ranks not in problem order
    c = select_case("many")
    assert (len(c["frame_of"]) * 4) % 256 != 0 and len(c["frame_of"]) * 4 > 256
    c = select_case("two_rigs")
    one = dict(c, Pm=c["Pm"][[0, 0]])
    assert not np.array_equal(select_reference(one)[2], select_reference(c)[2])  # the second rig's cameras decide its rows
    c = select_case("beyond_counts")
    decoy = [bf.reproj_dist(c["joints"][0], q, c["Pm"][0, 3]) for q in c["kps17"].reshape(-1, 17, 3)[8:11]]      # what slots 2 .. 4 would be
    assert max(decoy) < select_reference(c)[1][0, 3] and c["counts"][0, 3] == 2 + 3
    # ---- the length step
    reasons, rejected, counts, held = {}, [], set(), {}
    for name in LENGTH_CASES:
        for i, ref in enumerate(length_reference(name)):
            reasons.setdefault(stop_reason(ref, step_args(name)["max_iter"]), []).append(name)
            if 0 in ref["info"][4:].tolist():
                rejected.append(name)
            counts.add(len(length_case(name)["ids"][i]["obs"]))
            if name in HELD:
                held[name] = [s for s in range(11) if not ref["free"][s]]
    rep["stop_reasons"] = {k: sorted(set(v)) for k, v in reasons.items()}
    rep["rejected_trials"] = rejected
    rep["held"] = held
    assert set(reasons) >= {"xtol", "pred", "ftol", "max_iter"}, reasons          # each LM stop reason
    assert set(FAR) <= set(rejected)                                             # a rejected trial
    assert any(length_reference(n)[0]["info"][2] == MAX_ITER_CAP for n in FAR)   # the cap of 12
    for name, (_, slots) in HELD.items():
        assert held[name] == sorted(set(slots) | {7}), (name, held[name])        # each held-slot pattern
    assert {0, 1, 2, 63, 64, 65, 70} <= counts                                   # problem counts on both sides of 64
    full = length_reference(FIX_FREE_CASE)[0]["mask"]
    assert FIX_FREE_MASK & ~full == 0 and bin(FIX_FREE_MASK).count("1") < bin(full).count("1")
    for name in LENGTH_CASES:
        mem = length_case(name)["members"]
        assert (mem < 0).any() or mem.shape[0] < 2
    c = length_case("two_rigs")
    P = c["kps17"].shape[2]
    assert len(set((c["members"][c["members"] >= 0] % P).tolist())) == P and set(c["rig_of"].tolist()) == {0, 1}
    k = length_case("midhip")["kps17"]
    assert (k[..., [5, 6, 11, 12], 2].prod(axis=-1) == 0).any()
    for name in LENGTH_CASES:
        if name != "midhip" and name not in HELD:
            w = length_case(name)["kps17"][..., [5, 6, 11, 12], 2].prod(axis=-1)
            assert (w > 0).all() and (w < 1).all()
    return rep
