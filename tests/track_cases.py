"""Inputs shared by the tests of the temporal-layer kernels (tests/test_track_np_cpu.py, tests/test_gpu_track_kernels.py): small,
deterministic cases -- synthetic scenes for the spatial-time graph, hand-built label tensors and tables for the tracker's state
machine, no association solve anywhere -- each the smallest shape at which one path of csrc/mvmc_track.hip differs, and their
expected results by tests/track_np.py, computed once and shared (treat everything returned here as read-only).
check_coverage() proves on the restatement alone that every branch the cases are meant to reach is taken in at least one chain and
not taken in at least one other, and that no affinity sits at the cut; the GPU test then asks the device for the same numbers."""
import functools

import numpy as np

import oracle_np as o
import track_np as tn

MIN_SCORE = 0.125          # a power of two, so that scores can sit EXACTLY at the threshold (0.25 x 0.5, 0.125)
CUT = 1e-3                 # spatial_time_affinity's cut
N_FRAMES = 5


def _scene(C, P, F, seed):
    """kps17 (F,C,P,17,3) f64, P (C,3,4), gt (F,P,18,3), F2 (C,C,3,3) by the reference's rule."""
    from multiview_motion_capture_amd import synth
    g = synth.generate(F, C, P, seed, dtype=np.float64)
    Pm = g["P"]
    F2 = np.array([[o.fundamental_from_projections(Pm[a], Pm[b]) for b in range(C)] for a in range(C)])
    return np.ascontiguousarray(o.openpose25_to_coco17(g["kps25"])), Pm, g["gt_joints"], F2


def _tracklets(gt, frame_idx, T, rng, reach=0.35, far=()):
    """track_joints (B,T,18,3): slot t of chain b is person t % P of the chain's frame, moved as a whole by up to ``reach`` metres in a
    random direction (0 .. ~100 px in the images: both sides of the sigmoid's cut at 56 px) plus 5 mm of jitter per joint; chains in
    ``far`` are lifted by a metre instead (every reprojection lands beyond the cut)."""
    B, Pn = len(frame_idx), gt.shape[1]
    tj = np.zeros((B, T, 18, 3))
    for b in range(B):
        for t in range(T):
            d = rng.normal(size=3)
            d *= rng.uniform(0.0, reach) / np.linalg.norm(d)
            if b in far:
                d = np.array([0.0, 0.0, 1.0 + 0.1 * t])
            tj[b, t] = gt[frame_idx[b], t % Pn] + d + rng.normal(0.0, 0.005, size=(18, 3))
    return tj


@functools.lru_cache(maxsize=None)
def affinity_case(name):
    """-> dict(kps17, counts, frame_idx, track_joints, n_tracks, P, F2, C, Pn, T, min_score) of 'small' or 'limit'."""
    if name == "small":
        C, Pn, T = 3, 3, 4
        kps17, Pm, gt, F2 = _scene(C, Pn, N_FRAMES, 11)
        counts = np.array([[3, 3, 3], [-1, 3, 2], [Pn + 4, 1, 3], [2, 0, 3], [2, 0, 0]], np.int32)
        frame_idx = np.array([4, 3, 3, 1, 0, 2, 0, 4, 2], np.int32)           # repeated, descending, non-contiguous
        n_tracks = np.array([4, -3, 4, 1, T + 5, 0, 4, T + 5, 1], np.int32)
        # scores exactly at the threshold: 0.25 x 0.5 in a 2-D / 2-D pair, 0.125 for a reprojection (frame 0: chains 4 and 6)
        kps17[0, 0, 0, 5, 2], kps17[0, 1, 1, 5, 2], kps17[0, 2, 0, 7, 2] = 0.25, 0.5, 0.125
        kps17[0, 0, 0, 5, :2] += 1.0          # (present also where the generator dropped the joint)
        kps17[3, 2, 1] = 0.0                  # a pose without a single valid joint (frame 3: chain 2)
        tj = _tracklets(gt, frame_idx, T, np.random.default_rng([11, 1]), far=(0,))
    elif name == "limit":
        C, Pn, T = 8, 8, 16                   # NS = 80 = MVMC_MAX_NODES
        kps17, Pm, gt, F2 = _scene(C, Pn, 2, 12)
        counts = np.full((2, C), Pn, np.int32)
        frame_idx = np.array([1, 0], np.int32)
        n_tracks = np.array([16, 9], np.int32)
        tj = _tracklets(gt, frame_idx, T, np.random.default_rng([12, 1]))
    else:
        raise KeyError(name)
    return dict(kps17=kps17, counts=counts, frame_idx=frame_idx, track_joints=tj, n_tracks=n_tracks, P=Pm, F2=F2, C=C, Pn=Pn, T=T,
                min_score=MIN_SCORE)


@functools.lru_cache(maxsize=None)
def affinity_reference(name):
    """-> (W, D, group_counts) of tn.st_affinity_np on the case (F2 by the reference's own rule)."""
    c = affinity_case(name)
    return tn.st_affinity_np(c["kps17"], c["counts"], c["frame_idx"], c["track_joints"], c["n_tracks"], c["P"], c["F2"], c["min_score"])


# ------------------------------------------------------------------------------------------------------------------------------------
# assignment: label tensors made by hand
# ------------------------------------------------------------------------------------------------------------------------------------
ASSIGN_SHAPES = {"a334": (3, 3, 4, 2, 2), "a548": (5, 4, 8, 6, 6), "a8816": (8, 8, 16, 32, 64)}     # (C, P, T, K, V)
B_CHAINS = 67              # one thread per chain: one block of 64 and a ragged second one


def _counts(C, P, rng):
    counts = rng.integers(0, P + 1, size=(N_FRAMES, C)).astype(np.int32)
    counts[0] = P                                       # frame 0 is full (the chains made by hand use it)
    counts[1, 0], counts[2, C - 1], counts[3, 0] = -1, P + 4, P + 4
    return counts


def _random_labels(n, rng, coarse):
    """Labels of n nodes: coarse = a few large clusters, else many small ones; -1 in both."""
    ncl = int(rng.integers(1, 4)) if coarse else int(rng.integers(1, max(2, n // 2) + 1))
    return rng.integers(-1, ncl, size=n).astype(np.int32), ncl


def _put(lab_row, values):
    lab_row[:len(values)] = values


@functools.lru_cache(maxsize=None)
def assign_case(name):
    """-> dict(labels_sp, ncl_sp, labels_st, ncl_st, counts, frame_idx, n_tracks, track_params, C, P, T, K, V).  The label row of the
    path a chain does NOT take, and the tail of the row it takes, hold plausible labels that must not be read."""
    if name == "cut64":
        # the match_spatial walk keeps at most 64 poses of a cluster: 70 (cut, to be reported), exactly 64 (not cut), 65 (cut)
        C, P, T, K, V, B = 10, 8, 4, 4, 80, 3
        counts = np.full((1, C), P, np.int32)
        lab_sp = np.full((B, C * P), -1, np.int32)
        lab_sp[0, :70], lab_sp[0, 70:] = 0, 1
        lab_sp[1, :64], lab_sp[1, 64:] = 0, 1
        lab_sp[2, 5:70] = 0
        return dict(labels_sp=lab_sp, ncl_sp=np.array([2, 2, 1], np.int32), labels_st=np.zeros((B, T + C * P), np.int32),
                    ncl_st=np.full(B, 3, np.int32), counts=counts, frame_idx=np.zeros(B, np.int32), n_tracks=np.zeros(B, np.int32),
                    track_params=_table((B, T, 68), 0.25), C=C, P=P, T=T, K=K, V=V)
    C, P, T, K, V = ASSIGN_SHAPES[name]
    B, N = B_CHAINS, C * P
    rng = np.random.default_rng([21, C, P, T])
    counts = _counts(C, P, rng)
    frame_idx = rng.integers(0, N_FRAMES, size=B).astype(np.int32)
    n_tracks = np.array([[0, T, 1, T + 3, -2, T // 2, T, 2][b % 8] for b in range(B)], np.int32)
    lab_sp, lab_st = np.zeros((B, N), np.int32), np.zeros((B, T + N), np.int32)
    ncl_sp, ncl_st = np.zeros(B, np.int32), np.zeros(B, np.int32)
    for b in range(B):
        nt = tn.clamp(n_tracks[b], 0, T)
        n_pose = sum(tn.clamp(k, 0, P) for k in counts[frame_idx[b]])
        coarse = (b // 8) % 2 == 1
        lab_sp[b], ncl_sp[b] = _random_labels(N, rng, coarse)
        lab_st[b], ncl_st[b] = _random_labels(T + N, rng, coarse)
        used, n = (lab_sp[b], n_pose) if nt == 0 else (lab_st[b], nt + n_pose)
        used[n:] = 0                                    # beyond the graph: label 0, which a reader past the end would count
    if name == "a334":
        # chains made by hand on the full frame 0 (poses by view: 3 + 3 + 3)
        frame_idx[[8, 9, 10]] = 0
        n_tracks[8], ncl_st[8] = 1, 3                   # three new clusters (K = 2), two of them of three views (V = 2); tracklet alone
        _put(lab_st[8], [-1, 0, 1, 2, 0, 1, 2, 0, 1, -1])
        n_tracks[9], ncl_st[9] = 4, 3                   # two tracklets in one cluster, two poses of one view, exactly one pose, alone
        _put(lab_st[9], [0, 0, 1, 2, 0, 0, 1, 0, -1, -1, -1, -1, -1])
        n_tracks[10], ncl_sp[10] = 0, 2                 # match_spatial: both poses of view 0 stay members
        _put(lab_sp[10], [0, 0, -1, 0, 1, -1, -1, 1, -1])
    return dict(labels_sp=lab_sp, ncl_sp=ncl_sp, labels_st=lab_st, ncl_st=ncl_st, counts=counts, frame_idx=frame_idx, n_tracks=n_tracks,
                track_params=_table((B, T, 68), 0.25), C=C, P=P, T=T, K=K, V=V)


def _table(shape, offset):
    """Distinct values per element: a copy from another row, slot or chain cannot pass."""
    return np.arange(int(np.prod(shape)), dtype=np.float64).reshape(shape) + offset


@functools.lru_cache(maxsize=None)
def assign_reference(name):
    """-> (members, cold, init, status, n_new, overflow) of tn.assign_np."""
    c = assign_case(name)
    return tn.assign_np(c["labels_sp"], c["ncl_sp"], c["labels_st"], c["ncl_st"], c["counts"], c["frame_idx"], c["n_tracks"],
                        c["track_params"], c["P"], c["K"], c["V"])


def assign_features(name):
    """Per chain, which of the awkward inputs it holds -> dict of (B,) bool arrays."""
    c = assign_case(name)
    _, _, _, status, n_new, ovf = assign_reference(name)
    B, T, C, P, K, V = len(c["n_tracks"]), c["T"], c["C"], c["P"], c["K"], c["V"]
    keys = ("sp_path", "two_tracklets", "one_pose", "tracklet_alone", "dup_view_sp", "dup_view_st", "unlabelled", "over_K", "over_V",
            "straddle_64", "ignored_small", "overflow")
    ft = {k: np.zeros(B, bool) for k in keys}
    for b in range(B):
        nt = tn.clamp(c["n_tracks"][b], 0, T)
        cnt = [tn.clamp(k, 0, P) for k in c["counts"][c["frame_idx"][b]]]
        lab, ncl = (c["labels_sp"][b], c["ncl_sp"][b]) if nt == 0 else (c["labels_st"][b], c["ncl_st"][b])
        cls = tn.chain_clusters(lab, ncl, nt, cnt)
        ft["sp_path"][b] = nt == 0
        ft["unlabelled"][b] = (lab[:nt + sum(cnt)] == -1).any()
        ft["one_pose"][b] = (status[b] == 1).any()
        ft["overflow"][b] = ovf[b] != 0
        n_newcl = 0
        for cl in cls:
            tr = [x for x in cl if x[0] == 0]
            poses = [x for x in cl if x[0] > 0]
            views = [x[0] for x in poses]
            dup = len(set(views)) < len(views)
            m = len(poses) if nt == 0 else len(set(views))
            ft["two_tracklets"][b] |= len(tr) >= 2
            ft["tracklet_alone"][b] |= len(tr) >= 1 and not poses
            ft["dup_view_sp"][b] |= nt == 0 and dup
            ft["dup_view_st"][b] |= nt > 0 and dup
            ft["over_V"][b] |= m >= 2 and m > V
            ft["ignored_small"][b] |= not tr and m < 2
            ft["straddle_64"][b] |= m >= 2 and any(x[2] < 64 for x in poses) and any(x[2] >= 64 for x in poses)
            n_newcl += (not tr) and m >= 2
        ft["over_K"][b] = n_newcl > K
        assert int(n_new[b]) == min(n_newcl, K)
    return ft


# ------------------------------------------------------------------------------------------------------------------------------------
# commit: status patterns and tables made by hand
# ------------------------------------------------------------------------------------------------------------------------------------
COMMIT_SHAPES = {"c4": (4, 2), "c16": (16, 32)}        # (T, K)


@functools.lru_cache(maxsize=None)
def commit_case(name):
    """-> dict(status, n_new, ik_params, ik_joints, track_params, track_joints, meta, n_tracks, next_id, n_dead, T, K)."""
    T, K = COMMIT_SHAPES[name]
    B = B_CHAINS
    rng = np.random.default_rng([31, T])
    n_tracks = np.array([[T, T + 3, T, T - 1, T, 1, T, 0][b % 8] for b in range(B)], np.int32)
    status = rng.integers(0, 3, size=(B, T)).astype(np.int32)
    if T == 4:
        for b in range(B):                              # every mix of 0, 1, 2 over four slots that 67 chains can hold: 5 b mod 81 in base 3
            status[b] = [((5 * b) % 81) // 3 ** s % 3 for s in range(4)]
    else:
        status[1], status[2], status[3] = 0, 1, 2
    n_new = np.zeros(B, np.int32)
    for b in range(B):
        nt = tn.clamp(n_tracks[b], 0, T)
        free = T - int((status[b, :nt] != 0).sum())
        n_new[b] = min(K, max(0, [free - 1, free, free + 1, free + 3][(b // 2) % 4]))       # room, exact fit, over by one, by more
    meta = np.zeros((B, T, 4), np.int32)
    for b in range(B):
        for s in range(T):
            meta[b, s] = (1000 * b + s, 1 + (b + s) % 2, (b + 2 * s) % 4, 5 + (3 * b + s) % 7)    # hits 0 .. 3: at, short of and past n_inits
    return dict(status=status, n_new=n_new, ik_params=_table((B, T + K, 68), 1e6), ik_joints=_table((B, T + K, 18, 3), 2e6),
                track_params=_table((B, T, 68), 0.25), track_joints=-_table((B, T, 18, 3), 0.5), meta=meta, n_tracks=n_tracks,
                next_id=(100 + 3 * np.arange(B)).astype(np.int32), n_dead=(7 + np.arange(B)).astype(np.int32), T=T, K=K)


@functools.lru_cache(maxsize=None)
def commit_reference(name, n_inits):
    c = commit_case(name)
    return tn.commit_np(c["status"], c["n_new"], c["ik_params"], c["ik_joints"], c["track_params"], c["track_joints"], c["meta"],
                        c["n_tracks"], c["next_id"], c["n_dead"], c["K"], n_inits)


def commit_features(name, n_inits):
    c, r = commit_case(name), commit_reference(name, n_inits)
    B, T = c["status"].shape
    keys = ("st0", "st1", "st2", "promoted", "one_short", "room", "exact", "over_1", "over_more", "clamped", "moved_down")
    ft = {k: np.zeros(B, bool) for k in keys}
    for b in range(B):
        nt = tn.clamp(c["n_tracks"][b], 0, T)
        st, mt = c["status"][b, :nt], c["meta"][b, :nt]
        surv = int((st != 0).sum())
        for v in (0, 1, 2):
            ft[f"st{v}"][b] = (st == v).any()
        upd = (st == 2) & (mt[:, 1] == tn.TENTATIVE)
        ft["promoted"][b] = (upd & (mt[:, 2] + 1 == n_inits)).any()                  # exactly at the boundary
        ft["one_short"][b] = (upd & (mt[:, 2] + 1 == n_inits - 1)).any()             # and not before it
        over = surv + int(c["n_new"][b]) - T
        ft["room"][b], ft["exact"][b] = over < 0, over == 0 and c["n_new"][b] > 0
        ft["over_1"][b], ft["over_more"][b] = over == 1, over > 1
        assert bool(r["overflow"][b] & 2) == (over > 0) and r["next_id"][b] - c["next_id"][b] == r["n_tracks"][b] - surv
        ft["clamped"][b] = c["n_tracks"][b] > T
        ft["moved_down"][b] = surv > 0 and (np.flatnonzero(st != 0) != np.arange(surv)).any()
    return ft


# ------------------------------------------------------------------------------------------------------------------------------------
# several frames: assign -> a stand-in solve -> commit
# ------------------------------------------------------------------------------------------------------------------------------------
N_STEPS = 6
MULTI_SHAPES = {"m334": "a334", "m548": "a548"}


def fake_solve(B, NP, step):
    """IK results that name their (chain, slot, step): ik_params (B,NP,68), ik_joints (B,NP,18,3)."""
    base = 1e4 * (step + 1) + 100.0 * np.arange(B)[:, None, None] + np.arange(NP)[None, :, None]
    return base + 1e-3 * np.arange(68)[None, None, :], (-base - 1e-3 * np.arange(54)[None, None, :]).reshape(B, NP, 18, 3)


@functools.lru_cache(maxsize=None)
def multistep(name, n_inits=3):
    """-> (start, steps): start = the tables before the first frame; steps[k] = dict(inputs of frame k's assignment (labels made for
    the table the restatement holds at that point), assign = tn.assign_np's result, ik_params, ik_joints, after = tn.commit_np's
    result with 'overflow' accumulated over the frames)."""
    C, P, T, K, V = ASSIGN_SHAPES[MULTI_SHAPES[name]]
    B, N = B_CHAINS, C * P
    rng = np.random.default_rng([41, C, P, T])
    counts = _counts(C, P, rng)
    quiet = np.arange(B) % 9 == 4                       # chains where nothing is ever matched: what they hold dies, nothing is born
    n_tracks = np.array([0 if (b % 3 == 0 or b % 18 == 4) else b % (T + 1) for b in range(B)], np.int32)
    meta = np.zeros((B, T, 4), np.int32)
    for b in range(B):
        for s in range(T):
            meta[b, s] = (1000 * b + s, 1 + (b + s) % 2, 1 + (b + 2 * s) % 3, 5 + s)
    start = dict(params=_table((B, T, 68), 0.25), joints=-_table((B, T, 18, 3), 0.5), meta=meta, n_tracks=n_tracks,
                 next_id=(100 + 3 * np.arange(B)).astype(np.int32), n_dead=(7 + np.arange(B)).astype(np.int32),
                 overflow=np.zeros(B, np.int32))
    cur, steps = start, []
    for k in range(N_STEPS):
        frame_idx = ((np.arange(B) + k) % N_FRAMES).astype(np.int32)
        lab_sp, lab_st = np.zeros((B, N), np.int32), np.zeros((B, T + N), np.int32)
        ncl_sp, ncl_st = np.zeros(B, np.int32), np.zeros(B, np.int32)
        for b in range(B):
            lab_sp[b], ncl_sp[b] = _random_labels(N, rng, (b + k) % 4 == 0)
            lab_st[b], ncl_st[b] = _random_labels(T + N, rng, (b + k) % 4 == 0)
        lab_sp[quiet], lab_st[quiet] = -1, -1
        a = tn.assign_np(lab_sp, ncl_sp, lab_st, ncl_st, counts, frame_idx, cur["n_tracks"], cur["params"], P, K, V)
        ikp, ikj = fake_solve(B, T + K, k)
        after = tn.commit_np(a[3], a[4], ikp, ikj, cur["params"], cur["joints"], cur["meta"], cur["n_tracks"], cur["next_id"],
                             cur["n_dead"], K, n_inits)
        after["overflow"] = cur["overflow"] | a[5] | after["overflow"]
        steps.append(dict(labels_sp=lab_sp, ncl_sp=ncl_sp, labels_st=lab_st, ncl_st=ncl_st, counts=counts, frame_idx=frame_idx,
                          assign=a, ik_params=ikp, ik_joints=ikj, after=after))
        cur = after
    return start, steps


# ------------------------------------------------------------------------------------------------------------------------------------
def _both(flags, what):
    assert flags.any(), f"no chain with: {what}"
    assert not flags.all(), f"every chain with: {what}"


def check_coverage():
    """Asserts, on the restatement alone, that the cases reach what they are for.  -> dict of counts (printed by the CPU test)."""
    rep = {}
    # ---- the graph
    c = affinity_case("small")
    W, D, gc = affinity_reference("small")
    B, T = len(c["n_tracks"]), c["T"]
    assert sorted(set(c["n_tracks"].tolist())) == [-3, 0, 1, T, T + 5]
    assert (c["counts"] == -1).any() and (c["counts"] == c["Pn"] + 4).any()
    fi = c["frame_idx"].tolist()
    assert len(set(fi)) < len(fi) and any(a > b for a, b in zip(fi, fi[1:])) and any(abs(a - b) > 1 for a, b in zip(fi, fi[1:]))
    n = gc.sum(axis=1)
    assert (n[np.clip(c["n_tracks"], 0, T) == 0] == 0).all() and (n[c["n_tracks"] > 0] > 0).all()
    nan_rows = cut = kept = far_chains = 0
    margin = np.inf
    for name in ("small", "limit"):
        cc, (Wn, Dn, gcn) = affinity_case(name), affinity_reference(name)
        for b in range(len(cc["n_tracks"])):
            nb = int(gcn[b].sum())
            if nb == 0:
                assert not Wn[b].any() and not Dn[b].any()
                continue
            S = tn.uncut_affinity(Dn[b], nb)
            margin = min(margin, float(np.abs(S - CUT).min()))
            off = ~np.eye(nb, dtype=bool)
            fin = off & ~np.isnan(Dn[b, :nb, :nb])
            nan_rows += int((np.isnan(Dn[b, :nb, :nb]) | ~off).all(axis=1).sum())
            cut += int((fin & (Wn[b, :nb, :nb] == 0)).sum())
            kept += int((fin & (Wn[b, :nb, :nb] > 0)).sum())
            far_chains += int(fin.any() and not (fin & (Wn[b, :nb, :nb] > 0)).any())
            assert not Wn[b, nb:].any() and not Wn[b, :, nb:].any() and not Dn[b, nb:].any() and not Dn[b, :, nb:].any()
    assert margin > 1e-8, margin          # no affinity at the cut: the comparison never has to leave an entry out
    assert nan_rows >= 1 and cut >= 1 and kept >= 1 and far_chains >= 1
    assert affinity_reference("limit")[2].sum(axis=1).tolist() == [80, 73]
    # scores exactly at the threshold decide entries: with the threshold one ulp lower the distances differ
    lower = tn.st_affinity_np(c["kps17"], c["counts"], c["frame_idx"], c["track_joints"], c["n_tracks"], c["P"], c["F2"],
                              np.nextafter(MIN_SCORE, 0.0))[1]
    diff = ~np.isclose(lower, D, rtol=0, atol=1e-6, equal_nan=True)
    on_frame0 = c["frame_idx"] == 0
    assert diff[on_frame0].any() and not diff[~on_frame0].any()
    k = c["kps17"][0]
    assert k[0, 0, 5, 2] * k[1, 1, 5, 2] == MIN_SCORE and k[2, 0, 7, 2] == MIN_SCORE
    n_2d = int((diff[on_frame0][:, T:, T:]).sum())
    n_3d = int(diff[on_frame0].sum()) - n_2d
    assert n_2d >= 1 and n_3d >= 1
    rep["graph"] = dict(nan_rows=nan_rows, cut_entries=cut, kept_entries=kept, chains_all_beyond_cut=far_chains, margin_at_cut=margin,
                        entries_decided_by_threshold_scores=(n_2d, n_3d))
    # ---- the assignment
    fts = {name: assign_features(name) for name in ASSIGN_SHAPES}
    for key in fts["a334"]:
        flags = np.concatenate([fts[name][key] for name in ASSIGN_SHAPES])
        _both(flags, key)
        rep.setdefault("assign", {})[key] = int(flags.sum())
    assert fts["a8816"]["straddle_64"].any() and fts["a334"]["over_K"].any() and fts["a334"]["over_V"].any()
    for name in ASSIGN_SHAPES:
        st = assign_reference(name)[3]
        for v in (0, 1, 2):
            rep["assign"][f"{name}_status{v}"] = int((st == v).any(axis=1).sum())
            assert (st == v).any(), (name, v)
    assert assign_reference("cut64")[5].tolist() == [1, 0, 1]
    # ---- the commit
    for name in COMMIT_SHAPES:
        for n_inits in (1, 3):
            ft = commit_features(name, n_inits)
            for key, flags in ft.items():
                if key == "one_short" and n_inits == 1:
                    continue                            # (nothing can be one short of n_inits = 1)
                _both(flags, f"{name} n_inits={n_inits} {key}")
                rep.setdefault(f"commit_{name}_{n_inits}", {})[key] = int(flags.sum())
            r = commit_reference(name, n_inits)
            _both((r["overflow"] & 2) != 0, f"{name} overflow bit 1")
    c4 = commit_case("c4")
    full = c4["n_tracks"] >= 4
    assert len({tuple(r) for r in c4["status"][full]}) >= 30 and {(0,) * 4, (1,) * 4, (2,) * 4} <= {tuple(r) for r in c4["status"]}
    # ---- several frames
    for name in MULTI_SHAPES:
        start, steps = multistep(name)
        nts = np.array([s["after"]["n_tracks"] for s in steps])
        born = steps[-1]["after"]["next_id"] - start["next_id"]
        died = steps[-1]["after"]["n_dead"] - start["n_dead"]
        _both(born > 0, f"{name} births")
        _both(died > 0, f"{name} deaths")
        assert (nts > 0).any(axis=1).all() and (nts == 0).any()
        rep[f"multi_{name}"] = dict(born=int(born.sum()), died=int(died.sum()), overflow_chains=int((steps[-1]["after"]["overflow"] != 0).sum()))
    return rep
