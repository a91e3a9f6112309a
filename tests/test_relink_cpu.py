"""CPU: the re-linking step's NumPy restatement (tests/relink_np.py) on ground truth and against scipy's assignment, the host side of
multiview_motion_capture_amd/relinking.py (packing, record building, input errors), and the switches of the batched entry points."""
import inspect

import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

import relink_np as rn
from relink_cases import CUT_CASES, PARAMS, cut_case, make_tracklets, shelf_oracle_records, true_links


def _objective(a, col_of):
    return float(a[np.arange(a.shape[0]), col_of].sum())


@pytest.mark.parametrize("C,P,seed", CUT_CASES)
def test_restatement_returns_exactly_the_true_links_of_cut_ground_truth(C, P, seed):
    """Every person's ground-truth track (1 cm noise) cut at 3 frames, a hole of 1 .. 16 frames after each cut, the pieces shuffled:
    the links taken are the next piece of the same person wherever the hole is <= 16 -- none wrong, none missed -- and the assignment's
    objective is scipy's on the same n x 2n matrix."""
    people, recs = cut_case(C, P, seed)
    res = rn.relink(recs, **PARAMS)
    got, true = rn.record_links(recs, res), true_links(people, recs)
    print(f"C{C} P{P} seed {seed}: {len(recs)} pieces, {len(true)} true links, {len(got)} taken, largest cost {res['cost'].max():.3f} m")
    assert got == true, (sorted(got - true), sorted(true - got))
    r, c = linear_sum_assignment(res["matrix"])
    assert abs(_objective(res["matrix"], res["col_of"]) - float(res["matrix"][r, c].sum())) <= 1e-12


def test_restatement_assignment_is_optimal_on_random_sparse_matrices():
    rng = np.random.default_rng(20270601)
    for _ in range(200):
        n = int(rng.integers(1, 41))
        a = np.full((n, 2 * n), rn.BIG)
        allowed = rng.random((n, n)) < rng.uniform(0.02, 0.4)
        np.fill_diagonal(allowed, False)
        a[:, :n][allowed] = rng.uniform(0.0, 0.5, size=int(allowed.sum()))
        a[np.arange(n), n + np.arange(n)] = 0.5
        col_of = rn.assign_rows(a)
        assert np.unique(col_of).size == n
        r, c = linear_sum_assignment(a)
        assert abs(_objective(a, col_of) - float(a[r, c].sum())) <= 1e-12


def test_shelf_oracle_records_take_exactly_three_links():
    recs = shelf_oracle_records()
    res = rn.relink(recs, **PARAMS)
    ids = [r[0] for r in recs]
    links = sorted((ids[a], ids[b]) for a, b in rn.record_links(recs, res))
    assert links == [(7, 10), (10, 11), (14, 15)], links
    o = res["order"]
    for k in range(len(recs)):
        if len(recs[o[k]][1]) == 300:
            assert res["succ"][k] < 0 and res["head"][k] == k
    assert sum(len(r[1]) == 300 for r in recs) == 2


def _packed_cost_matrix(packed, s, max_gap, max_dist, near_dist, speed):
    """The kernel's formula on the packed arrays of sequence s, in NumPy."""
    a0, n = int(packed["seq"][s, 0]), int(packed["seq"][s, 1])
    rec, fr = packed["rec"][a0:a0 + n], packed["frames"][a0:a0 + n].astype(np.int64)
    a = np.full((n, 2 * n), rn.BIG)
    for i in range(n):
        for j in range(n):
            gap = fr[j, 0] - fr[i, 1]
            if i == j or gap < 1 or gap > max_gap:
                continue
            vs = []
            if fr[i, 2] > 0:
                vs.append((rec[i, 108:111] - rec[i, 111:114]) / fr[i, 2])
            if fr[j, 3] > 0:
                vs.append((rec[j, 117:120] - rec[j, 114:117]) / fr[j, 3])
            v = np.mean(vs, axis=0) if vs else np.zeros(3)
            c = np.linalg.norm(rec[i, :54].reshape(18, 3) + v * gap - rec[j, 54:108].reshape(18, 3), axis=-1).mean()
            if np.isfinite(c) and c <= min(max_dist, near_dist + speed * gap):
                a[i, j] = c
        a[i, n + i] = max_dist
    return a


def test_packed_arrays_carry_the_statement():
    """pack_records: nodes in (first frame, track id) order whatever the order of the list, and the launch's arrays give the
    restatement's cost matrix."""
    from multiview_motion_capture_amd.relinking import pack_records
    recs = shelf_oracle_records()
    _, cut = cut_case(5, 4, 20270501)
    packed = pack_records([make_tracklets(recs), [], make_tracklets(cut)])
    assert packed["seq"][:, :2].tolist() == [[0, len(recs)], [len(recs), 0], [len(recs), len(cut)]] and packed["work_words"] == 0
    for s, rr in ((0, recs), (2, cut)):
        res = rn.relink(rr, **PARAMS)
        assert np.array_equal(packed["order"][s], res["order"])
        a = _packed_cost_matrix(packed, s, **PARAMS)
        assert np.array_equal(a >= rn.BIG, res["matrix"] >= rn.BIG) and np.abs(a - res["matrix"]).max() <= 1e-12
    big = pack_records([make_tracklets([(i, np.array([3 * i]), np.zeros((1, 18, 3))) for i in range(65)])])
    assert big["work_words"] == 65 * 65


def _merged(recs, **kw):
    """Restatement links -> merge_records: what relink_tracklets returns, without a device."""
    from multiview_motion_capture_amd.relinking import merge_records, pack_records
    tl = make_tracklets(recs)
    order = pack_records([tl])["order"][0]
    res = rn.relink(recs, **dict(PARAMS, **kw))
    assert np.array_equal(order, res["order"])
    return tl, merge_records(tl, order, res["head"], res["pos"], res["cost"]), res


def test_order_independence_and_the_merged_record():
    from multiview_motion_capture_amd.motion_capture import MvTracklet, TrackState
    people, recs = cut_case(5, 4, 20270502)
    tl, out, res = _merged(recs)
    perm = np.random.default_rng(3).permutation(len(recs))
    _, out2, _ = _merged([recs[i] for i in perm])
    key = lambda t: t.track_id
    assert [(t.track_id, t.relink_parts, t.relink_costs, t.frame_idxs) for t in sorted(out, key=key)] == \
           [(t.track_id, t.relink_parts, t.relink_costs, t.frame_idxs) for t in sorted(out2, key=key)]
    assert [len(t) for t in out] == sorted((len(t) for t in out), reverse=True)
    assert sum(len(t.relink_parts) for t in out) == len(recs) and len(out) == len(recs) - int((res["succ"] >= 0).sum())
    by_id = {t.track_id: t for t in tl}
    joined = [t for t in out if len(t.relink_parts) > 1]
    assert joined
    before = [(list(t.frame_idxs), list(t.poses), t.hits) for t in tl]
    for t in out:
        assert isinstance(t, MvTracklet) and t not in tl
        parts = [by_id[p[0]] for p in t.relink_parts]
        assert t.relink_parts == [(p.track_id, p.frame_idxs[0], p.frame_idxs[-1]) for p in parts]
        assert len({people[p.track_id] for p in parts}) == 1
        assert t.track_id == parts[0].track_id == min(parts, key=lambda p: p.frame_idxs[0]).track_id
        assert t.frame_idxs == [f for p in parts for f in p.frame_idxs] and np.all(np.diff(t.frame_idxs) > 0)
        assert len(t.poses) == len(t.frame_idxs) == t.hits
        assert all(a is b for a, b in zip(t.poses, [q for p in parts for q in p.poses]))      # no pose changed, none invented
        assert t.state == parts[-1].state == TrackState.Confirmed and t.time_since_update == parts[-1].time_since_update
        assert len(t.relink_costs) == len(parts) - 1 and all(0 < c <= 0.5 for c in t.relink_costs)
        assert not hasattr(t, "bone_lens")
    for t in joined:
        assert any(b - a > 1 for a, b in zip(t.frame_idxs[:-1], t.frame_idxs[1:]))       # the hole stays a hole
    assert before == [(list(t.frame_idxs), list(t.poses), t.hits) for t in tl]           # the inputs are untouched


def _walk(f0, n, x0, step=0.02, hole=()):
    """A rigid 18-joint body walking along x from x0 at frame f0: (frames, joints)."""
    frames = np.array([f for f in range(f0, f0 + n) if f not in hole])
    body = np.random.default_rng(1).normal(0, 0.3, size=(18, 3))
    return frames, body[None] + np.stack([x0 + step * (frames - f0), 0 * frames, 0 * frames], axis=-1)[:, None, :]


def test_gates():
    # the same walk continued after a hole: one link at (nearly) zero cost, whatever the hole within max_gap
    a = _walk(0, 20, 0.0)
    for gap in (1, 5, 16):
        b = _walk(19 + gap, 10, 0.02 * (19 + gap))
        res = rn.relink([(0, *a), (1, *b)], **PARAMS)
        assert res["succ"].tolist() == [1, -1] and res["cost"][0] <= 1e-12
    # gap max_gap + 1: not taken
    b = _walk(19 + 17, 10, 0.02 * (19 + 17))
    assert rn.relink([(0, *a), (1, *b)], **PARAMS)["succ"].tolist() == [-1, -1]
    assert rn.relink([(0, *a), (1, *b)], **dict(PARAMS, max_gap=17))["succ"].tolist() == [1, -1]
    # records that overlap in time (also by one frame) are left alone, however close
    for f0 in (10, 19):
        b = _walk(f0, 10, 0.02 * f0)
        assert rn.relink([(0, *a), (1, *b)], **PARAMS)["succ"].tolist() == [-1, -1]
    # a link just above / just below its gate near_dist + speed gap (gap 2: 0.21 m), and above max_dist at a long gap
    for gap, off, taken in ((2, 0.2101, False), (2, 0.2099, True), (16, 0.5001, False), (16, 0.4999, True)):
        fb, jb = _walk(19 + gap, 10, 0.02 * (19 + gap))
        jb = jb + np.array([0.0, off, 0.0])
        res = rn.relink([(0, *a), (1, fb, jb)], **PARAMS)
        assert res["succ"].tolist() == ([1, -1] if taken else [-1, -1]), (gap, off)
        if taken:
            assert abs(res["cost"][0] - off) <= 1e-9
    # two one-pose records: no velocity, the last pose is held
    one = [(0, np.array([5]), a[1][:1]), (1, np.array([7]), a[1][:1] + 0.1)]
    res = rn.relink(one, **PARAMS)
    assert res["succ"].tolist() == [1, -1] and abs(res["cost"][0] - 0.1 * np.sqrt(3)) <= 1e-12
    # a non-finite joint: no link
    bad = a[1].copy()
    bad[-1, 3, 1] = np.nan
    b = _walk(21, 10, 0.02 * 21)
    assert rn.relink([(0, a[0], bad), (1, *b)], **PARAMS)["succ"].tolist() == [-1, -1]
    # two candidates for one successor: the cheaper link wins, the other record stays alone
    c = _walk(0, 20, 0.0)
    jc = c[1] + np.array([0.0, 0.05, 0.0])
    b = _walk(22, 10, 0.02 * 22)
    res = rn.relink([(0, c[0], jc), (1, *a), (2, *b)], **PARAMS)
    assert res["succ"].tolist() == [-1, 2, -1]


def test_value_errors_before_any_device_work():
    from multiview_motion_capture_amd.relinking import MAX_RECORDS, relink_sequences, relink_tracklets
    good = make_tracklets([(0, *_walk(0, 10, 0.0)), (1, *_walk(12, 10, 0.24))])
    for kw in (dict(max_gap=0), dict(max_gap=-3), dict(max_gap=2.5), dict(max_dist=-0.1), dict(max_dist=float("nan")),
               dict(max_dist=float("inf")), dict(near_dist=-1.0), dict(near_dist=float("inf")), dict(speed=-0.01),
               dict(speed=float("nan"))):
        with pytest.raises(ValueError):
            relink_sequences([good], **kw)
    bad = make_tracklets([(0, *_walk(0, 10, 0.0))])
    bad[0].frame_idxs = [0, 1, 2, 3, 3, 5, 6, 7, 8, 9]
    with pytest.raises(ValueError, match="increase"):
        relink_tracklets(good + bad)
    bad[0].frame_idxs = list(range(9, -1, -1))
    with pytest.raises(ValueError, match="increase"):
        relink_tracklets(bad)
    bad = make_tracklets([(0, *_walk(0, 10, 0.0))])
    bad[0].poses[-1][2].keypoints = np.zeros((17, 3))
    with pytest.raises(ValueError, match="18 x 3"):
        relink_tracklets(bad)
    bad = make_tracklets([(0, *_walk(0, 10, 0.0))])
    bad[0].poses = bad[0].poses[:-1]
    with pytest.raises(ValueError):
        relink_tracklets(bad)
    many = make_tracklets([(i, np.array([2 * i]), np.zeros((1, 18, 3))) for i in range(MAX_RECORDS + 1)])
    with pytest.raises(ValueError, match="at most"):
        relink_sequences([good, many])
    assert relink_sequences([]) == [] and relink_sequences([[], []]) == [[], []]


def test_relink_is_off_by_default():
    from multiview_motion_capture_amd.motion_capture import run_main_batched
    from multiview_motion_capture_amd.sequences import track_sequences
    for fn in (track_sequences, run_main_batched):
        p = inspect.signature(fn).parameters["relink"]
        assert p.default is False


def test_header_capacity_matches_the_package():
    import os
    import re

    from conftest import ROOT
    from multiview_motion_capture_amd import _cabi, relinking
    text = open(os.path.join(ROOT, "include", "mvmc.h")).read()
    assert int(re.search(r"#define\s+MVMC_RELINK_MAX_RECORDS\s+(\d+)", text).group(1)) == relinking.MAX_RECORDS == \
        _cabi.RELINK_MAX_RECORDS >= 512
    assert int(re.search(r"#define\s+MVMC_RELINK_REC_DOUBLES\s+(\d+)", text).group(1)) == relinking._REC == _cabi.RELINK_REC_DOUBLES
    lib = _cabi.load()
    assert lib.mvmc_relink_work_words(64) == 0 and lib.mvmc_relink_work_words(65) == 65 * 65
    assert lib.mvmc_relink_work_words(513) == -1 and lib.mvmc_relink_work_words(-1) == -1
    assert lib.mvmc_relink(None, None, None, 0, 1, 0, 0.5, 0.15, 0.03, None, None, None, None, None, None, 0, None) == 1
    assert lib.mvmc_relink(None, None, None, 0, 1, 16, float("nan"), 0.15, 0.03, None, None, None, None, None, None, 0, None) == 1
    assert lib.mvmc_relink(None, None, None, 4, 1, 16, 0.5, 0.15, 0.03, None, None, None, None, None, None, 0, None) == 1
