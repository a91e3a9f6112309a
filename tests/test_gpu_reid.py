"""GPU: re-identification by bone lengths (relinking.reidentify_sequences; csrc/mvmc_relink.hip: mvmc_reid_signature, mvmc_reid_link)
against its NumPy restatement (tests/reid_np.py) to the last bit, each entry directly and through the Python API, and end to end
through the real tracker on a scene whose people are hidden for seconds."""
import ctypes

import numpy as np
import pytest

import reid_cases as rc
import reid_np as rp
from relink_cases import identity_shares, label_poses, make_tracklets

pytestmark = pytest.mark.gpu

SENT_F, SENT_I = -7.25, -77


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else None)


def _signature(joints, rec, min_poses, n_poses=None, work_words=0, null=()):
    """mvmc_reid_signature directly: (return code, sig, cnt, ends, status); the outputs start as sentinels."""
    import torch
    from multiview_motion_capture_amd import _cabi
    from multiview_motion_capture_amd.device import _stream
    lib = _cabi.load()
    rec = np.asarray(rec, np.int32).reshape(-1, 2)
    N = rec.shape[0]
    j_d, r_d = _dev(np.asarray(joints, np.float64).reshape(-1, 18, 3)), _dev(rec)
    t = dict(sig=torch.full((max(N, 1), 20), SENT_F, dtype=torch.float64, device="cuda:0"),
             cnt=torch.full((max(N, 1), 10), SENT_I, dtype=torch.int32, device="cuda:0"),
             ends=torch.full((max(N, 1), 6), SENT_F, dtype=torch.float64, device="cuda:0"),
             status=torch.full((max(N, 1),), SENT_I, dtype=torch.int32, device="cuda:0"))
    work = torch.zeros((max(1, work_words),), dtype=torch.float64, device="cuda:0")
    a = {k: (None if k in null else v) for k, v in dict(t, joints=j_d, rec=r_d, work=work).items()}
    code = lib.mvmc_reid_signature(_ptr(a["joints"]), _ptr(a["rec"]), j_d.shape[0] if n_poses is None else n_poses, N, min_poses,
                                   _ptr(a["sig"]), _ptr(a["cnt"]), _ptr(a["ends"]), _ptr(a["status"]), _ptr(a["work"]),
                                   ctypes.c_longlong(work_words), _stream())
    torch.cuda.synchronize()
    return (code,) + tuple(t[k].cpu().numpy()[:N] for k in ("sig", "cnt", "ends", "status"))


def _link(sig, ends, frames, seq, par, n_records=None, work_words=0, null=()):
    """mvmc_reid_link directly: (return code, succ, head, pos, cost, status); the outputs start as sentinels."""
    import torch
    from multiview_motion_capture_amd import _cabi
    from multiview_motion_capture_amd.device import _stream
    lib = _cabi.load()
    seq = np.asarray(seq, np.int32).reshape(-1, 4)
    N, S = np.asarray(sig).reshape(-1, 20).shape[0], seq.shape[0]
    ins = dict(sig=_dev(np.asarray(sig, np.float64).reshape(-1, 20)), ends=_dev(np.asarray(ends, np.float64).reshape(-1, 6)),
               frames=_dev(np.asarray(frames, np.int32).reshape(-1, 2)), seq=_dev(seq))
    t = {k: torch.full((max(N, 1),), SENT_I, dtype=torch.int32, device="cuda:0") for k in ("succ", "head", "pos")}
    t["cost"] = torch.full((max(N, 1),), SENT_F, dtype=torch.float64, device="cuda:0")
    t["status"] = torch.full((max(S, 1),), SENT_I, dtype=torch.int32, device="cuda:0")
    work = torch.zeros((max(1, work_words),), dtype=torch.float64, device="cuda:0")
    a = {k: (None if k in null else v) for k, v in dict(t, work=work, **ins).items()}
    code = lib.mvmc_reid_link(_ptr(a["sig"]), _ptr(a["ends"]), _ptr(a["frames"]), _ptr(a["seq"]), N if n_records is None else n_records,
                              S, int(par.get("max_gap") or 0), par["max_z"], par["ratio"], par["floor"], par["reach"], par["speed"],
                              _ptr(a["succ"]), _ptr(a["head"]), _ptr(a["pos"]), _ptr(a["cost"]), _ptr(a["status"]), _ptr(a["work"]),
                              ctypes.c_longlong(work_words), _stream())
    torch.cuda.synchronize()
    return (code,) + tuple(t[k].cpu().numpy()[:(S if k == "status" else N)] for k in ("succ", "head", "pos", "cost", "status"))


def _bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def _same_nan_or_bits(a, b):
    """Equal to the last bit; a NaN equals a NaN whatever its payload."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and _bits(np.nan_to_num(a), np.nan_to_num(b))


SIG_POSES = (1, 2, 9, 10, 11, 63, 64, 65, 256, 257, 512, 513)     # 512: the LDS capacity (MVMC_REID_LDS_POSES)


def _signature_records():
    """Noisy skeletons of the poses counts above (duplicated values, a NaN joint here and there), then the hand-built cases' records."""
    rng = np.random.default_rng(20280801)
    blocks = []
    for m in SIG_POSES:
        J = np.repeat(rc.skeleton(rc.BASE * rng.uniform(0.9, 1.1), rng.uniform(-2, 2, size=3))[None], m, axis=0)
        J = J + np.round(rng.normal(0, 0.01, size=J.shape), 3)          # rounding makes duplicates
        if m >= 9:
            J[m // 2], J[m - 2] = J[0], J[1]
            J[rng.integers(m, size=m // 8), rng.integers(18, size=m // 8)] = np.nan
        blocks.append(J)
    for recs, _, _ in rc.link_cases().values():
        blocks += [r[2] for r in recs]
    return blocks


@pytest.mark.parametrize("min_poses", [10, 1])
def test_signature_equals_the_restatement_to_the_last_bit(min_poses):
    blocks = _signature_records()
    n = [b.shape[0] for b in blocks]
    rec = np.stack([np.cumsum([0] + n[:-1]), n], axis=1)
    joints = np.concatenate(blocks)
    code, sig, cnt, ends, status = _signature(joints, rec, min_poses, work_words=10 * joints.shape[0])
    assert code == 0 and np.all(status == 0)
    for k, J in enumerate(blocks):
        med, se, c = rp.signature(J, min_poses)
        assert np.array_equal(cnt[k], c), (k, n[k])
        assert _same_nan_or_bits(sig[k, :10], med) and _same_nan_or_bits(sig[k, 10:], se), (k, n[k], sig[k], med, se)
        assert _same_nan_or_bits(ends[k], rp.end_centroids(J)), (k, n[k])
    # a record beyond the LDS capacity without a workspace is refused alone
    code, sig2, cnt2, ends2, status2 = _signature(joints, rec, min_poses)
    big = np.array(n) > 512
    assert code == 0 and np.array_equal(status2, np.where(big, 2, 0))
    assert np.all(sig2[big] == SENT_F) and np.all(cnt2[big] == SENT_I) and np.all(ends2[big] == SENT_F)
    assert _same_nan_or_bits(sig2[~big], sig[~big]) and np.array_equal(cnt2[~big], cnt[~big])


def test_signature_refuses_malformed_rows_and_arguments():
    J = np.repeat(rc.skeleton(rc.BASE)[None], 30, axis=0)
    rec = [[0, 10], [-1, 5], [10, 0], [25, 6], [10, 20], [0, 65537]]
    code, sig, cnt, ends, status = _signature(J, rec, 1)
    assert code == 0 and status.tolist() == [0, 2, 2, 2, 0, 2]
    bad = status == 2
    assert np.all(sig[bad] == SENT_F) and np.all(cnt[bad] == SENT_I) and np.all(ends[bad] == SENT_F)
    assert np.array_equal(sig[0, :10], rc.BASE) and np.array_equal(sig[4, :10], rc.BASE)
    for kw in (dict(min_poses=0), dict(n_poses=-1), dict(work_words=-1), dict(null=("rec",)), dict(null=("sig",)), dict(null=("cnt",)),
               dict(null=("ends",)), dict(null=("status",)), dict(null=("joints",)), dict(null=("work",), work_words=8)):
        kw = dict(dict(min_poses=1), **kw)
        code, sig, cnt, ends, status = _signature(J, rec, **kw)
        assert code == 1, kw
        assert np.all(sig == SENT_F) and np.all(cnt == SENT_I) and np.all(ends == SENT_F) and np.all(status == SENT_I), kw


LINK_SIZES = (0, 1, 2, 3, 64, 65)      # 64 / 65: the LDS / workspace boundary


def _api(recs_per_sequence, par=None, **kw):
    from multiview_motion_capture_amd.relinking import reidentify_sequences
    links = []
    out = reidentify_sequences([make_tracklets(r) if r else [] for r in recs_per_sequence], links=links, **dict(par or rc.PARAMS, **kw))
    return out, links


def _equal_to_restatement(link, recs, par, what):
    res = rp.reidentify(recs, **par)
    for k in ("order", "succ", "head", "pos", "cnt"):
        assert np.array_equal(link[k], res[k]), (what, k, link[k], res[k])
    assert _bits(link["cost"], res["cost"]), (what, link["cost"], res["cost"])
    assert _same_nan_or_bits(link["sig"], res["sig"]) and _same_nan_or_bits(link["ends"], res["ends"]), what
    return res


def _all_bits(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("order", "succ", "head", "pos", "cnt")) and _bits(a["cost"], b["cost"]) and \
        _same_nan_or_bits(a["sig"], b["sig"]) and _same_nan_or_bits(a["ends"], b["ends"])


def test_links_equal_the_restatement_at_every_size():
    seqs = [rc.random_sequence(n, 20280810 + n) for n in LINK_SIZES]
    _, links = _api(seqs)
    n_links = 0
    for n, recs, ln in zip(LINK_SIZES, seqs, links):
        res = _equal_to_restatement(ln, recs, rc.PARAMS, f"{n} records")
        n_links += int((res["succ"] >= 0).sum())
        print(f"{n} records: {int((res['succ'] >= 0).sum())} links, {int((res['matrix'][:, :n] < rp.BIG).sum())} allowed")
    assert n_links >= 10


def test_hand_built_cases_link_for_link():
    cases = rc.link_cases()
    for name, (recs, want, par) in cases.items():
        out, links = _api([recs], par)
        _equal_to_restatement(links[0], recs, par, name)
        assert rc.taken(recs, links[0]) == want, name
        parts = {tuple(p[0] for p in t.reid_parts) for t in out[0] if len(t.reid_parts) > 1}
        assert {(a, b) for p in parts for a, b in zip(p[:-1], p[1:])} == want, name
        # the order of the caller's list does not matter
        assert rc.taken(recs[::-1], _api([recs[::-1]], par)[1][0]) == want, name


def test_records_are_new_and_carry_the_links():
    recs, _, par = rc.link_cases()["a chain of three"]
    tl = make_tracklets(recs)
    for t in tl:
        t.relink_parts, t.relink_costs = [(t.track_id, t.frame_idxs[0], t.frame_idxs[-1])], []
    from multiview_motion_capture_amd.relinking import reidentify_tracklets
    before = [(t.track_id, list(t.frame_idxs), len(t.poses)) for t in tl]
    out = reidentify_tracklets(tl, **par)
    assert [(t.track_id, list(t.frame_idxs), len(t.poses)) for t in tl] == before and len(out) == 1
    t = out[0]
    assert t.track_id == 5 and t.reid_parts == [(5, 0, 19), (3, 50, 69), (4, 120, 139)] and t.reid_costs == [0.0, 0.0]
    assert t.relink_parts == t.reid_parts and t.relink_costs == []
    assert t.frame_idxs == list(range(20)) + list(range(50, 70)) + list(range(120, 140)) and len(t.poses) == 60 == t.hits
    assert all(a is b for a, b in zip(t.poses[:20], tl[0].poses))
    assert np.array_equal(t.reid_lengths, rc.BASE) and np.array_equal(t.reid_sigma, np.zeros(10))


def test_five_sequences_alone_together_and_twice():
    seqs = [rc.random_sequence(n, 20280820 + n) for n in (7, 30, 64, 65, 12)]
    _, together = _api(seqs)
    _, again = _api(seqs)
    for s in range(5):
        assert _all_bits(together[s], again[s]), s
        assert _all_bits(_api([seqs[s]])[1][0], together[s]), s


def _link_inputs(n, seed):
    recs = rc.random_sequence(n, seed)
    res = rp.reidentify(recs, **rc.PARAMS)
    nodes = [recs[i] for i in res["order"]]
    return res, res["sig"], res["ends"], np.array([[r[1][0], r[1][-1]] for r in nodes], np.int32)


def test_link_refuses_malformed_rows_and_arguments():
    res, sig, ends, frames = _link_inputs(6, 20280830)
    seq = [[0, 3, 0, 0], [3, 4, 0, 0], [-1, 2, 0, 0], [0, 513, 0, 0], [3, 3, 0, 0]]
    code, succ, head, pos, cost, status = _link(sig, ends, frames, seq, rc.PARAMS)
    assert code == 0 and status.tolist() == [0, 2, 2, 2, 0]
    assert np.all(succ != SENT_I) and np.all(cost != SENT_F)                   # rows 0 and 4 cover the six records
    # a sequence of 65 records without a workspace: status 2, nothing written
    res, sig, ends, frames = _link_inputs(65, 20280831)
    code, succ, head, pos, cost, status = _link(sig, ends, frames, [[0, 65, 0, 0]], rc.PARAMS)
    assert code == 0 and status.tolist() == [2]
    assert np.all(succ == SENT_I) and np.all(head == SENT_I) and np.all(pos == SENT_I) and np.all(cost == SENT_F)
    code, succ, head, pos, cost, status = _link(sig, ends, frames, [[0, 65, 0, 0]], rc.PARAMS, work_words=2 * 65 * 65)
    assert code == 0 and status.tolist() == [0] and np.array_equal(succ, res["succ"]) and _bits(cost, res["cost"])
    P = rc.PARAMS
    for kw in (dict(par=dict(P, max_z=-1.0)), dict(par=dict(P, max_z=float("nan"))), dict(par=dict(P, ratio=1.5)), dict(par=dict(P, ratio=-0.5)),
               dict(par=dict(P, floor=float("inf"))), dict(par=dict(P, floor=-1.0)), dict(par=dict(P, reach=float("nan"))),
               dict(par=dict(P, reach=-1.0)), dict(par=dict(P, speed=-1.0)), dict(par=dict(P, speed=float("inf"))), dict(par=dict(P, max_gap=-1)),
               dict(n_records=-1), dict(work_words=-1), dict(null=("work",), work_words=8), dict(null=("seq",)), dict(null=("status",)),
               dict(null=("sig",)), dict(null=("ends",)), dict(null=("frames",)), dict(null=("succ",)), dict(null=("head",)),
               dict(null=("pos",)), dict(null=("cost",))):
        kw = dict(dict(par=P), **kw)
        code, succ, head, pos, cost, status = _link(sig, ends, frames, [[0, 65, 0, 0]], **kw)
        assert code == 1, kw
        assert np.all(succ == SENT_I) and np.all(head == SENT_I) and np.all(pos == SENT_I) and np.all(cost == SENT_F), kw
        assert np.all(status == SENT_I), kw


def _calibs(g):
    from multiview_motion_capture_amd.common import Calib
    return [Calib.from_k_rt(g["K"][c], g["Rt"][c]) for c in range(g["K"].shape[0])]


def _state(t):
    return (t.track_id, list(t.frame_idxs), t.state, t.hits, t.time_since_update, sorted(k for k in vars(t) if k.startswith(("reid", "relink"))),
            np.array([p[2].keypoints for p in t.poses]).tobytes(), np.array([np.concatenate([np.ravel(x) for x in vars(p[1]).values()])
                                                                             for p in t.poses]).tobytes())


def test_the_keyword_off_is_the_code_path_of_today():
    from multiview_motion_capture_amd import synth
    from multiview_motion_capture_amd.sequences import track_sequences
    g = synth.generate(48, 4, 3, 20280840, walk="scene")
    seqs = [(g["kps25"], g["counts"], _calibs(g))]
    for kw in (dict(), dict(relink=True)):
        a, b = track_sequences(seqs, chain_len=16, **kw)[0], track_sequences(seqs, chain_len=16, reidentify=False, **kw)[0]
        assert len(a) == len(b) and all(_state(x) == _state(y) for x, y in zip(a, b))
        assert not any(hasattr(t, "reid_parts") for t in b)
    tm = {}
    c = track_sequences(seqs, chain_len=16, relink=True, reidentify=True, timings=tm)[0]
    assert "reidentify" in tm and all(hasattr(t, "reid_parts") and t.reid_lengths.shape == (10,) for t in c)


E2E_SEED = 20280851
E2E_HIDDEN = [(0, 60, 60), (1, 130, 40)]      # (person, first frame, frames): hidden in every view


def test_end_to_end_through_the_real_tracker():
    """One scene walk, 4 views x 3 people, 240 frames; person 0 is hidden in every view for 60 frames and person 1 for 40.  Through
    track_sequences(relink=True), then re-identified: the device's links equal the restatement's on the same records; no link joins
    two people, none has an unlabelled end; the share of each hidden person's tracked frames that lie in their longest record rises."""
    from multiview_motion_capture_amd import synth
    from multiview_motion_capture_amd.relinking import reidentify_sequences
    from multiview_motion_capture_amd.sequences import track_sequences
    g = rc.hide_people(synth.generate(240, 4, 3, E2E_SEED, walk="scene"), E2E_HIDDEN)
    tl = track_sequences([(g["kps25"], g["counts"], _calibs(g))], chain_len=16, relink=True)[0]
    links = []
    out = reidentify_sequences([tl], links=links)[0]
    recs = rp.records_of(tl)
    res = _equal_to_restatement(links[0], recs, rc.defaults(), "tracked records")
    gt = g["gt_joints"]
    lab = [(r[1], label_poses(r[1], r[2], gt)) for r in recs]
    o = res["order"]
    n_links = 0
    for a, b in enumerate(res["succ"]):
        if b >= 0:
            pa, pb = int(lab[o[a]][1][-1]), int(lab[o[b]][1][0])
            print(f"link {recs[o[a]][0]} (person {pa}, to frame {recs[o[a]][1][-1]}) -> {recs[o[b]][0]} (person {pb}, from frame "
                  f"{recs[o[b]][1][0]}), z = {res['cost'][a]:.3f}")
            assert pa >= 0 and pb >= 0 and pa == pb
            n_links += 1
    before = identity_shares(lab, 3)
    after = identity_shares([(np.asarray(t.frame_idxs), label_poses(t.frame_idxs, np.array([p[2].keypoints for p in t.poses]), gt))
                             for t in out], 3)
    print("records", [(r[0], int(r[1][0]), int(r[1][-1])) for r in recs], "links", n_links, "shares before", before, "after", after)
    assert [n for n, _ in before] == [n for n, _ in after]
    for person, _, _ in E2E_HIDDEN:
        assert after[person][1] > before[person][1], (person, before, after)
    assert all(a[1] >= b[1] for a, b in zip(after, before))


def test_shelf_coverage_does_not_fall(tmp_path, shelf_inputs):
    """run_main_batched(relink=True) beside relink=True, reidentify=True on the 300 Shelf frames, both against run_main's tracklets of
    >= 100 frames (tests/test_gpu_relink.py's measure): the best identity's coverage of none of them may fall.  What the cue gains on
    Shelf's one-frame cuts is printed, not gated."""
    from multiview_motion_capture_amd.motion_capture import run_main, run_main_batched
    from test_gpu_relink import _coverage, _shelf_pickles
    pose_dir = _shelf_pickles(tmp_path, shelf_inputs)
    linked = run_main_batched([pose_dir], [tmp_path / "a"], n_test=300, relink=True)[0]
    people = run_main_batched([pose_dir], [tmp_path / "b"], n_test=300, relink=True, reidentify=True)[0]
    long_ref = [t for t in run_main(None, pose_dir, tmp_path / "ref", n_test=300) if len(t) >= 100]
    rl, rp_ = [_coverage(t, linked) for t in long_ref], [_coverage(t, people) for t in long_ref]
    print("\nshelf, run_main's long tracklets", [len(t) for t in long_ref])
    print("best coverage, re-linked:     ", [round(r[0], 3) for r in rl], "records", len(linked))
    print("best coverage, re-identified: ", [round(r[0], 3) for r in rp_], "records", len(people))
    for t in people:
        if len(t.reid_parts) > 1:
            print("identity", t.track_id, "parts", t.reid_parts, "z", [round(c, 3) for c in t.reid_costs])
    assert len(long_ref) == 4
    for (a, _, ua), (b, _, ub) in zip(rl, rp_):
        assert b >= a and ub == ua, (rl, rp_)
