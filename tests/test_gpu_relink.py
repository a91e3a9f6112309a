"""GPU: the re-linking step (multiview_motion_capture_amd/relinking.py, csrc/mvmc_relink.hip) against its NumPy restatement
(tests/relink_np.py) link for link, on ground truth through the real tracker, on Shelf against run_main, and through fit, smoothing
and BVH export."""
import pickle

import numpy as np
import pytest

import relink_np as rn
from conftest import load_golden
from relink_cases import CUT_CASES, PARAMS, cut_case, fragments, make_tracklets, shelf_oracle_records

pytestmark = pytest.mark.gpu

SCENE_SEEDS = (20270701, 20270702, 20270703, 20270704)     # 6(c) / 7: four scene walks, 5 x 4, 300 frames, occlusion 0.3, a rig each


def _calibs(K, Rt):
    from multiview_motion_capture_amd.common import Calib
    return [Calib.from_k_rt(K[c], Rt[c]) for c in range(K.shape[0])]


def _device_links(tracklets_per_sequence):
    from multiview_motion_capture_amd.relinking import relink_sequences
    links = []
    out = relink_sequences(tracklets_per_sequence, links=links, **PARAMS)
    return out, links


def _same_bits(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("order", "succ", "head", "pos", "cost"))


def _compare(link, recs, what):
    """Device = restatement: the same nodes, succ, head and position; costs to 1e-12 m.  Returns (links, worst cost difference)."""
    res = rn.relink(recs, **PARAMS)
    assert np.array_equal(link["order"], res["order"]), what
    assert np.array_equal(link["succ"], res["succ"]), (what, link["succ"], res["succ"])
    assert np.array_equal(link["head"], res["head"]) and np.array_equal(link["pos"], res["pos"]), what
    diff = float(np.abs(link["cost"] - res["cost"]).max()) if len(recs) else 0.0
    assert diff <= 1e-12, (what, diff)
    return int((res["succ"] >= 0).sum()), diff


def _check_all(tracklets_per_sequence, recs_per_sequence, what):
    """One call for all sequences against the restatement, and every sequence alone gives the bits it gives among the others."""
    _, links = _device_links(tracklets_per_sequence)
    for s, (ln, recs) in enumerate(zip(links, recs_per_sequence)):
        n, diff = _compare(ln, recs, f"{what} {s}")
        print(f"{what} {s}: {len(recs)} records, {n} links, worst cost difference {diff:.1e} m")
    for s in range(len(tracklets_per_sequence)):
        assert _same_bits(_device_links([tracklets_per_sequence[s]])[1][0], links[s]), (what, s)
    return links


def test_device_equals_the_restatement_on_cut_ground_truth_and_shelf_records():
    recs = [cut_case(C, P, seed)[1] for C, P, seed in CUT_CASES] + [shelf_oracle_records()]
    links = _check_all([make_tracklets(r) for r in recs], recs, "cut ground truth / shelf oracle records")
    assert int((links[-1]["succ"] >= 0).sum()) == 3


def _shelf_records():
    from multiview_motion_capture_amd.sequences import track_sequences
    si = load_golden("shelf_inputs.npz")
    kps, cnt = si["kps25"], si["counts"].astype(np.int32)
    return track_sequences([(kps[1:], cnt[1:], _calibs(si["K"], si["Rt"]))], chain_len=16, frame_idx0=1)[0]


def test_device_equals_the_restatement_on_tracked_shelf():
    tl = _shelf_records()
    _check_all([tl], [rn.records_of(tl)], "track_sequences on Shelf")


def _scene_sequences():
    from multiview_motion_capture_amd import synth
    from multiview_motion_capture_amd.sequences import track_sequences
    gts = [synth.generate(300, 5, 4, s, walk="scene", occlusion=0.3) for s in SCENE_SEEDS]
    seqs = [(g["kps25"], g["counts"], _calibs(g["K"], g["Rt"])) for g in gts]
    return gts, seqs, track_sequences(seqs, chain_len=16)


def test_device_equals_the_restatement_on_tracked_scene_walks():
    _, _, recs = _scene_sequences()
    _check_all(recs, [rn.records_of(tl) for tl in recs], "track_sequences on a scene walk")


def test_device_equals_the_restatement_beyond_the_lds_matrix():
    """One sequence of more than 256 records (8 people over 3,000 frames, 40 cuts each): the cost matrix lives in the workspace."""
    from multiview_motion_capture_amd import synth
    gt = synth.generate(3000, 8, 8, 20270505, walk="scene")["gt_joints"]
    pieces = fragments(gt, 20270505, 40, 16, 0.01)
    recs = [(i, f, j) for i, (_, f, j) in enumerate(pieces)]
    assert len(recs) > 256
    small = cut_case(5, 4, 20270501)[1]
    links = _check_all([make_tracklets(small), make_tracklets(recs)], [small, recs], "a short and a long sequence")
    people = [p for p, _, _ in pieces]
    o = links[1]["order"]
    assert all(people[o[a]] == people[o[b]] for a, b in enumerate(links[1]["succ"]) if b >= 0)


def _labelled(tracklets, gt, frame_idx0=0):
    from relink_cases import label_poses
    return [(np.asarray(t.frame_idxs), label_poses(t.frame_idxs, np.array([p[2].keypoints for p in t.poses]), gt, frame_idx0))
            for t in tracklets]


def test_ground_truth_through_the_real_tracker():
    """Four scene walks (5 cameras, 4 people, 300 frames, occlusion 0.3, a rig each) through track_sequences, then re-linked.  A record
    end is labelled with the ground-truth person nearest to its pose when within 0.2 m.  There must be something to do (more records
    of >= 10 poses than people in at least three sequences), at most one link in ten may have an unlabelled end, NO link may join two
    different people, and per person the share of the tracked frames that lie in the person's longest record must not fall, and must
    rise for at least one person in every sequence that had fragments.
    Measured on one MI355X (records of >= 10 poses before -> after, links, share of the longest record per person before -> after):
      sequence 0: 39 ->  9, 36 links, [0.364, 0.265, 0.270, 0.108] -> [1.000, 1.000, 0.589, 0.518]
      sequence 1: 31 -> 11, 23 links, [0.411, 0.170, 0.273, 0.327] -> [0.589, 0.594, 0.436, 0.523]
      sequence 2: 38 -> 10, 29 links, [0.163, 0.268, 0.161, 0.218] -> [0.307, 1.000, 0.786, 1.000]
      sequence 3: 59 -> 17, 45 links, [0.112, 0.233, 0.110, 0.166] -> [0.536, 0.767, 0.422, 0.487]
    no link with an unlabelled end, none between two people."""
    from relink_cases import identity_shares
    gts, _, recs = _scene_sequences()
    out, links = _device_links(recs)
    n_links = n_unlabelled = 0
    fragmented = []
    for s, (g, tl, new, ln) in enumerate(zip(gts, recs, out, links)):
        gt = g["gt_joints"]
        lab = _labelled(tl, gt)
        fragmented.append(sum(len(t) >= 10 for t in tl) > gt.shape[1])
        o = ln["order"]
        for a, b in enumerate(ln["succ"]):
            if b < 0:
                continue
            pa, pb = int(lab[o[a]][1][-1]), int(lab[o[b]][1][0])
            n_links += 1
            n_unlabelled += pa < 0 or pb < 0
            assert pa < 0 or pb < 0 or pa == pb, (s, tl[o[a]].track_id, tl[o[b]].track_id, pa, pb, float(ln["cost"][a]))
        before = identity_shares(lab, gt.shape[1])
        after = identity_shares(_labelled(new, gt), gt.shape[1])
        sb = [round(l / max(n, 1), 3) for n, l in before]
        sa = [round(l / max(n, 1), 3) for n, l in after]
        print(f"\nsequence {s}: records of >= 10 poses {sum(len(t) >= 10 for t in tl)} -> {sum(len(t) >= 10 for t in new)}, "
              f"links {int((ln['succ'] >= 0).sum())}, share of the longest record per person {sb} -> {sa}")
        assert [n for n, _ in before] == [n for n, _ in after]                     # re-linking moves no pose
        assert all(a >= b for (_, a), (_, b) in zip(after, before)), (s, before, after)
        if fragmented[-1]:
            assert any(a > b for (_, a), (_, b) in zip(after, before)), (s, before, after)
    assert sum(fragmented) >= 3, fragmented
    assert n_links > 0 and 10 * n_unlabelled <= n_links, (n_links, n_unlabelled)


def _shelf_pickles(tmp_path, g):
    from multiview_motion_capture_amd.common import Calib
    from multiview_motion_capture_amd.motion_capture import frame_data_from_batch
    calibs = [Calib.from_k_rt(g["K"][c], g["Rt"][c]) for c in range(g["K"].shape[0])]
    pose_dir = tmp_path / "poses"
    pose_dir.mkdir()
    for f in range(g["kps25"].shape[0]):
        with open(pose_dir / f"{f}.pkl", "wb") as fh:
            pickle.dump(frame_data_from_batch(f, g["kps25"][f], g["counts"][f], calibs), fh)
    return pose_dir


def _on(t, b):
    """Frames of record b that lie (mean joint distance < 0.2 m) on record t, and the distances over the frames they share."""
    rj = {f: p[2].keypoints for f, p in zip(t.frame_idxs, t.poses)}
    fr = [f for f in b.frame_idxs if f in rj]
    dist = np.array([np.linalg.norm(p[2].keypoints - rj[f], axis=-1).mean() for f, p in zip(b.frame_idxs, b.poses) if f in rj])
    return {f for f, d in zip(fr, dist) if d < 0.2}, dist


def _coverage(t, tl):
    """test_shelf_through_run_main_batched's measure: (coverage of t's frames by the identity of tl that lies on it in the most frames,
    that identity's mean joint distance, coverage by all identities together)."""
    best, near = (0, 0.0, np.inf), set()
    for b in tl:
        on, dist = _on(t, b)
        near |= on
        if dist.size and len(on) > best[0]:
            best = (len(on), len(on) / len(t), float(dist.mean()))
    return best[1], best[2], len(near) / len(t)


SHELF_COVERAGE_AFTER = (1.0, 0.67, 0.891, 0.714)     # measured (the docstring below); each is gated at its value minus 0.05


def test_shelf_against_run_main(tmp_path, shelf_inputs):
    """run_main_batched(relink=True) beside relink=False on the 300 Shelf frames, both against run_main (update_4d frame by frame):
    for each of run_main's tracklets of >= 100 frames the best batched identity's coverage must not fall, its mean joint distance stays
    <= 2 cm and the coverage by all identities together is unchanged; summed over the tracklets the best coverage must rise; and the two
    fragments of every link taken, where both lie (>= 10 frames within 0.2 m) on a long run_main tracklet, lie on the same one.
    Measured on one MI355X for run_main's four tracklets of >= 100 frames (300, 300, 156, 105 frames): best coverage 1.0, 0.32, 0.891,
    0.714 batched -> 1.0, 0.67, 0.891, 0.714 re-linked (mean joint distance 1.2, 1.4, 8.4, 4.9 mm; all identities together 1.0, 0.99,
    0.987, 0.981 either way); 8 links, the second person's identity 7 = fragments 7 (frames 98 - 192) + 25 (194 - 224) + 31 (226 -
    300) at costs 0.025 and 0.040 m.  Each coverage is also gated at its measured value minus 0.05: one 16-frame chain of a 300-frame
    tracklet, the grain at which these numbers move when one chain head falls differently."""
    from multiview_motion_capture_amd.motion_capture import run_main, run_main_batched
    pose_dir = _shelf_pickles(tmp_path, shelf_inputs)
    before = run_main_batched([pose_dir], [tmp_path / "a"], n_test=300)[0]
    after = run_main_batched([pose_dir], [tmp_path / "b"], n_test=300, relink=True)[0]
    assert pickle.loads(open(tmp_path / "b" / "tracklets.pkl", "rb").read())["tracklets"][0].relink_parts == after[0].relink_parts
    ref = run_main(None, pose_dir, tmp_path / "ref", n_test=300)
    long_ref = [t for t in ref if len(t) >= 100]
    assert long_ref
    rb, ra = [_coverage(t, before) for t in long_ref], [_coverage(t, after) for t in long_ref]
    print("\nshelf, run_main's long tracklets", [len(t) for t in long_ref])
    print("best coverage / mean joint distance / union, batched:   ", [tuple(round(x, 4) for x in r) for r in rb])
    print("best coverage / mean joint distance / union, re-linked: ", [tuple(round(x, 4) for x in r) for r in ra])
    by_id = {t.track_id: t for t in before}
    n_links = 0
    for t in after:
        print("identity", t.track_id, len(t), "poses, parts", t.relink_parts, "costs", [round(c, 4) for c in t.relink_costs])
        for pa, pb in zip(t.relink_parts[:-1], t.relink_parts[1:]):
            n_links += 1
            homes = []
            for part in (pa, pb):
                on = [len(_on(r, by_id[part[0]])[0]) for r in long_ref]
                homes.append(int(np.argmax(on)) if max(on) >= 10 else -1)
            assert homes[0] < 0 or homes[1] < 0 or homes[0] == homes[1], (pa, pb, homes)
    assert n_links > 0
    for (cb, _, ub), (ca, da, ua) in zip(rb, ra):
        assert ca >= cb and da <= 0.02 and ua == ub, (rb, ra)
    assert sum(r[0] for r in ra) > sum(r[0] for r in rb), (rb, ra)
    assert len(ra) == len(SHELF_COVERAGE_AFTER)
    for (ca, _, _), m in zip(ra, SHELF_COVERAGE_AFTER):
        assert ca >= m - 0.05, (ra, SHELF_COVERAGE_AFTER)


def test_it_composes_into_fit_smoothing_and_bvh(tmp_path):
    """relink -> fit_sequences -> smooth_sequences(fill_gaps=True) -> save_bvh on the Shelf records: a joined identity's smoothed
    record has every frame from its first to its last, and the frames of the hole between two fragments are flagged smooth_filled."""
    from multiview_motion_capture_amd.body_fit import fit_sequences
    from multiview_motion_capture_amd.bvh_export import save_bvh
    from multiview_motion_capture_amd.relinking import relink_tracklets
    from multiview_motion_capture_amd.smoothing import smooth_sequences
    si = load_golden("shelf_inputs.npz")
    seqs = [(si["kps25"], si["counts"].astype(np.int32), _calibs(si["K"], si["Rt"]))]
    linked = relink_tracklets(_shelf_records())
    joined = [t for t in linked if len(t.relink_parts) > 1]
    assert joined
    fitted = fit_sequences(seqs, [linked])
    smooth = smooth_sequences(seqs, fitted, fill_gaps=True)[0]
    assert [t.track_id for t in smooth] == [t.track_id for t in linked]
    for t, src in zip(smooth, linked):
        assert t.frame_idxs == list(range(src.frame_idxs[0], src.frame_idxs[-1] + 1))
        filled = dict(zip(t.frame_idxs, t.smooth_filled))
        assert [f for f in t.frame_idxs if filled[f]] == sorted(set(t.frame_idxs) - set(src.frame_idxs))
        for (_, _, last), (_, first, _) in zip(src.relink_parts[:-1], src.relink_parts[1:]):
            assert all(filled[f] for f in range(last + 1, first))
        save_bvh(str(tmp_path / f"{t.track_id}.bvh"), t)
        lines = open(tmp_path / f"{t.track_id}.bvh").read().splitlines()
        assert int(lines[lines.index("MOTION") + 1].split()[1]) == len(t.frame_idxs)
