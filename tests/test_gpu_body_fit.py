"""GPU: the body fit (multiview_motion_capture_amd/body_fit.py, csrc/mvmc_bodyfit.hip) against its NumPy restatement
(tests/body_fit_np.py) on Shelf, run to run and batch to batch bit-identity, ground truth on synthetic scene walks, Shelf through the
public path, and the edge cases."""
import numpy as np
import pytest
import torch

import body_fit_np as bf
import oracle_np as o
from conftest import load_golden

pytestmark = pytest.mark.gpu


def _calibs(K, Rt):
    from multiview_motion_capture_amd.common import Calib
    return [Calib.from_k_rt(K[c], Rt[c]) for c in range(K.shape[0])]


def _oracle_records(fx, n):
    """MvTracklet records of the noise-free oracle tracker's first n Shelf frames (frame k of the tables is Shelf frame k + 1)."""
    from multiview_motion_capture_amd.sequences import tables_to_tracklets
    ids = int(fx["meta"][:n, :, 0].max()) + 1
    recs = tables_to_tracklets(fx["meta"][:n], fx["n_tracks"][:n], fx["params"][:n], fx["joints"][:n], np.arange(ids)[None], n, n, 1)
    return sorted(recs, key=lambda t: t.track_id)


def _np_records(recs):
    out = []
    for t in recs:
        p = np.array([np.concatenate([q[1].root, np.ravel(q[1].euler_angles), q[1].bone_lens]) for q in t.poses])
        out.append(dict(frames=np.array(t.frame_idxs), params=p, joints=np.array([q[2].keypoints for q in t.poses])))
    return out


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


def test_device_equals_the_oracle_on_shelf():
    """Gates per identity: the selected poses exactly, the same accept / reject sequence in every length step, lengths within 1e-9 m
    and E within 1e-9 (relative) after every step, joints within 1e-8 m."""
    from multiview_motion_capture_amd.body_fit import fit_tracklets
    si, fx = load_golden("shelf_inputs.npz"), load_golden("shelf_clean_oracle_tracker.npz")
    N = 80
    recs = _oracle_records(fx, N)
    kps, cnt = si["kps25"][:N + 1], si["counts"][:N + 1].astype(np.int32)
    got = fit_tracklets(recs, kps, cnt, _calibs(si["K"], si["Rt"]))
    exp = bf.fit([bf.ingest_np(kps, cnt)], [si["P"]], [_np_records(recs)])[0]
    worst = dict(lens=0.0, cost=0.0, joints=0.0)
    for t, e in zip(got, exp):
        assert np.array_equal(t.fit_select, e["sel"]), t.track_id
        assert np.array_equal(t.fit_views, e["views"])
        assert t.fit_trials == e["traces"], (t.track_id, t.fit_trials, e["traces"])
        worst["lens"] = max(worst["lens"], float(np.abs(t.bone_lens - e["lens"]).max()))
        worst["cost"] = max([worst["cost"]] + [_rel(a, b) for a, b in zip(t.fit_cost, e["cost"])])
        J = np.array([q[2].keypoints for q in t.poses])
        worst["joints"] = max(worst["joints"], float(np.abs(J - e["joints"]).max()))
        print(f"\nidentity {t.track_id}: {len(t)} frames, views {np.bincount(t.fit_views)}, E {np.array2string(t.fit_cost, precision=3)}, "
              f"trials {t.fit_trials}")
    print("worst differences from the oracle:", worst)
    assert worst["lens"] <= 1e-9 and worst["cost"] <= 1e-9 and worst["joints"] <= 1e-8


def _synth_sequences(seeds, n_frames=300, n_people=4, n_views=5):
    from multiview_motion_capture_amd import synth
    seqs, gts = [], []
    for s in seeds:
        g = synth.generate(n_frames, n_views, n_people, s, walk="scene")
        seqs.append((g["kps25"], g["counts"], _calibs(g["K"], g["Rt"])))
        gts.append(g)
    return seqs, gts


def _same(a, b):
    for t, u in zip(a, b):
        assert t.track_id == u.track_id and t.frame_idxs == u.frame_idxs
        assert np.array_equal(t.bone_lens, u.bone_lens) and np.array_equal(t.fit_cost, u.fit_cost)
        assert np.array_equal(t.fit_select, u.fit_select) and np.array_equal(t.fit_views, u.fit_views)
        for p, q in zip(t.poses, u.poses):
            assert np.array_equal(p[1].root, q[1].root) and np.array_equal(p[1].euler_angles, q[1].euler_angles)
            assert np.array_equal(p[2].keypoints, q[2].keypoints)
    assert len(a) == len(b)


def test_runs_are_bit_identical_and_a_sequence_fits_the_same_alone_and_in_a_batch():
    from multiview_motion_capture_amd import synth
    from multiview_motion_capture_amd.body_fit import fit_sequences
    from multiview_motion_capture_amd.sequences import track_sequences
    seqs = []
    for seed, (C, P) in zip((11, 12, 13), ((5, 4), (4, 3), (5, 2))):
        g = synth.generate(90, C, P, seed, walk="scene")
        seqs.append((g["kps25"], g["counts"], _calibs(g["K"], g["Rt"])))
    recs = track_sequences(seqs, chain_len=16)
    batch = fit_sequences(seqs, recs)
    again = fit_sequences(seqs, recs)
    for a, b in zip(batch, again):
        _same(a, b)
    for s in range(3):
        _same(fit_sequences([seqs[s]], [recs[s]])[0], batch[s])
    assert sum(len(r) for r in batch) >= 6


def _raw_slot_maps(g):
    """ingest order -> raw slot, per (frame, camera) of a synthetic sequence"""
    F, C = g["counts"].shape
    out = {}
    for f in range(F):
        for c in range(C):
            good = [p for p in range(int(g["counts"][f, c])) if o.pose_is_good(o.openpose25_to_coco17(g["kps25"][f, c, p].astype(np.float64)))]
            out[f, c] = good
    return out


# Every slot but 7 within 1 cm of the truth, except the two the guessed mid-spine observation biases: the mid-spine row
# (inverse_kinematics.py:339-348, the mean of the shoulders and hips in the image) stands for the Spine joint, so the spine (slot 8)
# and neck (slot 9) lengths carry the guess's error.  Measured on these sequences (the device equals the oracle to 1e-10 m, so these
# are the algorithm's own errors): slot 8 up to 11.9 mm (the per-frame median l0: 10.5 mm), slot 9 up to 8.4 mm (l0: 8.2 mm); every
# other slot below 1 mm.  Slots 8 and 9 are gated at 15 mm.
SLOT_BOUND = {s: (0.015 if s in (8, 9) else 0.01) for s in range(11) if s != 7}
GUESSED = (7, 8, 9)


def test_ground_truth_lengths_of_synthetic_scene_walks():
    from multiview_motion_capture_amd.body_fit import fit_sequences
    from multiview_motion_capture_amd.sequences import track_sequences
    seeds = (21, 22)
    seqs, gts = _synth_sequences(seeds)
    recs = track_sequences(seqs, chain_len=16)
    fitted = fit_sequences(seqs, recs)
    _, side = o.skeleton_constants()
    n_checked, err_fit_all, err_med_all = 0, [], []
    for s, (seed, g) in enumerate(zip(seeds, gts)):
        true = side * np.random.default_rng([seed, 4]).uniform(0.9, 1.1, size=(4, 1)) * np.ones((4, 11))
        maps = _raw_slot_maps(g)
        for t, r in zip(fitted[s], recs[s]):
            if int((t.fit_views > 0).sum()) < 100:
                continue
            votes = []
            for k, f in enumerate(t.frame_idxs):
                for c in range(t.fit_select.shape[1]):
                    sl = int(t.fit_select[k, c])
                    if sl >= 0:
                        votes.append(int(g["gt_order"][f, c, maps[f, c][sl]]))
            votes = [v for v in votes if v >= 0]
            person = int(np.bincount(votes).argmax())
            l_med = np.median(np.array([q[1].bone_lens for q in r.poses])[t.fit_views >= 2], axis=0)
            e_fit = np.abs(t.bone_lens - true[person])
            e_med = np.abs(l_med - true[person])
            print(f"\nseq {s} identity {t.track_id} -> person {person}, {len(t)} frames: |l - true| (mm) fitted "
                  f"{np.array2string(1e3 * e_fit, precision=2)}, per-frame median {np.array2string(1e3 * e_med, precision=2)}")
            mask = ~np.isin(np.arange(11), GUESSED)
            err_fit_all.append(e_fit[mask].mean())
            err_med_all.append(e_med[mask].mean())
            for sl, b in SLOT_BOUND.items():
                assert e_fit[sl] <= b, (s, t.track_id, sl, e_fit[sl])
            n_checked += 1
    assert n_checked >= 6
    print("mean error over the measured slots (all but 7, 8, 9): fitted", np.mean(err_fit_all), "per-frame median l0", np.mean(err_med_all))
    # Measured: fitted 0.29 mm, per-frame median 0.24 mm.  On these 2 px-noise sequences the per-frame lengths' median is already
    # sub-millimetre and the shared fit is NOT more accurate on the measured slots; its gain is one consistent body per identity.  Gated
    # at "no worse than the median by more than 0.1 mm" instead of "below the median".
    assert np.mean(err_fit_all) <= np.mean(err_med_all) + 1e-4


def _spread(recs):
    rows = []
    for t in recs:
        L = np.array([q[1].bone_lens for q in t.poses])
        med = np.median(L, axis=0)
        sp = (np.percentile(L, 95, axis=0) - np.percentile(L, 5, axis=0)) / np.maximum(np.abs(med), 1e-12)
        rows.append((t.track_id, len(t), np.delete(sp, 7)))
    return rows


def test_shelf_through_the_public_path():
    from multiview_motion_capture_amd import motion_capture as mc
    from multiview_motion_capture_amd.body_fit import fit_tracklets
    from multiview_motion_capture_amd.sequences import track_sequences
    from test_gpu_update_4d import _shelf_frames
    si = load_golden("shelf_inputs.npz")
    cal = _calibs(si["K"], si["Rt"])
    kps, cnt = si["kps25"], si["counts"].astype(np.int32)
    recs_ts = track_sequences([(kps[1:], cnt[1:], cal)], chain_len=16, frame_idx0=1)[0]
    trk = mc.MvTracker()
    for fi in range(1, 301):
        trk.update_4d(fi, _shelf_frames(si, cal, fi), None)
    recs_u4 = [t for t in trk.tracklets + trk.dead_tracklets if len(t) >= 1]
    for name, recs in (("track_sequences", recs_ts), ("update_4d", recs_u4)):
        out = fit_tracklets(recs, kps, cnt, cal)
        assert [t.track_id for t in out] == [t.track_id for t in recs]
        before = {tid: sp for tid, _, sp in _spread(recs)}
        print(f"\n{name}: {len(out)} identities")
        for t in out:
            L = np.array([q[1].bone_lens for q in t.poses])
            assert np.all(L == t.bone_lens)
            # (E after a length step is summed from the linear form root + A l, after a pose step by the IK's FK: the two agree to
            # rounding, so a pose step that accepts nothing may report E a few ulps above the length step's)
            c = t.fit_cost
            assert c[-1] <= c[0] * (1 + 1e-12), (t.track_id, c)
            assert np.all(np.diff(c) <= 1e-12 * max(c[0], 1e-300)), (t.track_id, c)
            if len(t) >= 50:
                print(f"  identity {t.track_id}: {len(t)} frames, p5-p95 spread before {100 * before[t.track_id].min():.1f}-"
                      f"{100 * before[t.track_id].max():.1f} %, after 0; E {c[0]:.1f} -> {c[-1]:.1f}; l = {np.round(t.bone_lens, 3)}")
            J = np.array([q[2].keypoints for q in t.poses])
            assert np.isfinite(J).all()
    # the inputs are left as they were
    assert all(not hasattr(t, "fit_cost") for t in recs_ts)


def test_empty_lists_sequences_without_records_and_all_frozen_records():
    from multiview_motion_capture_amd.body_fit import fit_sequences
    from multiview_motion_capture_amd.inverse_kinematics import PoseShapeParam
    from multiview_motion_capture_amd.motion_capture import MvTracklet
    from multiview_motion_capture_amd.pose_def import KpsFormat, Pose
    si = load_golden("shelf_inputs.npz")
    cal = _calibs(si["K"], si["Rt"])
    kps, cnt = si["kps25"][:10], si["counts"][:10].astype(np.int32)
    assert fit_sequences([(kps, cnt, cal)], [[]]) == [[]]
    assert fit_sequences([(kps, cnt, cal), (kps, cnt, cal)], [[], []]) == [[], []]
    # a record far from every pose: every frame frozen; no launch with zero identities
    _, ref = o.skeleton_constants()
    x = np.concatenate([[50.0, 50.0, 1.0], np.zeros(54), ref])
    J = o.forward_kinematics(x[:3], x[3:57], x[57:])[0]
    t = MvTracklet(7, 2, PoseShapeParam(x[:3], x[3:57].reshape(18, 3), x[57:].copy()), Pose(KpsFormat.BASIC_18, J, np.ones((18, 1)), None))
    t.frame_idxs = [2, 3]
    t.poses = t.poses + [(3, t.poses[0][1], t.poses[0][2])]
    out = fit_sequences([(kps, cnt, cal), (kps, cnt, cal)], [[], [t]])
    assert out[0] == [] and len(out[1]) == 1
    r = out[1][0]
    assert r.track_id == 7 and r.frame_idxs == [2, 3] and np.array_equal(r.fit_views, [0, 0])
    assert np.array_equal(r.bone_lens, ref) and np.all(r.fit_cost == 0)
    assert np.abs(np.array([q[2].keypoints for q in r.poses]) - J).max() < 1e-12
