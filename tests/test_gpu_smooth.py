"""GPU: the trajectory smoother (multiview_motion_capture_amd/smoothing.py, csrc/mvmc_smooth.hip) against its NumPy restatement
(tests/smooth_np.py) on Shelf and on synthetic scene walks with holes, bit-identity (run to run, alone against in a batch, several
launches against one), ground truth on synthetic scene walks, and Shelf through the public path into BVH."""
import numpy as np
import pytest

import oracle_np as o
import smooth_np as sm
from conftest import load_golden
from test_gpu_body_fit import _calibs, _np_records, _oracle_records, _raw_slot_maps

pytestmark = pytest.mark.gpu


def _weights():
    from multiview_motion_capture_amd import smoothing as S
    return (S.ROOT_VEL, S.ROOT_ACC, S.ANG_VEL, S.ANG_ACC)


def _compare(got, exp, what):
    worst = dict(params=0.0, cost=0.0, joints=0.0)
    for t, e in zip(got, exp):
        assert t.frame_idxs == e["frames"].tolist(), (what, t.track_id)
        assert np.array_equal(t.smooth_filled, e["filled"])
        assert np.array_equal(t.smooth_views, e["views"]), (what, t.track_id)
        # the same selected pose per (record frame, camera); none on the filled frames
        assert np.array_equal(t.smooth_select[~t.smooth_filled], e["sel"]), (what, t.track_id)
        assert np.all(t.smooth_select[t.smooth_filled] == -1)
        assert t.smooth_trials == e["trace"], (what, t.track_id, t.smooth_trials, e["trace"])
        P = np.array([np.concatenate([q[1].root, np.ravel(q[1].euler_angles), q[1].bone_lens]) for q in t.poses])
        J = np.array([q[2].keypoints for q in t.poses])
        worst["params"] = max(worst["params"], float(np.abs(P - e["params"]).max()))
        worst["joints"] = max(worst["joints"], float(np.abs(J - e["joints"]).max()))
        worst["cost"] = max([worst["cost"]] + [abs(a - b) / max(abs(b), 1e-300) for a, b in zip(t.smooth_cost, e["cost"])])
    print(f"\n{what}: worst differences from the restatement", worst)
    assert worst["params"] <= 1e-9 and worst["cost"] <= 1e-9 and worst["joints"] <= 1e-8
    assert len(got) == len(exp)


def test_device_equals_the_restatement_on_shelf():
    from multiview_motion_capture_amd.body_fit import fit_tracklets
    from multiview_motion_capture_amd.smoothing import smooth_tracklets
    si, fx = load_golden("shelf_inputs.npz"), load_golden("shelf_clean_oracle_tracker.npz")
    N = 80
    kps, cnt = si["kps25"][:N + 1], si["counts"][:N + 1].astype(np.int32)
    cal = _calibs(si["K"], si["Rt"])
    fitted = fit_tracklets(_oracle_records(fx, N), kps, cnt, cal)
    got = smooth_tracklets(fitted, kps, cnt, cal)
    exp = sm.smooth([sm.bf.ingest_np(kps, cnt)], [si["P"]], [_np_records(fitted)], _weights())[0]
    for t in got:
        print(f"identity {t.track_id}: {len(t)} frames, E {np.array2string(t.smooth_cost, precision=3)}, trials {t.smooth_trials}")
    _compare(got, exp, "Shelf")


def _synth(seeds=(31, 32, 33), rigs=((5, 4), (4, 3), (5, 2)), n_frames=60, occlusion=0.3):
    from multiview_motion_capture_amd import synth
    seqs, gts = [], []
    for seed, (C, P) in zip(seeds, rigs):
        g = synth.generate(n_frames, C, P, seed, walk="scene", occlusion=occlusion)
        seqs.append((g["kps25"], g["counts"], _calibs(g["K"], g["Rt"])))
        gts.append(g)
    return seqs, gts


def _cut(recs, rng, lo=10, hi=20):
    """Copies of the records with one hole of lo..hi frames cut out of every other long record."""
    out = []
    for k, t in enumerate(recs):
        if k % 2 == 0 and len(t) > hi + 10:
            n = int(rng.integers(lo, hi + 1))
            a = int(rng.integers(3, len(t) - n - 3))
            keep = [i for i in range(len(t)) if not a <= i < a + n]
            u = type(t).__new__(type(t))
            u.__dict__.update(t.__dict__)
            u.frame_idxs = [t.frame_idxs[i] for i in keep]
            u.poses = [t.poses[i] for i in keep]
            out.append(u)
        else:
            out.append(t)
    return out


def _synth_records(seqs, seed=5):
    from multiview_motion_capture_amd.body_fit import fit_sequences
    from multiview_motion_capture_amd.sequences import track_sequences
    fitted = fit_sequences(seqs, track_sequences(seqs, chain_len=16))
    rng = np.random.default_rng(seed)
    return [_cut(r, rng) for r in fitted]


def test_device_equals_the_restatement_on_synthetic_rigs_with_holes():
    from multiview_motion_capture_amd.smoothing import smooth_sequences
    seqs, gts = _synth()
    recs = _synth_records(seqs)
    got = smooth_sequences(seqs, recs)
    assert sum(int(t.smooth_filled.sum()) for r in got for t in r) >= 20
    for s, (g, r) in enumerate(zip(gts, recs)):
        exp = sm.smooth([sm.bf.ingest_np(g["kps25"], g["counts"])], [g["P"]], [_np_records(r)], _weights())[0]
        _compare(got[s], exp, f"sequence {s}")


def _same(a, b):
    assert len(a) == len(b)
    for t, u in zip(a, b):
        assert t.track_id == u.track_id and t.frame_idxs == u.frame_idxs and t.smooth_trials == u.smooth_trials
        assert np.array_equal(t.smooth_cost, u.smooth_cost) and np.array_equal(t.smooth_views, u.smooth_views)
        for p, q in zip(t.poses, u.poses):
            assert np.array_equal(p[1].root, q[1].root) and np.array_equal(p[1].euler_angles, q[1].euler_angles)
            assert np.array_equal(p[2].keypoints, q[2].keypoints)


def test_bit_identity_run_to_run_alone_and_across_launches():
    from multiview_motion_capture_amd.smoothing import smooth_sequences
    seqs, _ = _synth(seeds=(41, 42, 43), n_frames=90)
    recs = _synth_records(seqs, seed=6)
    batch = smooth_sequences(seqs, recs)
    again = smooth_sequences(seqs, recs)
    split = smooth_sequences(seqs, recs, max_work_bytes=200 * 46 * 1024)
    for s in range(3):
        _same(batch[s], again[s])
        _same(batch[s], split[s])
        _same(batch[s], smooth_sequences([seqs[s]], [recs[s]])[0])
    assert sum(len(r) for r in batch) >= 6


def _person(t, g, maps, fit_select):
    votes = []
    for k, f in enumerate(t.frame_idxs):
        for c in range(fit_select.shape[1]):
            sl = int(fit_select[k, c])
            if sl >= 0:
                votes.append(int(g["gt_order"][f, c, maps[f, c][sl]]))
    votes = [v for v in votes if v >= 0]
    return int(np.bincount(votes).argmax()) if votes else -1


def test_ground_truth_of_synthetic_scene_walks():
    """MPJPE against the generator's joints, default weights, 2 px noise, occlusion 0.3, 10-20-frame holes, on scenes held out from the
    weight sweep (tools/smooth_weight_sweep.py tunes on seeds 51, 52 and hole stream 7; this test uses seeds 61, 62 and hole stream 8).
    Measured on one MI355X: filled frames 52.1 mm smoothed against 89.4 mm holding the previous frame (ratio 0.58, where a
    Brownian-bridge estimate gave about 0.58), frames with data 7.65 mm against 8.90 mm fitted (0.86), jitter 43.8 against
    53.9 mm/frame^2 (0.81).  Gates: the tighter of the issue's bound and 1.25 x the observed ratio: 0.73, 1.0 and below 1."""
    from multiview_motion_capture_amd.body_fit import fit_sequences
    from multiview_motion_capture_amd.sequences import track_sequences
    from multiview_motion_capture_amd.smoothing import smooth_sequences
    seqs, gts = _synth(seeds=(61, 62), rigs=((5, 4), (5, 4)), n_frames=300)
    fitted = fit_sequences(seqs, track_sequences(seqs, chain_len=16))
    rng = np.random.default_rng(8)
    cut = [_cut(r, rng) for r in fitted]
    out = smooth_sequences(seqs, cut)
    e_fill_s, e_fill_h, e_data_s, e_data_f, jit_s, jit_f = [], [], [], [], [], []
    for s, g in enumerate(gts):
        maps = _raw_slot_maps(g)
        for t_fit, t_cut, t in zip(fitted[s], cut[s], out[s]):
            if len(t_fit) < 60:
                continue
            person = _person(t_fit, g, maps, t_fit.fit_select)
            if person < 0:
                continue
            fr = np.array(t.frame_idxs)
            J = np.array([q[2].keypoints for q in t.poses])
            gt = g["gt_joints"][fr, person]
            err = np.linalg.norm(J - gt, axis=-1).mean(-1)
            # holding the previous frame (bvh_text's rule) on the filled frames
            kf = np.array(t_cut.frame_idxs)
            Jc = np.array([q[2].keypoints for q in t_cut.poses])
            src = np.searchsorted(kf, fr, side="right") - 1
            err_hold = np.linalg.norm(Jc[src] - gt, axis=-1).mean(-1)
            fl = t.smooth_filled
            data = ~fl & (t.smooth_views > 0)
            if fl.any():
                e_fill_s.append(err[fl])
                e_fill_h.append(err_hold[fl])
            e_data_s.append(err[data])
            e_data_f.append(err_hold[data])
            # jitter: the mean second difference of the joints over runs of frames present in both
            ok = ~fl
            seg = ok[2:] & ok[1:-1] & ok[:-2]
            jit_s.append(np.linalg.norm(J[2:] - 2 * J[1:-1] + J[:-2], axis=-1).mean(-1)[seg])
            jit_f.append(np.linalg.norm(Jc[src][2:] - 2 * Jc[src][1:-1] + Jc[src][:-2], axis=-1).mean(-1)[seg])
    m = {k: float(np.mean(np.concatenate(v))) for k, v in dict(fill_smooth=e_fill_s, fill_hold=e_fill_h, data_smooth=e_data_s,
                                                                  data_fitted=e_data_f, jitter_smooth=jit_s, jitter_fitted=jit_f).items()}
    print("\nground truth (m):", m, "ratios: filled", m["fill_smooth"] / m["fill_hold"], "data", m["data_smooth"] / m["data_fitted"],
          "jitter", m["jitter_smooth"] / m["jitter_fitted"])
    assert len(e_fill_s) >= 3
    assert m["fill_smooth"] <= 0.73 * m["fill_hold"]
    assert m["data_smooth"] <= m["data_fitted"]
    assert m["jitter_smooth"] < m["jitter_fitted"]


def test_shelf_through_the_public_path_into_bvh():
    from multiview_motion_capture_amd.body_fit import fit_sequences
    from multiview_motion_capture_amd.bvh_export import bvh_text
    from multiview_motion_capture_amd.sequences import track_sequences
    from multiview_motion_capture_amd.smoothing import smooth_sequences
    si = load_golden("shelf_inputs.npz")
    cal = _calibs(si["K"], si["Rt"])
    kps, cnt = si["kps25"], si["counts"].astype(np.int32)
    seqs = [(kps, cnt, cal)]
    recs = track_sequences([(kps[1:], cnt[1:], cal)], chain_len=16, frame_idx0=1)
    fitted = fit_sequences(seqs, recs)
    out = smooth_sequences(seqs, fitted)[0]
    from multiview_motion_capture_amd.pose_def import KpsFormat, get_kps_order
    all_names = [kk.name for kk in get_kps_order(KpsFormat.BASIC_18)]
    assert [t.track_id for t in out] == [t.track_id for t in fitted[0]]
    for t, f in zip(out, fitted[0]):
        c = t.smooth_cost
        assert c[2] + c[3] <= c[0] + c[1], (t.track_id, c)
        assert t.frame_idxs == list(range(f.frame_idxs[0], f.frame_idxs[-1] + 1))
        text = bvh_text(t)
        lines = text.splitlines()
        k = lines.index("MOTION")
        assert int(lines[k + 1].split()[1]) == f.frame_idxs[-1] - f.frame_idxs[0] + 1
        rows = np.array([[float(v) for v in ln.split()] for ln in lines[k + 3:]])
        # every column: the root translation, then each joint's Euler angles in degrees, in the hierarchy's joint order
        names = [ln.split()[1] for ln in lines[:k] if ln.strip().split()[0] in ("ROOT", "JOINT")]
        order = [all_names.index(nm) for nm in names]
        exp = np.array([np.concatenate([q[1].root, np.degrees(np.asarray(q[1].euler_angles).reshape(18, 3)[order].ravel())])
                        for q in t.poses])
        assert rows.shape == exp.shape and np.abs(rows - exp).max() <= 1e-8, (t.track_id, np.abs(rows - exp).max())
        if len(f) >= 50:
            J0 = np.array([q[2].keypoints for q in f.poses])
            J1 = np.array([q[2].keypoints for q in t.poses])[~t.smooth_filled]
            j0 = np.linalg.norm(J0[2:] - 2 * J0[1:-1] + J0[:-2], axis=-1).mean()
            j1 = np.linalg.norm(J1[2:] - 2 * J1[1:-1] + J1[:-2], axis=-1).mean()
            # per-view reprojection RMS (px, score-weighted, the 32 residuals of every selected view), before and after
            n_res = 32 * int(t.smooth_views.sum())
            rms0, rms1 = np.sqrt(2 * c[0] / n_res), np.sqrt(2 * c[2] / n_res)
            print(f"\nidentity {t.track_id}: {len(t)} frames ({int(t.smooth_filled.sum())} filled), jitter {1e3 * j0:.2f} -> "
                  f"{1e3 * j1:.2f} mm/frame^2, reprojection RMS {rms0:.2f} -> {rms1:.2f} px, E_data {c[0]:.1f} -> {c[2]:.1f}, "
                  f"E_prior {c[1]:.1f} -> {c[3]:.1f}, trials {t.smooth_trials}")
