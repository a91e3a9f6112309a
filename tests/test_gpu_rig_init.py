"""Rig calibration on the device (multiview_motion_capture_amd/rig_init.py, csrc/mvmc_riginit.hip) against its NumPy restatement
(tests/rig_init_np.py) and against synthetic ground truth.  The small cases (tests/rig_init_cases.py: SMALL) share ONE launch --
sequences of 1, 24, 40 and 65 frames and 2, 3 and 4 cameras, views with counts 0 and 2, frames without a common joint -- and
tests/test_rig_init_cpu.py proves on the restatement alone that every decision of theirs is clear of its threshold."""
import functools

import numpy as np
import pytest

import rig_init_cases as rc
import rig_init_np as ri
import rig_refine_np as rr
from test_rig_init_cpu import BASELINE_GATE, PAIR_GATE_DEG, RIG_GATE, _distances, floor_checks, floor_premise

pytestmark = pytest.mark.gpu

SMALL = sorted(rc.SMALL)


def _row(w):
    return (w["kps25"], w["counts"], [(w["K"][c], (1032, 776)) for c in range(w["K"].shape[0])])


def _rt(r):
    return np.array([c.Rt for c in r.calibs])


@functools.lru_cache(maxsize=None)
def _small_launch():
    """The SMALL cases calibrated in one call -> (results, detail): computed once, read-only."""
    from multiview_motion_capture_amd.rig_init import calibrate_rigs
    detail = []
    out = calibrate_rigs([_row(rc.case(n)[0]) for n in SMALL], detail=detail, **rc.case(SMALL[0])[1])
    return out, detail


def _pairs(name):
    """(device's dict, restatement's (moments, consensus, refit)) of every pair of a small case."""
    _, det = rc.reference(name)
    dev = _small_launch()[1][SMALL.index(name)]
    for p in dev["pairs"]:
        a, b = p["a"], p["b"]
        yield p, det["mos"][a, b], det["conss"][a, b], det["fits"][a, b]


@pytest.mark.parametrize("name", SMALL)
def test_pair_moments(name):
    """mvmc_pair_moments: the normalisation and every frame's moment matrix within 1e-12 relative (of the pair's largest entry: sums
    of <= 17 products), the counts and the compacted list of usable frames equal."""
    w, _ = rc.case(name)
    xn = ri.observations(w["k17"], w["counts"], w["K"], 0.1)[0]
    dev = _small_launch()[1][SMALL.index(name)]
    assert np.array_equal(np.isnan(dev["xn"]), np.isnan(xn)) and np.allclose(dev["xn"], xn, rtol=1e-13, atol=1e-15, equal_nan=True)
    n = 0
    for p, mo, _, _ in _pairs(name):
        n += 1
        assert p["norm"][6] == mo["n_corr"]
        assert np.allclose(p["norm"][:6], mo["norm"], rtol=1e-12, atol=1e-15)
        assert np.abs(p["mom"] - mo["mom"]).max() <= 1e-12 * max(np.abs(mo["mom"]).max(), 1.0)
        assert np.array_equal(p["cnt"], mo["cnt"])
        nu = mo["usable"].shape[0]
        assert p["n_usable"] == nu and np.array_equal(p["usable"][:nu], mo["usable"]) and np.all(p["usable"][nu:] == -1)
    assert n == w["K"].shape[0] * (w["K"].shape[0] - 1) // 2


@pytest.mark.parametrize("name", SMALL)
def test_pair_consensus(name):
    """mvmc_pair_consensus with H = 32, m = 6: the inlier counts equal; E up to sign within 1e-9 (|E|_F = 1) where the eigen-gap
    condition (l1 - l0) / l8 >= 1e-8 holds."""
    for p, mo, cons, _ in _pairs(name):
        assert np.array_equal(p["count"], cons["count"]), (p["a"], p["b"])
        for h in np.flatnonzero(cons["gap"] >= 1e-8):
            e = min(np.abs(p["E"][h] - cons["E"][h]).max(), np.abs(p["E"][h] + cons["E"][h]).max())
            assert e <= 1e-9, (p["a"], p["b"], h, e)


@pytest.mark.parametrize("name", SMALL)
def test_pair_refit(name):
    """mvmc_pair_refit: the same winner, per-round counts and chosen round; the same (R, t) within 1e-9; the same inlier mask; the
    triangulated points within 1e-9 (of the pair's baseline = 1)."""
    for p, mo, cons, fit in _pairs(name):
        pose = p["pose"]
        if fit["n_inl"] == 0:
            assert not pose.any() and not p["mask"].any() and np.isnan(p["pts"]).all()
            continue
        k = len(fit["round_count"])
        assert int(pose[21]) == fit["hyp"] and list(p["rounds"][:k]) == fit["round_count"] and np.all(p["rounds"][k:] == -1)
        assert int(pose[22]) == fit["round"] and int(pose[23]) == fit["n_inl"]
        assert np.abs(pose[:9].reshape(3, 3) - fit["R"]).max() <= 1e-9 and np.abs(pose[9:12] - fit["t"]).max() <= 1e-9
        assert sorted(pose[24:28].astype(int)) == sorted(fit["votes"])
        assert np.array_equal(p["mask"].astype(bool), fit["mask"])
        assert np.array_equal(np.isnan(p["pts"]), np.isnan(fit["pts"]))
        assert np.nanmax(np.abs(p["pts"] - fit["pts"])) <= 1e-9


def _against_restatement(r, ref):
    assert r.stop == ref["stop"] and [tuple(e) for e in r.tree] == [tuple(e) for e in ref["tree"]]
    assert np.array_equal(r.pair_inliers, ref["pair_inliers"])
    if ref["Rt"] is None:
        assert r.calibs is None
        return
    got = _rt(r)
    assert np.abs(rr.centres(got) - rr.centres(ref["Rt"])).max() <= 1e-6
    assert max(rr.rot_angle(got[c, :, :3] @ ref["Rt"][c, :, :3].T) for c in range(got.shape[0])) <= 1e-6
    assert r.scale_source == ref["scale_source"] and r.polish.stop == ref["polish"]["stop"]
    assert abs(r.rms_px - ref["rms_px"]) <= 1e-6 * ref["rms_px"]


@pytest.mark.parametrize("name", SMALL)
def test_whole_calls_against_the_restatement(name):
    """The same stop and tree; camera centres within 1e-6 m and rotations within 1e-6 rad (the polish's existing gates); the
    ``disconnected`` (a view that detects nobody) and ``few_frames`` (one frame) returns carry no calibration."""
    r = _small_launch()[0][SMALL.index(name)]
    _against_restatement(r, rc.reference(name)[0])
    assert r.stop == {"c3_f40_drop": "disconnected", "c2_f1": "few_frames"}.get(name, "ok")


@pytest.mark.parametrize("name", ["clean_11", "dirty_11"])
def test_ground_truth(name):
    """One 5 x 120 walk, clean and contaminated: the device equals the restatement, and meets the gates of tests/test_rig_init_cpu.py
    (2 x what the restatement measures) against ground truth: every pair's rotation and baseline direction, the rig's centres and
    rotations after the polish.
    Measured on one MI355X: clean pairs 0.161 / 0.072 degrees, rig 0.7 mm / 0.017 degrees, rms 2.33 px; contaminated pairs 0.691 /
    0.733 degrees, rig 8.1 mm / 0.245 degrees, rms 14.2 px."""
    from multiview_motion_capture_amd.rig_init import calibrate_rig
    w, _ = rc.case(name)
    det = []
    r = calibrate_rig(*_row(w), detail=det)
    _against_restatement(r, rc.reference(name)[0])
    kind = name.split("_")[0]
    e = np.degrees([ri.pair_errors(p["pose"][:9].reshape(3, 3), p["pose"][9:12], w["Rt"], p["a"], p["b"]) for p in det[0]["pairs"]])
    ce, re = rr.rig_errors(_rt(r), w["Rt"])
    print(f"\n{name}: worst pair rotation {e[:, 0].max():.3f} deg, direction {e[:, 1].max():.3f} deg; rig centre {ce.max():.4f} m, "
          f"rotation {np.degrees(re.max()):.3f} deg; rms {r.rms_px:.2f} px")
    assert e[:, 0].max() <= PAIR_GATE_DEG[kind][0] and e[:, 1].max() <= PAIR_GATE_DEG[kind][1]
    assert ce.max() <= RIG_GATE[kind][0] and np.degrees(re.max()) <= RIG_GATE[kind][1]


def test_argument_checks():
    """Input errors raise ValueError before any device work; a Calib with a lens model is refused."""
    from multiview_motion_capture_amd import lens
    from multiview_motion_capture_amd.common import Calib
    from multiview_motion_capture_amd.rig_init import calibrate_rigs
    w, _ = rc.case("c2_f24")
    row = _row(w)
    for kw in (dict(hypotheses=0), dict(sample_frames=0), dict(sample_frames=33), dict(refit_rounds=9), dict(polish_iter=25),
               dict(inlier_px=0.0), dict(world="up"), dict(baseline=(0, 0, 1.0)), dict(baseline=(0, 2, 1.0)), dict(baseline=(0, 1, -1.0)),
               dict(min_pair_inliers=3)):
        with pytest.raises(ValueError):
            calibrate_rigs([row], **kw)
    with pytest.raises(ValueError):
        calibrate_rigs([])
    with pytest.raises(ValueError):
        calibrate_rigs([(row[0], row[1][:, :1], row[2])])
    with pytest.raises(ValueError):
        calibrate_rigs([(row[0], row[1], row[2][:1])])
    with pytest.raises(ValueError):
        calibrate_rigs([(row[0][:, :1], row[1][:, :1], row[2][:1])])           # one camera
    cal = [Calib.from_k_rt(w["K"][c], np.eye(3, 4), (1032, 776), lens=lens.Lens.brown(-0.1, 0.01, 0.0, 0.0) if c else None) for c in range(2)]
    with pytest.raises(ValueError, match="lens"):
        calibrate_rigs([(row[0], row[1], cal)])


def _bits(r):
    return (None if r.calibs is None else _rt(r).tobytes(), r.stop, tuple(r.tree), r.pair_inliers.tobytes(),
            None if r.points is None else r.points.tobytes())


def test_batching_is_bit_identical():
    """A sequence calibrated alone, among three others of other frame and camera counts, and twice in a row: identical bits."""
    from multiview_motion_capture_amd.rig_init import calibrate_rigs
    kw = rc.case(SMALL[0])[1]
    batch, _ = _small_launch()
    again = calibrate_rigs([_row(rc.case(n)[0]) for n in SMALL], **kw)
    for i, n in enumerate(SMALL):
        alone = calibrate_rigs([_row(rc.case(n)[0])], **kw)[0]
        assert _bits(alone) == _bits(batch[i]) == _bits(again[i]), n
    assert sum(b.stop == "ok" for b in batch) >= 3


def test_floor_world_on_the_device():
    """world="floor" with a known baseline on the upright walker: true up within 3 degrees of +z, ankles at z = 0, camera 0 above the
    origin, and centre distances metric to the CPU file's gate.  Measured on one MI355X: 1.576 degrees, 7.71e-4 (the restatement's)."""
    from multiview_motion_capture_amd.rig_init import calibrate_rig
    w, _ = rc.case("upright_57")
    assert floor_premise(w) < 2.0
    c_true = rr.centres(w["Rt"])
    r = calibrate_rig(*_row(w), baseline=(0, 1, float(np.linalg.norm(c_true[0] - c_true[1]))), world="floor")
    assert r.stop == "ok" and r.scale_source == "baseline"
    ang = floor_checks(_rt(r), r.points, w["Rt"])
    err = np.abs(_distances(rr.centres(_rt(r))) / _distances(c_true) - 1.0).max()
    print(f"\nfloor: true up {ang:.3f} deg from +z; worst relative distance error {err:.2e}")
    assert ang <= 3.0 and err <= BASELINE_GATE["upright_57"]


def _mpjpe(recs, g, sim):
    err = []
    for t in recs:
        fr = np.array(t.frame_idxs)
        J = sim[0] * np.array([q[2].keypoints for q in t.poses]) @ sim[1].T + sim[2]
        err.append(np.linalg.norm(J[:, None] - g["gt_joints"][fr], axis=-1).mean(-1).min(axis=1))
    return float(np.concatenate(err).mean())


def test_downstream_tracking_on_the_calibrated_rig():
    """A 5 x 4 scene of 64 frames tracked on the rig calibrated from a SEPARATE one-person walk on the same cameras (world="floor",
    baseline from ground truth): after the similarity that aligns the centres, the MPJPE is within 1.25 x that of the records
    tracked on the true rig -- the ratio of refine_rigs' downstream gate.  Measured on one MI355X: 8.70 mm against 8.66 mm."""
    from multiview_motion_capture_amd import synth
    from multiview_motion_capture_amd.common import Calib
    from multiview_motion_capture_amd.rig_init import calibrate_rig
    from multiview_motion_capture_amd.sequences import track_sequences
    seed = 57
    w, _ = rc.case("upright_57")
    g = synth.generate(64, 5, 4, seed, walk="scene", segment=3)         # (later frames of the scene than the walk was cut from)
    assert np.array_equal(g["Rt"], w["Rt"])
    c_true = rr.centres(w["Rt"])
    r = calibrate_rig(*_row(w), baseline=(0, 1, float(np.linalg.norm(c_true[0] - c_true[1]))), world="floor")
    assert r.stop == "ok"
    true = [Calib.from_k_rt(w["K"][c], w["Rt"][c], (1032, 776)) for c in range(5)]
    recs, recs_true = track_sequences([(g["kps25"], g["counts"], r.calibs), (g["kps25"], g["counts"], true)], chain_len=16)
    m_cal = _mpjpe(recs, g, rr.similarity(rr.centres(_rt(r)), c_true))
    m_true = _mpjpe(recs_true, g, (1.0, np.eye(3), np.zeros(3)))
    print(f"\nMPJPE mm: calibrated rig {1e3 * m_cal:.2f}, true rig {1e3 * m_true:.2f}")
    assert m_cal <= 1.25 * m_true
