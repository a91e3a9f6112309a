"""CPU: lens distortion at the door of the pipeline (multiview_motion_capture_amd/lens.py, include/mvmc.h: mvmc_lens_undistort /
mvmc_lens_distort) -- what can be checked without a GPU: the oracle's own round trips (tests/lens_np.py, which the GPU tests compare the
kernels with), the Lens / lens_table / load_calib host side, that a Calib without a lens is yesterday's Calib, the guards that refuse a
calibration with a lens wherever pixels are read as pinhole pixels, and the entry points' argument errors."""
import ctypes
import dataclasses
import json
import pickle

import numpy as np
import pytest

import lens_np as ln
from lens_cases import recorded_case, round_trip_case, sensor_sample

W, H = ln.IMG_WH
BROWN_SETS = {"mild5": ln.MILD5, "wide5": ln.WIDE5, "rational8": ln.RATIONAL8}


@pytest.mark.parametrize("name", sorted(BROWN_SETS))
def test_oracle_round_trip_brown(name):
    f, k = BROWN_SETS[name]
    r = ln.row(ln.BROWN, f, k)
    uv = sensor_sample(r, 20000, 20261018)
    raw, det = ln.distort_points(r, uv)
    print(f"{name}: min Jacobian determinant {det.min():.3f}")
    assert det.min() > 0.1          # so the accept rule has nothing to reject on this sample
    back, ok, it = ln.undistort_points(r, raw)
    err = np.abs(back - uv).max()
    print(f"{name}: max {it.max()} Newton steps, max error {err:.2e} px")
    assert ok.all()
    assert it.max() <= 6
    assert err <= 1e-9


def test_oracle_round_trip_fisheye():
    f, k = ln.FISHEYE4
    r = ln.row(ln.FISHEYE, f, k)
    rng = np.random.default_rng(7)
    th, phi = rng.uniform(0, np.deg2rad(80.0), 20000), rng.uniform(0, 2 * np.pi, 20000)
    th[0] = 0.0                                      # the limit r -> 0
    x, y = np.tan(th) * np.cos(phi), np.tan(th) * np.sin(phi)
    xd, yd, dthd = ln.distort_normalised(r, x, y)
    assert dthd.min() > 0.1
    xb, yb, ok, it = ln.undistort_normalised(r, xd, yd)
    rel = (np.hypot(xb - x, yb - y) / np.maximum(np.hypot(x, y), 1.0)).max()
    print(f"fisheye: max {it.max()} Newton steps, max relative error {rel:.2e}")
    assert ok.all() and it.max() <= 6 and rel <= 1e-12
    assert xb[0] == 0.0 and yb[0] == 0.0


def test_the_gpu_tests_inputs_are_inside_the_oracles_domain():
    """The kernel tests' round-trip case and the recorded sequences: the oracle inverts its own forward model on every scored triple
    (recorded_case asserts determinant > 0.1 and no drop itself)."""
    case = round_trip_case(3, 3, 2, 25)
    back, dropped = ln.undistort_keypoints(case["raw"], case["table"], case["rig"])
    assert not dropped.any() and np.abs(back - case["truth"]).max() <= 1e-9
    assert 0.05 < case["zero"].mean() < 0.15
    for i in range(3):
        rec = recorded_case(i)
        assert np.abs(rec["raw"][..., :2] - rec["kps"][..., :2]).max() > 20.0       # (the lenses do move the keypoints: pixels)


def test_oracle_rejects_the_drop_cases():
    """The points of the GPU drop test: far outside a Brown model's injective range, and fisheye angles past the cap."""
    pts = np.array([[3.0, 3.0], [-4.0, 2.0], [5.0, -5.0]])
    for f, k in (ln.MILD5, ln.WIDE5):
        assert not ln.undistort_normalised(ln.row(ln.BROWN, f, k), pts[:, 0], pts[:, 1])[2].any()
    thd = np.array([2.5, 2.2, 2.404])
    assert not ln.undistort_normalised(ln.row(ln.FISHEYE, *ln.FISHEYE4), thd * 0.6, thd * 0.8)[2].any()


def test_lens_from_opencv():
    from multiview_motion_capture_amd.lens import BROWN, FISHEYE, Lens
    assert Lens.from_opencv([1, 2, 3, 4]) == Lens(BROWN, (1, 2, 3, 4, 0, 0, 0, 0)) == Lens.brown(1, 2, 3, 4)
    assert Lens.from_opencv(np.array([[1, 2, 3, 4, 5.0]])) == Lens.brown(1, 2, 3, 4, 5)
    assert Lens.from_opencv(range(1, 9)).k == (1, 2, 3, 4, 5, 6, 7, 8)
    assert Lens.from_opencv([1, 2, 3, 4], fisheye=True) == Lens.fisheye(1, 2, 3, 4) == Lens(FISHEYE, (1, 2, 3, 4, 0, 0, 0, 0))
    for bad in ([1, 2, 3], [1] * 6, [1] * 12, [1] * 14):
        with pytest.raises(ValueError, match="4, 5 or 8"):
            Lens.from_opencv(bad)
    with pytest.raises(ValueError, match="fisheye model has 4"):
        Lens.from_opencv([1, 2, 3, 4, 5], fisheye=True)
    with pytest.raises(ValueError):
        Lens(7, (0,) * 8)
    with pytest.raises(ValueError):
        Lens.brown(np.nan, 0, 0, 0)


def _calibs(lenses, skew=0.0):
    from multiview_motion_capture_amd.common import Calib
    out = []
    for c, lens in enumerate(lenses):
        K = np.array([[1000.0 + c, skew, 960.0 - c], [0, 1010.0 + c, 540.0 + c], [0, 0, 1]])
        Rt = np.concatenate([np.eye(3), np.array([[0.1 * c], [0.0], [3.0]])], 1)
        out.append(Calib.from_k_rt(K, Rt, (W, H), lens=lens))
    return out


def test_lens_table_packing():
    from multiview_motion_capture_amd.lens import Lens, lens_table, pinhole
    rig0 = _calibs([Lens.brown(*ln.WIDE5[1]), None, Lens.fisheye(*ln.FISHEYE4[1])], skew=1.5)
    rig1 = _calibs([None, Lens.brown(*ln.RATIONAL8[1]), None])
    t = lens_table([rig0, rig1])
    assert t.shape == (2, 3, 16) and t.dtype == np.float64
    assert np.array_equal(t[0, 0], [1, 1000, 1010, 960, 540, 1.5, -0.28, 0.09, 1e-3, -5e-4, -0.012, 0, 0, 0, 0, 0])
    assert np.array_equal(t[0, 1], [0, 1001, 1011, 959, 541, 1.5] + [0] * 10)
    assert np.array_equal(t[0, 2], [2, 1002, 1012, 958, 542, 1.5, -0.02, 0.005, -0.001, 0.0002] + [0] * 6)
    assert np.array_equal(t[1, 1, 6:14], ln.RATIONAL8[1]) and t[1, 1, 0] == 1 and t[1, 1, 5] == 0
    assert np.array_equal(t[:, :, 14:], np.zeros((2, 3, 2)))
    assert np.array_equal(lens_table([pinhole(rig0)])[0, :, 0], [0, 0, 0])
    assert all(c.lens is None for c in pinhole(rig0)) and rig0[0].lens is not None
    with pytest.raises(ValueError, match="same number of cameras"):
        lens_table([rig0, rig1[:2]])


def test_load_calib_with_and_without_a_lens(tmp_path):
    from multiview_motion_capture_amd.lens import Lens
    from multiview_motion_capture_amd.motion_capture import load_calib
    K = [[1000.0, 0, 960], [0, 1000, 540], [0, 0, 1]]
    RT = np.concatenate([np.eye(3), [[0.0], [0.0], [2.0]]], 1).tolist()
    base = {"K": K, "RT": RT, "imgSize": [W, H]}

    def js(name, **extra):
        p = tmp_path / name
        p.write_text(json.dumps(dict(base, **extra)))
        return load_calib(p)

    plain = js("a.json")
    assert plain.lens is None and plain.img_wh_size == (W, H) and np.array_equal(plain.P, np.array(K) @ np.array(RT))
    assert js("b.json", lensModel="fisheye").lens is None          # a model without coefficients says nothing
    assert js("c.json", distCoef=list(ln.WIDE5[1])).lens == Lens.brown(*ln.WIDE5[1])
    assert js("d.json", distCoef=list(ln.RATIONAL8[1]), lensModel="brown").lens == Lens.brown(*ln.RATIONAL8[1])
    assert js("e.json", distCoef=list(ln.FISHEYE4[1]), lensModel="fisheye").lens == Lens.fisheye(*ln.FISHEYE4[1])
    with pytest.raises(ValueError, match="lensModel"):
        js("f.json", distCoef=[0, 0, 0, 0], lensModel="division")
    for name, extra, want in (("g.pkl", {}, None), ("h.pkl", {"dist": np.array(ln.MILD5[1])}, Lens.brown(*ln.MILD5[1]))):
        with open(tmp_path / name, "wb") as fh:
            pickle.dump(dict({"K": np.array(K), "R": np.eye(3), "t": np.array([0.0, 0, 2])}, **extra), fh)
        cal = load_calib(tmp_path / name)
        assert cal.lens == want and cal.img_wh_size == (1920, 1080) and np.array_equal(cal.Rt, np.array(RT))


def test_a_calib_without_a_lens_is_yesterdays_calib():
    from multiview_motion_capture_amd.common import Calib
    K, Rt = np.diag([1000.0, 1000.0, 1.0]), np.concatenate([np.eye(3), np.ones((3, 1))], 1)
    assert [f.name for f in dataclasses.fields(Calib)] == ["K", "Rt", "P", "Kr_inv", "img_wh_size", "lens"]
    a = Calib.from_k_rt(K, Rt, (10, 20))
    b = Calib(a.K, a.Rt, a.P, a.Kr_inv, a.img_wh_size)          # the five positional fields of every existing caller
    assert a.lens is None and b.lens is None
    same = lambda u, v: all(np.array_equal(getattr(u, f.name), getattr(v, f.name)) for f in dataclasses.fields(Calib))
    assert same(a, b)
    assert np.array_equal(a.P, K @ Rt) and a.img_wh_size == (10, 20)
    # a pickle written before the field existed carries no "lens" in its state
    old = Calib.__new__(Calib)
    old.__dict__.update({k: v for k, v in a.__dict__.items() if k != "lens"})
    back = pickle.loads(pickle.dumps(old))
    assert "lens" not in back.__dict__ and back.lens is None and same(back, a)


def test_require_pinhole_guards_every_door():
    from multiview_motion_capture_amd import body_fit, rig_refine, smoothing
    from multiview_motion_capture_amd.lens import Lens, pinhole, require_pinhole
    from multiview_motion_capture_amd.live import check_open
    from multiview_motion_capture_amd.live_smoothing import LiveSmoother
    from multiview_motion_capture_amd.sequences import check_sequences
    lensed = _calibs([None, Lens.brown(*ln.MILD5[1]), None])
    plain = pinhole(lensed)
    kps, counts = np.zeros((4, 3, 2, 25, 3)), np.zeros((4, 3), np.int32)
    msg = r"undistort first: lens\.undistort_sequences / LensBank"
    require_pinhole(plain, "x")
    with pytest.raises(ValueError, match="x: camera 1 .*" + msg):
        require_pinhole(lensed, "x")
    assert check_sequences([(kps, counts, plain)]) == [(4, 3, 2)]
    with pytest.raises(ValueError, match="track_sequences: sequence 1: camera 1 .*" + msg):
        check_sequences([(kps, counts, plain), (kps, counts, lensed)])
    check_open(0, 4, 3, 3, plain)
    with pytest.raises(ValueError, match="LivePool.open_session: camera 1 .*" + msg):
        check_open(0, 4, 3, 3, lensed)
    with pytest.raises(ValueError, match="fit_sequences: .*" + msg):
        body_fit._check([(kps, counts, lensed)], [[]], 3, 10, 20)
    with pytest.raises(ValueError, match="smooth_sequences: .*" + msg):
        smoothing._check([(kps, counts, lensed)], [[]])
    with pytest.raises(ValueError, match="refine_rigs: .*" + msg):
        rig_refine.check_refine([(kps, counts, lensed)], [[]], 10, 20.0, 0.1, 2, 0, 1)
    sm = LiveSmoother(3, 2)
    with pytest.raises(ValueError, match="LiveSmoother.open_session: camera 1 .*" + msg):
        sm.open_session(lensed)
    assert sm.open_session(plain) == 0


def test_track_sequences_refuses_a_lens_before_any_device_work():
    from multiview_motion_capture_amd.lens import Lens
    from multiview_motion_capture_amd.sequences import track_sequences
    lensed = _calibs([Lens.fisheye(*ln.FISHEYE4[1]), None, None])
    with pytest.raises(ValueError, match="track_sequences: sequence 0: camera 0 .*undistort first"):
        track_sequences([(np.zeros((4, 3, 2, 25, 3)), np.zeros((4, 3), np.int32), lensed)])


def test_argument_errors_come_before_any_hip_call():
    from multiview_motion_capture_amd import _cabi
    lib = _cabi.load()
    fake = ctypes.c_void_p(0x1000)
    for fn in (lib.mvmc_lens_undistort, lib.mvmc_lens_distort):
        assert fn(None, 0, 1, 1, 1, None, None, 1, None, None, None) == 1
        assert fn(None, 1, 4, 5, 25, fake, None, 1, fake, fake, None) == 1      # NULL input
        assert fn(fake, 1, 4, 5, 25, None, None, 1, fake, fake, None) == 1      # NULL table
        assert fn(fake, 1, 4, 5, 25, fake, None, 1, None, fake, None) == 1      # NULL output
        assert fn(fake, 1, 4, 5, 25, fake, None, 1, fake, None, None) == 1      # NULL dropped
        assert fn(fake, 2, 4, 5, 25, fake, None, 1, fake, fake, None) == 1      # dtype
        assert fn(fake, 1, -1, 5, 25, fake, None, 1, fake, fake, None) == 1
        assert fn(fake, 1, 4, 0, 25, fake, None, 1, fake, fake, None) == 1
        assert fn(fake, 1, 4, 5, 0, fake, None, 1, fake, fake, None) == 1
        assert fn(fake, 1, 4, 5, 25, fake, None, 0, fake, fake, None) == 1      # no rig
        assert fn(fake, 1, 0, 5, 25, fake, None, 1, fake, fake, None) == 0      # no frames: nothing to do, nothing launched
    assert (_cabi.LENS_DOUBLES, _cabi.LENS_PINHOLE, _cabi.LENS_BROWN, _cabi.LENS_FISHEYE, _cabi.LENS_MAX_ITER) == (16, 0, 1, 2, 12)
    header = open(_cabi.__file__.replace("multiview_motion_capture_amd/_cabi.py", "include/mvmc.h")).read()
    for name, val in (("MVMC_LENS_DOUBLES", "16"), ("MVMC_LENS_MAX_ITER", "12"), ("MVMC_LENS_FISHEYE_MAX_THETA", "1.5"),
                      ("MVMC_LENS_PINHOLE", "0"), ("MVMC_LENS_BROWN", "1"), ("MVMC_LENS_FISHEYE", "2")):
        assert f"#define {name} {val}\n" in header
    assert (ln.MAX_ITER, ln.FISHEYE_MAX_THETA) == (_cabi.LENS_MAX_ITER, _cabi.LENS_FISHEYE_MAX_THETA)
