"""CPU: the NumPy restatement of the smoother's per-frame covariance (tests/smooth_cov_np.py) -- the banded backward recursion against
the dense inverse, D_K of all 18 joints against central differences of the FK, the effective degrees of freedom --, and the argument
checks of smoothing.smooth_sequences(covariance=, noise_px=), which run before any device call."""
import functools

import numpy as np
import pytest

import smooth_cov_np as sc
import smooth_np as sm
from conftest import load_golden

W = (1e4, 1e4, 1e4, 1e4)
CASES = [(2, None), (3, None), (4, None), (5, None), (6, None), (11, None), (6, 3), (11, 5)]


@functools.lru_cache(maxsize=None)
def _shelf():
    """The noise-free oracle tracker's records of the first 12 Shelf frames (both people on every one) and the ingested views."""
    from test_gpu_body_fit import _np_records, _oracle_records
    si, fx = load_golden("shelf_inputs.npz"), load_golden("shelf_clean_oracle_tracker.npz")
    recs = _np_records(_oracle_records(fx, 12))
    assert len(recs) >= 2 and all(len(r["frames"]) >= 11 for r in recs)
    return recs, sm.bf.ingest_np(si["kps25"][:13], si["counts"][:13].astype(np.int32)), si["P"]


@functools.lru_cache(maxsize=None)
def _case(n, drop):
    """Per Shelf identity (x (m,68) after two LM trials, obs, prs) of its first n record frames without frame ``drop``."""
    recs, views, P = _shelf()
    keep = [i for i in range(n) if i != drop]
    cut = [dict(frames=r["frames"][keep], params=r["params"][keep], joints=r["joints"][keep]) for r in recs]
    out = []
    for rec, (obs, prs) in zip(cut, sc.problems(views, P, cut)):
        x0, filled = sm.init_traj(rec["frames"], rec["params"])
        assert int(filled.sum()) == (drop is not None)
        x, _ = sm.lm(x0, obs, prs, W, max_iter=2)
        out.append((x, obs, prs))
    return out


@pytest.mark.parametrize("n,drop", CASES)
def test_banded_recursion_equals_the_dense_inverse(n, drop):
    """max|Sigma_tt(banded) - Sigma_tt(dense)| / max|Sigma_tt| per identity, measured (both Shelf identities give the same figure: it
    is set by the two knee-twist angles' block, which sees the prior and the damping alone): 2 rows 9.1e-9, 3 rows 6.4e-9, 4 rows
    7.3e-9, 5 rows 3.0e-9, 6 rows 4.7e-9, 11 rows 1.0e-9, (6, drop 3) 4.7e-9, (11, drop 5) 1.0e-9; the worst is 9.1e-9.  It is the
    yardstick of the device gate (tests/test_gpu_smooth_cov.py: TOL = 10 x 9.1e-9 = 9.1e-8), which may never be looser than 1e-6: the
    bound here is therefore 1e-7.  (cond(A + mu diag A) is about 4e6 / (1e-8 x 1e4) = 4e10 for two rows, so 4e-6 would be the
    a-priori figure; the recursion does much better than that.)"""
    worst = 0.0
    for x, obs, prs in _case(n, drop):
        H = sm.data_terms(x, obs, prs)[2]
        if drop is not None:
            assert np.all(H[drop] == 0.0)
        band = sc.banded_blocks(H, W)
        dense = sc.dense_inverse(H, W)[1]
        worst = max(worst, float(np.abs(band - dense).max() / np.abs(dense).max()))
    print(f"\n{n} rows, drop {drop}: banded against dense, worst relative difference {worst:.3e}")
    assert worst <= 1e-7


def test_banded_recursion_stays_accurate_over_many_rows():
    """60 rows with a 12-row hole (test_smooth_cpu._scene's walk in 4 cameras): the recursion makes every Sigma_tt symmetric before it
    carries it to the next row.  Without that the antisymmetric part of the rounding errors grows 1.85 x per row: 2.6e-4 of the largest
    entry after these 60 rows (1e19 after 150), where the symmetric recursion measures 2.2e-9 at every row.  Bound: the yardstick's 1e-7."""
    from test_smooth_cpu import _scene
    views, Ps, rec, _ = _scene(60, 11, tuple(range(30, 42)))
    (obs, prs), = sc.problems(views, Ps, [rec])
    x0, filled = sm.init_traj(rec["frames"], rec["params"])
    assert int(filled.sum()) == 12
    H = sm.data_terms(x0, obs, prs)[2]
    band, dense = sc.banded_blocks(H, W), sc.dense_inverse(H, W)[1]
    rel = np.abs(band - dense).max(axis=(1, 2)) / np.abs(dense).max()
    print(f"\n60 rows: banded against dense per row, first {rel[0]:.3e}, last {rel[-1]:.3e}, worst {rel.max():.3e}")
    assert rel.max() <= 1e-7
    assert np.array_equal(band, band.transpose(0, 2, 1))


def test_joint_jacobians_equal_central_differences_of_the_fk():
    worst = 0.0
    for x, _, _ in _case(6, 3):
        for p in x[[0, 3, 5]]:
            D = sc.joint_jacobians(p)
            num = np.zeros_like(D)
            h = 1e-6
            for q, c in enumerate(sm.COLS):
                pp, pm = p.copy(), p.copy()
                pp[c] += h
                pm[c] -= h
                num[:, :, q] = (sc.fk(pp) - sc.fk(pm)) / (2 * h)
            worst = max(worst, float(np.abs(D - num).max()))
            # the six held joints' columns are absent, and only strict ancestors move a joint: the root joint follows the translation alone
            assert np.array_equal(D[0, :, :3], np.eye(3)) and np.all(D[0, :, 3:] == 0.0)
    print("\nD_K against central differences of the FK (m / rad):", worst)
    assert worst <= 1e-8


@pytest.mark.parametrize("n,drop", [(2, None), (6, 3), (11, None)])
def test_edof_is_the_dense_trace_and_lies_between_zero_and_the_parameter_count(n, drop):
    for x, obs, prs in _case(n, drop):
        c = sc.covariance(x, obs, prs, W)
        m = x.shape[0]
        A = sc.dense_A(c["H"], W)
        JtJ = np.zeros_like(A)
        for r in range(m):
            JtJ[r * sc.K:(r + 1) * sc.K, r * sc.K:(r + 1) * sc.K] = c["H"][r]
        dense = float(np.trace(np.linalg.solve(A, JtJ)))
        print(f"\n{n} rows, drop {drop}: edof {c['edof']:.6f} (dense {dense:.6f}) of {39 * m}, n_res {c['n_res']}, noise {c['noise_px']:.3f} px")
        assert abs(c["edof"] - dense) <= 1e-9 * dense
        assert 0.0 < c["edof"] < 39 * m
        if drop is not None:
            assert c["e"][drop] == 0.0 and np.all(np.isfinite(c["joint_sigma"][drop])) and np.all(c["joint_sigma"][drop] > 0)
        assert c["n_res"] == 2 * sum(int(np.count_nonzero(ob[:, :, 2])) for ob in obs if ob is not None) > c["edof"]
        assert np.isfinite(c["noise_px"]) and c["noise_px"] > 0
        d = sc.covariance(x, obs, prs, W, noise_px=2.0 * c["noise_px"])
        assert np.allclose(d["joint_sigma"], 2.0 * c["joint_sigma"], rtol=1e-14, atol=0)


def test_covariance_argument_checks_run_before_any_device_call(monkeypatch):
    from multiview_motion_capture_amd import _cabi, device as dev, smoothing
    from multiview_motion_capture_amd.common import Calib
    from test_body_fit_cpu import _Rec
    import oracle_np as o

    def boom(*a, **k):
        raise AssertionError("device called")
    for name in ("ingest", "body_observe", "smooth_blocks", "smooth_step", "smooth_cov", "fk"):
        monkeypatch.setattr(dev, name, boom)
    monkeypatch.setattr(_cabi, "load", boom)
    cal = [Calib.from_k_rt(np.eye(3), np.concatenate([np.eye(3), np.zeros((3, 1))], 1)) for _ in range(4)]
    kps = np.zeros((5, 4, 2, 25, 3))
    cnt = np.zeros((5, 4), np.int32)
    _, ref = o.skeleton_constants()
    p = np.concatenate([np.zeros(57), ref])
    good = _Rec([0, 1], [p, p], np.zeros((2, 18, 3)))
    for kw, what in [(dict(covariance="full"), "covariance"), (dict(covariance=True), "covariance"),
                     (dict(covariance="joints", noise_px=0.0), "noise_px"), (dict(covariance="joints", noise_px=-1.0), "noise_px"),
                     (dict(covariance="joints", noise_px=np.nan), "noise_px"), (dict(covariance="joints", noise_px=np.inf), "noise_px"),
                     (dict(covariance="joints", noise_px="2"), "noise_px"), (dict(noise_px=2.0), "without covariance")]:
        with pytest.raises(ValueError, match=what):
            smoothing.smooth_tracklets([good], kps, cnt, cal, **kw)
        with pytest.raises(ValueError, match=what):
            smoothing.smooth_sequences([(kps, cnt, cal)], [[good]], **kw)
    assert smoothing.smooth_sequences([], [], covariance="joints", noise_px=1.5) == []
