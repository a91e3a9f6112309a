"""CPU: the trajectory smoother's NumPy restatement (tests/smooth_np.py) -- Euler unwrapping, gradient, banded solve, monotone E --, the
host side of multiview_motion_capture_amd/smoothing.py (unwrapping, initial trajectory, output records) and its input checks (before
any device call)."""
import numpy as np
import pytest

import oracle_np as o
import smooth_np as sm
from test_body_fit_cpu import _cameras, _coco, _Rec

W = (1e4, 1e4, 1e4, 1e4)


def _fk(p):
    return o.forward_kinematics(p[:3], p[3:57], p[57:])[0]


def _walk(n, seed, step=0.02):
    rng = np.random.default_rng(seed)
    _, ref = o.skeleton_constants()
    root = np.array([0.0, 0.0, 1.0]) + np.cumsum(rng.normal(0, step, (n, 3)), axis=0)
    ang = rng.normal(0, 0.3, (18, 3)) + np.cumsum(rng.normal(0, step, (n, 18, 3)), axis=0)
    return np.concatenate([root, ang.reshape(n, 54), np.tile(ref, (n, 1))], axis=1)


def test_unwrap_keeps_fk_and_removes_jumps():
    from multiview_motion_capture_amd.smoothing import unwrap_euler
    p = _walk(40, 1)
    wrapped = p.copy()
    ang = wrapped[:, 3:57].reshape(40, 18, 3)
    rng = np.random.default_rng(2)
    ang[10:, 4, 0] += 2 * np.pi                      # a 2 pi jump inside the record
    ang[25:, 9] = np.stack([ang[25:, 9, 0] + np.pi, np.pi - ang[25:, 9, 1], ang[25:, 9, 2] - np.pi], -1)   # a branch flip
    ang[30] += 2 * np.pi * rng.integers(-2, 3, (18, 3))   # random multiples of 2 pi on one frame
    for un in (unwrap_euler(ang), sm.unwrap(ang)):
        q = wrapped.copy()
        q[:, 3:57] = un.reshape(40, 54)
        worst = max(np.abs(_fk(a) - _fk(b)).max() for a, b in zip(wrapped, q))
        # (the FK's quaternions carry the reference's 1 / (1 + 1e-10) factor on the sines, so a branch flip is exact only to ~1e-10)
        assert worst <= 1e-9, worst
        assert np.abs(np.diff(un, axis=0)).max() <= np.pi
        assert np.abs(un - p[:, 3:57].reshape(40, 18, 3)).max() < 1e-9   # the smooth original comes back
    assert np.array_equal(unwrap_euler(ang), sm.unwrap(ang))
    # a 2 pi jump alone: FK equal to 1e-12 m
    q = p.copy()
    q[20:, 3 + 3 * 5] += 2 * np.pi
    un = unwrap_euler(q[:, 3:57].reshape(40, 18, 3))
    r = q.copy()
    r[:, 3:57] = un.reshape(40, 54)
    assert max(np.abs(_fk(a) - _fk(b)).max() for a, b in zip(q, r)) <= 1e-12
    assert np.abs(np.diff(un, axis=0)).max() <= np.pi


def _scene(n_frames=9, seed=0, holes=(), one_view=()):
    """Noisy observations of a walk in 4 cameras; records drop the frames in ``holes``."""
    rng = np.random.default_rng(seed)
    Ps = _cameras()
    p = _walk(n_frames, seed)
    views = []
    for f in range(n_frames):
        J = _fk(p[f])
        row = []
        for c in range(4):
            k = _coco(J, Ps[c], [5, 6, 11, 12][c])
            k[:, :2] += rng.normal(0, 2.0, (17, 2))
            row.append(k[None] if (f not in one_view or c == 0) else np.zeros((0, 17, 3)))
        views.append(row)
    keep = [f for f in range(n_frames) if f not in holes]
    noisy = p.copy()
    noisy[:, :57] += rng.normal(0, 0.01, (n_frames, 57))
    rec = dict(frames=np.array(keep), params=noisy[keep], joints=np.array([_fk(q) for q in noisy[keep]]))
    return views, Ps, rec, p


def _problem(seed=0, holes=(3, 4), n=9):
    views, Ps, rec, _ = _scene(n, seed, holes)
    sel, _, nv = sm.bf.select([(0, int(f), 0, rec["joints"][k]) for k, f in enumerate(rec["frames"])], [views], [Ps])
    x0, filled = sm.init_traj(rec["frames"], rec["params"])
    obs, prs = [None] * len(x0), [None] * len(x0)
    for k, f in enumerate(rec["frames"]):
        ob, pr = sm.bf.observations(sel[k], views[f], Ps)
        obs[f - rec["frames"][0]], prs[f - rec["frames"][0]] = ob, pr
    return x0, filled, obs, prs


def test_gradient_matches_central_differences():
    x0, filled, obs, prs = _problem()
    assert filled.tolist() == [False, False, False, True, True, False, False, False, False]
    Ed, _, H, gd = sm.data_terms(x0, obs, prs)
    Ep, gp = sm.prior(x0[:, sm.COLS], W)[:2]
    g = gd + gp
    num = np.zeros_like(g)
    h = 1e-6
    for r in range(x0.shape[0]):
        for q, c in enumerate(sm.COLS):
            xp, xm = x0.copy(), x0.copy()
            xp[r, c] += h
            xm[r, c] -= h
            num[r, q] = (sum(sm.energy(xp, obs, prs, W)) - sum(sm.energy(xm, obs, prs, W))) / (2 * h)
    err = np.abs(num - g).max() / np.abs(g).max()
    print("\nrelative gradient error:", err)
    assert err < 1e-6
    assert np.all(H[3] == 0) and np.all(gd[4] == 0)         # the holes have no data term


def test_banded_solve_matches_dense():
    x0, _, obs, prs = _problem(seed=3, holes=(2, 5, 6))
    _, _, H, gd = sm.data_terms(x0, obs, prs)
    Ep, gp, Hv, Ha, wv, wa = sm.prior(x0[:, sm.COLS], (3e3, 1e4, 2e3, 5e4))
    for mu in (1e-3, 1.0):
        d, _, ok = sm.banded_solve(H, gd + gp, Hv, Ha, wv, wa, mu)
        e = sm.dense_solve(H, gd + gp, Hv, Ha, wv, wa, mu)
        assert ok
        assert np.abs(d - e).max() <= 1e-9 * np.abs(e).max()


def test_e_never_increases_and_the_smoother_reduces_jitter():
    views, Ps, rec, truth = _scene(16, seed=5, holes=(6, 7, 8))
    res = sm.smooth([views], [Ps], [[rec]], W, max_iter=10)[0][0]
    h = np.array(res["history"])
    print("\nE over the trials:", h, "trace", res["trace"])
    assert np.all(np.diff(h) <= 0) and len(res["trace"]) >= 1 and res["trace"][0] == 1
    c = res["cost"]
    assert c[2] + c[3] < c[0] + c[1]
    assert res["frames"].tolist() == list(range(16)) and res["filled"].tolist() == [f in (6, 7, 8) for f in range(16)]
    J_true = np.array([_fk(p) for p in truth])
    err_s = np.linalg.norm(res["joints"] - J_true, axis=-1).mean()
    err_0 = np.linalg.norm(np.array([_fk(p) for p in res["x0"]]) - J_true, axis=-1).mean()
    assert err_s < err_0, (err_s, err_0)


def test_one_frame_records_and_max_iter_zero():
    views, Ps, rec, _ = _scene(4, seed=6)
    one = dict(frames=rec["frames"][:1], params=rec["params"][:1], joints=rec["joints"][:1])
    out = sm.smooth([views], [Ps], [[one, rec]], W, max_iter=0)[0]
    assert np.array_equal(out[0]["params"], one["params"]) and out[0]["trace"] == []
    assert out[1]["trace"] == [] and np.array_equal(out[1]["params"], out[1]["x0"])
    assert out[1]["cost"][0] == out[1]["cost"][2]


def test_initial_trajectory_and_the_host_records():
    from multiview_motion_capture_amd import smoothing as S
    p = _walk(10, 7)
    frames = np.array([3, 4, 7, 8, 12])
    par = p[frames - 3]
    par[:, 57:] *= np.linspace(1.0, 1.04, 5)[:, None]
    x, filled = S.initial_trajectory(frames, par)
    xe, fe = sm.init_traj(frames, par)
    assert np.abs(x - xe).max() <= 1e-12 and np.array_equal(filled, fe)
    assert filled.tolist() == [False, False, True, True, False, False, True, True, True, False]
    assert np.array_equal(x[4, 57:], par[2, 57:]) and np.array_equal(x[6, 57:], par[3, 57:])   # lengths: nearest earlier record frame
    assert np.array_equal(x[~filled], par)
    assert np.allclose(x[2, :57], par[1, :57] + (par[2, :57] - par[1, :57]) / 3)
    # the records: contiguous frames, filled flags, fill_gaps=False, one-frame records unchanged
    J = np.array([_fk(q) for q in par])
    rec = _Rec(frames, par, J, tid=4)
    rec.bone_lens = par[0, 57:].copy()
    single = _Rec([5], par[:1], J[:1], tid=9)
    recs = [(frames, par, J), (np.array([5]), par[:1], J[:1])]
    m = x.shape[0]
    jn = np.array([_fk(q) for q in x])
    inf = np.concatenate([[5.0, 1.0, 4.0, 0.5, 3, 2, 1e-3, 3], [1, 0, 1], -np.ones(21)])
    Pg = 3
    mem = np.where(filled[:, None], -1, np.arange(m)[:, None] * 4 * Pg + np.arange(4)[None] * Pg + 1).astype(np.int32)
    mem_h = np.concatenate([mem[~filled], [[-1, 7, -1, 11]]]).astype(np.int32)
    traj = [(0, x, filled, mem, np.where(filled, 0, 4), 0)]
    for fill in (True, False):
        out = [[None, None]]
        S._records(out, [(0, 0), (0, 1)], [recs], [[rec, single]], traj, {0: (x, jn, inf)}, mem_h, np.array([4] * 5 + [2]),
                   np.array([0, 5, 6]), fill, Pg)
        t, u = out[0]
        if fill:
            assert t.frame_idxs == list(range(3, 13)) and np.array_equal(t.smooth_filled, filled)
        else:
            assert t.frame_idxs == frames.tolist() and not t.smooth_filled.any()
        assert t.track_id == 4 and t.smooth_trials == [1, 0, 1] and np.array_equal(t.smooth_cost, [5, 1, 4, 0.5])
        assert np.array_equal(t.bone_lens, rec.bone_lens) and t.bone_lens is not rec.bone_lens
        assert len(t.poses) == len(t.frame_idxs) == len(t.smooth_views) == len(t.smooth_select)
        sel = np.where(mem >= 0, 1, -1)
        assert np.array_equal(t.smooth_select, sel if fill else sel[~filled])
        assert u.frame_idxs == [5] and u.smooth_trials == [] and u.smooth_views.tolist() == [2]
        assert u.smooth_select.tolist() == [[-1, 1, -1, 2]]
        # a one-frame record: equal to the input, but new objects (changing the output leaves the input as it was)
        q, q0 = u.poses[0], single.poses[0]
        assert q[1] is not q0[1] and q[2] is not q0[2] and q[0] == q0[0]
        assert np.array_equal(q[1].root, q0[1].root) and np.array_equal(np.ravel(q[1].euler_angles), np.ravel(q0[1].euler_angles))
        assert np.array_equal(q[1].bone_lens, q0[1].bone_lens) and np.array_equal(q[2].keypoints, q0[2].keypoints)
        q[1].root[0] += 1.0
        assert q0[1].root[0] == par[0, 0]
        assert not hasattr(rec, "smooth_cost")


def test_smooth_input_checks_run_before_any_device_call(monkeypatch):
    from multiview_motion_capture_amd import _cabi, device as dev, smoothing
    from multiview_motion_capture_amd.common import Calib

    def boom(*a, **k):
        raise AssertionError("device called")
    for name in ("ingest", "body_observe", "smooth_blocks", "smooth_step", "fk"):
        monkeypatch.setattr(dev, name, boom)
    monkeypatch.setattr(_cabi, "load", boom)
    cal = [Calib.from_k_rt(np.eye(3), np.concatenate([np.eye(3), np.zeros((3, 1))], 1)) for _ in range(4)]
    kps = np.zeros((5, 4, 2, 25, 3))
    cnt = np.zeros((5, 4), np.int32)
    _, ref = o.skeleton_constants()
    p = np.concatenate([np.zeros(57), ref])
    good = _Rec([0, 1], [p, p], np.zeros((2, 18, 3)))
    bad_cases = [
        dict(root_vel=-1.0), dict(ang_acc=np.nan), dict(root_vel=np.inf), dict(root_vel=0.0, root_acc=0.0),
        dict(ang_vel=0.0, ang_acc=0.0), dict(max_iter=-1), dict(max_iter=smoothing.MAX_ITER_CAP + 1), dict(max_work_bytes=0),
    ]
    for kw in bad_cases:
        with pytest.raises(ValueError):
            smoothing.smooth_tracklets([good], kps, cnt, cal, **kw)
    q = p.copy()
    q[5] = np.nan
    with pytest.raises(ValueError, match="finite"):
        smoothing.smooth_tracklets([_Rec([0, 1], [p, q], np.zeros((2, 18, 3)))], kps, cnt, cal)
    with pytest.raises(ValueError, match="increase"):
        smoothing.smooth_tracklets([_Rec([2, 1], [p, p], np.zeros((2, 18, 3)))], kps, cnt, cal)
    with pytest.raises(ValueError, match="outside"):
        smoothing.smooth_tracklets([_Rec([0, 5], [p, p], np.zeros((2, 18, 3)))], kps, cnt, cal)
    with pytest.raises(ValueError, match="twice"):
        smoothing.smooth_tracklets([_Rec([1, 1], [p, p], np.zeros((2, 18, 3)))], kps, cnt, cal)
    with pytest.raises(ValueError, match="calibrations"):
        smoothing.smooth_tracklets([good], kps, cnt, cal[:3])
    with pytest.raises(ValueError, match="record lists"):
        smoothing.smooth_sequences([(kps, cnt, cal)], [[good], []])
    with pytest.raises(ValueError, match="PoseShapeParam"):
        smoothing.smooth_tracklets([_Rec([0, 1], [p[:60], p[:60]], np.zeros((2, 18, 3)))], kps, cnt, cal)
    assert smoothing.smooth_sequences([], []) == []
