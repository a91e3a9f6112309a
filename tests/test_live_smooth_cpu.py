"""CPU: the fixed-lag live smoother's NumPy restatement (tests/live_smooth_np.py) -- window energy identities, gradient, window solve,
monotone E, streaming unwrap, quality against the raw poses --, LiveSmoother's input checks (before any device call) and the C entry
point mvmc_smooth_window: declared, exported, bound, argument errors before any HIP call."""
import ctypes
import os
import re

import numpy as np
import pytest

import live_smooth_np as ls
import oracle_np as o
import smooth_np as sm
from test_smooth_cpu import W, _fk, _problem, _scene, _walk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _window(h, seed=0):
    x0, _, obs, prs = _problem(seed=seed, holes=(3, 4), n=9)
    obs, prs = [None] * h + obs[h:], [None] * h + prs[h:]
    return x0, obs, prs


def test_window_energy_identities():
    x0, obs, prs = _window(0)
    assert ls.window_energy(x0, 0, obs, prs, W) == sm.energy(x0, obs, prs, W)      # no history: smooth_np.energy exactly
    rng = np.random.default_rng(1)
    for h in (1, 2):
        x0, obs, prs = _window(h)
        x1 = x0.copy()
        x1[h:, :57] += rng.normal(0, 0.01, (9 - h, 57))                            # the free rows move, the history does not
        diff = [sum(sm.energy(x, obs, prs, W)) - sum(ls.window_energy(x, h, obs, prs, W)) for x in (x0, x1)]
        wv = sm.prior_weights(W)[0]
        const = 0.5 * np.sum(wv * (x0[1, sm.COLS] - x0[0, sm.COLS]) ** 2) if h == 2 else 0.0
        scale = sum(sm.energy(x0, obs, prs, W))
        assert abs(diff[0] - const) <= 1e-12 * scale and abs(diff[1] - const) <= 1e-12 * scale, (h, diff, const)


def test_free_rows_gradient_matches_central_differences():
    for h in (1, 2):
        x0, obs, prs = _window(h)
        g = ls.window_system(x0, h, obs, prs, W)[3]
        num = np.zeros_like(g)
        eps = 1e-6
        for r in range(h, x0.shape[0]):
            for q, c in enumerate(sm.COLS):
                xp, xm = x0.copy(), x0.copy()
                xp[r, c] += eps
                xm[r, c] -= eps
                num[r - h, q] = (sum(ls.window_energy(xp, h, obs, prs, W)) - sum(ls.window_energy(xm, h, obs, prs, W))) / (2 * eps)
        err = np.abs(num - g).max() / np.abs(g).max()
        print(f"\nh = {h}: relative gradient error {err}")
        assert err < 1e-6


def test_banded_window_solve_matches_a_dense_solve_of_the_whole_problem():
    """The dense system is built over all h + m rows from the full prior matrices, then the history rows and columns are struck out."""
    w = (3e3, 1e4, 2e3, 5e4)
    for h in (0, 1, 2):
        x0, obs, prs = _window(h, seed=3)
        n = x0.shape[0]
        _, _, H, g, Hv, Ha, wv, wa = ls.window_system(x0, h, obs, prs, w)
        Dv, Da = sm.prior_mats(n)
        A = np.kron(Dv.T @ Dv, np.diag(wv)) + np.kron(Da.T @ Da, np.diag(wa))
        for r in range(h, n):
            A[r * sm.K:(r + 1) * sm.K, r * sm.K:(r + 1) * sm.K] += H[r - h]
        A = A[h * sm.K:, h * sm.K:]
        for mu in (1e-3, 1.0):
            d, _, ok = sm.banded_solve(H, g, Hv, Ha, wv, wa, mu)
            e = np.linalg.solve(A + mu * np.diag(np.diag(A)), -g.ravel()).reshape(-1, sm.K)
            assert ok and np.abs(d - e).max() <= 1e-9 * np.abs(e).max(), (h, mu)


def test_streaming_unwrap_equals_unwrap_euler_of_the_whole_record():
    from multiview_motion_capture_amd.smoothing import unwrap_euler, unwrap_euler_many
    p = _walk(40, 1)
    ang = p[:, 3:57].reshape(40, 18, 3).copy()
    rng = np.random.default_rng(2)
    ang[10:, 4, 0] += 2 * np.pi
    ang[25:, 9] = np.stack([ang[25:, 9, 0] + np.pi, np.pi - ang[25:, 9, 1], ang[25:, 9, 2] - np.pi], -1)
    ang[30] += 2 * np.pi * rng.integers(-2, 3, (18, 3))
    whole = unwrap_euler(ang)
    a, b = [ang[0].copy()], [ang[0].copy()]
    for k in range(1, 40):
        a.append(ls.unwrap_towards(a[-1], ang[k]))                         # the restatement's step
        b.append(unwrap_euler_many([np.stack([b[-1], ang[k]])])[0][1])     # LiveSmoother's step
    assert np.array_equal(np.array(a), whole) and np.array_equal(np.array(b), whole)


def _stream_scene(n=48, holes=(20, 21, 22), window=12, lag=6, n_iter=2):
    views, Ps, rec, truth = _scene(n, seed=5, holes=holes)
    st = ls.Stream(Ps, window, lag, n_iter, W)
    hits, k = 0, 0
    emitted, infos = {}, []
    for f in range(n):
        data = f not in holes
        if data:
            hits += 1
            par, jn = rec["params"][k], rec["joints"][k]
            k += 1
        out = st.tick(f, views[f], np.array([[7, 2, hits, 0]]), par[None], jn[None])
        for tid, fr, p, j, filled, nv in out["emitted"]:
            emitted[fr] = (j, filled)
        infos += list(out["solved"].values())
    return emitted, infos, rec, truth, st


def test_e_never_increases_within_a_tick_and_the_emitted_poses_beat_the_raw_ones():
    emitted, infos, rec, truth, st = _stream_scene()
    trials = sum(len(i["trace"]) for i in infos)
    for i in infos:
        assert np.all(np.diff(np.array(i["history"])) <= 0)
    assert trials >= 47 and sum(sum(i["trace"]) for i in infos) >= 1
    J_true = np.array([_fk(p) for p in truth])
    raw = dict(zip(rec["frames"].tolist(), rec["joints"]))
    assert sorted(emitted) == list(range(42))                               # frames 0 .. 47 - lag
    assert [f for f in emitted if emitted[f][1]] == [20, 21, 22]             # the holes are emitted, flagged filled
    data = [f for f in emitted if f in raw]
    mp = lambda J, f: np.linalg.norm(J - J_true[f], axis=-1).mean()
    e_s = np.mean([mp(emitted[f][0], f) for f in data])
    e_r = np.mean([mp(raw[f], f) for f in data])
    jit = lambda seq: np.linalg.norm(seq[2:] - 2 * seq[1:-1] + seq[:-2], axis=-1).mean()
    j_s, j_r = jit(np.array([emitted[f][0] for f in range(20)])), jit(np.array([raw[f] for f in range(20)]))
    e_f = np.mean([mp(emitted[f][0], f) for f in (20, 21, 22)])
    print(f"\n{trials} trials, {sum(sum(i['trace']) for i in infos)} accepted; emitted MPJPE on data frames {1e3 * e_s:.1f} mm against "
          f"{1e3 * e_r:.1f} mm raw; on the filled frames {1e3 * e_f:.1f} mm; jitter over frames 0-19 {j_s:.3f} against {j_r:.3f} raw")
    assert e_s < e_r and j_s < j_r
    # the finished record: contiguous, ends on a data row, every row final
    done = st.close()[0]
    assert done["frames"].tolist() == list(range(48)) and done["final"].all() and done["filled"].sum() == 3


def test_trailing_missing_rows_are_dropped_when_the_identity_finishes_and_jumps_fill_in():
    views, Ps, rec, _ = _scene(12, seed=6)
    st = ls.Stream(Ps, 4, 1, 1, W)
    tab = lambda k, hits: (np.array([[3, 2, hits, 0]]), rec["params"][k][None], rec["joints"][k][None])
    st.tick(0, views[0], *tab(0, 1))
    st.tick(1, views[1], *tab(1, 2))
    out = st.tick(4, views[4], *tab(4, 3))                                # a jump of 3: two missing rows
    assert st.ids[3].data == [True, True, False, False, True] and [e[1] for e in out["emitted"]] == [3] and out["emitted"][0][4]
    st.tick(5, views[5], *tab(4, 3))                                      # in the table without data
    st.tick(6, views[6], *tab(4, 3))
    out = st.tick(7, views[7], np.zeros((0, 4)), np.zeros((0, 68)), np.zeros((0, 18, 3)))
    assert len(out["finished"]) == 1 and out["finished"][0]["frames"].tolist() == [0, 1, 2, 3, 4]
    with pytest.raises(ValueError):
        st.tick(7, views[7], *tab(4, 3))
    with pytest.raises(ValueError):
        st.tick(12, views[7], *tab(4, 3))                                  # 4 missing rows >= the window


def test_live_smoother_input_checks_run_before_any_device_call(monkeypatch):
    from multiview_motion_capture_amd import _cabi, device as dev
    from multiview_motion_capture_amd.common import Calib
    from multiview_motion_capture_amd.live_smoothing import LiveSmoother
    from multiview_motion_capture_amd.tracker import T_WIDE

    def boom(*a, **k):
        raise AssertionError("device called")
    for name in ("ingest", "body_observe", "smooth_window", "fk"):
        monkeypatch.setattr(dev, name, boom)
    monkeypatch.setattr(_cabi, "load", boom)
    for kw in (dict(window=1), dict(window=33), dict(lag=-1), dict(lag=24), dict(window=8, lag=8), dict(n_iter=0), dict(n_iter=9),
               dict(root_vel=-1.0), dict(ang_acc=np.nan), dict(root_vel=np.inf), dict(root_vel=0.0, root_acc=0.0),
               dict(ang_vel=0.0, ang_acc=0.0)):
        with pytest.raises(ValueError):
            LiveSmoother(4, 2, **kw)
    with pytest.raises(ValueError):
        LiveSmoother(4, 0)
    cal = [Calib.from_k_rt(np.eye(3), np.concatenate([np.eye(3), np.zeros((3, 1))], 1)) for _ in range(4)]
    sm_ = LiveSmoother(4, 2, p_max=3, window=6, lag=2)
    key = sm_.open_session(cal)
    with pytest.raises(ValueError, match="cameras"):
        sm_.open_session(cal[:3])
    sm_.open_session(cal)
    with pytest.raises(ValueError, match="slots"):
        sm_.open_session(cal)
    _, ref = o.skeleton_constants()
    p = np.concatenate([np.zeros(57), ref])
    kps, cnt = np.zeros((4, 3, 25, 3)), np.zeros(4, np.int32)
    tab = lambda n, tid0=0: (np.array([[tid0 + k, 1, 1, 1] for k in range(n)]).reshape(n, 4), np.tile(p, (n, 1)), np.zeros((n, 18, 3)))
    bad = p.copy()
    bad[4] = np.nan
    cases = [
        ({99: (0, (kps, cnt)) + tab(1)}, "no open session"),
        ({key: (0, (kps[:3], cnt)) + tab(1)}, "kps"),
        ({key: (0, (np.zeros((4, 4, 25, 3)), cnt)) + tab(1)}, "kps"),
        ({key: (0, (kps, cnt[:3])) + tab(1)}, "counts"),
        ({key: (0, (kps, cnt + 4)) + tab(1)}, "counts"),
        ({key: (0, (kps, cnt)) + tab(T_WIDE + 1)}, "live identities"),
        ({key: (0, (kps, cnt), np.array([[1, 1, 1, 1], [1, 1, 1, 1]]), np.tile(p, (2, 1)), np.zeros((2, 18, 3)))}, "twice"),
        ({key: (0, (kps, cnt), np.array([[1, 1, 1, 1]]), bad[None], np.zeros((1, 18, 3)))}, "finite"),
        ({key: (0, (kps, cnt), np.array([[1, 1, 1, 1]]), p[None, :60], np.zeros((1, 18, 3)))}, "table"),
        ({key: (0, (kps, cnt)) + tab(1), 1: (0, (np.zeros((4, 3, 17, 3)), cnt)) + tab(1)}, "25-row or all 17-row"),
    ]
    for tables, msg in cases:
        with pytest.raises(ValueError, match=msg):
            sm_.update_tables(tables)
    sm_._sessions[key].f_last = 5
    with pytest.raises(ValueError, match="does not increase"):
        sm_.update_tables({key: (5, (kps, cnt)) + tab(1)})
    with pytest.raises(ValueError, match="jumps"):
        sm_.update_tables({key: (12, (kps, cnt)) + tab(1)})
    assert sm_._sessions[key].f_last == 5 and not sm_._sessions[key].ids and sm_._st is None     # nothing was stepped
    assert sm_.update_tables({key: (5, (kps, cnt)) + tab(1)}, failed={key}) == {}
    with pytest.raises(ValueError, match="follows no pool"):
        sm_.update_4d({})
    with pytest.raises(ValueError, match="no open session"):
        sm_.close_session(17)


def test_smooth_window_is_declared_exported_and_bound():
    from multiview_motion_capture_amd import _cabi, live_smoothing as L
    header = open(os.path.join(ROOT, "include", "mvmc.h")).read()
    m = re.search(r"int\s+mvmc_smooth_window\s*\(([^)]*)\)", header)
    assert m, "mvmc_smooth_window is not declared in include/mvmc.h"
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1)).split(",")]
    assert len(args) == 28
    assert re.search(r"long long\s+mvmc_smooth_window_work_doubles\s*\(", header)
    assert "mvmc_smooth_window" in _cabi.SYMBOLS and "mvmc_smooth_window_work_doubles" in _cabi.SYMBOLS
    lib = _cabi.load()
    fn = lib.mvmc_smooth_window          # AttributeError if the library does not export it
    assert len(fn.argtypes) == 28 and fn.restype is ctypes.c_int and fn.argtypes[26] is ctypes.c_longlong
    assert lib.mvmc_smooth_window_work_doubles.restype is ctypes.c_longlong
    consts = {k: int(v) for k, v in re.findall(r"#define\s+MVMC_SMOOTH_WIN_(\w+)\s+(\d+)", header)}
    assert consts == dict(MAX=L.WINDOW_MAX, RING=L.RING, ITEM_INTS=_cabi.SMOOTH_WIN_ITEM_INTS, INFO_DOUBLES=_cabi.SMOOTH_WIN_INFO_DOUBLES)
    assert L.N_ITER_MAX == consts["INFO_DOUBLES"] - 8 and consts["RING"] >= 2 * consts["MAX"] + 2
    assert _cabi.MVMC_ABI == 6
    # the workspace is sized by the tick's items, not by slots
    w = lib.mvmc_smooth_window_work_doubles
    assert w(0, 24) == 0 and w(3, 24) == 3 * w(1, 24) and w(1, 24) > w(1, 12) > 0
    assert w(1, 1) == -1 and w(1, 33) == -1 and w(-1, 24) == -1


def test_smooth_window_argument_errors_come_before_any_hip_call():
    from multiview_motion_capture_amd import _cabi
    lib = _cabi.load()
    fn = lib.mvmc_smooth_window
    sk = ctypes.byref(_cabi.MvmcSkeleton())
    fake = lambda k: ctypes.c_void_p(0x1000 * (k + 1))    # never dereferenced: the call must refuse first
    need = lib.mvmc_smooth_window_work_doubles(2, 24)

    def call(skel=sk, n_views=5, p_max=4, n_rigs=1, n_items=2, n_new=1, n_slots=8, window=24, n_iter=2, w=(1e4, 1e4, 1e4, 1e4),
             mu0=1e-3, work=need, null=()):
        ptr = lambda name, k: None if name in null else fake(k)
        return fn(skel, ptr("kps17", 0), n_views, p_max, ptr("Pmats", 1), n_rigs, ptr("items", 2), n_items, ptr("new_params", 3),
                  ptr("new_members", 4), n_new, ptr("rows", 5), ptr("members", 6), ptr("count", 7), n_slots, window, n_iter, w[0], w[1],
                  w[2], w[3], mu0, 1e-12, 1e-10, ptr("info", 8), ptr("work", 9), work, None)
    assert call(skel=None) == 1
    for kw in (dict(n_views=0), dict(n_views=65), dict(p_max=0), dict(n_rigs=0), dict(n_items=-1), dict(n_new=-1), dict(window=1),
               dict(window=33), dict(n_iter=0), dict(n_iter=9), dict(w=(-1.0, 1, 1, 1)), dict(w=(1, 1, 1, float("nan"))), dict(mu0=0.0),
               dict(work=need - 1)):
        assert call(**kw) == 1, kw
    for name in ("kps17", "Pmats", "items", "new_params", "new_members", "rows", "members", "count", "info", "work"):
        assert call(null=(name,)) == 1, name
    assert call(n_items=0) == 0                           # nothing to do: no launch either
