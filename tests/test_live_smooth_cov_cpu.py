"""CPU: the NumPy restatement of the live smoother's covariance (tests/live_smooth_cov_np.py) -- the banded recursion over the window's
factor against the dense inverse of the window's matrix with 0, 1 and 2 frozen history rows, the emitted row anywhere in the window,
missing rows; without history it is smooth_cov_np.covariance; conditioning on the history never raises a variance --, the argument
checks of LiveSmoother(covariance=, noise_px=), which run before any device call, and the C entry's declaration and argument errors.
The gate of the device tests (tests/test_gpu_live_smooth_cov.py) is set here."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import live_smooth_cov_np as lc
import live_smooth_np as ls
import smooth_cov_np as sc
import smooth_np as sm
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = (1e4, 1e4, 1e4, 1e4)
WINDOW = 6
# (rows of the identity, missing row or None, the emitted row's index among the free rows): identity ages 2, 3 and 6 have no history,
# 7 has one frozen row, 8 and 11 two; the emitted row is the last free row (lag 0), one in the middle, and free row 0 (lag = window - 1
# once the window is full); (7, 4) and (11, 8): a missing row inside the window, emitted itself (e = 3) or not
CASES = [(2, None, 1), (2, None, 0), (3, None, 2), (3, None, 1), (3, None, 0), (6, None, 5), (6, None, 3), (6, None, 0),
         (7, None, 5), (7, None, 3), (7, None, 0), (8, None, 5), (8, None, 2), (8, None, 0), (11, None, 5), (11, None, 3), (11, None, 0),
         (7, 4, 3), (7, 4, 5), (11, 8, 3), (11, 8, 0)]

# The device gate: 10 x the worst relative difference, against the largest entry, between the banded restatement and the dense
# inverse over CASES and both Shelf identities, as measured by test_banded_recursion_equals_the_dense_inverse_of_the_window below
# (WORST_BANDED; the figures per case are in its docstring).  The margin is tests/test_gpu_smooth_cov.py's, for the same reason: the
# device runs the banded recursion in another summation order.  The figure comes from this CPU restatement, never from the device.
WORST_BANDED = 9.1e-9
TOL = 10 * WORST_BANDED
assert TOL <= 1e-6


@functools.lru_cache(maxsize=None)
def shelf():
    """The noise-free oracle tracker's records of the first 12 Shelf frames (both people on every one), the ingested views, P."""
    from test_gpu_body_fit import _np_records, _oracle_records
    si, fx = load_golden("shelf_inputs.npz"), load_golden("shelf_clean_oracle_tracker.npz")
    recs = _np_records(_oracle_records(fx, 12))
    assert len(recs) >= 2 and all(len(r["frames"]) >= 11 for r in recs)
    return recs, sm.bf.ingest_np(si["kps25"][:13], si["counts"][:13].astype(np.int32)), si["P"]


@functools.lru_cache(maxsize=None)
def identity_rows(n, drop):
    """Per Shelf identity dict(x (n,68) after two LM trials of the whole record, obs, prs per row, sel (n,C) the selected pose of
    every camera (-1: none, and on the missing row), f0 the first frame): its first n record frames without frame ``drop``."""
    recs, views, P = shelf()
    keep = [i for i in range(n) if i != drop]
    out = []
    for rec in recs:
        fr, pr, jo = rec["frames"][keep], rec["params"][keep], rec["joints"][keep]
        sel, _, _ = sm.bf.select([(0, int(f), 0, np.asarray(jo[k], np.float64)) for k, f in enumerate(fr)], [views], [P])
        x0, filled = sm.init_traj(fr, pr)
        assert x0.shape[0] == n and int(filled.sum()) == (drop is not None)
        obs, prs, sl = [None] * n, [None] * n, -np.ones((n, P.shape[0]), int)
        for k, f in enumerate(fr):
            ob, p = sm.bf.observations(sel[k], views[int(f)], P)
            if len(ob):
                obs[f - fr[0]], prs[f - fr[0]] = ob, p
            sl[f - fr[0]] = sel[k]
        x, _ = sm.lm(x0, obs, prs, W, max_iter=2)
        out.append(dict(x=x, obs=obs, prs=prs, sel=sl, f0=int(fr[0])))
    return out


def window_of(idn, window=WINDOW):
    """An identity's rows -> (x (h + m, 68), h, obs, prs of the window problem at the end of a tick, the first free row)."""
    n = idn["x"].shape[0]
    m = min(window, n)
    h = min(2, n - m)
    lo = n - m - h
    return idn["x"][lo:], h, [None] * h + idn["obs"][n - m:], [None] * h + idn["prs"][n - m:], n - m


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


@pytest.mark.parametrize("n,drop,e", CASES)
def test_banded_recursion_equals_the_dense_inverse_of_the_window(n, drop, e):
    """Sigma_ee, C_K, p and edof of the banded recursion (down to row 0, and stopped at row e) against np.linalg.inv of the dense
    window matrix, relative to the largest entry.  Measured, worst of the two Shelf identities per case (n, drop, e): see
    WORST_BANDED above for the worst of all; 2 rows 9.1e-9, 3 rows 6.4e-9, 6 rows 4.7e-9 (smooth_cov_np's figures: without history
    the window is the offline problem), wherever the emitted row lies; 7, 8 and 11 rows (one and two frozen history rows), with and
    without a missing row, 4.8e-15 .. 3.0e-14 -- the frozen history pins the common mode of the knees' twist angles, whose block
    sets the figure without it."""
    worst = 0.0
    for idn in identity_rows(n, drop):
        x, h, obs, prs, _ = window_of(idn)
        assert h == (0 if n <= WINDOW else min(2, n - WINDOW))
        if drop is not None:
            assert obs[h + 3] is None
        d = lc.window_cov(x, h, obs, prs, W, e, blocks="dense")
        b = lc.window_cov(x, h, obs, prs, W, e)
        s = lc.window_cov(x, h, obs, prs, W, e, noise_px=1.0, full=False)
        assert d["status"] == b["status"] == s["status"] == 0 and b["n_res"] == d["n_res"] > 0
        worst = max(worst, rel(b["sigma"], d["sigma"]), rel(b["jcov"], d["jcov"]), rel(b["pvar"], d["pvar"]),
                    abs(b["edof"] - d["edof"]) / d["edof"], abs(b["noise_px"] - d["noise_px"]) / d["noise_px"])
        # stopping at the emitted row changes nothing above it: the same bits
        assert np.array_equal(s["jcov"], b["jcov"]) and np.array_equal(s["pvar"], b["pvar"]) and np.isnan(s["edof"]) and np.isnan(s["n_res"])
        assert 0.0 < d["edof"] < 39 * d["m"] and np.all(d["pvar"] > 0)
    print(f"\n{n} rows, drop {drop}, emitted free row {e}: banded against dense, worst relative difference {worst:.3e}")
    assert worst <= WORST_BANDED


@pytest.mark.parametrize("n,e", [(2, 0), (3, 1), (6, 5), (6, 0)])
def test_without_history_it_is_the_offline_covariance_of_the_same_rows(n, e):
    for idn in identity_rows(n, None):
        x, h, obs, prs, _ = window_of(idn)
        assert h == 0
        got, exp = lc.window_cov(x, 0, obs, prs, W, e), sc.covariance(x, obs, prs, W)
        assert rel(got["jcov"], exp["jcov"][e]) <= 1e-12 and rel(got["pvar"], exp["pvar"][e]) <= 1e-12
        assert abs(got["edof"] - exp["edof"]) <= 1e-12 * exp["edof"] and got["n_res"] == exp["n_res"]
        assert abs(got["noise_px"] - exp["noise_px"]) <= 1e-12 * exp["noise_px"]


@pytest.mark.parametrize("n,drop,e", [(7, None, 0), (7, 4, 3), (8, None, 0), (8, None, 5), (11, None, 3), (11, 8, 0)])
def test_conditioning_on_the_history_never_raises_a_variance(n, drop, e):
    """At the same x: A_w is the free-free block of the matrix of the problem whose history rows are free too (no data on them), so
    (that matrix's inverse)_ee - A_w^-1_ee is positive semi-definite (a Schur complement) and every joint's variance D_K . D_K^T can
    only grow.  Slack: 1e-9 relative, the dense inverses' own rounding (the banded-against-dense figure above)."""
    for idn in identity_rows(n, drop):
        x, h, obs, prs, _ = window_of(idn)
        assert h >= 1
        cond = lc.window_cov(x, h, obs, prs, W, e, noise_px=1.0, blocks="dense")
        free = lc.window_cov(x, 0, obs, prs, W, h + e, noise_px=1.0, blocks="dense")
        vc, vf = np.trace(cond["jcov"], axis1=-2, axis2=-1), np.trace(free["jcov"], axis1=-2, axis2=-1)
        print(f"\n{n} rows, drop {drop}, free row {e}: conditional / free joint variance {np.min(vc / vf):.4f} .. {np.max(vc / vf):.4f}")
        assert np.all(vc <= vf * (1 + 1e-9)) and np.all(vc > 0)
        assert np.all(cond["pvar"] <= free["pvar"] * (1 + 1e-9))
        assert np.min(np.linalg.eigvalsh(free["sigma"] - cond["sigma"])) >= -1e-9 * np.abs(free["sigma"]).max()


def test_stream_yields_the_covariance_of_every_emitted_row_and_the_records_keep_it():
    """The Stream wrapper on 10 Shelf ticks: an entry per emitted row, status 2 on an identity's first tick at lag 0, and the records'
    per-row arrays hold the emitted values with NaN on the rows that never were emitted."""
    si, fx = load_golden("shelf_inputs.npz"), load_golden("shelf_clean_oracle_tracker.npz")
    for lag in (0, 2):
        st = lc.Stream(si["P"], WINDOW, lag, 1, W)
        seen = {}
        for r in range(10):
            n = int(fx["n_tracks"][r])
            kps, cnt = si["kps25"][r + 1], si["counts"][r + 1].astype(np.int32)
            out = st.tick(r + 1, ls.bf.ingest_np(kps[None], cnt[None])[0], fx["meta"][r, :n], fx["params"][r, :n], fx["joints"][r, :n])
            assert sorted(out["cov"]) == sorted(e[0] for e in out["emitted"])
            for tid, c in out["cov"].items():
                assert c["status"] == (2 if r == 0 and lag == 0 else 0)
                seen.setdefault(tid, []).append(c)
        assert (len(seen) >= 2) and all(len(v) == 10 - lag for v in seen.values())
        for rec in st.records():
            js, ps, s = st.record_cov(rec)
            k = len(rec["frames"]) - lag
            got = seen[rec["track_id"]]
            assert np.all(np.isnan(js[k:])) and np.all(np.isnan(ps[k:])) and np.all(np.isnan(s[k:])) and js.shape == (k + lag, 18)
            for r in range(k):
                assert np.array_equal(js[r], got[r]["joint_sigma"], equal_nan=True) and np.array_equal(s[r], got[r]["noise_px"], equal_nan=True)
            first = 1 if lag == 0 else 0
            assert np.all(np.isfinite(js[first:k])) and np.all(js[first:k] > 0) and np.all(s[first:k] > 0)


def test_covariance_argument_checks_run_before_any_device_call(monkeypatch):
    from multiview_motion_capture_amd import _cabi, device as dev
    from multiview_motion_capture_amd.live_smoothing import LiveSmoother, TickOutput

    def boom(*a, **k):
        raise AssertionError("device called")
    for name in ("ingest", "body_observe", "smooth_window", "smooth_window_cov", "fk"):
        monkeypatch.setattr(dev, name, boom)
    monkeypatch.setattr(_cabi, "load", boom)
    for kw, msg in ((dict(covariance="joint"), "covariance must be None"), (dict(covariance=True), "covariance must be None"),
                    (dict(covariance=b"joints"), "covariance must be None"), (dict(noise_px=2.0), "without covariance"),
                    (dict(covariance="joints", noise_px=0.0), "finite number > 0"), (dict(covariance="joints", noise_px=-1.0), "finite number"),
                    (dict(covariance="joints", noise_px=np.nan), "finite number"), (dict(covariance="joints", noise_px=np.inf), "finite number"),
                    (dict(covariance="joints", noise_px="2"), "finite number"), (dict(covariance="joints", noise_px=True), "finite number")):
        with pytest.raises(ValueError, match=msg):
            LiveSmoother(4, 2, window=6, lag=2, **kw)
    a, b, c = LiveSmoother(4, 2), LiveSmoother(4, 2, covariance="joints"), LiveSmoother(4, 2, covariance="joints", noise_px=np.float32(2.0))
    assert (a._cov, a._noise_px) == (False, None) and (b._cov, b._noise_px) == (True, None) and (c._cov, c._noise_px) == (True, 2.0)
    assert TickOutput().cov == {}

    class _Pool:
        C, capacity, P, device = 4, 2, 3, None
    assert LiveSmoother.for_pool(_Pool(), covariance="joints", noise_px=1.5)._noise_px == 1.5
    with pytest.raises(ValueError, match="without covariance"):
        LiveSmoother.for_pool(_Pool(), noise_px=1.5)


def test_smooth_window_cov_is_declared_exported_and_bound():
    from multiview_motion_capture_amd import _cabi
    header = open(os.path.join(ROOT, "include", "mvmc.h")).read()
    m = re.search(r"int\s+mvmc_smooth_window_cov\s*\(([^)]*)\)", header)
    assert m, "mvmc_smooth_window_cov is not declared in include/mvmc.h"
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1)).split(",")]
    assert len(args) == 27
    assert re.search(r"long long\s+mvmc_smooth_window_cov_work_doubles\s*\(", header)
    assert "mvmc_smooth_window_cov" in _cabi.SYMBOLS and "mvmc_smooth_window_cov_work_doubles" in _cabi.SYMBOLS
    assert int(re.search(r"#define\s+MVMC_SMOOTH_COV_ITEM_INTS\s+(\d+)", header).group(1)) == _cabi.SMOOTH_COV_ITEM_INTS == 4
    lib = _cabi.load()
    fn = lib.mvmc_smooth_window_cov          # AttributeError if the library does not export it
    assert len(fn.argtypes) == 27 and fn.restype is ctypes.c_int and fn.argtypes[22] is ctypes.c_longlong
    w = lib.mvmc_smooth_window_cov_work_doubles
    assert w.restype is ctypes.c_longlong
    assert w(0, 24) == 0 and w(3, 24) == 3 * w(1, 24) and w(1, 24) > w(1, 12) > 0      # sized by the tick's emitted rows
    assert w(1, 1) == -1 and w(1, 33) == -1 and w(-1, 24) == -1
    assert _cabi.MVMC_ABI == 6


def test_smooth_window_cov_argument_errors_come_before_any_hip_call():
    from multiview_motion_capture_amd import _cabi
    lib = _cabi.load()
    fn = lib.mvmc_smooth_window_cov
    sk = ctypes.byref(_cabi.MvmcSkeleton())
    fake = lambda k: ctypes.c_void_p(0x1000 * (k + 1))    # never dereferenced: the call must refuse first
    need = lib.mvmc_smooth_window_cov_work_doubles(2, 24)

    def call(skel=sk, n_views=5, p_max=4, n_rigs=1, n_items=2, n_slots=8, window=24, w=(1e4, 1e4, 1e4, 1e4), mu=1e-8, full=1, loss=0,
             loss_px=0.0, work=need, null=()):
        ptr = lambda name, k: None if name in null else fake(k)
        return fn(skel, ptr("kps17", 0), n_views, p_max, ptr("Pmats", 1), n_rigs, ptr("items", 2), n_items, ptr("rows", 3),
                  ptr("members", 4), ptr("count", 5), n_slots, window, w[0], w[1], w[2], w[3], mu, full, loss, loss_px, ptr("work", 6),
                  work, ptr("jcov", 7), ptr("pvar", 8), ptr("cinfo", 9), None)
    assert call(skel=None) == 1
    for kw in (dict(n_views=0), dict(n_views=65), dict(p_max=0), dict(n_rigs=0), dict(n_items=-1), dict(n_slots=-1), dict(window=1),
               dict(window=33), dict(w=(-1.0, 1, 1, 1)), dict(w=(1, 1, 1, float("nan"))), dict(mu=-1e-8), dict(mu=float("nan")),
               dict(loss=3), dict(loss=-1), dict(loss=1, loss_px=0.0), dict(loss=2, loss_px=float("inf")), dict(work=need - 1)):
        assert call(**kw) == 1, kw
    for name in ("kps17", "Pmats", "items", "rows", "members", "count", "work", "jcov", "pvar", "cinfo"):
        assert call(null=(name,)) == 1, name
    assert call(n_items=0) == 0                           # nothing to do: no launch either
