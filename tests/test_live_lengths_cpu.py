"""CPU: the live smoother's running skeleton (tests/live_lengths_np.py, the definition of lengths="auto") -- the Jacobian in the lengths,
noise-free rows, streaming with holes, a jump and a commit, quality against the per-frame lengths --, LiveSmoother's argument checks
(before any device call) and the C entries mvmc_live_lengths_apply / _update: declared, exported, bound, argument errors before any
HIP call."""
import ctypes
import os
import re

import numpy as np
import pytest

import body_fit_np as bf
import live_lengths_np as ll
import live_smooth_np as ls
import oracle_np as o
from test_smooth_cpu import W, _fk, _scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURV = np.array([s for s in range(11) if s != 7])      # slot 7 has a zero reference length and no curvature


def test_lengths_arguments_are_checked_before_any_device_call(monkeypatch):
    from multiview_motion_capture_amd import _cabi, device as dev
    from multiview_motion_capture_amd.live_smoothing import LENGTHS_PRIOR, LiveSmoother, check_lengths, committed_part

    def boom(*a, **k):
        raise AssertionError("device called")
    for name in ("ingest", "body_observe", "smooth_window", "fk", "live_lengths_apply", "live_lengths_update"):
        monkeypatch.setattr(dev, name, boom)
    monkeypatch.setattr(_cabi, "load", boom)
    for kw in (dict(lengths="fit"), dict(lengths=True), dict(lengths=1), dict(lengths="auto", lengths_prior=0.0),
               dict(lengths="auto", lengths_prior=-1.0), dict(lengths="auto", lengths_prior=np.nan),
               dict(lengths="auto", lengths_prior=np.inf), dict(lengths="auto", lengths_prior="1"),
               dict(lengths="auto", lengths_commit=0), dict(lengths="auto", lengths_commit=-3), dict(lengths="auto", lengths_commit=2.5),
               dict(lengths="auto", lengths_commit=True), dict(lengths_prior=2.0), dict(lengths_prior=LENGTHS_PRIOR),
               dict(lengths_commit=10)):
        with pytest.raises(ValueError, match="lengths"):
            LiveSmoother(4, 2, **kw)
    assert check_lengths(None, None, None) is None
    assert check_lengths("auto", 3, 20) == dict(prior=3.0, commit=20)
    assert check_lengths("auto", None, None) == dict(prior=float(LENGTHS_PRIOR), commit=None)
    sm_ = LiveSmoother(4, 2, lengths="auto", lengths_commit=5)
    assert sm_._st is None and sm_._len == dict(prior=float(LENGTHS_PRIOR), commit=5)

    class R:
        pass
    with pytest.raises(ValueError, match="committed"):
        committed_part(R())                                  # not a record of a smoother with lengths
    r = R()
    r.live_lengths_committed_row = -1
    with pytest.raises(ValueError, match="committed"):
        committed_part(r)


def test_the_two_entries_are_declared_exported_and_bound():
    from multiview_motion_capture_amd import _cabi
    header = open(os.path.join(ROOT, "include", "mvmc.h")).read()
    for name, n_args in (("mvmc_live_lengths_apply", 7), ("mvmc_live_lengths_update", 18)):
        m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)", header)
        assert m, f"{name} is not declared in include/mvmc.h"
        assert len([a for a in m.group(1).split(",")]) == n_args
        assert name in _cabi.SYMBOLS
        fn = getattr(_cabi.load(), name)                     # AttributeError if the library does not export it
        assert len(fn.argtypes) == n_args and fn.restype is ctypes.c_int
    consts = {k: int(v) for k, v in re.findall(r"#define\s+MVMC_LIVE_LEN_(\w+)\s+(\d+)", header)}
    assert consts == dict(STATE_DOUBLES=_cabi.LIVE_LEN_STATE_DOUBLES, INFO_DOUBLES=_cabi.LIVE_LEN_INFO_DOUBLES)
    assert consts["STATE_DOUBLES"] == 66 + 3 * 11 + 4 and consts["INFO_DOUBLES"] == 5 + 11 + 1
    assert _cabi.MVMC_ABI == 6
    src = open(os.path.join(ROOT, "multiview_motion_capture_amd", "csrc", "Makefile")).read()
    assert "mvmc_live_lengths.hip" in src


def test_argument_errors_come_before_any_hip_call():
    from multiview_motion_capture_amd import _cabi
    lib = _cabi.load()
    sk = ctypes.byref(_cabi.MvmcSkeleton())
    fake = lambda k: ctypes.c_void_p(0x1000 * (k + 1))    # never dereferenced: the call must refuse first

    def apply(n_items=2, n_new=1, n_slots=8, null=()):
        ptr = lambda name, k: None if name in null else fake(k)
        return lib.mvmc_live_lengths_apply(ptr("items", 0), n_items, ptr("new_params", 1), n_new, ptr("lens_state", 2), n_slots, None)
    for kw in (dict(n_items=-1), dict(n_new=-1), dict(n_slots=-1), dict(null=("items",)), dict(null=("new_params",)),
               dict(null=("lens_state",))):
        assert apply(**kw) == 1, kw
    assert apply(n_items=0) == 0                          # nothing to do: no launch either

    def update(skel=sk, n_views=4, p_max=3, n_rigs=1, n_items=2, n_slots=8, lag=4, prior=1.0, commit=0, null=()):
        ptr = lambda name, k: None if name in null else fake(k)
        return lib.mvmc_live_lengths_update(skel, ptr("kps17", 0), n_views, p_max, ptr("Pmats", 1), n_rigs, ptr("items", 2), n_items,
                                            ptr("rows", 3), ptr("members", 4), ptr("count", 5), n_slots, lag, prior, commit,
                                            ptr("lens_state", 6), ptr("linfo", 7), None)
    assert update(skel=None) == 1
    for kw in (dict(n_views=0), dict(n_views=65), dict(p_max=0), dict(n_rigs=0), dict(n_items=-1), dict(n_slots=-1), dict(lag=-1),
               dict(lag=32), dict(prior=0.0), dict(prior=-1.0), dict(prior=float("nan")), dict(prior=float("inf")), dict(commit=-1)):
        assert update(**kw) == 1, kw
    for name in ("kps17", "Pmats", "items", "rows", "members", "count", "lens_state", "linfo"):
        assert update(null=(name,)) == 1, name
    assert update(n_items=0) == 0


def _row(seed, noise=0.0, scale=None):
    """One row of a scene with its observations: (params (68,), ob (4,16,3), pr (4,3,4), true lengths)."""
    views, Ps, rec, truth = _scene(3, seed=seed)
    p = truth[1].copy()
    true = p[57:68].copy()
    if scale is not None:
        p[57:68] = true * scale
    if noise == 0.0:      # the scene's keypoints carry 2 px noise: project the true pose instead
        from test_body_fit_cpu import _coco
        J = _fk(truth[1])
        views = [None, [_coco(J, Ps[c], [5, 6, 11, 12][c])[None] for c in range(4)]]
    ob, pr = bf.observations(np.zeros(4, int), views[1], Ps)
    return p, ob, pr, true


def test_jacobian_matches_central_differences_of_the_residual():
    rng = np.random.default_rng(3)
    p, ob, pr, _ = _row(2, noise=2.0, scale=1 + rng.normal(0, 0.05, 11))
    res, J = ll.row_terms(p, ob, pr)
    assert res.shape == (2 * 4 * 16,) and J.shape == (2 * 4 * 16, 11)
    num = np.zeros_like(J)
    eps = 1e-6
    for s in range(11):
        a, b = p.copy(), p.copy()
        a[57 + s] += eps
        b[57 + s] -= eps
        num[:, s] = (ll.row_terms(a, ob, pr)[0] - ll.row_terms(b, ob, pr)[0]) / (2 * eps)
    err = np.abs(num - J).max() / np.abs(J).max()
    print(f"\nrelative Jacobian error {err}")
    assert err < 1e-7
    assert np.all(J[:, 7] == 0.0)                           # slot 7: a zero reference direction, no curvature
    # the same residual and normal equations as body_fit_np.len_terms
    root, A = bf.len_basis(p)
    E, H, g = bf.len_terms(root[None], A[None], np.zeros(4, int), pr, ob, p[57:68])
    assert abs(0.5 * res @ res - E) <= 1e-12 * E and np.abs(J.T @ J - H).max() <= 1e-12 * np.abs(H).max()
    assert np.abs(J.T @ res - g).max() <= 1e-12 * np.abs(g).max()


def test_noise_free_rows_at_the_true_pose_return_the_true_lengths():
    st = None
    for seed in range(4):
        p, ob, pr, true = _row(seed)
        if st is None:
            st = ll.LenState(true * 1.2)                    # the prior's mean is 20 % off
            l_star = true
        p[57:68] = l_star                                   # (every scene has the reference lengths)
        res, J = ll.row_terms(p, ob, pr)
        assert np.abs(res).max() < 1e-9                     # the mid-spine observation has weight 0: the rows are exact
        st.A += J.T @ J
        st.b += J.T @ (J @ p[57:68] - res)
    assert np.abs(st.b - st.A @ l_star).max() <= 1e-9 * np.abs(st.b).max()
    l, ok = ll.solve(st.A, st.b, st.l0, 1.0)
    assert ok and np.abs(l - l_star)[CURV].max() < 1e-7
    assert abs(l[7] - st.l0[7]) < 1e-12                     # only the prior holds slot 7
    bad = st.A.copy()
    bad[3, 3] = -1e9
    assert ll.solve(bad, st.b, st.l0, 1.0) == (None, False)


def _tables(n=48, holes=(20, 21, 22), seed=5, skip=()):
    """test_live_smooth_cpu._stream_scene's session with per-frame lengths 5 % off: per delivered frame (f, views_f, meta, params,
    joints), and (rec, truth).  Frames in ``skip`` are not delivered (a jump of the frame index)."""
    views, Ps, rec, truth = _scene(n, seed=seed, holes=holes)
    rng = np.random.default_rng(seed + 100)
    rec = dict(rec)
    rec["params"] = rec["params"].copy()
    rec["params"][:, 57 + CURV] *= 1 + rng.normal(0, 0.05, (len(rec["frames"]), len(CURV)))
    rec["joints"] = np.array([_fk(q) for q in rec["params"]])
    ticks, hits, k = [], 0, 0
    for f in range(n):
        data = f not in holes
        if data:
            hits += 1
            par, jn = rec["params"][k], rec["joints"][k]
            k += 1
        if f not in skip:
            ticks.append((f, views[f], np.array([[7, 2, hits, 0]]), par[None].copy(), jn[None].copy()))
    return ticks, Ps, rec, truth


def _run(stream, ticks):
    emitted, lens = {}, []
    for f, v, meta, par, jn in ticks:
        out = stream.tick(f, v, meta, par, jn)
        for tid, fr, p, j, filled, nv in out["emitted"]:
            emitted[fr] = (p, j, filled)
        lens.append(out.get("lengths", {}).get(7))
    return emitted, lens


def test_streaming_holes_a_jump_and_the_commit():
    ticks, Ps, rec, truth = _tables()
    st = ll.Stream(Ps, 12, 4, 2, W, prior=1.0, commit=20)
    emitted, lens = _run(st, ticks)
    rows = [r for i in lens for r in i["rows"]]
    assert rows == [r for r in range(48 - 4) if r not in (20, 21, 22)][:20]     # each data row once, in order, until the commit
    assert all(i["status"] == 0 for i in lens)
    c = next(k for k, i in enumerate(lens) if i["committed"])
    crow = lens[c]["committed_row"]
    assert lens[c]["contributed"] == 20 and crow == (c + 1) - 4 and lens[-1]["committed_row"] == crow
    done = st.close()[0]
    assert all(np.array_equal(done["params"][r, 57:68], lens[-1]["lengths"]) for r in range(crow, 48))
    assert all(np.array_equal(emitted[f][0][57:68], lens[-1]["lengths"]) for f in range(crow, 44))
    assert not np.array_equal(done["params"][crow - 1, 57:68], lens[-1]["lengths"])
    # an emitted pose was solved against the lengths it carries: the record's final row has the emitted lengths
    assert all(np.array_equal(done["params"][f, 57:68], emitted[f][0][57:68]) for f in range(44))
    # quality: the committed skeleton against the per-frame lengths, the emitted poses against the plain stream's
    true = truth[0, 57:68]
    err_in = np.median(np.abs(rec["params"][:, 57:68] - true)[:, CURV].mean(axis=1))
    err_c = np.abs(lens[-1]["lengths"] - true)[CURV].mean()
    plain, _ = _run(ls.Stream(Ps, 12, 4, 2, W), ticks)
    J_true = np.array([_fk(p) for p in truth])
    mp = lambda em: np.mean([np.linalg.norm(em[f][1] - J_true[f], axis=-1).mean() for f in range(44)])
    print(f"\ncommitted at row {crow}: mean |l - truth| {1e3 * err_c:.2f} mm against {1e3 * err_in:.2f} mm per frame (median); emitted MPJPE "
          f"{1e3 * mp(emitted):.2f} mm against {1e3 * mp(plain):.2f} mm plain")
    assert err_c < err_in
    assert mp(emitted) < mp(plain)
    # a jump of the frame index: frames 30..33 are not delivered.  The missing rows contribute nothing, and neither do the rows from
    # before the jump that had not contributed yet (26..29: the keypoint ring may have lost them)
    ticks_j = _tables(skip=(30, 31, 32, 33))[0]
    st = ll.Stream(Ps, 12, 4, 2, W, prior=1.0, commit=None)
    _, lens = _run(st, ticks_j)
    rows = [r for i in lens for r in i["rows"]]
    assert rows == [r for r in range(44) if r not in (20, 21, 22) and not 26 <= r <= 33]
    assert lens[-1]["committed"] == 0 and lens[-1]["committed_row"] == -1 and lens[-1]["contributed"] == len(rows)
