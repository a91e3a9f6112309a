"""GPU: the live smoother's covariance (live_smoothing.LiveSmoother(covariance="joints"), csrc/mvmc_smooth_window_cov.hip) against the
NumPy restatement's dense inverse (tests/live_smooth_cov_np.py): direct launches on hand-built device state at the identity ages and
emitted rows of tests/test_live_smooth_cov_cpu.py, through update_tables tick by tick on Shelf tables, against mvmc_smooth_cov without
history, nothing else moves, bit identity, the robust loss, a singular factor and malformed items, launch counts, the noise scale.
Window 6, lag 2, 5 views.  The gate is tests/test_live_smooth_cov_cpu.py's TOL (10 x the CPU restatement's banded-against-dense figure)."""
import functools

import numpy as np
import pytest

import live_smooth_cov_np as lc
import live_smooth_np as ls
import smooth_robust_np as rb
from conftest import load_golden
from test_gpu_body_fit import _calibs
from test_gpu_live_smooth import _rec_signature, _shelf_table, _signature
from test_live_smooth_cov_cpu import CASES, TOL, W, WINDOW, identity_rows, rel, window_of
from test_smooth_robust_cpu import LOSS_PX, move_keypoints

pytestmark = pytest.mark.gpu

LAG, RING, TICKS = 2, 66, 12
KW = dict(window=WINDOW, lag=LAG, n_iter=2)


def _T(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _shelf_device():
    """The first 13 Shelf frames ingested on the device and the rig -> (kps17 (13,C,P,17,3), Pm (1,C,3,4)); read only."""
    from multiview_motion_capture_amd import device as dev
    si = load_golden("shelf_inputs.npz")
    k17, _ = dev.ingest(_T(si["kps25"][:13].astype(np.float64)), _T(si["counts"][:13].astype(np.int32)))
    return k17, _T(np.asarray(si["P"], np.float64)[None])


def _hand_state(idns):
    """Identities (test_live_smooth_cov_cpu.identity_rows' dicts) -> the device state a smoother would hold for them, one slot each:
    rows (S,66,68), members (S,66,C), count (S,2)."""
    k17, _ = _shelf_device()
    C, P = k17.shape[1], k17.shape[2]
    S = len(idns)
    rows, mem, cnt = np.zeros((S, RING, 68)), -np.ones((S, RING, C), np.int32), np.zeros((S, 2), np.int32)
    for s, idn in enumerate(idns):
        n = idn["x"].shape[0]
        fr = idn["f0"] + np.arange(n)
        rows[s, :n] = idn["x"]
        mem[s, :n] = np.where(idn["sel"] >= 0, (fr[:, None] * C + np.arange(C)[None]) * P + idn["sel"], -1)
        cnt[s] = (n, idn["f0"])
    return _T(rows), _T(mem), _T(cnt)


def _launch(state, items, full, mu=lc.MU, w=W, **loss):
    from multiview_motion_capture_amd import device as dev
    k17, Pm = _shelf_device()
    jc, pv, ci = dev.smooth_window_cov(k17, Pm, _T(np.array(items, np.int32).reshape(-1, 4)), *state, WINDOW, w, mu, full, **loss)
    return jc.cpu().numpy(), pv.cpu().numpy(), ci.cpu().numpy()


def _six(c):
    return np.stack([c[:, 0, 0], c[:, 0, 1], c[:, 0, 2], c[:, 1, 1], c[:, 1, 2], c[:, 2, 2]], axis=-1)


@functools.lru_cache(maxsize=None)
def _hand_cases():
    """Every (case, Shelf identity) of the CPU test in a slot of its own -> (the identities, items, their dense expectations)."""
    idns, items, exp = [], [], []
    for n, drop, e in CASES:
        for idn in identity_rows(n, drop):
            x, h, obs, prs, first = window_of(idn)
            items.append([len(idns), 0, first + e, len(idns) * WINDOW])
            idns.append(idn)
            exp.append(lc.window_cov(x, h, obs, prs, W, e, blocks="dense"))
    return idns, items, exp


def test_direct_launches_equal_the_dense_inverse_and_full_0_gives_the_same_bits():
    """Hand-built state: identity ages 2, 3, 6 (no history), 7 (one frozen row), 8 and 11 (two); the emitted row last, in the middle and
    free row 0; a missing row in the window, emitted itself or not.  jcov, pvar, edof and E_data within the gate of the dense inverse
    at the same rows, n_res exactly; full=0: the same jcov / pvar bits, NaN edof and n_res."""
    idns, items, exp = _hand_cases()
    state = _hand_state(idns)
    jc, pv, ci = _launch(state, items, True)
    jc0, pv0, ci0 = _launch(state, items, False)
    worst = {}
    for k, ((n, drop, e), x) in enumerate(zip([c for c in CASES for _ in range(2)], exp)):
        m = min(n, WINDOW)
        assert ci[k, 0] == 0.0 and ci[k, 4] == m and ci[k, 5] == e and np.all(ci[k, 6:] == 0.0), (n, drop, e, ci[k])
        assert ci[k, 2] == x["n_res"]                                            # exact
        d = dict(jcov=rel(jc[k], _six(x["jcov"])), pvar=rel(pv[k], x["pvar"]), edof=abs(ci[k, 3] - x["edof"]) / x["edof"],
                 E_data=abs(ci[k, 1] - x["E_data"]) / x["E_data"])
        for q, v in d.items():
            worst[q] = max(worst.get(q, 0.0), v)
        assert all(v <= TOL for v in d.values()), (n, drop, e, d)
        assert np.all(pv[k] > 0) and 0.0 < ci[k, 3] < 39 * m
    print("\ndirect launches against the dense inverse, worst relative differences:", {q: f"{v:.2e}" for q, v in worst.items()})
    assert np.array_equal(jc0, jc) and np.array_equal(pv0, pv)
    assert np.all(np.isnan(ci0[:, 2:4])) and np.array_equal(ci0[:, [0, 1, 4, 5, 6, 7]], ci[:, [0, 1, 4, 5, 6, 7]])


def test_without_history_the_launch_equals_mvmc_smooth_cov_on_the_same_rows():
    """Six rows, window 6: the window IS the offline problem.  mvmc_smooth_blocks + mvmc_smooth_cov on the same rows give every row's
    jcov / pvar, the identity's edof, n_res and E_data; the live launch's emitted row (free rows 0, 3 and 5) within the gate."""
    import torch

    from multiview_motion_capture_amd import device as dev
    k17, Pm = _shelf_device()
    idns = identity_rows(6, None) + identity_rows(6, 3)
    rows, mem, cnt = _hand_state(idns)
    S, n = len(idns), 6
    x = rows[:, :n].reshape(S * n, 68).contiguous()
    members = mem[:, :n].reshape(S * n, -1).contiguous()
    d = x.device
    ctl = torch.zeros((S, 4), dtype=torch.int32, device=d)
    ctl[:, 1] = 1
    blk = torch.empty((2, S * n, 820), dtype=torch.float64, device=d)
    rig = torch.zeros((S * n,), dtype=torch.int32, device=d)
    id_of = _T(np.repeat(np.arange(S, dtype=np.int32), n))
    id_lo = _T((np.arange(S + 1) * n).astype(np.int32))
    jo, po = torch.zeros((S * n, 18, 6), dtype=torch.float64, device=d), torch.zeros((S * n, 39), dtype=torch.float64, device=d)
    co, work = torch.zeros((S, 8), dtype=torch.float64, device=d), torch.empty((S * n, 3940), dtype=torch.float64, device=d)
    dev.smooth_blocks(k17, Pm, rig, members, x, id_of, ctl, blk)
    dev.smooth_cov(x, blk[0], id_lo, W, lc.MU, k17, Pm, rig, members, work, jo, po, co)
    jo, po, co = jo.cpu().numpy().reshape(S, n, 18, 6), po.cpu().numpy().reshape(S, n, 39), co.cpu().numpy()
    assert np.all(co[:, 0] == 0.0)
    worst = 0.0
    for e in (0, 3, 5):
        jc, pv, ci = _launch((rows, mem, cnt), [[s, 0, e, s * WINDOW] for s in range(S)], True)
        for s in range(S):
            assert ci[s, 0] == 0.0 and ci[s, 2] == co[s, 2]
            v = max(rel(jc[s], jo[s, e]), rel(pv[s], po[s, e]), abs(ci[s, 3] - co[s, 3]) / co[s, 3], abs(ci[s, 1] - co[s, 1]) / co[s, 1])
            worst = max(worst, v)
    print(f"\nwindow without history against mvmc_smooth_cov: worst relative difference {worst:.2e}")
    assert worst <= TOL


def test_a_singular_factor_is_status_1_and_a_malformed_item_its_own_status_with_the_neighbours_intact():
    """mu = 0: (a) identities of six rows whose row 3 has no data, all four prior weights 0 (tests/test_gpu_smooth_cov.py's system):
    row 3's pivot block is exactly zero, the Cholesky reports it without dividing -- status 1, NaN outputs, E_data finite.
    (With the default weights mu = 0 is no such case: with history the frozen rows pin the common mode of the knees' twist angles
    and the factor is regular; without history the last pivot is a rounding residue of either sign -- measured on one MI355X: status
    1 at 2 rows, status 0 with a twist variance of 1.6e11 at 6 rows -- so it is not gated.)
    (b) every kind of malformed item between two good ones: slot and rig out of range, an empty slot (n < 1), an emitted row below
    the window and past the last row, a workspace row out of range (13 items: rows 0 .. 77) -- status 6 and NaN, and the good items have the bits they have in
    a launch of their own."""
    holed = identity_rows(6, 3)
    state = _hand_state(holed)
    jc, pv, ci = _launch(state, [[s, 0, 3, s * WINDOW] for s in range(len(holed))], True, mu=0.0, w=(0.0, 0.0, 0.0, 0.0))
    print("\nmu 0, all weights 0: cinfo", ci[:, :6])
    assert np.all(ci[:, 0] == 1.0) and np.all(np.isnan(jc)) and np.all(np.isnan(pv)) and np.all(np.isnan(ci[:, 2:4]))
    assert np.all(np.isfinite(ci[:, 1])) and np.all(ci[:, 1] > 0) and np.all(ci[:, 4] == 6) and np.all(ci[:, 5] == 3)
    # (b) slots 0, 1: 11 rows (free rows 5..10); slot 2: empty
    import torch
    idns = identity_rows(11, None)
    rows, mem, cnt = _hand_state(idns)
    pad = lambda t, fill: torch.cat([t, torch.full((1,) + tuple(t.shape[1:]), fill, dtype=t.dtype, device=t.device)])
    state = (pad(rows, 0.0), pad(mem, -1), pad(cnt, 0))
    good = [[0, 0, 8, 0], [1, 0, 10, 9 * WINDOW]]
    bad = [[3, 0, 8, WINDOW], [-1, 0, 8, 2 * WINDOW], [0, 1, 8, 3 * WINDOW], [0, -1, 8, 4 * WINDOW], [2, 0, 0, 5 * WINDOW],
           [0, 0, 4, 6 * WINDOW], [0, 0, 11, 7 * WINDOW], [0, 0, -2 ** 31, 8 * WINDOW], [0, 0, 8, -1], [0, 0, 8, 12 * WINDOW + 1],
           [0, 0, 8, 2 ** 31 - 1]]
    items = good[:1] + bad[:9] + good[1:] + bad[9:]
    jc, pv, ci = _launch(state, items, True)
    g = [0, 10]
    b = [k for k in range(len(items)) if k not in g]
    assert np.all(ci[b, 0] == 6.0) and np.all(np.isnan(jc[b])) and np.all(np.isnan(pv[b])), ci[:, 0]
    jc1, pv1, ci1 = _launch(state, [[0, 0, 8, 0], [1, 0, 10, WINDOW]], True)
    assert np.all(ci1[:, 0] == 0.0) and np.all(np.isfinite(jc1)) and np.all(np.isfinite(pv1))
    assert np.array_equal(jc[g], jc1) and np.array_equal(pv[g], pv1) and np.array_equal(ci[g], ci1)
    # an identity of one row: nothing was solved
    one = [dict(x=i["x"][:1], sel=i["sel"][:1], f0=i["f0"]) for i in identity_rows(2, None)]
    jc, pv, ci = _launch(_hand_state(one), [[0, 0, 0, 0], [1, 0, 0, WINDOW]], True)
    assert np.all(ci[:, 0] == 2.0) and np.all(np.isnan(jc)) and np.all(np.isnan(pv)) and np.all(ci[:, 4] == 1)


def _cov_signature(out):
    return sorted((tid, c["joint_cov"].tobytes(), c["joint_sigma"].tobytes(), c["param_sigma"].tobytes(), np.float64(c["noise_px"]).tobytes(),
                   np.float64(c["edof"]).tobytes(), c["nres"], c["status"]) for tid, c in out.cov.items())


def _device_window(sm, key, tid):
    """The h + m rows of identity ``tid`` as they stand on the device."""
    idn = sm._sessions[key].ids[tid]
    n = idn.n
    m = min(sm.W, n)
    h = min(2, n - m)
    ring = sm._state()["rows"][idn.slot].cpu().numpy()
    return ring[[r % RING for r in range(n - m - h, n)]]


def _run(rows=range(TICKS), moved=None, stream=None, check=None, **kw):
    """Shelf tables ``rows`` through one session -> (per tick the TickOutput, the closed records, the device state at the end)."""
    from multiview_motion_capture_amd.live_smoothing import LiveSmoother
    si, fx = load_golden("shelf_inputs.npz"), load_golden("shelf_clean_oracle_tracker.npz")
    sm = LiveSmoother(5, 1, **KW, **kw)
    key = sm.open_session(_calibs(si["K"], si["Rt"]))
    outs = []
    for r in rows:
        f, (kps, cnt), meta, params, joints = _shelf_table(si, fx, r)
        if moved is not None:
            kps = moved[r + 1]
        out = sm.update_tables({key: (f, (kps, cnt), meta, params, joints)})[key]
        if stream is not None:
            stream.tick(f, ls.bf.ingest_np(kps[None], cnt[None])[0], meta, params, joints)
            check(sm, key, f, out)
        outs.append(out)
    st = sm._state()
    state = tuple(st[k].clone() for k in ("rows", "members", "count"))
    live = sm.tracklets(key)
    return outs, live, sm.close_session(key), state


def _compare_entry(c, x, worst, what):
    assert c["status"] == x["status"], what
    if x["status"] != 0:
        assert np.all(np.isnan(c["joint_cov"])) and np.all(np.isnan(c["joint_sigma"])) and np.all(np.isnan(c["param_sigma"])), what
        assert c["nres"] == 0 and np.isnan(c["edof"]), what
        return
    assert c["joint_cov"].shape == (18, 3, 3) and np.array_equal(c["joint_cov"], c["joint_cov"].transpose(0, 2, 1)), what
    assert c["joint_sigma"].shape == (18,) and c["param_sigma"].shape == (39,), what
    d = dict(joint_cov=rel(c["joint_cov"], x["joint_cov"]), joint_sigma=rel(c["joint_sigma"], x["joint_sigma"]),
             param_var=rel(c["param_sigma"] ** 2, x["param_sigma"] ** 2), noise_px=abs(c["noise_px"] - x["noise_px"]) / x["noise_px"])
    if np.isfinite(x["edof"]):
        assert c["nres"] == x["n_res"], what
        d["edof"] = abs(c["edof"] - x["edof"]) / x["edof"]
    else:
        assert c["nres"] == 0 and np.isnan(c["edof"]), what
    for q, v in d.items():
        worst[q] = max(worst.get(q, 0.0), v)
    assert all(v <= TOL for v in d.values()), (what, d)


def _ticks_against_the_restatement(what, moved=None, **kw):
    si = load_golden("shelf_inputs.npz")
    st = lc.Stream(si["P"], WINDOW, LAG, KW["n_iter"], W, noise_px=kw.get("noise_px"), blocks="dense")
    worst, seen = {}, dict(entries=0, history=0, filled=0)

    def check(sm, key, f, out):
        assert sorted(out.cov) == sorted(e[0] for e in out.emitted), (what, f)
        for e in out.emitted:
            tid = e[0]
            x = st.cov_at(tid, f, _device_window(sm, key, tid))                 # the restatement AT the device's rows
            _compare_entry(out.cov[tid], x, worst, (what, f, tid))
            seen["entries"] += 1
            seen["history"] += len(st.ids[tid].x) > WINDOW
            seen["filled"] += bool(e[4])
    res = _run(moved=moved, stream=st, check=check, covariance="joints", **kw)
    print(f"\n{what}: {seen['entries']} entries against the restatement, worst relative differences", {q: f"{v:.2e}" for q, v in worst.items()})
    assert seen["entries"] >= 18 and seen["history"] >= 6
    return res, st


def test_every_tick_equals_the_restatement_and_the_records_hold_the_emitted_values():
    (outs, live, done, _), st = _ticks_against_the_restatement("12 Shelf ticks, W 6, lag 2")
    emitted = {}
    for out in outs:
        for e in out.emitted:
            c = out.cov[e[0]]
            assert np.isfinite(c["noise_px"]) and c["noise_px"] > 0 and c["nres"] > 0 and 0 < c["edof"] < 39 * WINDOW
            emitted[(e[0], e[1])] = c
    assert len(done) >= 2 and len(live) == len(done)
    for recs in (live, done):
        for t in recs:
            n = len(t)
            assert t.smooth_joint_sigma.shape == (n, 18) and t.smooth_param_sigma.shape == (n, 39) and t.smooth_noise_px.shape == (n,)
            for k, f in enumerate(t.frame_idxs):
                c = emitted.get((t.track_id, f))
                if c is None:                                                        # never emitted: the last <= lag rows
                    assert k >= n - LAG
                    assert np.all(np.isnan(t.smooth_joint_sigma[k])) and np.all(np.isnan(t.smooth_param_sigma[k])) and np.isnan(t.smooth_noise_px[k])
                else:
                    assert np.array_equal(t.smooth_joint_sigma[k], c["joint_sigma"]) and np.array_equal(t.smooth_param_sigma[k], c["param_sigma"])
                    assert t.smooth_noise_px[k] == c["noise_px"]
            assert np.all(np.isnan(t.smooth_noise_px[n - LAG:])) and np.all(np.isfinite(t.smooth_noise_px[:n - LAG]))


def test_nothing_else_moves():
    """The emitted poses, ``solved``, the live and closed records and the device state rows / members / count are the bits of a
    smoother without covariance, whose outputs and records carry none of the new fields."""
    plain, with_cov = _run(), _run(covariance="joints")
    assert [_signature(o) for o in plain[0]] == [_signature(o) for o in with_cov[0]]
    assert all(len(e) == 6 for o in with_cov[0] for e in o.emitted) and sum(len(o.emitted) for o in with_cov[0]) >= 18
    for a, b in ((plain[1], with_cov[1]), (plain[2], with_cov[2])):
        assert [_rec_signature(t) for t in a] == [_rec_signature(t) for t in b] and len(a) >= 2
        assert all(np.array_equal(t.smooth_final, u.smooth_final) for t, u in zip(a, b))
        assert not any(hasattr(t, f) for t in a for f in ("smooth_joint_sigma", "smooth_param_sigma", "smooth_noise_px"))
    assert all(bool((x == y).all()) for x, y in zip(plain[3], with_cov[3]))
    assert all(o.cov == {} for o in plain[0]) and any(o.cov for o in with_cov[0])


def test_bit_identity_of_the_covariance_alone_among_other_sessions_and_run_to_run():
    from multiview_motion_capture_amd.live_smoothing import LiveSmoother
    si, fx = load_golden("shelf_inputs.npz"), load_golden("shelf_clean_oracle_tracker.npz")
    a = [_cov_signature(o) for o in _run(covariance="joints")[0]]
    assert a == [_cov_signature(o) for o in _run(covariance="joints")[0]] and sum(len(s) for s in a) >= 18      # run to run
    # among three others on shifted rigs at other rows of the tables, one opened late
    sm = LiveSmoother(5, 4, covariance="joints", **KW)
    main = sm.open_session(_calibs(si["K"], si["Rt"]), key="main")
    others = []
    for k in range(3):
        Rt = si["Rt"].copy()
        Rt[:, :, 3] += 0.01 * (k + 1)
        others.append(dict(cal=_calibs(si["K"], Rt), r=20 * (k + 1), open_at=3 * k, key=None))
    sig = []
    for r in range(TICKS):
        tables = {main: _shelf_table(si, fx, r)}
        for q in others:
            if r == q["open_at"]:
                q["key"] = sm.open_session(q["cal"])
            if q["key"] is not None:
                tables[q["key"]] = _shelf_table(si, fx, q["r"])
                q["r"] += 1
        out = sm.update_tables(tables)
        sig.append(_cov_signature(out[main]))
        assert all(o.cov or not o.emitted for o in out.values())
    assert sig == a


def test_under_a_huber_loss_every_tick_equals_the_restatement_on_the_weighted_blocks():
    """15 % of the keypoints moved by 30 - 150 px (tests/test_gpu_smooth_robust.py's contamination), loss="huber" at
    test_smooth_robust_cpu.LOSS_PX: the loss votes keypoints down (the weighted and the plain restatement differ by far more than the
    gate at the same rows), and every entry equals the restatement on smooth_robust_np.data_terms."""
    si = load_golden("shelf_inputs.npz")
    moved = np.array(si["kps25"][:TICKS + 1], copy=True).astype(np.float64)
    move_keypoints(moved, np.random.default_rng(15), 0.15)
    with rb.robust("huber", LOSS_PX):
        (outs, _, _, _), st = _ticks_against_the_restatement("12 contaminated Shelf ticks, huber", moved=moved, loss="huber", loss_px=LOSS_PX)
        tid = sorted(outs[-1].cov)[0]
        robust = st.cov_at(tid, TICKS)
    plain = st.cov_at(tid, TICKS)
    gap = rel(plain["jcov"], robust["jcov"])
    print(f"\nthe plain blocks' jcov at the same rows differs from the weighted blocks' by {gap:.2e} of the largest entry")
    assert gap > 100 * TOL


@pytest.mark.parametrize("S", [1, 5, 16])
def test_one_covariance_launch_per_tick_beside_the_one_window_launch(S, monkeypatch):
    from multiview_motion_capture_amd import _cabi
    from multiview_motion_capture_amd.live_smoothing import LiveSmoother
    si, fx = load_golden("shelf_inputs.npz"), load_golden("shelf_clean_oracle_tracker.npz")
    lib = _cabi.load()
    calls = dict(win=[], cov=[])

    def counted(name, kind):
        orig = getattr(lib, name)

        def f(*a):
            calls[kind].append(int(a[7]))
            return orig(*a)
        monkeypatch.setattr(lib, name, f, raising=False)
    counted("mvmc_smooth_window", "win")
    counted("mvmc_smooth_window_cov", "cov")
    for cov in ("joints", None):
        calls["win"].clear()
        calls["cov"].clear()
        sm = LiveSmoother(5, S, covariance=cov, **KW)
        keys = [sm.open_session(_calibs(si["K"], si["Rt"])) for _ in range(S)]
        for r in range(6):
            before = (len(calls["win"]), len(calls["cov"]))
            out = sm.update_tables({k: _shelf_table(si, fx, r) for k in keys})
            n_emitted = sum(len(o.emitted) for o in out.values())
            assert (n_emitted == 0) == (r < LAG) and n_emitted % S == 0
            assert len(calls["win"]) == before[0] + 1 and calls["win"][-1] == S * int(fx["n_tracks"][r])
            if cov is None or n_emitted == 0:                                      # not asked for, or nothing is emitted: no launch
                assert len(calls["cov"]) == before[1]
            else:
                assert len(calls["cov"]) == before[1] + 1 and calls["cov"][-1] == n_emitted


def test_noise_px_is_a_pure_scale_and_an_estimated_one_is_finite_and_positive():
    """noise_px given: full = 0, edof NaN and nres 0; 2 s doubles every sigma of s (s^2 x 4 and the square root are exact) and both
    have the unit-variance bits of the estimated run, whose noise_px is finite and positive on every Shelf window."""
    one, two, est = (_run(covariance="joints", noise_px=s)[0] for s in (1.5, 3.0, None))
    n = 0
    for a, b, c in zip(one, two, est):
        assert sorted(a.cov) == sorted(b.cov) == sorted(c.cov)
        for tid in a.cov:
            p, q, r = a.cov[tid], b.cov[tid], c.cov[tid]
            assert p["noise_px"] == 1.5 and q["noise_px"] == 3.0 and np.isnan(p["edof"]) and p["nres"] == 0 and p["status"] == 0
            assert np.isfinite(r["noise_px"]) and r["noise_px"] > 0 and np.isfinite(r["edof"]) and r["nres"] > 0
            for f in ("joint_sigma", "param_sigma"):
                assert np.all(np.abs(q[f] - 2.0 * p[f]) <= 2.0 ** -52 * np.abs(q[f])), (tid, f)
                assert np.all(np.abs(r[f] / r["noise_px"] - p[f] / 1.5) <= 4 * 2.0 ** -52 * np.abs(p[f] / 1.5)), (tid, f)
            assert np.all(np.abs(q["joint_cov"] - 4.0 * p["joint_cov"]) <= 2.0 ** -52 * np.abs(q["joint_cov"]))
            n += 1
    assert n >= 18
