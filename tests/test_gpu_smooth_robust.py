"""GPU: the smoothers' robust loss (smoothing.smooth_sequences(loss=...), live_smoothing.LiveSmoother(loss=...); csrc/mvmc_smooth_row.h:
sm_row_block<LOSS>, mvmc_smooth_blocks_robust, mvmc_smooth_obs_weights, mvmc_smooth_window_robust) against its NumPy restatement
(tests/smooth_robust_np.py) on test_gpu_smooth_small.py's 12 Shelf frames with 15 % of the keypoints moved by 30 - 150 px, the weights
launch, loss=None bit for bit, bit identity alone / in a batch / across partitions, the covariance on the weighted blocks, what the
loss buys on the CPU test's contaminated scenes, and the live smoother tick by tick.  Tolerances against the restatement are
tests/test_gpu_smooth.py's, tests/test_gpu_smooth_cov.py's and tests/test_gpu_live_smooth.py's."""
import functools

import numpy as np
import pytest

import live_smooth_np as ls
import smooth_cov_np as sc
import smooth_np as sm
import smooth_robust_np as rb
from conftest import load_golden
from test_body_fit_cpu import _cameras, _Rec
from test_gpu_live_smooth import _compare_record, _compare_tick, _shelf_table, _signature, _Worst
from test_gpu_smooth import _calibs, _compare, _np_records, _same, _weights
from test_gpu_smooth_cov import TOL, _params
from test_gpu_smooth_small import _first, _shelf
from test_smooth_robust_cpu import (EFFECT_KINDS, EFFECT_SEEDS, LOSS_PX, check_effect, data_error, effect_scene, move_keypoints)

pytestmark = pytest.mark.gpu

LOSSES = ("huber", "cauchy")


@functools.lru_cache(maxsize=None)
def _moved_shelf():
    """test_gpu_smooth_small._shelf() with a fixed 15 % of the keypoints of kps25 moved by 30 - 150 px (a copy: the cached clean arrays
    stay as they are); the records are the clean fit's, the smoother's start.  Nothing here is modified afterwards."""
    si, kps, cnt, cal, fitted, _ = _shelf()
    moved = np.array(kps, copy=True)
    hit = move_keypoints(moved, np.random.default_rng(15), 0.15)
    assert 0.13 < hit.mean() < 0.17
    return si, moved, cnt, cal, fitted, sm.bf.ingest_np(moved, cnt)


@functools.lru_cache(maxsize=None)
def _restated(n, drop, loss):
    """The restatement's records of the first n record frames (without frame ``drop``) under ``loss``, and per record its (obs, prs)."""
    si, kps, cnt, cal, fitted, views = _moved_shelf()
    nrec = _np_records(_first(fitted, n, drop))
    with rb.robust(loss, LOSS_PX):
        exp = sm.smooth([views], [si["P"]], [nrec], _weights())[0]
    return exp, sc.problems(views, si["P"], nrec)


def _expected_weights(e, obs, prs, loss, C):
    """The restatement's weights at its own trajectory as the device lays them out: (m, C, 16), NaN without a pair."""
    w = rb.obs_weights(e["params"], obs, prs, loss, LOSS_PX)
    out = np.full((len(w), C, 16), np.nan)
    rows = np.flatnonzero(~e["filled"])
    for k, r in enumerate(rows):
        if w[r] is not None:
            out[r, np.flatnonzero(e["sel"][k] >= 0)] = w[r]
    return out


def test_the_contamination_bites():
    for loss in LOSSES:
        exp, probs = _restated(11, 5, loss)
        w = np.concatenate([_expected_weights(e, *p, loss, 5).ravel() for e, p in zip(exp, probs)])
        w = w[~np.isnan(w)]
        print(f"\n{loss}: {w.size} pairs, {(w < 0.5).sum()} with w < 0.5, {(w == 1.0).sum()} with w == 1")
        assert (w < 0.5).sum() >= 20 and w.max() > 0.5
        if loss == "huber":
            assert (w == 1.0).sum() >= 20


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("n,drop", [(2, None), (3, None), (6, 3), (11, 5)])
def test_device_equals_the_restatement(n, drop, loss):
    from multiview_motion_capture_amd.smoothing import smooth_tracklets
    si, kps, cnt, cal, fitted, _ = _moved_shelf()
    recs = _first(fitted, n, drop)
    got = smooth_tracklets(recs, kps, cnt, cal, loss=loss)
    exp, _ = _restated(n, drop, loss)
    for t in got:
        print(f"identity {t.track_id}: {len(t)} rows, E {np.array2string(t.smooth_cost, precision=3)}, trials {t.smooth_trials}")
    assert any(len(t.smooth_trials) >= 1 for t in got)
    _compare(got, exp, f"{loss}, {n} rows" + ("" if drop is None else f", row {drop} without data"))


@pytest.mark.parametrize("loss", LOSSES)
def test_the_weights_launch_and_the_records_weights(loss):
    import torch

    from multiview_motion_capture_amd import device as dev
    from multiview_motion_capture_amd.smoothing import smooth_tracklets
    si, kps, cnt, cal, fitted, _ = _moved_shelf()
    exp, probs = _restated(6, 3, loss)
    C, P = kps.shape[1], kps.shape[2]
    d = torch.device("cuda:0")
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(d)
    xs, mems, want = [], [], []
    for e, (obs, prs) in zip(exp, probs):
        sel = -np.ones((len(e["frames"]), C), np.int64)
        sel[~e["filled"]] = e["sel"]
        mems.append(np.where(sel >= 0, (e["frames"][:, None] * C + np.arange(C)[None]) * P + sel, -1).astype(np.int32))
        xs.append(e["params"])
        want.append(_expected_weights(e, obs, prs, loss, C))
    want = np.concatenate(want)
    k17, _ = dev.ingest(T(kps), T(cnt))
    Pm = T(np.array([[np.asarray(c.P, np.float64).reshape(3, 4) for c in cal]]))
    x, mem = T(np.concatenate(xs)), T(np.concatenate(mems))
    rig = torch.zeros((x.shape[0],), dtype=torch.int32, device=d)
    got = dev.smooth_obs_weights(k17, Pm, rig, mem, x, loss, LOSS_PX).cpu().numpy()
    assert got.shape == want.shape == (x.shape[0], C, 16)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    worst = float(np.abs(got[ok] - want[ok]).max())
    print(f"\n{loss}: {int(ok.sum())} pairs, weights {got[ok].min():.3g} .. {got[ok].max():.3g}, worst difference {worst:.2e}")
    assert worst <= 1e-9 and int(ok.sum()) >= 300 and np.all(np.isnan(got[3])) and np.all(got[ok] > 0) and np.all(got[ok] <= 1)
    ones = dev.smooth_obs_weights(k17, Pm, rig, mem, x, None, None).cpu().numpy()          # loss=None: 1 where there is a pair
    assert np.array_equal(np.isnan(ones), np.isnan(want)) and np.all(ones[ok] == 1.0)
    # the records: (n, C, 16), rows as poses, NaN rows where the frame was filled; the pattern is the restatement's
    at = 0
    full = smooth_tracklets(_first(fitted, 6, 3), kps, cnt, cal, loss=loss)
    for t in full:
        w = t.smooth_obs_weight
        assert w.shape == (len(t), C, 16) and np.all(np.isnan(w[t.smooth_filled])) and t.smooth_filled[3]
        assert np.array_equal(np.isnan(w), np.isnan(want[at:at + len(t)]))
        at += len(t)
    # fill_gaps=False leaves the filled rows out; a one-frame record has nothing solved: NaN
    for t, u in zip(full, smooth_tracklets(_first(fitted, 6, 3), kps, cnt, cal, loss=loss, fill_gaps=False)):
        assert len(u) == 5 and np.array_equal(u.smooth_obs_weight, t.smooth_obs_weight[~t.smooth_filled], equal_nan=True)
    one = smooth_tracklets(_first(fitted[:1], 1), kps, cnt, cal, loss=loss)[0]
    assert one.smooth_obs_weight.shape == (1, C, 16) and np.all(np.isnan(one.smooth_obs_weight))


def test_loss_none_is_the_call_without_the_argument_and_a_huge_huber_equals_it():
    from multiview_motion_capture_amd.smoothing import smooth_tracklets
    si, kps, cnt, cal, fitted, _ = _moved_shelf()
    recs = _first(fitted, 11, 5)
    tm0, tm1 = {}, {}
    plain = smooth_tracklets(recs, kps, cnt, cal, timings=tm0)
    none = smooth_tracklets(recs, kps, cnt, cal, loss=None, loss_px=3.0, timings=tm1)
    _same(plain, none)
    assert set(tm0) == set(tm1) and "weights" not in tm1
    assert not any(hasattr(t, "smooth_obs_weight") for t in plain + none)
    tm2 = {}
    big = smooth_tracklets(recs, kps, cnt, cal, loss="huber", loss_px=1e12, timings=tm2)
    assert set(tm2) == set(tm0) | {"weights"} and tm2["weights"] > 0.0
    worst = 0.0
    for t, u in zip(plain, big):
        assert t.smooth_trials == u.smooth_trials and t.frame_idxs == u.frame_idxs
        worst = max(worst, float(np.abs(_params(t) - _params(u)).max()))
        assert np.abs(t.smooth_cost - u.smooth_cost).max() <= 1e-12 * np.abs(t.smooth_cost).max()
        w = u.smooth_obs_weight
        assert np.all(w[~np.isnan(w)] == 1.0)
    print("\nhuber at loss_px = 1e12 against loss=None: parameters differ by", worst)
    assert worst <= 1e-12


@pytest.mark.parametrize("loss", LOSSES)
def test_bit_identity_alone_beside_the_other_identity_and_across_partitions(loss):
    from multiview_motion_capture_amd.smoothing import smooth_tracklets
    si, kps, cnt, cal, fitted, _ = _moved_shelf()
    recs = _first(fitted, 11, 5)
    assert len(recs) >= 2
    both = smooth_tracklets(recs, kps, cnt, cal, loss=loss)
    split = smooth_tracklets(recs, kps, cnt, cal, loss=loss, max_work_bytes=12 * 48 * 1024)      # 11 rows fit, 22 do not
    _same(both, split)
    _same(both, smooth_tracklets(recs, kps, cnt, cal, loss=loss))
    for k, t in enumerate(both):
        alone = smooth_tracklets([recs[k]], kps, cnt, cal, loss=loss)
        assert np.array_equal(alone[0].smooth_select, t.smooth_select), "the selection of an identity alone differs: not this test's case"
        _same([t], alone)
        for u in (split[k], alone[0]):
            assert np.array_equal(t.smooth_obs_weight, u.smooth_obs_weight, equal_nan=True)


def test_the_covariance_on_the_weighted_blocks():
    """covariance="joints" with "cauchy" on the 6-row problem with a row without data, against the restatement's DENSE inverse of
    J^T W J + the prior at the device's trajectory: test_gpu_smooth_cov.py's gate."""
    from multiview_motion_capture_amd.smoothing import smooth_tracklets
    si, kps, cnt, cal, fitted, views = _moved_shelf()
    recs = _first(fitted, 6, 3)
    got = smooth_tracklets(recs, kps, cnt, cal, covariance="joints", loss="cauchy")
    probs = sc.problems(views, si["P"], _np_records(recs))
    plain = smooth_tracklets(recs, kps, cnt, cal, loss="cauchy")
    _same(got, plain)
    assert len(got) == len(probs) >= 2
    for t, (obs, prs) in zip(got, probs):
        x = _params(t)
        assert t.smooth_cov_status == 0
        with rb.robust("cauchy", LOSS_PX):
            e = sc.covariance(x, obs, prs, _weights(), blocks="dense")
        quad = sc.covariance(x, obs, prs, _weights(), blocks="dense")
        jc, pv = t.smooth_joint_cov, t.smooth_param_sigma ** 2
        d = dict(joint_cov=np.abs(jc - e["joint_cov"]).max() / np.abs(e["joint_cov"]).max(),
                 param_var=np.abs(pv - e["param_sigma"] ** 2).max() / np.abs(e["param_sigma"] ** 2).max(),
                 edof=abs(t.smooth_edof - e["edof"]) / e["edof"], noise_px=abs(t.smooth_noise_px - e["noise_px"]) / e["noise_px"])
        print(f"\nidentity {t.track_id}: relative differences from the dense inverse " + ", ".join(f"{k} {v:.2e}" for k, v in d.items())
              + f"; noise {t.smooth_noise_px:.2f} px under the loss, {quad['noise_px']:.2f} px from the quadratic cost at the same x")
        assert t.smooth_nres == e["n_res"] and all(v <= TOL for v in d.values()), d
        assert abs(t.smooth_cost[2] - e["E_data"]) <= 1e-9 * e["E_data"]
        assert t.smooth_noise_px < quad["noise_px"]       # the documented bias: rho <= 1/2 e^2


def _effect_sequence(seed, kind):
    """test_smooth_robust_cpu.effect_scene as smooth_tracklets takes it: P = 1, Calibs from _cameras()' K and P."""
    from multiview_motion_capture_amd.common import Calib
    views, Ps, rec, J_true = effect_scene(seed, kind)
    kps = np.array([[v for v in row] for row in views])                    # (F, C, 1, 17, 3)
    K = np.array([[1000.0, 0, 500], [0, 1000.0, 400], [0, 0, 1.0]])
    assert np.array_equal(Ps, _cameras())
    cal = [Calib.from_k_rt(K, np.linalg.solve(K, P)) for P in Ps]
    return kps, np.ones(kps.shape[:2], np.int32), cal, _Rec(rec["frames"], rec["params"], rec["joints"]), J_true


def test_what_the_loss_buys_on_the_cpu_tests_scenes():
    """The three gates of test_smooth_robust_cpu.test_what_the_loss_buys_on_contaminated_keypoints through smooth_tracklets."""
    from multiview_motion_capture_amd.smoothing import smooth_tracklets
    err = {}
    for kind in EFFECT_KINDS:
        for seed in EFFECT_SEEDS:
            kps, cnt, cal, rec, J_true = _effect_sequence(seed, kind)
            for loss in (None,) + LOSSES:
                t = smooth_tracklets([rec], kps, cnt, cal, loss=loss)[0]
                err[kind, seed, loss] = data_error([q[2].keypoints for q in t.poses], t.smooth_filled, J_true)
        print(f"\n{kind or 'clean'}: " + "; ".join(f"{loss or 'None'} " + " ".join(f"{1e3 * err[kind, s, loss]:.1f}" for s in EFFECT_SEEDS)
                                                   for loss in (None,) + LOSSES) + " mm (seeds 5 6 7)")
    check_effect(err)


def _moved_table(si, fx, r, moved25):
    f, (_, cnt), meta, params, joints = _shelf_table(si, fx, r)
    return f, (moved25[r + 1], cnt), meta, params, joints


def test_live_equals_the_restatement_after_every_tick():
    """Shelf rows 60 - 91 (identity 2 lives for one row, identity 3 misses rows 87, 89 and 90 inside its window), the same
    contamination, window 6, lag 2, 2 trials, "cauchy": after every tick and for the closed records, test_gpu_live_smooth.py's gates."""
    from multiview_motion_capture_amd.live_smoothing import LiveSmoother
    si, fx = load_golden("shelf_inputs.npz"), load_golden("shelf_clean_oracle_tracker.npz")
    moved25 = np.array(si["kps25"][:101], copy=True)
    move_keypoints(moved25, np.random.default_rng(15), 0.15)
    kw = dict(window=6, lag=2, n_iter=2)
    smr = LiveSmoother(5, 1, loss="cauchy", **kw)
    key = smr.open_session(_calibs(si["K"], si["Rt"]))
    st = ls.Stream(si["P"], kw["window"], kw["lag"], kw["n_iter"], _weights())
    worst, filled, solved = _Worst(), 0, 0
    with rb.robust("cauchy", LOSS_PX):
        for r in range(60, 92):
            f, (kps, cnt), meta, params, joints = _moved_table(si, fx, r, moved25)
            got = smr.update_tables({key: (f, (kps, cnt), meta, params, joints)})[key]
            exp = st.tick(f, ls.bf.ingest_np(kps[None], cnt[None])[0], meta, params, joints)
            _compare_tick(got, exp, worst, f"row {r}")
            filled += sum(1 for e in got.emitted if e[4])
            solved += sum(1 for s in got.solved.values() if len(s["trials"]) >= 1)
            if r % 10 == 9:
                for t, e in zip(smr.tracklets(key), st.records()):
                    _compare_record(t, e, worst, f"records after row {r}")
                    assert not hasattr(t, "smooth_obs_weight")          # the live path sets no weights attribute
        for t, e in zip(smr.close_session(key), st.close()):
            _compare_record(t, e, worst, "closed")
    worst.check("Shelf rows 60-91 with moved keypoints, W 6, lag 2, 2 trials, cauchy")
    assert filled >= 1 and solved >= 50


def test_live_loss_none_is_the_smoother_without_the_argument():
    from multiview_motion_capture_amd.live_smoothing import LiveSmoother
    si, fx = load_golden("shelf_inputs.npz"), load_golden("shelf_clean_oracle_tracker.npz")
    cal = _calibs(si["K"], si["Rt"])
    kw = dict(window=6, lag=2, n_iter=2)

    def run(**more):
        s = LiveSmoother(5, 1, **kw, **more)
        key = s.open_session(cal)
        return [_signature(s.update_tables({key: _shelf_table(si, fx, r)})[key]) for r in range(60, 75)]
    plain = run()
    assert run(loss=None, loss_px=3.0) == plain
    assert run(loss="cauchy") != plain
