"""GPU: the fixed-lag live smoother (multiview_motion_capture_amd/live_smoothing.py, csrc/mvmc_smooth_window.hip) against its NumPy
restatement (tests/live_smooth_np.py) tick by tick on Shelf tables and through LivePool on synthetic scene walks, bit-identity (alone
against among other sessions, run to run, a failed session untouched), one window launch per tick, ground truth on held-out synthetic
scene walks, and the finished records into BVH.  Tolerances against the restatement are tests/test_gpu_smooth.py's."""
import numpy as np
import pytest

import live_smooth_np as ls
from conftest import load_golden
from test_gpu_body_fit import _calibs, _raw_slot_maps
from test_gpu_smooth import _person, _weights

pytestmark = pytest.mark.gpu


def _p68(q):
    return np.concatenate([np.ravel(q.root), np.ravel(q.euler_angles), np.ravel(q.bone_lens)])


class _Worst:
    def __init__(self):
        self.params = self.joints = self.cost = 0.0

    def rows(self, P, J, eP, eJ):
        self.params = max(self.params, float(np.abs(np.asarray(P) - eP).max()))
        self.joints = max(self.joints, float(np.abs(np.asarray(J) - eJ).max()))

    def check(self, what):
        print(f"\n{what}: worst differences from the restatement", dict(params=self.params, joints=self.joints, cost=self.cost))
        assert self.params <= 1e-9 and self.cost <= 1e-9 and self.joints <= 1e-8


def _compare_record(t, e, worst, what):
    assert t.track_id == e["track_id"] and t.frame_idxs == e["frames"].tolist(), (what, t.track_id)
    assert np.array_equal(t.smooth_filled, e["filled"]) and np.array_equal(t.smooth_views, e["views"]), (what, t.track_id)
    assert np.array_equal(t.smooth_select, e["sel"]) and np.array_equal(t.smooth_final, e["final"]), (what, t.track_id)
    worst.rows([_p68(q[1]) for q in t.poses], [q[2].keypoints for q in t.poses], e["params"], e["joints"])


def _compare_tick(got, exp, worst, what):
    assert [(e[0], e[1], e[4], e[5]) for e in got.emitted] == [(e[0], e[1], e[4], e[5]) for e in exp["emitted"]], what
    for g, e in zip(got.emitted, exp["emitted"]):
        worst.rows(_p68(g[2]), g[3].keypoints, e[2], e[3])
    assert sorted(got.solved) == sorted(exp["solved"]), what
    for tid, info in exp["solved"].items():
        s = got.solved[tid]
        assert s["trials"] == info["trace"], (what, tid, s["trials"], info["trace"])
        for a, b in zip(s["cost"], [*info["E0"], *info["E"]]):
            worst.cost = max(worst.cost, abs(a - b) / max(abs(b), 1e-300))
    assert len(got.finished) == len(exp["finished"]), what
    for t, e in zip(got.finished, exp["finished"]):
        _compare_record(t, e, worst, what)


def _shelf_table(si, fx, r):
    """Row r of the oracle tracker's tables (Shelf frame r + 1) as update_tables takes it."""
    n = int(fx["n_tracks"][r])
    return (r + 1, (si["kps25"][r + 1], si["counts"][r + 1].astype(np.int32)), fx["meta"][r, :n], fx["params"][r, :n], fx["joints"][r, :n])


def _stream_shelf(r0, r1, **kw):
    from multiview_motion_capture_amd.live_smoothing import LiveSmoother
    si, fx = load_golden("shelf_inputs.npz"), load_golden("shelf_clean_oracle_tracker.npz")
    sm = LiveSmoother(5, 2, **kw)
    key = sm.open_session(_calibs(si["K"], si["Rt"]))
    st = ls.Stream(si["P"], kw["window"], kw["lag"], kw["n_iter"], _weights())
    worst = _Worst()
    seen = dict(history=False, filled=[], finished={}, emitted=0)
    for r in range(r0, r1):
        f, (kps, cnt), meta, params, joints = _shelf_table(si, fx, r)
        got = sm.update_tables({key: (f, (kps, cnt), meta, params, joints)})[key]
        exp = st.tick(f, ls.bf.ingest_np(kps[None], cnt[None])[0], meta, params, joints)
        _compare_tick(got, exp, worst, f"row {r}")
        seen["history"] |= any(len(idn.x) > kw["window"] + 2 for idn in st.ids.values())
        seen["filled"] += [(e[0], e[1] - 1) for e in got.emitted if e[4]]          # (identity, table row)
        seen["emitted"] += len(got.emitted)
        for t in got.finished:
            seen["finished"][t.track_id] = t
        if r % 10 == 9 or r == r1 - 1:
            for t, e in zip(sm.tracklets(key), st.records()):
                _compare_record(t, e, worst, f"records after row {r}")
    done = sm.close_session(key)
    for t, e in zip(done, st.close()):
        _compare_record(t, e, worst, "closed")
    return worst, seen, done


def test_shelf_tables_equal_the_restatement_after_every_tick():
    worst, seen, done = _stream_shelf(0, 100, window=12, lag=6, n_iter=2)
    worst.check("Shelf rows 0-99, W 12, lag 6, 2 trials")
    # every case of the input was seen: frozen history; identity 3 misses rows 87, 89, 90 inside its window; identity 2 lives for one
    # row; identity 4 has data at row 95, stays without data at 96 and 97, then dies: its trailing missing rows are dropped
    assert seen["history"]
    assert [(3, r) for r in (87, 89, 90)] == [x for x in seen["filled"] if x[0] == 3]
    assert seen["finished"][2].frame_idxs == [66]
    assert seen["finished"][4].frame_idxs == [96]
    assert sorted(t.track_id for t in done) == [0, 1, 3] and all(len(t) >= 30 for t in done)
    assert all(t.smooth_final.all() and not t.smooth_filled[-1] for t in done)


def test_shelf_tables_at_the_filter_end_of_the_parameter_range():
    worst, seen, _ = _stream_shelf(60, 100, window=8, lag=0, n_iter=1)
    worst.check("Shelf rows 60-99, W 8, lag 0, 1 trial")
    assert seen["emitted"] >= 100 and (4, 96) in seen["filled"] and (4, 97) in seen["filled"]     # emitted before it died: stays emitted
    assert seen["finished"][4].frame_idxs == [96]


def _signature(out):
    return ([(e[0], e[1], _p68(e[2]).tobytes(), e[3].keypoints.tobytes(), e[4], e[5]) for e in out.emitted],
            sorted((tid, s["cost"].tobytes(), tuple(s["trials"]), s["stop"]) for tid, s in out.solved.items()),
            [_rec_signature(t) for t in out.finished])


def _rec_signature(t):
    return (t.track_id, tuple(t.frame_idxs), b"".join(_p68(q[1]).tobytes() + q[2].keypoints.tobytes() for q in t.poses),
            t.smooth_filled.tobytes(), t.smooth_views.tobytes(), t.smooth_select.tobytes())


def test_bit_identity_alone_among_other_sessions_run_to_run_and_a_failed_session_is_untouched():
    from multiview_motion_capture_amd.live_smoothing import LiveSmoother
    si, fx = load_golden("shelf_inputs.npz"), load_golden("shelf_clean_oracle_tracker.npz")
    cal = _calibs(si["K"], si["Rt"])
    kw = dict(window=8, lag=2, n_iter=2)
    rows = list(range(60, 100))

    def alone():
        sm = LiveSmoother(5, 1, **kw)
        key = sm.open_session(cal)
        sig = [_signature(sm.update_tables({key: _shelf_table(si, fx, r)})[key]) for r in rows]
        return sig, [_rec_signature(t) for t in sm.close_session(key)]
    a, b = alone(), alone()
    assert a == b                                                                   # run to run
    # among four others with other rigs (shifted cameras), staggered opens, a close, ticks the session sits out, a failed tick
    others = []
    for k in range(4):
        Rt = si["Rt"].copy()
        Rt[:, :, 3] += 0.01 * (k + 1)
        others.append(dict(cal=_calibs(si["K"], Rt), r=10 * k, open_at=2 * k, close_at=25 if k == 1 else None, key=None))
    sm = LiveSmoother(5, 5, **kw)
    main = sm.open_session(cal, key="main")
    sig, at, tick = [], 0, 0
    while at < len(rows):
        tables = {}
        for q in others:
            if tick == q["open_at"]:
                q["key"] = sm.open_session(q["cal"])
            if q["key"] is not None and tick == q["close_at"]:
                sm.close_session(q["key"])
                q["key"] = None
            if q["key"] is not None:
                tables[q["key"]] = _shelf_table(si, fx, q["r"])
                q["r"] += 1
        if tick % 7 == 3:                                                            # the session sits this tick out
            sm.update_tables(tables)
        elif tick % 7 == 5:                                                          # named in failed=: not stepped, state bit for bit
            st = sm._state()
            slots = [i.slot for i in sm._sessions[main].ids.values()]
            before = (st["rows"][slots].clone(), st["members"][slots].clone(), st["count"][slots].clone(), sm._sessions[main].f_last)
            tables[main] = _shelf_table(si, fx, rows[at])
            out = sm.update_tables(tables, failed={main})
            assert main not in out and sm._sessions[main].f_last == before[3]
            assert all(bool((x == y).all()) for x, y in zip(before[:3], (st["rows"][slots], st["members"][slots], st["count"][slots])))
        else:
            tables[main] = _shelf_table(si, fx, rows[at])
            sig.append(_signature(sm.update_tables(tables)[main]))
            at += 1
        tick += 1
    assert tick > len(rows) + 8 and sum(q["key"] is not None for q in others) == 3
    assert (sig, [_rec_signature(t) for t in sm.close_session(main)]) == a


def _synth_rig(seed, n_frames, occlusion=0.3):
    from multiview_motion_capture_amd import synth
    g = synth.generate(n_frames, 5, 4, seed, walk="scene", occlusion=occlusion)
    return g, _calibs(g["K"], g["Rt"])


def _pool_frames(g, cal, f):
    """Frame f as FrameData of the device-ingested poses (what LivePool's solo route packs back)."""
    import torch

    from multiview_motion_capture_amd import device as dev
    from multiview_motion_capture_amd.live import _frame_data
    k17, c17 = dev.ingest(torch.from_numpy(g["kps25"][f:f + 1]).cuda(), torch.from_numpy(g["counts"][f:f + 1].astype(np.int32)).cuda())
    return _frame_data(f, k17[0].cpu().numpy(), c17[0].cpu().numpy(), cal)


def _table_of(sess, fi):
    """The restatement's table from the pool's public records."""
    trs = list(sess.tracklets)
    meta = np.array([[t.track_id, t.state.value, t.hits, len(t)] for t in trs]).reshape(len(trs), 4)
    return (meta, np.array([_p68(t.poses[-1][1]) for t in trs]).reshape(len(trs), 68),
            np.array([t.poses[-1][2].keypoints for t in trs]).reshape(len(trs), 18, 3))


def test_through_the_live_pool_equals_the_restatement_and_both_routes_give_the_same_bits():
    from multiview_motion_capture_amd.live import LivePool
    from multiview_motion_capture_amd.live_smoothing import LiveSmoother
    F, kw = 40, dict(window=8, lag=3, n_iter=2)
    rigs = [_synth_rig(seed, F) for seed in (71, 72)]
    pool = LivePool(5, 2)
    sm = LiveSmoother.for_pool(pool, **kw)
    pa = LivePool(5, 2)
    sa = LiveSmoother.for_pool(pa, **kw)
    sids = [pool.open_session(cal) for _, cal in rigs]
    assert [pa.open_session(cal) for _, cal in rigs] == sids
    sts = [ls.Stream(g["P"], kw["window"], kw["lag"], kw["n_iter"], _weights()) for g, _ in rigs]
    worst = _Worst()
    missing_in_window, same_records = 0, True
    for f in range(F):
        frames = {sid: (f, _pool_frames(g, cal, f)) for sid, (g, cal) in zip(sids, rigs)}
        pool.update_4d(frames)
        out = sm.update_4d(frames)
        k25 = np.stack([g["kps25"][f] for g, _ in rigs]).astype(np.float64)
        cn = np.stack([g["counts"][f] for g, _ in rigs]).astype(np.int32)
        pa.update_4d_arrays(sids, [f] * 2, k25, cn)
        out_a = sa.update_4d_arrays(sids, [f] * 2, k25, cn)
        for i, sid in enumerate(sids):
            g = rigs[i][0]
            meta, params, joints = _table_of(pool.session(sid), f)
            exp = sts[i].tick(f, ls.bf.ingest_np(g["kps25"][f:f + 1], g["counts"][f:f + 1])[0], meta, params, joints)
            _compare_tick(out[sid], exp, worst, f"session {sid}, frame {f}")
            missing_in_window += sum(1 for idn in sts[i].ids.values() if not all(idn.data[-kw["window"]:]))
            ma, pa_, ja = _table_of(pa.session(sid), f)
            same_records &= np.array_equal(meta, ma) and np.array_equal(params, pa_) and np.array_equal(joints, ja)
            if same_records:
                assert _signature(out[sid]) == _signature(out_a[sid]), (sid, f)
    worst.check("two synthetic rigs through LivePool")
    assert missing_in_window >= 1, "the run holds no missing row inside a window: pick other seeds"
    assert same_records, "the pool's two routes gave different records: the route comparison did not cover the run"
    for i, sid in enumerate(sids):
        for t, e in zip(sm.close_session(sid), sts[i].close()):
            _compare_record(t, e, worst, "closed")
    worst.check("closed records")


@pytest.mark.parametrize("S", [1, 5, 16])
def test_one_window_launch_per_tick_whatever_the_number_of_sessions(S, monkeypatch):
    from multiview_motion_capture_amd import _cabi
    from multiview_motion_capture_amd.live_smoothing import LiveSmoother
    si, fx = load_golden("shelf_inputs.npz"), load_golden("shelf_clean_oracle_tracker.npz")
    lib = _cabi.load()
    orig, calls = lib.mvmc_smooth_window, []

    def counted(*a):
        calls.append(int(a[7]))
        return orig(*a)
    monkeypatch.setattr(lib, "mvmc_smooth_window", counted, raising=False)
    sm = LiveSmoother(5, S, window=6, lag=2, n_iter=2)
    keys = [sm.open_session(_calibs(si["K"], si["Rt"])) for _ in range(S)]
    for r in range(8):
        before = len(calls)
        sm.update_tables({k: _shelf_table(si, fx, r) for k in keys})
        assert len(calls) == before + 1 and calls[-1] == S * int(fx["n_tracks"][r])


def _pool_run(seed, F=300, **kw):
    """One synthetic rig through LivePool + LiveSmoother -> (g, emitted {(tid, frame): (joints, filled)}, smoother records, pool records)."""
    from multiview_motion_capture_amd.live import LivePool
    from multiview_motion_capture_amd.live_smoothing import LiveSmoother
    g, cal = _synth_rig(seed, F)
    pool = LivePool(5, 1)
    sm = LiveSmoother.for_pool(pool, **kw)
    sid = pool.open_session(cal)
    emitted, recs = {}, []
    for f in range(F):
        frames = {sid: (f, _pool_frames(g, cal, f))}
        pool.update_4d(frames)
        out = sm.update_4d(frames)[sid]
        for e in out.emitted:
            emitted[(e[0], e[1])] = (e[3].keypoints, e[4])
        recs += out.finished
    recs += sm.close_session(sid)
    s = pool.session(sid)
    return g, cal, emitted, recs, list(s.dead_tracklets) + list(s.tracklets)


def test_ground_truth_of_held_out_synthetic_scene_walks():
    """Default parameters (W 24, lag 8, 2 trials), two 5 x 4 scene walks of 300 frames, occlusion 0.3, seeds 81 and 82 (the weight sweep
    uses 51, 52; tests/test_gpu_smooth.py 31-33, 41-43, 61, 62), through LivePool.  The emitted poses against the tracker's raw poses of
    the same frames (MPJPE on data rows, jitter over runs of three data rows) and, on the filled rows, against holding the previous
    pose.  Each must be below its baseline; the gate is the tighter of 1.0 and 1.25 x the observed ratio.  The offline smoother's ratios
    on the finished records are printed beside them (the ceiling, not a gate).
    Measured on one MI355X (1,968 data rows, 72 filled rows, 1,815 triples): data rows 9.24 mm emitted against 9.97 mm raw (ratio 0.927;
    offline 0.927), jitter 45.9 against 54.9 mm/frame^2 (0.836; offline 0.836), filled rows 28.2 mm against 36.5 mm holding the previous
    pose (0.774; offline 0.774).  Gates: 1.0, 1.0 and 1.25 x 0.774 = 0.967."""
    from multiview_motion_capture_amd.smoothing import smooth_sequences
    acc = {k: [] for k in ("data_s", "data_r", "jit_s", "jit_r", "fill_s", "fill_h", "off_data", "off_jit_s", "off_fill")}
    for seed in (81, 82):
        g, cal, emitted, recs, raw_recs = _pool_run(seed)
        maps = _raw_slot_maps(g)
        raw = {t.track_id: t for t in raw_recs}
        off = {t.track_id: t for t in smooth_sequences([(g["kps25"], g["counts"], cal)], [raw_recs])[0]}
        for t in recs:
            if len(t) < 60:
                continue
            person = _person(t, g, maps, t.smooth_select)
            if person < 0:
                continue
            rt = raw[t.track_id]
            rj = {f: q[2].keypoints for f, q in zip(rt.frame_idxs, rt.poses)}
            oj = {f: q[2].keypoints for f, q in zip(off[t.track_id].frame_idxs, off[t.track_id].poses)}
            fr = [f for f in t.frame_idxs if (t.track_id, f) in emitted]
            gt = lambda f: g["gt_joints"][f, person]
            err = lambda J, f: float(np.linalg.norm(J - gt(f), axis=-1).mean())
            hold = None
            for f in fr:
                J, filled = emitted[(t.track_id, f)]
                if not filled:
                    acc["data_s"].append(err(J, f))
                    acc["data_r"].append(err(rj[f], f))
                    acc["off_data"].append(err(oj[f], f))
                    hold = rj[f]
                elif hold is not None:
                    acc["fill_s"].append(err(J, f))
                    acc["fill_h"].append(err(hold, f))
                    acc["off_fill"].append(err(oj[f], f))
            for a, b, c in zip(fr, fr[1:], fr[2:]):
                if c - a == 2 and not (emitted[(t.track_id, a)][1] or emitted[(t.track_id, b)][1] or emitted[(t.track_id, c)][1]):
                    j2 = lambda S: float(np.linalg.norm(S[c] - 2 * S[b] + S[a], axis=-1).mean())
                    acc["jit_s"].append(j2({f: emitted[(t.track_id, f)][0] for f in (a, b, c)}))
                    acc["jit_r"].append(j2(rj))
                    acc["off_jit_s"].append(j2(oj))
    m = {k: float(np.mean(v)) for k, v in acc.items()}
    ratios = dict(data=m["data_s"] / m["data_r"], jitter=m["jit_s"] / m["jit_r"], filled=m["fill_s"] / m["fill_h"])
    offline = dict(data=m["off_data"] / m["data_r"], jitter=m["off_jit_s"] / m["jit_r"], filled=m["off_fill"] / m["fill_h"])
    print("\nground truth (m):", m, "\nemitted / baseline:", ratios, "\noffline smoother / baseline (the ceiling):", offline,
          "\nrows:", {k: len(v) for k, v in acc.items()})
    assert len(acc["fill_s"]) >= 10 and len(acc["data_s"]) >= 1000
    assert ratios["data"] < 1.0
    assert ratios["jitter"] < 1.0
    assert ratios["filled"] < 0.967


def test_closed_records_go_into_bvh():
    """A BVH file has one skeleton, and the live smoother holds the lengths per row as the offline one does: the tables streamed here
    carry the body fit's poses (one length vector per identity), the recorded-tables use of update_tables."""
    from multiview_motion_capture_amd.body_fit import fit_tracklets
    from multiview_motion_capture_amd.bvh_export import bvh_text
    from multiview_motion_capture_amd.live_smoothing import LiveSmoother
    from test_gpu_body_fit import _oracle_records
    si, fx = load_golden("shelf_inputs.npz"), load_golden("shelf_clean_oracle_tracker.npz")
    cal = _calibs(si["K"], si["Rt"])
    fitted = fit_tracklets(_oracle_records(fx, 100), si["kps25"][:101], si["counts"][:101].astype(np.int32), cal)
    pose_at = {t.track_id: dict(zip(t.frame_idxs, t.poses)) for t in fitted}
    sm = LiveSmoother(5, 1, window=8, lag=2, n_iter=1)
    key = sm.open_session(cal)
    recs, last = [], {}
    for r in range(60, 100):
        f, inputs, meta, params, joints = _shelf_table(si, fx, r)
        params, joints = params.copy(), joints.copy()
        for k, tid in enumerate(int(t) for t in meta[:, 0]):
            last[tid] = pose_at[tid].get(f, last.get(tid))            # (a row without data: its values are not read)
            params[k], joints[k] = _p68(last[tid][1]), last[tid][2].keypoints
        recs += sm.update_tables({key: (f, inputs, meta, params, joints)})[key].finished
    recs += sm.close_session(key)
    assert sorted(t.track_id for t in recs) == [0, 1, 2, 3, 4] and sum(int(t.smooth_filled.sum()) for t in recs) == 3
    for t in recs:
        assert t.frame_idxs == list(range(t.frame_idxs[0], t.frame_idxs[0] + len(t)))
        lines = bvh_text(t).splitlines()
        k = lines.index("MOTION")
        assert int(lines[k + 1].split()[1]) == len(t) == len(lines[k + 3:])
        rows = np.array([[float(v) for v in ln.split()] for ln in lines[k + 3:]])
        assert np.abs(rows[:, :3] - np.array([q[1].root for q in t.poses])).max() <= 1e-8
