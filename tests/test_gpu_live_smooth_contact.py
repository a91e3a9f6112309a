"""GPU: the live smoother's foot contacts (live_smoothing.LiveSmoother(contacts="auto"), csrc/mvmc_smooth_window.hip:
smooth_window_kernel<LOSS, true>, mvmc_smooth_window_cov_contact) against the NumPy restatement (tests/live_smooth_contact_np.py) tick
by tick on Shelf tables -- with jumps of the frame index, under a Cauchy loss, with the covariance -- and through LivePool on a planted
synthetic walk; bit identity (contact_speed 0 against contacts=None, alone against among other sessions, run to run) and one launch
per tick.  Tolerances: tests/test_gpu_live_smooth.py's (_Worst: parameters and relative cost 1e-9, joints 1e-8); labels exactly; anchors
1e-9 m.  E_contact = 1/2 wc sum |ankle - a|^2 moves by at most sqrt(2 wc E_contact n_terms) x the ankles' difference, so contact_cost is
held to that with the joints' own 1e-8 m (plus 1e-9 relative)."""
import functools

import numpy as np
import pytest

import live_smooth_contact_np as lct
import live_smooth_cov_np as lc
import live_smooth_np as ls
import smooth_contact_np as ct
import smooth_robust_np as rb
from conftest import load_golden
from test_gpu_body_fit import _calibs
from test_gpu_live_smooth import _compare_record, _compare_tick, _pool_frames, _rec_signature, _shelf_table, _signature, _table_of, _Worst
from test_gpu_smooth import _weights

pytestmark = pytest.mark.gpu

WC = 1e6            # smoothing.CONTACT_WEIGHT
ANCHOR_TOL = 1e-9   # m
MARGIN = 1e-7       # no tentative row's speed may lie this close to the threshold: its label would be decided by rounding
KW = dict(window=8, lag=3, n_iter=2)


class _Contact:
    """What the contact comparisons saw."""

    def __init__(self):
        self.anchor = self.cost = 0.0
        self.labels = self.emitted_labels = 0

    def pair(self, c, a, ec, ea, what):
        assert np.array_equal(np.asarray(c, bool), np.asarray(ec, bool)), (what, c, ec)
        assert np.array_equal(np.isnan(a), np.isnan(ea)) and np.array_equal(np.isnan(np.asarray(ea)[..., 0]), ~np.asarray(ec, bool)), what
        if np.asarray(ec).any():
            self.anchor = max(self.anchor, float(np.nanmax(np.abs(np.asarray(a) - ea))))
        self.labels += int(np.asarray(ec).sum())

    def check(self, what):
        print(f"{what}: worst anchor difference {self.anchor:.2e} m, worst contact_cost excess over its bound {self.cost:.2e}; "
              f"{self.labels} labels compared, {self.emitted_labels} on emitted rows")
        assert self.anchor <= ANCHOR_TOL and self.cost <= 0.0


def _compare_contact(got, exp, seen, what, n_free):
    assert sorted(got.contact) == sorted(exp["contact"]) == sorted(e[0] for e in got.emitted), what
    for tid, e in exp["contact"].items():
        seen.pair(got.contact[tid]["contact"], got.contact[tid]["anchor"], e["contact"], e["anchor"], (what, tid))
        seen.emitted_labels += int(e["contact"].sum())
    for tid, info in exp["solved"].items():
        for a, b in zip(got.solved[tid]["contact_cost"], info["contact_cost"]):
            bound = 1e-9 * b + np.sqrt(2.0 * WC * b * 2 * n_free) * 1e-8
            seen.cost = max(seen.cost, abs(a - b) - bound)


def _compare_records(ts, es, worst, seen, what):
    assert len(ts) == len(es), what
    for t, e in zip(ts, es):
        _compare_record(t, e, worst, what)
        assert t.smooth_contact.shape == (len(t), 2) and t.smooth_contact.dtype == bool and t.smooth_contact_anchor.shape == (len(t), 2, 3)
        seen.pair(t.smooth_contact, t.smooth_contact_anchor, e["contact"], e["anchor"], (what, t.track_id))


def _cases(st, cases):
    """The restatement's state after a tick -> which cases of the model the run has met so far."""
    lag = st.lag
    for tid, idn in st.ids.items():
        n = len(idn.x)
        c = np.array(idn.c).reshape(n, 2)
        first = max(n - lag, 0)
        for f in range(2):
            for a, b in ct.runs(c[:, f]):
                if a >= first:
                    cases["tentative"].add((tid, idn.f0, f, a))                     # a run without a frozen row
                elif (tid, idn.f0, f, a) in cases["tentative"]:
                    cases["committed"].add((tid, idn.f0, f, a))                     # ... whose first row froze with its label
                if b - a > st.W + 2:
                    cases["long"].add((tid, f, a))                                   # it continues from rows that left the window
                if any(not idn.data[i] for i in range(a, b)):
                    cases["missing_in_run"].add((tid, f, a))
            cases["feet"].setdefault((tid, idn.f0, f), [0, 0])
            cases["feet"][(tid, idn.f0, f)] = [n, int(c[:, f].sum())]


def _stream_shelf(rows, kw=KW, ckw=None, what="", **more):
    """Shelf table rows ``rows`` (any increasing sequence: a gap is a jump of the frame index) through one session and the restatement."""
    from multiview_motion_capture_amd.live_smoothing import LiveSmoother
    si, fx = load_golden("shelf_inputs.npz"), load_golden("shelf_clean_oracle_tracker.npz")
    ckw = ckw or {}
    sm = LiveSmoother(5, 2, contacts="auto", **kw, **ckw, **more)
    key = sm.open_session(_calibs(si["K"], si["Rt"]))
    st = lct.Stream(si["P"], kw["window"], kw["lag"], kw["n_iter"], _weights(), **ckw)
    worst, seen = _Worst(), _Contact()
    cases = dict(tentative=set(), committed=set(), long=set(), missing_in_run=set(), feet={})
    rows = list(rows)
    for k, r in enumerate(rows):
        f, (kps, cnt), meta, params, joints = _shelf_table(si, fx, r)
        got = sm.update_tables({key: (f, (kps, cnt), meta, params, joints)})[key]
        exp = st.tick(f, ls.bf.ingest_np(kps[None], cnt[None])[0], meta, params, joints)
        _compare_tick(got, exp, worst, f"row {r}")
        _compare_contact(got, exp, seen, f"row {r}", kw["window"])
        _compare_records(got.finished, exp["finished"], worst, seen, f"finished at row {r}")
        _cases(st, cases)
        if k % 10 == 9 or k == len(rows) - 1:
            _compare_records(sm.tracklets(key), st.records(), worst, seen, f"records after row {r}")
    _compare_records(sm.close_session(key), st.close(), worst, seen, "closed")
    print(f"\n{what}: restatement's runs {st.seen}, closest speed to the threshold {st.margin:.3e}")
    worst.check(what)
    seen.check(what)
    assert st.margin >= MARGIN, f"a tentative row's speed lies within {MARGIN} of contact_speed ({st.margin}): choose another contact_speed"
    return st, cases, seen


def test_shelf_rows_60_to_99_equal_the_restatement_tick_by_tick_and_meet_every_case():
    st, cases, seen = _stream_shelf(range(60, 100), what="Shelf rows 60-99, W 8, lag 3, 2 trials, contact_speed 0.01")
    never = [k for k, (n, labels) in cases["feet"].items() if n >= 20 and labels == 0]
    print("cases:", {k: len(v) for k, v in cases.items()}, "feet never labelled:", never)
    assert cases["committed"], "no run started tentative and was committed later"
    assert cases["long"] and st.seen["continued"] >= 1, "no run longer than W + 2 rows: none continued from frozen history"
    assert st.seen["dropped"] >= 1, "no tentative run was dropped for shortness"
    assert cases["missing_in_run"], "no missing row inside a run"
    assert never, "every foot of every long identity was labelled at some time"
    assert seen.emitted_labels >= 20


def test_shelf_rows_0_to_59_at_window_12_lag_6():
    st, cases, seen = _stream_shelf(range(0, 60), kw=dict(window=12, lag=6, n_iter=2), what="Shelf rows 0-59, W 12, lag 6, 2 trials")
    assert cases["committed"] and st.seen["continued"] >= 1 and seen.emitted_labels >= 20


def test_jumps_of_the_frame_index_append_rows_straight_into_the_frozen_zone():
    """Rows 60-99 without rows 66-67 and 75-76 (the frame index jumps by 3) and without 82-86 (by 6 > lag + 1 = 4: the first two of the
    five missing rows are appended past the emit position and are frozen without ever having been labelled)."""
    rows = [r for r in range(60, 100) if r not in (66, 67, 75, 76, 82, 83, 84, 85, 86)]
    st, cases, seen = _stream_shelf(rows, what="Shelf rows 60-99 with jumps of 3, 3 and 6")
    assert seen.emitted_labels >= 10 and (st.seen["kept"] >= 1 or st.seen["continued"] >= 1)


def _contact_signature(out):
    return (sorted((tid, c["contact"].tobytes(), c["anchor"].tobytes()) for tid, c in out.contact.items()),
            sorted((tid, s["contact_cost"].tobytes()) for tid, s in out.solved.items()),
            [(t.smooth_contact.tobytes(), t.smooth_contact_anchor.tobytes()) for t in out.finished])


def _rec_contact_signature(t):
    return _rec_signature(t) + (t.smooth_contact.tobytes(), t.smooth_contact_anchor.tobytes())


@pytest.mark.parametrize("S", [1, 5])
def test_contact_speed_0_gives_the_bits_of_contacts_none_and_one_launch_per_tick(S, monkeypatch):
    """contact_speed = 0.0 can never label a row (a speed is never < 0): every tick's signature and every record equal contacts=None's
    bit for bit.  Under a launch-counting recorder contacts="auto" makes exactly one mvmc_smooth_window_contact launch and no
    mvmc_smooth_window launch per tick, contacts=None today's one mvmc_smooth_window."""
    from multiview_motion_capture_amd import _cabi
    from multiview_motion_capture_amd.live_smoothing import LiveSmoother
    si, fx = load_golden("shelf_inputs.npz"), load_golden("shelf_clean_oracle_tracker.npz")
    lib = _cabi.load()
    calls = dict(plain=[], robust=[], contact=[])
    for name, kind in (("mvmc_smooth_window", "plain"), ("mvmc_smooth_window_robust", "robust"), ("mvmc_smooth_window_contact", "contact")):
        def counted(*a, _orig=getattr(lib, name), _kind=kind):
            calls[_kind].append(int(a[7]))
            return _orig(*a)
        monkeypatch.setattr(lib, name, counted, raising=False)
    rows = range(60, 72) if S == 5 else range(60, 100)
    sigs = {}
    for mode, kw in (("none", {}), ("auto", dict(contacts="auto", contact_speed=0.0))):
        for v in calls.values():
            v.clear()
        sm = LiveSmoother(5, S, **KW, **kw)
        keys = [sm.open_session(_calibs(si["K"], si["Rt"])) for _ in range(S)]
        sig = []
        for k, r in enumerate(rows):
            out = sm.update_tables({key: _shelf_table(si, fx, r) for key in keys})
            n_items = S * int(fx["n_tracks"][r])
            n_calls = {q: len(v) for q, v in calls.items()}
            assert n_calls == dict(plain=k + 1 if mode == "none" else 0, robust=0, contact=k + 1 if mode == "auto" else 0), (mode, r, n_calls)
            assert calls["plain" if mode == "none" else "contact"][-1] == n_items
            sig.append([_signature(out[key]) for key in keys])
            if mode == "auto":
                assert all(not c["contact"].any() and np.all(np.isnan(c["anchor"])) for o in out.values() for c in o.contact.values())
                assert all(np.all(s["contact_cost"] == 0.0) for o in out.values() for s in o.solved.values())
            else:
                assert all(o.contact == {} and "contact_cost" not in s for o in out.values() for s in o.solved.values())
        live = [_rec_signature(t) for t in sm.tracklets(keys[0])]
        done = [sm.close_session(key) for key in keys]
        sigs[mode] = (sig, live, [[_rec_signature(t) for t in d] for d in done])
        if mode == "none":
            assert "clab" not in sm._state() and not any(hasattr(t, "smooth_contact") for d in done for t in d)
        else:
            assert all(not t.smooth_contact.any() and np.all(np.isnan(t.smooth_contact_anchor)) for d in done for t in d)
    assert sigs["none"] == sigs["auto"]
    assert all(s == sigs["auto"][0][0][0] for s in sigs["auto"][0][0])                 # and every session of the tick has the same bits


def test_bit_identity_with_contacts_alone_among_other_sessions_and_run_to_run():
    from multiview_motion_capture_amd.live_smoothing import LiveSmoother
    si, fx = load_golden("shelf_inputs.npz"), load_golden("shelf_clean_oracle_tracker.npz")
    cal = _calibs(si["K"], si["Rt"])
    kw = dict(contacts="auto", **KW)
    rows = list(range(60, 100))

    def alone():
        sm = LiveSmoother(5, 1, **kw)
        key = sm.open_session(cal)
        sig = []
        for r in rows:
            out = sm.update_tables({key: _shelf_table(si, fx, r)})[key]
            sig.append((_signature(out), _contact_signature(out)))
        return sig, [_rec_contact_signature(t) for t in sm.close_session(key)]
    a, b = alone(), alone()
    assert a == b                                                                   # run to run
    assert sum(len(s[1][0]) for s in a[0]) >= 80 and any(c[1] != b"\x00\x00" for s in a[0] for c in s[1][0])     # labels were made
    # among four others on shifted rigs at other rows: staggered opens, a close, ticks the session sits out
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
        else:
            tables[main] = _shelf_table(si, fx, rows[at])
            out = sm.update_tables(tables)[main]
            sig.append((_signature(out), _contact_signature(out)))
            at += 1
        tick += 1
    assert (sig, [_rec_contact_signature(t) for t in sm.close_session(main)]) == a


def test_cauchy_loss_with_contacts_equals_the_restatement_under_both_bindings():
    """Fifteen rows; smooth_contact_np.contact stacks on smooth_robust_np.robust, the term stays outside the loss."""
    from test_smooth_robust_cpu import LOSS_PX
    with rb.robust("cauchy", LOSS_PX):
        st, cases, seen = _stream_shelf(range(60, 75), what="Shelf rows 60-74, cauchy + contacts", loss="cauchy", loss_px=LOSS_PX)
    assert seen.emitted_labels >= 5 and st.seen["kept"] >= 1
    assert ls.sm.data_terms is rb._plain_data_terms                                   # both bindings are undone


def test_covariance_with_contacts_equals_the_dense_inverse_and_moves_nothing_else():
    """Fifteen rows, covariance="joints" with contacts: every emitted row's entry against the dense inverse of the restatement's
    window matrix AT the device's rows under the contact binding of the labels and anchors as they stand after the tick (the
    restatement's, which the same tick's comparison holds equal to the device's).  tests/test_gpu_live_smooth_cov.py's gate.  The
    poses, ``solved``, the contacts, the records and the device state are the bits of the smoother without covariance."""
    from multiview_motion_capture_amd.live_smoothing import LiveSmoother
    from test_gpu_live_smooth_cov import _compare_entry, _device_window
    from test_live_smooth_cov_cpu import TOL, rel
    si, fx = load_golden("shelf_inputs.npz"), load_golden("shelf_clean_oracle_tracker.npz")
    w = _weights()

    def run(**more):
        sm = LiveSmoother(5, 1, contacts="auto", **KW, **more)
        key = sm.open_session(_calibs(si["K"], si["Rt"]))
        return sm, key
    sm, key = run(covariance="joints")
    sp, kp = run()
    st = lct.Stream(si["P"], KW["window"], KW["lag"], KW["n_iter"], w)
    worst, seen, cworst = _Worst(), _Contact(), {}
    entries = labelled = 0
    gap = 0.0
    for r in range(60, 75):
        f, (kps, cnt), meta, params, joints = _shelf_table(si, fx, r)
        got = sm.update_tables({key: (f, (kps, cnt), meta, params, joints)})[key]
        plain = sp.update_tables({kp: (f, (kps, cnt), meta, params, joints)})[kp]
        assert (_signature(got), _contact_signature(got)) == (_signature(plain), _contact_signature(plain)), r
        assert plain.cov == {} and sorted(got.cov) == sorted(e[0] for e in got.emitted)
        exp = st.tick(f, ls.bf.ingest_np(kps[None], cnt[None])[0], meta, params, joints)
        _compare_tick(got, exp, worst, f"row {r}")
        _compare_contact(got, exp, seen, f"row {r}", KW["window"])
        for e in got.emitted:
            tid = e[0]
            idn = st.ids[tid]
            n = len(idn.x)
            c = got.cov[tid]
            if n < 2:
                assert c["status"] == 2
                continue
            m = min(st.W, n)
            h = min(2, n - m)
            x = _device_window(sm, key, tid)
            obs, prs = [None] * h + idn.obs[n - m:], [None] * h + idn.prs[n - m:]
            cm, an = st.window_contact(tid)
            with ct.contact(cm, an, WC):
                xc = lc.window_cov(x, h, obs, prs, w, f - st.lag - idn.f0 - (n - m), blocks="dense")
            _compare_entry(c, xc, cworst, (r, tid))
            entries += 1
            if cm.any():
                labelled += 1
                gap = max(gap, rel(lc.window_cov(x, h, obs, prs, w, f - st.lag - idn.f0 - (n - m), blocks="dense")["jcov"], xc["jcov"]))
    worst.check("covariance + contacts")
    seen.check("covariance + contacts")
    print(f"{entries} entries ({labelled} with a label in the window), worst relative differences", {q: f"{v:.2e}" for q, v in cworst.items()},
          f"; without the term the jcov differs by {gap:.2e}")
    assert entries >= 30 and labelled >= 10 and gap > 100 * TOL
    a, b = sm._state(), sp._state()
    assert all(bool(((a[q] == b[q]) | ((a[q] != a[q]) & (b[q] != b[q]))).all()) for q in ("rows", "members", "count", "clab", "canc"))
    assert [_rec_contact_signature(t) for t in sm.close_session(key)] == [_rec_contact_signature(t) for t in sp.close_session(kp)]


@functools.lru_cache(maxsize=None)
def _planted(seed=91, F=48):
    from multiview_motion_capture_amd import synth
    g = synth.generate(F, 5, 2, seed, walk="planted")
    return g, _calibs(g["K"], g["Rt"])


def _skate_of(emitted, g):
    """emitted {(tid, frame): joints} -> (mean ankle displacement per frame over the true contact pairs, labels' ground truth lookup):
    every emitted pose belongs to the ground-truth person whose joints are nearest."""
    person = lambda f, J: int(np.argmin([np.linalg.norm(J - g["gt_joints"][f, p], axis=-1).mean() for p in range(g["gt_joints"].shape[1])]))
    d = []
    for (tid, f), J in emitted.items():
        nxt = emitted.get((tid, f + 1))
        if nxt is None:
            continue
        p = person(f, J)
        for k, K in enumerate(ct.FEET):
            if g["gt_contact"][f, p, k] and g["gt_contact"][f + 1, p, k]:
                d.append(float(np.linalg.norm(nxt[K] - J[K])))
    return float(np.mean(d)), len(d), person


def test_through_the_live_pool_both_routes_equal_the_restatement_and_the_planted_foot_slides_less():
    from multiview_motion_capture_amd.live import LivePool
    from multiview_motion_capture_amd.live_smoothing import LiveSmoother
    g, cal = _planted()
    F = g["kps25"].shape[0]
    pools = [LivePool(5, 1) for _ in range(3)]
    sms = [LiveSmoother.for_pool(pools[0], contacts="auto", **KW), LiveSmoother.for_pool(pools[1], contacts="auto", **KW),
           LiveSmoother.for_pool(pools[2], **KW)]
    sid = pools[0].open_session(cal)
    assert pools[1].open_session(cal) == sid == pools[2].open_session(cal)
    st = lct.Stream(g["P"], KW["window"], KW["lag"], KW["n_iter"], _weights())
    worst, seen = _Worst(), _Contact()
    em, em_none, lab = {}, {}, {}
    same_records = True
    for f in range(F):
        frames = {sid: (f, _pool_frames(g, cal, f))}
        pools[0].update_4d(frames)
        out = sms[0].update_4d(frames)[sid]
        k25, cn = g["kps25"][f:f + 1].astype(np.float64), g["counts"][f:f + 1].astype(np.int32)
        pools[1].update_4d_arrays([sid], [f], k25, cn)
        out_a = sms[1].update_4d_arrays([sid], [f], k25, cn)[sid]
        pools[2].update_4d(frames)
        out_n = sms[2].update_4d(frames)[sid]
        meta, params, joints = _table_of(pools[0].session(sid), f)
        exp = st.tick(f, ls.bf.ingest_np(g["kps25"][f:f + 1], g["counts"][f:f + 1])[0], meta, params, joints)
        _compare_tick(out, exp, worst, f"frame {f}")
        _compare_contact(out, exp, seen, f"frame {f}", KW["window"])
        ma, pa_, ja = _table_of(pools[1].session(sid), f)
        same_records &= np.array_equal(meta, ma) and np.array_equal(params, pa_) and np.array_equal(joints, ja)
        if same_records:
            assert (_signature(out), _contact_signature(out)) == (_signature(out_a), _contact_signature(out_a)), f
        for e in out.emitted:
            em[(e[0], e[1])] = e[3].keypoints
            lab[(e[0], e[1])] = out.contact[e[0]]["contact"]
        for e in out_n.emitted:
            em_none[(e[0], e[1])] = e[3].keypoints
    assert same_records, "the pool's two routes gave different records: the route comparison did not cover the run"
    _compare_records(sms[0].close_session(sid), st.close(), worst, seen, "closed")
    worst.check("a planted walk through LivePool")
    seen.check("a planted walk through LivePool")
    assert st.margin >= MARGIN
    s_c, n_c, person = _skate_of(em, g)
    s_n, n_n, _ = _skate_of(em_none, g)
    tp = sum(int((c & g["gt_contact"][f, person(f, em[(tid, f)])]).sum()) for (tid, f), c in lab.items())
    n_lab = sum(int(c.sum()) for c in lab.values())
    n_true = sum(int(g["gt_contact"][f, person(f, em[(tid, f)])].sum()) for (tid, f) in lab)
    print(f"skate over the true contact pairs: {1e3 * s_n:.2f} mm / frame without contacts ({n_n} pairs), {1e3 * s_c:.2f} with ({n_c}); "
          f"emitted labels: precision {tp / max(n_lab, 1):.2f}, recall {tp / max(n_true, 1):.2f} ({n_lab} labels, {n_true} true)")
    assert n_c >= 40 and n_lab >= 10
    assert s_c < s_n
