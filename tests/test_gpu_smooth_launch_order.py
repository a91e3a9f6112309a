"""GPU: the host drivers of the two smoothers (smoothing.smooth_sequences, live_smoothing.LiveSmoother) call the same C entries in the
same order as before their split into stages.  Every mvmc_* attribute of the loaded library is wrapped with a recorder (the way
test_gpu_live_smooth's one-launch-per-tick test wraps one), and the recorded names are compared with sequences written out below,
which were recorded with this test body on the commit before the split.  The size queries (*_work_doubles) and mvmc_status_string are
not launches and are not recorded."""
import numpy as np
import pytest

from test_body_fit_cpu import _cameras, _coco, _Rec
from test_smooth_cpu import _fk, _walk

pytestmark = pytest.mark.gpu

FRAMES = 8
LIVE_FRAMES = (0, 1, 2, 3, 5, 6, 7, 8, 9, 10)      # ten ticks, a jump of the frame index by 2 at the fifth


def record_calls(monkeypatch) -> list:
    """Wraps the library's entries; -> the list that receives their names (without the mvmc_ prefix) as they are called."""
    from multiview_motion_capture_amd import _cabi
    from multiview_motion_capture_amd import device  # noqa: F401  (torch, and with it the HIP runtime, before the library: the drivers' order)
    lib, calls = _cabi.load(), []
    for name in _cabi.SYMBOLS:
        if name in ("mvmc_abi_version", "mvmc_status_string") or name.endswith(("_doubles", "_words")):
            continue

        def recorded(*a, _fn=getattr(lib, name), _name=name[5:]):
            calls.append(_name)
            return _fn(*a)
        monkeypatch.setattr(lib, name, recorded, raising=False)
    return calls


def _calibs(Ps):
    from multiview_motion_capture_amd.common import Calib
    K = np.array([[1000.0, 0, 500], [0, 1000.0, 400], [0, 0, 1.0]])
    return [Calib.from_k_rt(K, np.linalg.inv(K) @ P) for P in Ps]


def _people(n_frames, seed):
    """Two people in 3 cameras over n_frames: kps (F,3,2,17,3) with 2 px noise, counts (F,3), the tracker-like noisy parameters
    (2,F,68) and their FK joints (2,F,18,3), the projections."""
    rng = np.random.default_rng(seed)
    Ps = _cameras(3)
    walks = [_walk(n_frames, seed), _walk(n_frames, seed + 1)]
    walks[1][:, :2] += (1.2, -0.8)
    kps = np.zeros((n_frames, 3, 2, 17, 3))
    for f in range(n_frames):
        for c in range(3):
            for p in range(2):
                kps[f, c, p] = _coco(_fk(walks[p][f]), Ps[c], [5, 6, 11][c])
                kps[f, c, p, :, :2] += rng.normal(0, 2.0, (17, 2))
    par = np.array(walks)
    par[:, :, :57] += rng.normal(0, 0.01, (2, n_frames, 57))
    return kps, np.full((n_frames, 3), 2, np.int32), par, np.array([[_fk(q) for q in w] for w in par]), Ps


def offline_inputs(seed=3):
    """One sequence of 3 cameras and 8 frames: identity 0 with a hole at frame 3, identity 1 with one frame -> (sequence, records,
    given contact labels aligned with the records)."""
    kps, cnt, par, jn, Ps = _people(FRAMES, seed)
    keep = [0, 1, 2, 4, 5, 6, 7]
    recs = [_Rec(keep, par[0, keep], jn[0, keep], tid=0), _Rec([5], par[1, 5:6], jn[1, 5:6], tid=1)]
    given = np.zeros((FRAMES, 2), bool)
    given[:4, 0] = True
    given[5:, 1] = True
    return (kps, cnt, _calibs(Ps)), recs, [given, None]


def offline_cases():
    seq, recs, given = offline_inputs()
    return {"none": {}, "loss": dict(loss="huber"), "covariance": dict(covariance="joints"),
            "auto": dict(contacts="auto", contact_rounds=2),
            "all": dict(loss="cauchy", covariance="joints", contacts=[given, given], floor=(0.0, 0.0, 1.0))}, seq, recs


def run_offline(kw, seq, recs):
    """Two copies of the sequence under a workspace cap of nine or ten rows (whatever the options add to a row's bytes): one camera
    group, the two 8-row identities in two partitions."""
    from multiview_motion_capture_amd.smoothing import smooth_sequences
    return smooth_sequences([seq, seq], [recs, recs], max_iter=2, max_work_bytes=10 * 46 * 1024, **kw)


def live_tables(seed):
    """One session's ten ticks: identity 0 throughout (without a new pose on the third tick), identity 1 on the first five ticks (it is
    finished by the sixth), identity 2 from the seventh on, in the slot identity 1 left."""
    kps, cnt, par, jn, Ps = _people(LIVE_FRAMES[-1] + 1, seed)
    ticks, hits = [], {0: 0, 1: 0, 2: 0}
    for t, f in enumerate(LIVE_FRAMES):
        rows = [(0, 0)] + ([(1, 1)] if t < 5 else []) + ([(2, 1)] if t >= 6 else [])
        for tid, _ in rows:
            hits[tid] += 0 if (tid, t) == (0, 2) else 1
        meta = np.array([[tid, 2, hits[tid], 0] for tid, _ in rows])
        ticks.append((f, (kps[f], cnt[f]), meta, np.array([par[p, f] for _, p in rows]), np.array([jn[p, f] for _, p in rows])))
    return ticks, _calibs(Ps)


LIVE_CASES = {"none": {}, "loss": dict(loss="huber"), "covariance": dict(covariance="joints"), "contacts": dict(contacts="auto"),
              "lengths": dict(lengths="auto", lengths_commit=3),
              "all": dict(loss="huber", covariance="joints", contacts="auto", lengths="auto", lengths_commit=3)}


def run_live(kw, mark=lambda sm: None):
    """Two sessions through ten ticks, then tracklets() of the first and close_session of both; mark(smoother) is called after every
    tick and at the end.  -> the ticks' outputs, the records of tracklets(), the closed records."""
    from multiview_motion_capture_amd.live_smoothing import LiveSmoother
    sm = LiveSmoother(3, 2, p_max=2, window=4, lag=1, n_iter=2, contact_min_frames=2, **kw)
    sessions = [live_tables(seed) for seed in (11, 21)]
    keys = [sm.open_session(cal) for _, cal in sessions]
    outs = []
    for t in range(len(LIVE_FRAMES)):
        outs.append(sm.update_tables({k: ticks[t] for k, (ticks, _) in zip(keys, sessions)}))
        mark(sm)
    live = sm.tracklets(keys[0])
    closed = [sm.close_session(k) for k in keys]
    mark(sm)
    return outs, live, closed


# ---- the sequences of the commit before the split ----
def _solve(blocks):
    return [blocks, "smooth_step"] * 3      # max_iter + 1 = 3 launches of each


# one camera group: its selection, then the two partitions one after the other
OFFLINE = {
    "none": ["ingest", "body_observe"] + (_solve("smooth_blocks") + ["fk"]) * 2,
    "loss": ["ingest", "body_observe"] + (_solve("smooth_blocks_robust") + ["smooth_obs_weights", "fk"]) * 2,
    "covariance": ["ingest", "body_observe"] + (_solve("smooth_blocks") + ["smooth_blocks", "smooth_cov", "fk"]) * 2,
    "auto": ["ingest", "body_observe"] + (_solve("smooth_blocks") + (["fk", "smooth_contact_anchors"] + _solve("smooth_blocks_contact")) * 2
                                          + ["fk"]) * 2,
    "all": ["ingest", "body_observe"] + (_solve("smooth_blocks_robust") + ["fk", "smooth_contact_anchors", "smooth_floor_anchors"]
                                         + _solve("smooth_blocks_floor") + ["smooth_blocks_floor", "smooth_cov", "smooth_obs_weights", "fk"]) * 2,
}


def _ticks(*launches):
    """The first tick emits nothing (lag 1) and reads no row back: no FK; the nine others end with the FK of the rows read back; after
    them tracklets() and the two close_session calls are one FK each."""
    head = ["ingest", "body_observe"]
    return [head + [n for n in launches if "_cov" not in n]] + [head + list(launches) + ["fk"]] * 9 + [["fk"] * 3]


LIVE = {
    "none": _ticks("smooth_window"),
    "loss": _ticks("smooth_window_robust"),
    "covariance": _ticks("smooth_window", "smooth_window_cov"),
    "contacts": _ticks("smooth_window_contact"),
    "lengths": _ticks("live_lengths_apply", "smooth_window", "live_lengths_update"),
    "all": _ticks("live_lengths_apply", "smooth_window_contact", "live_lengths_update", "smooth_window_cov_contact"),
}


@pytest.mark.parametrize("case", ["none", "loss", "covariance", "auto", "all"])
def test_smooth_sequences_calls_the_same_entries_in_the_same_order(case, monkeypatch):
    cases, seq, recs = offline_cases()
    calls = record_calls(monkeypatch)
    out = run_offline(cases[case], seq, recs)
    assert [len(r) for r in out] == [2, 2] and all(len(r[0]) == FRAMES and len(r[1]) == 1 for r in out)
    assert calls == OFFLINE[case], calls


@pytest.mark.parametrize("case", list(LIVE_CASES))
def test_live_smoother_calls_the_same_entries_in_the_same_order_on_every_tick(case, monkeypatch):
    calls, ticks = record_calls(monkeypatch), []

    slots = []      # per tick and session {track_id: slot}

    def mark(sm):
        ticks.append(calls[sum(len(t) for t in ticks):])
        slots.append([{tid: idn.slot for tid, idn in s.ids.items()} for s in sm._sessions.values()])
    outs, live, closed = run_live(LIVE_CASES[case], mark)
    assert len(ticks) == len(LIVE_FRAMES) + 1 == len(LIVE[case])
    for t, (got, exp) in enumerate(zip(ticks, LIVE[case])):
        assert got == exp, (t, got)
        if t < len(LIVE_FRAMES):      # exactly one window entry per tick, whatever the options
            assert sum(n.startswith("smooth_window") and not n.startswith("smooth_window_cov") for n in got) == 1, (t, got)
    # the input has every path: both sessions emit, identity 1 is finished at the sixth tick, identity 2 takes its slot
    assert all(len(o.finished) == (1 if t == 5 else 0) for t, out in enumerate(outs) for o in out.values())
    assert [r.track_id for r in live] == [0, 2] == [r.track_id for r in closed[1]]
    assert all(1 in s4 and 1 not in s5 and 2 not in s5 and s6[2] == s4[1] for s4, s5, s6 in zip(slots[4], slots[5], slots[6]))
