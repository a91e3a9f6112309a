"""GPU: many live rigs stepped frame by frame in one chain-kernel launch per tick -- idle chains in the kernel
(include/mvmc.h: mvmc_chain_run_sessions) and the session pool on top (multiview_motion_capture_amd/live.py).  Every session's
tracklets must be, after every tick, bit for bit those of its own MvTracker.update_4d fed the same frames; recovery of one session
(detach, widened replay, narrowing, re-attach, raise) must leave the others alone."""
import collections
import copy

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_gpu_update_4d import A01, A4, SCHEDULE, SEED, _shelf_frames, same_bits, state_of

pytestmark = pytest.mark.gpu

D = torch.device("cuda:0")


# ----------------------------------------------------------------------------------------------------------------------------------
# 1. the kernel: idle chains write nothing
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["latency", "throughput", "big"])
def test_idle_chains_write_nothing_and_active_chains_equal_a_launch_of_only_them(case):
    """B chains on three rigs (C5, four people), L = 3 frames stepped one launch per frame (ChainTracker with a rig per chain): every
    chain runs frames 0 and 1, about a third sit out frame 2 -- one of them with a rig index outside [0, n_rigs).  latency: B = 16
    (the 256-VGPR build), throughput: B = 600 (the 128-VGPR build), big: t_max 16 (the BIG layout).
    The idle chains' state bytes are unchanged and their out_* rows still hold the sentinel; their void words, flags[B + 2] and
    flags[B + 1] are 0 (no bit 4 for the bad index).  The active chains' state and output rows are bit for bit those of the same chains
    run alone, as whole chains of L frames, through mvmc_chain_run_rigs (run_chains_fused)."""
    from multiview_motion_capture_amd import device as dev, synth
    from multiview_motion_capture_amd.pipeline import HotPath
    from multiview_motion_capture_amd.tracker import ChainTracker, check_chain_flags, run_chains_fused
    B = {"latency": 16, "throughput": 600, "big": 16}[case]
    T = 16 if case == "big" else 8
    L, C, P = 3, 5, 4
    roc = np.arange(B) % 3
    data = [synth.generate(int((roc == r).sum()) * L, C, P, 20270501 + 11 * r, chain_len=L) for r in range(3)]
    rigs = [HotPath(d["K"], d["Rt"], device=D) for d in data]
    kps = np.zeros((B, L, C, P, 25, 3), np.float32)
    cnt = np.zeros((B, L, C), np.int32)
    for r in range(3):
        sel = np.nonzero(roc == r)[0]
        kps[sel] = data[r]["kps25"].reshape(len(sel), L, C, P, 25, 3)
        cnt[sel] = data[r]["counts"].reshape(len(sel), L, C)
    k17, c17 = dev.ingest(torch.from_numpy(kps.reshape(B * L, C, P, 25, 3)).to(D), torch.from_numpy(cnt.reshape(B * L, C)).to(D))
    k17, c17 = k17.view(B, L, C, P, 17, 3), c17.view(B, L, C)
    tr = ChainTracker(rigs[0], B, P, T, rigs=[rigs[r] for r in roc])
    assert tr.fused_ok
    idle = np.zeros(B, bool)
    idle[np.random.default_rng(5).permutation(B)[:B // 3]] = True
    bad = int(np.nonzero(idle)[0][0])
    for t in range(L - 1):
        tr.step_fused(k17[:, t].contiguous(), c17[:, t].contiguous())
    tr.check()
    before = {name: getattr(tr, name).clone() for name in tr._STATE}
    w = tr._fused
    outs = ("out_params", "out_joints", "out_meta", "out_n_tracks")
    for name in outs:
        w[name].fill_(-7)
    tr.rig_of_chain[bad] = B + 3                      # an idle chain's rig index is not judged
    tr.active.copy_(torch.from_numpy((~idle).astype(np.uint8)))
    tr.step_fused(k17[:, L - 1].contiguous(), c17[:, L - 1].contiguous(), fold_void=False)
    torch.cuda.synchronize()
    fl = tr.cflags.cpu().numpy()
    assert fl[B] == 0 and fl[B + 1] == 0 and fl[B + 2] == 0
    void = fl[B + 4:2 * B + 4]
    assert not void.any(), np.nonzero(void)
    idle_d = torch.from_numpy(idle).to(D)
    for name in tr._STATE:
        now = getattr(tr, name)
        assert torch.equal(now[idle_d], before[name][idle_d]), name
    assert not torch.equal(tr.params[~idle_d], before["params"][~idle_d])     # (the active chains did run)
    for name in outs:
        assert bool((w[name][idle_d] == -7).all()), name
    assert int(before["n_tracks"][idle_d].max()) > 0        # (the idle chains had tracklets to lose)
    # the active chains, alone: one launch of whole chains (L frames each) through mvmc_chain_run_rigs
    act = np.nonzero(~idle)[0]
    at = torch.from_numpy(act).to(D)
    ref = run_chains_fused(rigs[0], torch.from_numpy(kps[act].reshape(-1, C, P, 25, 3)).to(D),
                           torch.from_numpy(cnt[act].reshape(-1, C)).to(D), L, t_max=T, rigs=rigs, rig_of_chain=roc[act],
                           force_big=case == "big")
    torch.cuda.synchronize()
    check_chain_flags(ref)
    last = slice(L - 1, None, L)
    assert torch.equal(w["out_params"][at], ref["params"][last])
    assert torch.equal(w["out_joints"][at].reshape(len(act), T, 54), ref["joints"][last].reshape(len(act), T, 54))
    assert torch.equal(w["out_meta"][at], ref["meta"][last])
    assert torch.equal(w["out_n_tracks"][at], ref["n_tracks"][last])
    assert torch.equal(tr.n_dead[at], ref["n_dead"]) and torch.equal(tr.next_id[at], ref["next_id"])
    assert torch.equal(tr.params[at], ref["params"][last]) and torch.equal(tr.meta[at], ref["meta"][last])


def test_a_bad_rig_index_on_an_active_chain_is_named_by_check():
    """Two chains of one frame (C5 P4), a rig per chain, both active, chain 1 with rig index 5 of 2: the kernel checks the index and
    reads nothing; check() raises the ValueError that names the rig index, once (the report is per call)."""
    from multiview_motion_capture_amd import device as dev, synth
    from multiview_motion_capture_amd.pipeline import HotPath
    from multiview_motion_capture_amd.tracker import ChainTracker
    data = synth.generate(2, 5, 4, 20270501, chain_len=1)
    hp = HotPath(data["K"], data["Rt"], device=D)
    k17, c17 = dev.ingest(torch.from_numpy(data["kps25"]).to(D), torch.from_numpy(data["counts"]).to(D))
    tr = ChainTracker(hp, 2, 4, rigs=[hp, hp])
    tr.rig_of_chain[1] = 5
    tr.step_fused(k17, c17, fold_void=False)
    with pytest.raises(ValueError, match="rig index"):
        tr.check()
    tr.check()


# ----------------------------------------------------------------------------------------------------------------------------------
# 2. the pool against solo update_4d, tick by tick
# ----------------------------------------------------------------------------------------------------------------------------------
def _synth_session(n_frames, seed, n_people=4):
    """A synthetic C5 scene of its own rig: FrameData per frame (the poses as the oracle ingest leaves them)."""
    from multiview_motion_capture_amd import synth
    from multiview_motion_capture_amd.common import Calib
    from multiview_motion_capture_amd.live import _frame_data
    from helpers import oracle_ingest
    d = synth.generate(n_frames, 5, n_people, seed, walk="scene")
    calibs = [Calib.from_k_rt(d["K"][c], d["Rt"][c]) for c in range(5)]
    k17, c17 = oracle_ingest(d["kps25"].astype(np.float64), d["counts"])
    return calibs, [_frame_data(f, k17[f], c17[f], calibs) for f in range(n_frames)], d


def _shelf_session(n=300):
    from multiview_motion_capture_amd.common import Calib
    si = load_golden("shelf_inputs.npz")
    calibs = [Calib.from_k_rt(si["K"][c], si["Rt"][c], (1032, 776)) for c in range(5)]
    return calibs, [_shelf_frames(si, calibs, fi) for fi in range(1, n + 1)]


def _drive(pool, plan, n_ticks, check=None):
    """plan: list of dict(calibs, frames, open, close (tick or None), skip(tick) -> bool).  Opens / closes sessions at their ticks and
    feeds each open session its next frame unless skip(tick); a solo MvTracker per session gets the same frames.  After every tick
    every open session's state equals its solo tracker's, bit for bit.  Returns the number of session-frames compared."""
    from multiview_motion_capture_amd import motion_capture as mc
    live = {}
    n_cmp = 0
    for tick in range(n_ticks):
        for k, s in enumerate(plan):
            if s["open"] == tick:
                sid = pool.open_session(s["calibs"])
                live[k] = dict(sid=sid, pos=0, solo=mc.MvTracker(p_max=pool.P, t_max=pool.T))
            if s.get("close") == tick and k in live:
                pool.close_session(live.pop(k)["sid"])
        req = {}
        for k, st in live.items():
            s = plan[k]
            if st["pos"] < len(s["frames"]) and not s["skip"](tick):
                fi = s.get("frame0", 0) + st["pos"]
                req[st["sid"]] = (fi, s["frames"][st["pos"]])
                st["solo"].update_4d(fi, s["frames"][st["pos"]])
                st["pos"] += 1
        pool.update_4d(req)
        for k, st in live.items():
            got, exp = state_of(pool.session(st["sid"]).tracker), state_of(st["solo"])
            assert same_bits(got, exp), (tick, k)
            assert [len(t.frame_idxs) for t in pool.session(st["sid"]).dead_tracklets] == [len(t.frame_idxs) for t in st["solo"].dead_tracklets]
            n_cmp += 1
        if check:
            check(tick, live)
    return n_cmp


def test_pool_equals_solo_update_4d_on_every_tick():
    """Shelf frames 1..300 and five synthetic C5 scenes on their own rigs, of different lengths, in one pool at MvTracker's defaults
    (p_max 8, t_max 8) with five slots: sessions open at staggered ticks, one closes midway and its slot is taken by the sixth, and a
    scripted pattern leaves sessions without a frame on some ticks.  After every tick each open session's tables, joints, parameters,
    frame_idxs, dead count and next id equal a solo MvTracker's fed the same frames, exactly."""
    from multiview_motion_capture_amd.live import LivePool
    plan = []
    calibs, frames = _shelf_session()
    plan.append(dict(calibs=calibs, frames=frames, frame0=1, open=0, close=None, skip=lambda t: t % 11 == 5))
    for i, (n, t0) in enumerate(((120, 2), (200, 5), (90, 9), (150, 20), (100, 70))):
        c, f, _ = _synth_session(n, 20270301 + 13 * i)
        plan.append(dict(calibs=c, frames=f, open=t0, close=60 if i == 2 else None, skip=lambda t, i=i: (t * (i + 3)) % 7 == 1))
    pool = LivePool(5, capacity=5)
    assert (pool.P, pool.T) == (8, 8)
    n = _drive(pool, plan, 340)
    print(f"\npool vs solo update_4d: {n} session-ticks bit-identical; timings {pool.timings}")
    assert n > 1000


def test_pool_array_route_equals_solo_update_4d():
    """update_4d_arrays (the device ingest of OpenPose rows) on three synthetic sessions: each equals a solo MvTracker fed the FrameData
    of the same device-ingested poses."""
    from multiview_motion_capture_amd import device as dev, motion_capture as mc
    from multiview_motion_capture_amd.live import LivePool, _frame_data
    from multiview_motion_capture_amd.common import Calib
    from multiview_motion_capture_amd import synth
    F, S = 60, 3
    datas = [synth.generate(F, 5, 4, 20270401 + 3 * s, walk="scene") for s in range(S)]
    calibs = [[Calib.from_k_rt(d["K"][c], d["Rt"][c]) for c in range(5)] for d in datas]
    pool = LivePool(5, capacity=4)
    sids = [pool.open_session(c) for c in calibs]
    solos = [mc.MvTracker() for _ in range(S)]
    for f in range(F):
        who = [s for s in range(S) if (f + s) % 5 != 0]
        k25 = np.stack([datas[s]["kps25"][f] for s in who]).astype(np.float64)
        cn = np.stack([datas[s]["counts"][f] for s in who])
        pool.update_4d_arrays([sids[s] for s in who], [f] * len(who), k25, cn)
        k17, c17 = dev.ingest(torch.from_numpy(k25).to(D), torch.from_numpy(cn).to(D))
        k17, c17 = k17.cpu().numpy(), c17.cpu().numpy()
        for j, s in enumerate(who):
            solos[s].update_4d(f, _frame_data(f, k17[j], c17[j], calibs[s]))
        for s in range(S):
            assert same_bits(state_of(pool.session(sids[s]).tracker), state_of(solos[s])), (f, s)
    assert all(len(pool.session(sid).tracklets) > 0 for sid in sids)


# ----------------------------------------------------------------------------------------------------------------------------------
# 3. recovery of one session leaves the others alone
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def crowd_frames():
    """tests/test_gpu_update_4d.py's scripted crowd (SCHEDULE, seed 20260107) as FrameData per frame, and the rig."""
    from multiview_motion_capture_amd import synth
    from multiview_motion_capture_amd.common import Calib
    from multiview_motion_capture_amd.live import _frame_data
    from helpers import oracle_ingest
    data = synth.generate(len(SCHEDULE), 5, 6, SEED, walk="scene")
    calibs = [Calib.from_k_rt(data["K"][c], data["Rt"][c]) for c in range(5)]
    kps, order = data["kps25"].astype(np.float64), data["gt_order"]

    def frame(f, vis):
        k25 = np.zeros((1,) + kps.shape[1:])
        cnt = np.zeros((1, 5), np.int32)
        for c in range(5):
            keep = [k for k in range(6) if order[f, c, k] in vis]
            k25[0, c, :len(keep)] = kps[f, c, keep]
            cnt[0, c] = len(keep)
        k17, c17 = oracle_ingest(k25, cnt)
        return _frame_data(f, k17[0], c17[0], calibs)

    return calibs, frame


class PoolSpies:
    """Delegating spies: the pool's detach / attach and ChainTracker.widened / narrowed, as (tick, what, sid or t_max)."""

    def __init__(self, monkeypatch):
        from multiview_motion_capture_amd.live import LivePool
        from multiview_motion_capture_amd.tracker import ChainTracker
        self.tick = None
        self.events = []
        for cls, name, key in ((LivePool, "_detach", "sid"), (LivePool, "_attach", "sid"), (ChainTracker, "widened", "T"),
                               (ChainTracker, "narrowed", "T")):
            orig = getattr(cls, name)

            def spy(obj, *a, _orig=orig, _name=name, _key=key, **kw):
                self.events.append((self.tick, _name, getattr(a[0], "sid") if _key == "sid" else obj.T))
                return _orig(obj, *a, **kw)
            monkeypatch.setattr(cls, name, spy)


def test_crowd_recovers_alone_and_every_session_stays_bit_identical_to_solo(crowd_frames, monkeypatch):
    """The scripted crowd in a pool with p_max 6, t_max 2, next to three calm two-person sessions and a SECOND crowd one tick behind:
    the crowd voids at frame 6 (four people on two slots), detaches, is widened, takes the per-stage route, narrows after eight calm
    frames, re-attaches, and detaches again at frame 25; the second crowd voids on the next tick (two sessions void on consecutive ticks: the second is rolled back
    from the mirror the first one's tick patched).  Every session equals a solo MvTracker(p_max=6, t_max=2) on every tick."""
    from multiview_motion_capture_amd.live import LivePool
    calibs, frame = crowd_frames
    crowd = [frame(f, vis) for f, vis in enumerate(SCHEDULE)]
    plan = [dict(calibs=calibs, frames=crowd, open=0, skip=lambda t: False),
            dict(calibs=calibs, frames=crowd, open=1, skip=lambda t: False)]
    for i in range(3):
        c, f, _ = _synth_session(len(SCHEDULE) + 4, 20270601 + 5 * i, n_people=2)
        plan.append(dict(calibs=c, frames=f, open=i, skip=lambda t, i=i: t % (4 + i) == 3))
    spies = PoolSpies(monkeypatch)
    pool = LivePool(5, capacity=6, p_max=6, t_max=2)

    def check(tick, live):
        spies.tick = tick + 1

    spies.tick = 0
    _drive(pool, plan, len(SCHEDULE) + 4, check=check)
    ev = collections.defaultdict(list)
    for tick, what, v in spies.events:
        ev[what].append((tick, v))
    print("\nrecovery events:", dict(ev))
    # sids by opening order: crowd 0 -> 0, calm 0 -> 1 (tick 0), crowd 1 -> 2, calm 1 -> 3 (tick 1), calm 2 -> 4.  Measured: crowd 0 voids at
    # tick 6 (its frame 6), crowd 1 at tick 7 (its frame 6); each widens, narrows on its eighth calm frame (frame 22) and re-attaches on that
    # tick, and detaches again on its frame 25 (re-widened).  The calm sessions never leave the shared launch.  (widened / narrowed are also
    # called by the test's solo trackers: two events per tick.)
    assert ev["_detach"] == [(6, 0), (7, 2), (25, 0), (26, 2)]
    assert ev["_attach"] == [(22, 0), (23, 2)]
    assert sorted({t for t, v in ev["widened"]}) == [6, 7, 25, 26]
    assert sorted({t for t, v in ev["narrowed"]}) == [22, 23]

def _record(tlets):
    return [(t.track_id, t.state, t.hits, t.time_since_update, list(t.frame_idxs),
             [(fi, p.root.tobytes(), pose.keypoints.tobytes()) for fi, p, pose in t.poses]) for t in tlets]


def test_a_session_that_raises_is_left_as_it_was_and_the_others_commit(crowd_frames, monkeypatch):
    """tracker.T_WIDE = 3: the crowd's frame 6 (four people) voids the shared launch, the session detaches, its widened replay voids too
    and its update_4d raises.  The pool raises LiveSessionError naming that sid only; the session's row and host records are as before
    the tick, byte for byte; the calm sessions committed their frames.  The crowd then gets frame 7 with four people again (another void
    right after the raise: its row comes back from the mirror its re-attach patched) and frames 8-14 with {0, 1}: every tick equals a
    solo tracker that raised on the same frames."""
    from multiview_motion_capture_amd import motion_capture as mc, tracker
    from multiview_motion_capture_amd.live import LivePool, LiveSessionError
    monkeypatch.setattr(tracker, "T_WIDE", 3)
    calibs, frame = crowd_frames
    vis = [A01] * 6 + [A4, A4] + [A01] * 7
    crowd = [frame(f, v) for f, v in enumerate(vis)]
    calm = [_synth_session(len(vis), 20270701 + 5 * i, n_people=2)[:2] for i in range(2)]
    pool = LivePool(5, capacity=3, p_max=6, t_max=2)
    sids = [pool.open_session(calibs)] + [pool.open_session(c) for c, _ in calm]
    solos = [mc.MvTracker(p_max=6, t_max=2) for _ in range(3)]
    feeds = [crowd] + [f for _, f in calm]
    for f in range(len(vis)):
        req = {sids[k]: (f, feeds[k][f]) for k in range(3)}
        raised_solo = False
        for k in range(3):
            try:
                solos[k].update_4d(f, feeds[k][f])
            except ValueError:
                assert k == 0
                raised_solo = True
        slot = pool.session(sids[0]).slot
        before = pool._ch.state_rows([slot])
        rec = copy.deepcopy((_record(pool.session(sids[0]).tracklets), _record(pool.session(sids[0]).dead_tracklets)))
        if raised_solo:
            with pytest.raises(LiveSessionError) as ei:
                pool.update_4d(req)
            assert set(ei.value.errors) == {sids[0]} and "t_max" in str(ei.value.errors[sids[0]])
            after = pool._ch.state_rows([slot])
            assert all(np.array_equal(before[n], after[n]) for n in before)
            assert (_record(pool.session(sids[0]).tracklets), _record(pool.session(sids[0]).dead_tracklets)) == rec
            assert not pool.session(sids[0]).detached
        else:
            pool.update_4d(req)
        for k in range(3):
            assert same_bits(state_of(pool.session(sids[k]).tracker), state_of(solos[k])), (f, k)
    assert f == len(vis) - 1 and len(pool.session(sids[0]).tracklets) > 0
