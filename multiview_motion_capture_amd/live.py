"""Many live camera rigs, frame by frame: a pool of sessions -- one per rig, each with its own calibration -- stepped with
MvTracker.update_4d's semantics in ONE chain-kernel launch per tick (include/mvmc.h: mvmc_chain_run_sessions).

Every session owns one chain of a ChainTracker with a rig per chain.  A tick steps exactly the sessions that delivered a frame; every
other chain sits the launch out (its `active` byte is 0) and keeps its state.  A session's results are bit for bit those of its own
MvTracker.update_4d, because where update_4d would leave its one-launch route the session leaves the shared launch:

* a frame that update_4d would run through the per-stage launches (takes_one_launch), and a frame whose void word comes back non-zero
  (its row is rolled back from the host mirror of the last good tick), DETACH the session: its row's state goes into a one-chain
  ChainTracker on its own HotPath inside a plain MvTracker, whose own update_4d then runs the frame and every later one -- per-stage
  route, widened replay, raise, narrowing after eight calm frames;
* the session RE-ATTACHES on the first tick its solo tracker is back at the pool's t_max: the state is copied back into its row.

The pool's invariant: after every tick, the host mirror that the pool's ChainTracker marks good holds, for every attached session, the
state after its last committed frame (ChainTracker.restore_rows / put_rows keep it).  INTEGRATION.md section C.2."""
from __future__ import annotations

import time
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from . import device as dev
from .common import FrameData
from .motion_capture import MvTracker, commit_tables, pack_frame, takes_one_launch
from .pipeline import HotPath
from .pose_def import KpsFormat, Pose
from .tracker import ChainTracker


class LiveSessionError(RuntimeError):
    """Raised by LivePool.update_4d after the tick when the frames of some detached sessions raised: every other session's frame is
    committed, each failed session is left as it was before its frame.  ``errors``: sid -> the exception its update_4d raised."""

    def __init__(self, errors: Dict[int, BaseException]):
        self.errors = dict(errors)
        super().__init__("live sessions " + "; ".join(f"{sid}: {e}" for sid, e in sorted(self.errors.items())))


def check_open(n_open: int, capacity: int, n_views: int, n_cameras: int, calibs=None) -> None:
    """LivePool.open_session's checks (host only): the pool's camera count, a free slot, and -- given the calibrations -- that none
    carries a lens model (lens.require_pinhole)."""
    if calibs is not None:
        from .lens import require_pinhole
        require_pinhole(calibs, "LivePool.open_session")
    if n_cameras != n_views:
        raise ValueError(f"open_session: {n_cameras} cameras, the pool's sessions have {n_views} (one pool per camera count)")
    if n_open >= capacity:
        raise ValueError(f"open_session: all {capacity} session slots are taken")


def check_tick(open_sids, n_views: int, p_max: int, sids: Sequence, people: Sequence[Sequence[int]]) -> None:
    """A tick's checks (host only), before any device work: every sid open and named once, its frame of n_views views, at most p_max
    people in each.  people[i]: the number of people in every view of session sids[i]'s frame."""
    if len(sids) != len(people):
        raise ValueError(f"update_4d: {len(sids)} sessions, {len(people)} frames")
    seen = set()
    for sid, ppl in zip(sids, people):
        if sid in seen:
            raise ValueError(f"update_4d: session {sid} is named twice in one tick")
        seen.add(sid)
        if sid not in open_sids:
            raise ValueError(f"update_4d: no open session {sid}")
        if len(ppl) != n_views:
            raise ValueError(f"update_4d: session {sid}'s frame has {len(ppl)} views, the pool's sessions have {n_views}")
        for c, n in enumerate(ppl):
            if int(n) > p_max:
                raise ValueError(f"update_4d: session {sid}: more than p_max={p_max} people in view {c}")


class LiveSession:
    """One live rig: ``tracklets`` / ``dead_tracklets`` as MvTracker's (they are the records of an MvTracker, ``tracker``, whose
    update_4d runs the session's frames while it is detached)."""

    def __init__(self, sid: int, slot: int, calibs, hp: HotPath, tracker: MvTracker):
        self.sid, self.slot, self.calibs, self.hp, self.tracker = sid, slot, list(calibs), hp, tracker
        self.detached = False

    @property
    def tracklets(self):
        return self.tracker.tracklets

    @property
    def dead_tracklets(self):
        return self.tracker.dead_tracklets


class LivePool:
    """``capacity`` session slots of one camera count, one p_max and one t_max (MvTracker's defaults: 8, 8), stepped in one launch
    per tick.  Sessions of another camera count go to another pool."""

    def __init__(self, n_views: int, capacity: int, p_max: int = 8, t_max: int = 8, device=None, skel=None):
        from .motion_capture import _d, load_skeleton
        if capacity < 1:
            raise ValueError("LivePool: capacity >= 1")
        d = torch.device(device) if device is not None else _d()
        self.device, self.C, self.P, self.T, self.capacity = d, n_views, p_max, t_max, capacity
        self.skeleton = skel or load_skeleton()
        # free slots hold a placeholder rig (never read: their chains sit every launch out)
        K = np.repeat(np.eye(3)[None], n_views, 0)
        Rt = np.concatenate([np.repeat(np.eye(3)[None], n_views, 0),
                             np.arange(1, n_views + 1, dtype=np.float64)[:, None, None] * np.array([1.0, 0.5, 0.25])[None, :, None]], 2)
        hp0 = HotPath(K, Rt, device=d)
        self._ch = ChainTracker(hp0, capacity, p_max, t_max, rigs=[hp0] * capacity)
        self._in = self._ch.frame_inputs()
        self._sessions: Dict[int, LiveSession] = {}
        self._free = list(range(capacity))
        self._next_sid = 0
        self.timings = dict(pack=0.0, launch=0.0, records=0.0, solo=0.0)   # seconds by part of a tick, accumulated (the probe's split)

    # -- sessions ------------------------------------------------------------------------------------------------------------------
    def open_session(self, calibs) -> int:
        """A new session on the rig ``calibs`` (one Calib per camera, in the views' order); returns its sid."""
        check_open(len(self._sessions), self.capacity, self.C, len(calibs), calibs)
        hp = HotPath(np.array([c.K for c in calibs]), np.array([c.Rt for c in calibs]), device=self.device)   # (as MvTracker._ensure)
        slot = self._free.pop(0)
        self._ch.set_rig(slot, hp)
        self._ch.put_rows([slot], {})          # a fresh tracker's state, on the device and in the good mirror
        sid = self._next_sid
        self._next_sid += 1
        self._sessions[sid] = LiveSession(sid, slot, calibs, hp, MvTracker(self.skeleton, self.P, self.T))
        return sid

    def close_session(self, sid: int) -> LiveSession:
        """Ends a session: its slot's state is reset for the next session; the returned object keeps the tracklets."""
        if sid not in self._sessions:
            raise ValueError(f"close_session: no open session {sid}")
        s = self._sessions.pop(sid)
        self._ch.put_rows([s.slot], {})
        self._free.append(s.slot)
        self._free.sort()
        s.tracker._chain = None
        s.detached = False
        return s

    def session(self, sid: int) -> LiveSession:
        if sid not in self._sessions:
            raise ValueError(f"session: no open session {sid}")
        return self._sessions[sid]

    @property
    def sids(self) -> List[int]:
        return sorted(self._sessions)

    # -- ticks ---------------------------------------------------------------------------------------------------------------------
    def update_4d(self, frames: Dict[int, Tuple[int, List[FrameData]]]) -> None:
        """One tick: update_4d(frm_idx, d_frames) of every session named in ``frames`` (sid -> (frm_idx, List[FrameData])); the
        other sessions are not stepped."""
        items = list(frames.items())
        check_tick(self._sessions, self.C, self.P, [sid for sid, _ in items], [[len(f.poses) for f in fr] for _, (_, fr) in items])
        t0 = time.perf_counter()
        act = self._in["act_np"]
        act.fill(0)
        shared, solo = [], []
        for sid, (fi, fr) in items:
            s = self._sessions[sid]
            if s.detached:
                solo.append((s, fi, fr))
                continue
            n_nodes = pack_frame(self._in["kps_np"], self._in["cnt_np"], s.slot, fr, self.P)
            if takes_one_launch(self._ch, n_nodes, len(s.tracklets)):
                act[s.slot] = 1
                shared.append((s, fi, fr))
            else:
                solo.append((s, fi, fr))
        if shared:
            self._ch.upload_inputs()
        self.timings["pack"] += time.perf_counter() - t0
        self._tick(shared, solo)

    def update_4d_arrays(self, sids: Sequence[int], frm_idxs: Sequence[int], kps25, counts) -> None:
        """One tick from arrays: session sids[i]'s frame frm_idxs[i] is kps25[i] ((C,P,25,3) OpenPose rows, P <= p_max, zero padded)
        with counts[i] ((C,) people per view), through the device ingest (mvmc_ingest: the 25 -> 17 gather and filter_bad_pose) as
        run_chains_fused takes them."""
        sids = [int(s) for s in sids]
        frm_idxs = [int(f) for f in frm_idxs]
        cnt_h = counts.cpu().numpy() if isinstance(counts, torch.Tensor) else np.asarray(counts)
        S = len(sids)
        if len(frm_idxs) != S or cnt_h.ndim != 2 or cnt_h.shape[0] != S or kps25.shape[0] != S:
            raise ValueError(f"update_4d_arrays: {S} sessions, {len(frm_idxs)} frame indices, kps25 {tuple(kps25.shape)}, counts "
                             f"{tuple(cnt_h.shape)}")
        check_tick(self._sessions, self.C, self.P, sids, [list(r) for r in cnt_h])
        if kps25.shape[2] > self.P:
            raise ValueError(f"update_4d_arrays: kps25 holds {kps25.shape[2]} people per view, p_max is {self.P}")
        if S == 0:
            return
        t0 = time.perf_counter()
        d = self.device
        k = torch.as_tensor(kps25).to(d)
        if k.shape[2] < self.P:
            pad = torch.zeros((S, k.shape[1], self.P - k.shape[2]) + tuple(k.shape[3:]), dtype=k.dtype, device=d)
            k = torch.cat([k, pad], 2)
        k17, c17 = dev.ingest(k.contiguous(), torch.as_tensor(np.ascontiguousarray(cnt_h, dtype=np.int32)).to(d))
        n_nodes = c17.sum(1).cpu().numpy()
        act = self._in["act_np"]
        act.fill(0)
        shared, solo, rows, at = [], [], [], []
        for i, sid in enumerate(sids):
            s = self._sessions[sid]
            if not s.detached and takes_one_launch(self._ch, int(n_nodes[i]), len(s.tracklets)):
                act[s.slot] = 1
                shared.append((s, frm_idxs[i], None))
                rows.append(s.slot)
                at.append(i)
            else:
                solo.append((s, frm_idxs[i], i))
        if shared:
            rows_d = torch.as_tensor(rows, dtype=torch.int64).to(d)
            at_d = torch.as_tensor(at, dtype=torch.int64).to(d)
            self._in["kps_d"][rows_d] = k17[at_d]
            self._in["cnt_d"][rows_d] = c17[at_d]
            self._in["act_d"].copy_(self._in["act_h"], non_blocking=True)
        if solo:   # the frames of sessions run solo, as FrameData of the ingested poses (update_4d packs the same numbers back)
            sel = torch.as_tensor([i for _, _, i in solo], dtype=torch.int64).to(d)
            k_h, c_h = k17[sel].cpu().numpy(), c17[sel].cpu().numpy()
            solo = [(s, fi, _frame_data(fi, k_h[j], c_h[j], s.calibs)) for j, (s, fi, _) in enumerate(solo)]
        self.timings["pack"] += time.perf_counter() - t0
        self._tick(shared, solo)

    def _tick(self, shared, solo) -> None:
        ch = self._ch
        if shared:
            t0 = time.perf_counter()
            # the state in front of the tick, for a chain that comes back void: the good host mirror, or on the first launch a snapshot
            snap = None if ch.has_previous else ch.snapshot()
            ch.step_fused(self._in["kps_d"], self._in["cnt_d"], fold_void=False, active=self._in["act_d"])
            host = ch.read_back(raise_on_void=False)
            void = host["void"]
            bad = [s.slot for s, _, _ in shared if void[s.slot] != 0]
            if bad:
                ch.restore_rows(bad, snap)
            t1 = time.perf_counter()
            self.timings["launch"] += t1 - t0
            for s, fi, fr in shared:
                b = s.slot
                if void[b] != 0:
                    if fr is None:    # (update_4d_arrays: the frame as FrameData of the ingested poses in the staging rows)
                        fr = _frame_data(fi, self._in["kps_d"][b].cpu().numpy(), self._in["cnt_d"][b].cpu().numpy(), s.calibs)
                    solo.append((s, fi, fr))
                    continue
                n = int(host["n_tracks"][b])
                commit_tables(s.tracker, fi, host["meta"][b, :n], host["params"][b, :n], host["joints"][b, :n])
            self.timings["records"] += time.perf_counter() - t1
        if not solo:
            return
        t0 = time.perf_counter()
        errors = {}
        for s, fi, fr in solo:
            if not s.detached:
                self._detach(s)
            try:
                s.tracker.update_4d(fi, fr)
            except (ValueError, RuntimeError) as e:     # (update_4d has left the session as it was before the frame)
                errors[s.sid] = e
            if s.tracker._chain.T == self.T:
                self._attach(s)
        self.timings["solo"] += time.perf_counter() - t0
        if errors:
            raise LiveSessionError(errors)

    def _detach(self, s: LiveSession) -> None:
        """The session's row -> a one-chain ChainTracker on its own HotPath, run by its MvTracker's update_4d from now on."""
        solo = ChainTracker(s.hp, 1, self.P, self.T)
        solo.put_rows([0], self._ch.state_rows([s.slot]))
        s.tracker._chain = solo
        s.tracker._calm = 0        # (update_4d counts calm frames only on a widened tracker, and resets the count when it narrows)
        s.detached = True

    def _attach(self, s: LiveSession) -> None:
        """Back into the shared launch: the solo tracker's state -> the session's row (device and good mirror)."""
        self._ch.put_rows([s.slot], s.tracker._chain.state_rows([0]))
        s.tracker._chain = None
        s.detached = False


def _frame_data(fi: int, k17: np.ndarray, c17: np.ndarray, calibs) -> List[FrameData]:
    """One frame of ingested poses (k17 (C,P,17,3), c17 (C,)) as FrameData: update_4d's staging takes back exactly these numbers."""
    return [FrameData(fi, {p: Pose(KpsFormat.COCO, k17[c, p, :, :2].copy(), k17[c, p, :, 2:3].copy(), None) for p in range(int(c17[c]))},
                      calibs[c], c + 1) for c in range(len(calibs))]
