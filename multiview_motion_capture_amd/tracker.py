"""Temporal hot path: MvTracker.update_4d (motion_capture.py:873-963) for a batch of independent
chains (sub-sequences), every stage on the GPU and no host synchronisation inside a step.

Per step and chain: live tracklets + the frame's 2-D poses -> match_spatial_time graph -> ALS ->
tracklet-anchored clusters (warm IK from the previous parameters) and 2-D-only clusters (new tracklets,
cold IK); chains without live tracklets take the match_spatial path, exactly as
associate_tracking does (motion_capture.py:829-835).
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional, Sequence

import numpy as np
import torch

from . import _cabi, device as dev
from .pipeline import HotPath

T_WIDE = 16   # tracklet slots of the repair tier (include/mvmc.h: the stitch and the widest association variant hold 16)


class ChainFlags:
    """The chain kernel's flag words by name.  The comment of mvmcChainBuffers.flags in include/mvmc.h is the specification; this is its
    one restatement on the Python side.  ``words`` is a torch tensor or a NumPy array (it is only sliced) of n_chains chains."""
    CLUSTER, TRACKS, GRAPH, IK_PAIR, RIG = 1, 2, 4, 8, 16     # the bits of a void word (run_chains' overflow word: the first three)
    REPAIRABLE = CLUSTER | TRACKS | GRAPH                      # what repair_chains' wider tables take

    def __init__(self, words, n_chains: int):
        B = n_chains
        self.words, self.B, self._v0 = words, B, B + 4

    @staticmethod
    def length(n_chains: int, n_parts: int) -> int:
        return n_chains * (n_parts + 1) + 8

    done = property(lambda s: s.words[:s.B])                  # the chains' hand-over counters
    timeout = property(lambda s: s.words[s.B])                # != 0: a workgroup waited for its predecessor in vain
    graph = property(lambda s: s.words[s.B + 1])              # != 0: a graph beyond the layout's association variant
    capacity = property(lambda s: s.words[s.B + 2])           # the void bits of all chains but GRAPH, or'ed
    status = property(lambda s: s.words[s.B:s.B + 3])         # the three above: what a shard sends along (parallel.run_sharded)
    void = property(lambda s: s.words[s._v0:s._v0 + s.B])     # per chain: non-zero voids the chain's results
    tickets = property(lambda s: s.words[s._v0 + s.B])        # the ticket counter (the ready queue follows it)

    def host(self) -> "ChainFlags":
        """Device words, up to the ticket counter, on the host: one transfer (synchronises)."""
        return ChainFlags(self.words[:self._v0 + self.B + 1].cpu().numpy(), self.B)


def void_verdict(timeout: int, bits: int, n_void: int, who: str) -> Optional[Exception]:
    """What a launch's words mean to its caller ``who``: the exception to raise, or None.  timeout: the time-out word; bits: the void
    words of the chains, or'ed; n_void: how many are non-zero.  A RuntimeError is the kernel's own failure; a ValueError is data beyond
    a table (the reference has no such caps), which wider tables take -- update_4d replays the frame, repair_chains the chains."""
    F = ChainFlags
    if timeout:
        return RuntimeError(f"{who}: a hand-over between the workgroups of a chain timed out; results are void")
    if bits & F.IK_PAIR:
        return RuntimeError(f"{who}: internal: a meeting of two IK waves timed out (mvmc_ik_pair.h); results are void")
    if bits & F.RIG:
        return ValueError(f"{who}: a chain's rig index is outside [0, n_rigs): no calibration was read, its tables are empty "
                          f"({n_void} chain(s) void)")
    if bits & F.GRAPH:
        return ValueError(f"{who}: a frame's graph has more nodes than the association kernel holds (the chain kernel's small layout: "
                          f"24 without, 32 with tracklets; 80 otherwise) in {n_void} chain(s); repair_chains / run_chains take such data")
    if bits & (F.CLUSTER | F.TRACKS):
        what = [m for bit, m in ((F.CLUSTER, "a cluster, a member or a view block did not fit (k_max / v_max / the frame's poses)"),
                                 (F.TRACKS, "more than t_max live tracklets")) if bits & bit]
        return ValueError(f"{who}: capacity exceeded (" + "; ".join(what) + f") in {n_void} chain(s): their results are void")
    return None


def _verdict_of(timeout, void: np.ndarray, who: str) -> Optional[Exception]:
    return void_verdict(int(timeout), int(np.bitwise_or.reduce(void)), int(np.count_nonzero(void)), who)


def _raise_if_void(timeout, void: np.ndarray, who: str) -> None:
    exc = _verdict_of(timeout, void, who)
    if exc is not None:
        raise exc


def chain_workspace(B: int, n_out: int, C: int, P: int, T: int, K: int, V: int, d, want_info: bool, flags) -> dict:
    """The chain kernel's own buffers -- every pointer of mvmcChainBuffers but the frames, the calibration and the tracker state -- for B
    chains and n_out output frames.  flags: the tensor, or the length of one to allocate (ChainFlags.length)."""
    N, NS, NP = C * P, T + C * P, T + K
    f64, i32 = torch.float64, torch.int32
    e = lambda shape, dt: torch.empty(shape, dtype=dt, device=d)
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=d)
    return dict(
        seed_table=dev.als_seed_table(_cabi.MAX_NODES * _cabi.MAX_NODES, d),
        S_sp=e((B, N, N), torch.float32), W_st=e((B, NS, NS), f64), group_counts=e((B, C + 1), i32),
        labels_sp=e((B, N), i32), labels_st=e((B, NS), i32), n_clusters_sp=z((B,), i32), n_clusters_st=z((B,), i32),
        iters_sp=z((B,), i32), iters_st=z((B,), i32), members=e((B, NP, V), i32), n_members=z((B, NP), i32),
        cold=e((B, NP), torch.uint8), init=e((B, NP, 68), f64), status=e((B, T), i32), n_new=e((B,), i32),
        ik_params=e((B, NP, 68), f64), ik_joints=e((B, NP, 18, 3), f64), ik_info=e((B, NP, 8), f64),
        ik_scratch=dev.stream_buffer("chain_ik", B, (8, _cabi.IK_SCRATCH_DOUBLES), d),
        out_params=e((n_out, T, 68), f64), out_joints=e((n_out, T, 18, 3), f64), out_meta=e((n_out, T, 4), i32),
        out_n_tracks=e((n_out,), i32), out_info=e((n_out, NP, 8), f64) if want_info else None,
        out_als_iters=e((n_out,), i32) if want_info else None, out_phase_cycles=e((B, 8), f64) if want_info else None,
        flags=z((flags,), i32) if isinstance(flags, int) else flags)


def fill_chain_buffers(ints: dict, tensors: dict) -> "_cabi.MvmcChainBuffers":
    """mvmcChainBuffers of ``ints`` (name -> int) and ``tensors`` (name -> tensor, or None: the explicit NULL).  Every field is named."""
    buf = _cabi.MvmcChainBuffers()
    odd = (set(ints) ^ set(buf._INTS)) | (set(tensors) ^ set(buf._PTRS))
    if odd:
        raise ValueError(f"a chain buffer is not named or not known: {sorted(odd)}")
    for name in buf._INTS:
        setattr(buf, name, int(ints[name]))
    for name in buf._PTRS:
        setattr(buf, name, None if tensors[name] is None else tensors[name].data_ptr())
    return buf


def launch_chain(skeleton, buf, d, rig_of_chain: Optional[torch.Tensor] = None, n_rigs: int = 1,
                 active: Optional[torch.Tensor] = None) -> None:
    """One launch of the chain kernel on d's current stream: mvmc_chain_run_sessions with ``active``, mvmc_chain_run_rigs with
    ``rig_of_chain`` alone, mvmc_chain_run with neither (include/mvmc.h: the three are one kernel)."""
    lib, sk, bf = _cabi.load(), ctypes.byref(skeleton), ctypes.byref(buf)
    stream = ctypes.c_void_p(torch.cuda.current_stream(d).cuda_stream)
    rig = None if rig_of_chain is None else ctypes.c_void_p(rig_of_chain.data_ptr())
    if active is not None:
        _cabi.check(lib.mvmc_chain_run_sessions(sk, bf, rig, n_rigs, ctypes.c_void_p(active.data_ptr()), stream), "mvmc_chain_run_sessions")
    elif rig is not None:
        _cabi.check(lib.mvmc_chain_run_rigs(sk, bf, rig, n_rigs, stream), "mvmc_chain_run_rigs")
    else:
        _cabi.check(lib.mvmc_chain_run(sk, bf, stream), "mvmc_chain_run")


def default_caps(n_views: int, p_max: int):
    """(k_max, v_max) that a frame's own size rules out ever exceeding: a new tracklet needs two poses, so at most C P / 2 appear in a
    frame; clusters are disjoint sets of the frame's poses, so one holds at most C P (the reference has neither cap:
    motion_capture.py:417-446, :618-626, :763-808).  The kernels index members by lane: 64 at most."""
    n = n_views * p_max
    return max(1, n // 2), min(n, 64)


class ChainTracker:
    def __init__(self, hp: HotPath, n_chains: int, p_max: int, t_max: int = 8, k_max: Optional[int] = None,
                 v_max: Optional[int] = None, nfev_cold=50, nfev_warm=5, rigs: Optional[Sequence[HotPath]] = None):
        """rigs: one HotPath per chain (all with hp's cameras) -- a calibration per chain, held as a rig stack that set_rig() rewrites row
        by row, and a per-chain `active` byte word: step_fused() then runs mvmc_chain_run_sessions (the live session pool, live.py).
        hp still supplies the skeleton.  Without rigs the tracker is the one-calibration tracker it always was."""
        d = hp.device
        self.hp, self.B, self.P, self.T = hp, n_chains, p_max, t_max
        C = hp.K.shape[0]
        self.C = C
        k_def, v_def = default_caps(C, p_max)
        self.K = k_max or k_def
        self.V = v_max or v_def
        self.nfev_cold, self.nfev_warm = nfev_cold, nfev_warm
        if 2 * p_max > 16 or t_max > T_WIDE or C * p_max + t_max > 80 or t_max + self.K > 64 or self.V > 64:
            raise ValueError(f"ChainTracker: p_max={p_max}, t_max={t_max}, views={C}: the association kernels hold rank 2 p_max <= 16, "
                             f"t_max <= {T_WIDE} and views x p_max + t_max <= 80 graph nodes (more live tracklets than t_max in a frame is "
                             "reported by check())")
        self.F2 = dev.fmats_from_projections(hp.P)
        B, T = n_chains, t_max
        # The tracker state is ONE device allocation with typed views into it: snapshot() / restore() are one copy each (update_4d
        # saves the state in front of every frame), and the per-frame driver reads it back in one transfer (read_back()).
        # overflow -- per chain: bit 0 cluster / view capacity, bit 1 tracklet table, bit 2 a graph the association kernel could not
        # hold (iters < 0); accumulated on the device, read by check(): a non-zero word voids the chain's results
        layout = (("params", (B, T, 68), torch.float64), ("joints", (B, T, 18, 3), torch.float64), ("meta", (B, T, 4), torch.int32),
                  ("n_tracks", (B,), torch.int32), ("next_id", (B,), torch.int32), ("n_dead", (B,), torch.int32),
                  ("slot_src", (B, T), torch.int32), ("overflow", (B,), torch.int32),
                  # the chain kernel's flag words of step_fused (mvmc_chain_run, n_parts = 1): in the same allocation, so that
                  # read_back() brings state and verdict to the host in ONE transfer
                  ("cflags", (ChainFlags.length(B, 1),), torch.int32))
        offs, total = {}, 0
        for name, shape, dt in layout:
            nbytes = int(torch.Size(shape).numel()) * (8 if dt == torch.float64 else 4)
            offs[name] = (total, nbytes, shape, dt)
            total += (nbytes + 15) & ~15
        self._flat = torch.zeros((total,), dtype=torch.uint8, device=d)
        self._layout = offs
        for name in offs:
            setattr(self, name, self._field(self._flat, name))
        self.slot_src.fill_(-1)
        self.frame_idx = torch.arange(B, dtype=torch.int32, device=d)
        # two pinned host mirrors of _flat, allocated by read_back() and written alternately: the one NOT written by a call holds the
        # state after the last frame that went through, i.e. the state in front of this one -- what restore_previous() brings back
        # without a per-frame device snapshot
        self._host = None
        self._host_good = -1   # index of the mirror that holds the last good state (-1: none yet)
        self._host_prev = -1   # _host_good as the last read_back() found it: the mirror of the frame before (restore_rows())
        self._fused = None  # workspaces of step_fused (allocated on first use)
        self._fused_args = None   # (key, MvmcChainBuffers) of the last step_fused call: the struct is rebuilt only when a pointer changes
        self._in = None     # pinned host staging + device buffers of one frame's inputs (frame_inputs())
        self._void_pending = False   # step_fused(fold_void=False) left its void words for read_back()
        self.events = None  # set to a list to collect (start, end) CUDA events around every IK launch
        self.als_events = None  # same for the association (ALS) launches of the spatio-temporal graph
        self.assoc_done = None
        self.rig_stack = None     # (P (B,C,3,4), F (B,C,C,3,3) f32, F2 (B,C,C,3,3)) with rigs: chain b runs on row b
        self.rig_of_chain = None
        self.active = None        # (B) u8 device with rigs: 0 = the chain sits step_fused's launch out
        if rigs is not None:
            if len(rigs) != n_chains:
                raise ValueError(f"ChainTracker: {len(rigs)} rigs for {n_chains} chains (one per chain)")
            self.rig_stack = stack_rigs(rigs, C)
            self.rig_of_chain = torch.from_numpy(check_rig_of_chain(np.arange(B), B, B)).to(d)
            self.active = torch.ones((B,), dtype=torch.uint8, device=d)

    def _field(self, flat: torch.Tensor, name: str) -> torch.Tensor:
        """Field ``name`` of ``flat``, a buffer laid out as _flat is (the state itself, a snapshot or a host mirror)."""
        o, nb, shape, dt = self._layout[name]
        return flat[o:o + nb].view(dt).view(shape)

    def set_rig(self, b: int, hp: HotPath) -> None:
        """Row b of the rig stack := hp's calibration (a live session opening on chain b)."""
        if self.rig_stack is None:
            raise ValueError("ChainTracker.set_rig: the tracker was built without rigs")
        if hp.P.shape[0] != self.C:
            raise ValueError(f"ChainTracker.set_rig: {hp.P.shape[0]} cameras, the tracker has {self.C}")
        Pm, Fm, F2 = self.rig_stack
        Pm[b].copy_(hp.P)
        Fm[b].copy_(hp.F)
        F2[b].copy_(dev.fmats_from_projections(hp.P))

    def step(self, kps17: torch.Tensor, counts: torch.Tensor, want_debug=False):
        """kps17 (B,C,P,17,3) f64 + counts (B,C) i32 of the current frame of every chain."""
        B, C, P, T, K, V = self.B, self.C, self.P, self.T, self.K, self.V
        hp = self.hp
        has = (self.n_tracks > 0)
        # chains without tracklets: match_spatial (f32 affinity); the others get zero people there
        cnt_sp = torch.where(has[:, None], torch.zeros_like(counts), counts)
        _, S = dev.affinity(kps17, cnt_sp, hp.F, want_D=False)
        sp = dev.als_associate(S, cnt_sp, g_max=P)
        # chains with tracklets: match_spatial_time graph
        W, D, gc = dev.st_affinity(kps17, counts, self.frame_idx, self.joints, self.n_tracks, hp.P, self.F2,
                                   want_D=want_debug)
        if self.als_events is not None:
            a0, a1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a0.record()
        st = dev.als_associate(W, gc, g_max=max(P, T), want_mats=want_debug)
        if self.als_events is not None:
            a1.record()
            self.als_events.append((a0, a1))
        self.overflow |= (((sp["iters"] < 0) | (st["iters"] < 0)).to(torch.int32) * 4)
        mem, cold, init, status, n_new = dev.track_assign(sp["labels"], sp["n_clusters"], st["labels"],
                                                          st["n_clusters"], counts, self.frame_idx, self.n_tracks,
                                                          self.params, P, K, V, overflow=self.overflow)
        NP = T + K
        if self.assoc_done is not None:   # one-shot marker for run_chains' stream stagger
            self.assoc_done.record()
            self.assoc_done = None
        if self.events is not None:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        p, j, info = dev.ik_solve(kps17, hp.P, mem.reshape(B * NP, V), init.reshape(B * NP, 68),
                                  cold.reshape(B * NP), self.nfev_cold, self.nfev_warm, hp.skeleton)
        if self.events is not None:
            e1.record()
            self.events.append((e0, e1))
        p, j = p.reshape(B, NP, 68), j.reshape(B, NP, 18, 3)
        dev.track_commit(status, n_new, p, j, self.params, self.joints, self.meta, self.n_tracks, self.next_id,
                         self.n_dead, K, slot_src=self.slot_src, overflow=self.overflow)
        out = dict(members=mem, status=status, n_new=n_new, ik_params=p, ik_joints=j, ik_info=info.reshape(B, NP, 8))
        if want_debug:
            out.update(D=D, W=W, st=st, sp=sp, group_counts=gc)
        return out

    def frame_inputs(self):
        """Staging for the per-frame driver (MvTracker.update_4d): ONE pinned host buffer and ONE device buffer that hold a frame's
        keypoints (B,C,P,17,3) f64 and counts (B,C) i32 side by side -- the caller fills the NumPy views `kps_np` / `cnt_np`, calls
        upload_inputs() (one asynchronous copy instead of two pageable ones), and hands `kps_d` / `cnt_d` to step_fused() / step().
        The buffers are reused by the next frame: the driver synchronises at the end of every frame (read_back())."""
        if self._in is None:
            B, C, P = self.B, self.C, self.P
            nk, nc = B * C * P * 17 * 3 * 8, B * C * 4
            na = B if self.active is not None else 0     # (with rigs: the chains' active bytes travel with the frame, `act_np` / `act_d`)
            total = nk + ((nc + 15) & ~15) + ((na + 15) & ~15)
            host = torch.empty((total,), dtype=torch.uint8).pin_memory()
            devb = torch.empty((total,), dtype=torch.uint8, device=self._flat.device)
            self._in = dict(host=host, dev=devb,
                            kps_np=host[:nk].view(torch.float64).view(B, C, P, 17, 3).numpy(),
                            cnt_np=host[nk:nk + nc].view(torch.int32).view(B, C).numpy(),
                            kps_d=devb[:nk].view(torch.float64).view(B, C, P, 17, 3),
                            cnt_d=devb[nk:nk + nc].view(torch.int32).view(B, C))
            if na:
                a0 = nk + ((nc + 15) & ~15)
                self._in.update(act_h=host[a0:a0 + na], act_np=host[a0:a0 + na].numpy(), act_d=devb[a0:a0 + na])
        return self._in

    def upload_inputs(self) -> None:
        self._in["dev"].copy_(self._in["host"], non_blocking=True)

    def step_fused(self, kps17: torch.Tensor, counts: torch.Tensor, fold_void: bool = True, active: Optional[torch.Tensor] = None):
        """The same frame update as step() in ONE launch (mvmc_chain_run with chain_len 1 on this tracker's state): what
        the per-frame call surface (MvTracker.update_4d) uses.  Sizes outside the chain kernel's arena, or a frame whose graph
        is too large for it, are the caller's to route to step() (ChainTracker.fused_ok, check_chain_flags).
        fold_void=False: the launch's per-chain void words are NOT folded into the tracker's own (one small kernel less per frame) --
        for a caller that ends the frame with read_back(), which then reads them where the launch left them.
        A tracker with rigs runs mvmc_chain_run_sessions: chain b on rig row b, and only the chains whose byte in ``active`` ((B) u8 device,
        default: the tracker's own `active`) is non-zero -- an idle chain's state and words are left as they were."""
        B, d = self.B, kps17.device
        if self._fused is None:
            self._fused = chain_workspace(B, B, self.C, self.P, self.T, self.K, self.V, d, False, self.cflags)
        w = self._fused
        # the argument struct: every pointer in it but the frame's inputs belongs to this tracker, and the per-frame driver hands in
        # the same input buffers every frame (frame_inputs()) -- built once, rebuilt when an input pointer changes
        if active is None and self.rig_stack is not None:
            active = self.active
        Pm, Fm, F2 = self.rig_stack if self.rig_stack is not None else (self.hp.P, self.hp.F, self.F2)
        key = (kps17.data_ptr(), counts.data_ptr(), self.nfev_cold, self.nfev_warm, Pm.data_ptr(), Fm.data_ptr(), F2.data_ptr(),
               None if active is None else active.data_ptr())
        if self._fused_args is None or self._fused_args[0] != key:
            ints = dict(n_chains=B, chain_len=1, n_views=self.C, p_max=self.P, t_max=self.T, k_max=self.K, v_max=self.V,
                        max_nfev_cold=self.nfev_cold, max_nfev_warm=self.nfev_warm, n_inits=3, seed_len=w["seed_table"].numel(),
                        n_parts=1, force_big=0, hand_over=0)
            state = {name: getattr(self, name) for name in self._STATE}
            self._fused_args = (key, fill_chain_buffers(ints, dict(w, kps17=kps17, counts=counts, Pmats=Pm, Fmats=Fm, F2=F2, **state)))
        if active is not None and (active.dtype != torch.uint8 or active.numel() != B or active.device != d):
            raise ValueError(f"ChainTracker.step_fused: active must be ({B},) uint8 on {d}")
        launch_chain(self.hp.skeleton, self._fused_args[1], d, self.rig_of_chain, 1 if self.rig_of_chain is None else B, active)
        # the launch zeroes its flag words: fold this frame's per-chain void words into the tracker's own (read by check())
        void = ChainFlags(self.cflags, B).void
        self._void_pending = not fold_void
        if fold_void:
            self.overflow |= void
        return dict(members=w["members"], n_members=w["n_members"], status=w["status"], n_new=w["n_new"], ik_params=w["ik_params"],
                    ik_joints=w["ik_joints"], ik_info=w["ik_info"], flags=w["flags"], void=void, n_chains=B, chain_len=1)

    def check(self) -> None:
        """Raise if a capacity was exceeded since the last call (synchronises), and clear the words: the report is per call, so a
        caller that restores the state it saved before the frame (snapshot / restore) can go on -- MvTracker.update_4d does, with a
        wider table.  The reference has no such caps, so a frame that hits one is not tracked the way the reference would."""
        void, timeout = self.overflow.cpu().numpy(), 0
        if self._fused is not None:
            fl = ChainFlags(self.cflags, self.B)
            host = fl.host()
            fl.status.zero_()
            timeout = host.timeout
            if self._void_pending:      # (step_fused(fold_void=False) left the frame's void words where the launch wrote them)
                void = void | host.void
        self._void_pending = False
        self.overflow.zero_()
        _raise_if_void(timeout, void, "ChainTracker")

    _STATE = ("params", "joints", "meta", "n_tracks", "next_id", "n_dead", "slot_src")

    def snapshot(self):
        """The tracker state (one device copy): restore() brings it back, e.g. to redo a frame that exceeded a capacity."""
        return self._flat.clone()

    def restore(self, snap) -> None:
        self._flat.copy_(snap)
        self.overflow.zero_()

    def read_back(self, raise_on_void: bool = True):
        """The state on the host after ONE transfer and ONE synchronisation (the per-frame driver's end of frame): dict of NumPy views
        (params, joints, meta, n_tracks, ..., overflow, cflags) of one of two pinned buffers (the call after next overwrites it), and
        ``void``: every chain's void word, the launch's or'ed with the tracker's own.  Raises like check() if one is set; the words
        that made it raise are cleared on the device (nothing is cleared on a frame that went through: the next launch zeroes its own).
        raise_on_void=False (the live session pool): a void chain does not raise -- the mirror is marked good all the same, and the
        caller brings the chains of non-zero out["void"] back with restore_rows().  A hand-over time-out still raises."""
        n, B = self._flat.numel(), self.B
        if self._host is None:
            self._host = [torch.empty((n,), dtype=torch.uint8).pin_memory() for _ in range(2)]
        cur = 1 - self._host_good if self._host_good >= 0 else 0
        self._host_prev = self._host_good
        h = self._host[cur]
        h[:n].copy_(self._flat, non_blocking=True)          # (state AND the chain kernel's flag words: `cflags` is part of _flat)
        torch.cuda.current_stream(self._flat.device).synchronize()
        out = {name: self._field(h, name).numpy() for name in self._layout}
        void, timeout = out["overflow"].copy(), 0
        if self._fused is not None:
            host = ChainFlags(out["cflags"], B)
            timeout = host.timeout
            if self._void_pending:      # (step_fused(fold_void=False): read where the launch left them)
                void |= host.void
        self._void_pending = False
        out["void"] = void
        # clear what was set -- on the device only when something WAS set (the next launch zeroes its own words anyway): the common
        # frame ends with one transfer, one synchronisation and no further kernel
        if timeout or void.any():
            self.overflow.zero_()
            if timeout:
                fl = ChainFlags(self.cflags, B)
                fl.status.zero_(); fl.void.zero_()
            _raise_if_void(timeout, void if raise_on_void else void[:0], "ChainTracker")
        self._host_good = cur
        return out

    @property
    def has_previous(self) -> bool:
        """Whether read_back() has left a host mirror of the state after the last good frame (restore_previous())."""
        return self._host_good >= 0

    def restore_previous(self) -> None:
        """The state after the last frame that read_back() returned for -- the state in front of a frame that has just failed --
        back onto the device, from the pinned mirror (the per-frame driver then needs no device snapshot in front of every frame)."""
        self._flat.copy_(self._host[self._host_good][:self._flat.numel()], non_blocking=True)
        self.overflow.zero_()

    def _write_rows(self, rows, source) -> None:
        """Rows ``rows`` of every state field and of the overflow word := source(name, shape of the rows, dtype), a host tensor -- on the
        device and in the host mirror marked good, if there is one."""
        rows_h = torch.from_numpy(rows)
        rows_d = rows_h.to(self._flat.device)
        good = self._host[self._host_good] if self.has_previous else None
        for name in self._STATE + ("overflow",):
            _, _, shape, dt = self._layout[name]
            src = source(name, (rows.size,) + tuple(shape[1:]), dt)
            getattr(self, name)[rows_d] = src.to(rows_d.device)
            if good is not None:
                self._field(good, name)[rows_h] = src

    def restore_rows(self, rows, snap: Optional[torch.Tensor] = None) -> None:
        """Per-chain restore_previous(), for a read_back(raise_on_void=False) that found some chains void: the rows of ``rows`` come back,
        in every state field, from the host mirror of the read before (or from ``snap``, a device snapshot taken in front of the launch,
        when there was none) -- on the device AND in the mirror that read_back has just marked good, so that this mirror holds, for every
        chain, the state after its last committed frame (a void of another chain on the next frame restores from it)."""
        rows = np.asarray(rows, dtype=np.int64).reshape(-1)
        if rows.size == 0:
            return
        if snap is None and self._host_prev < 0:
            raise ValueError("ChainTracker.restore_rows: no host mirror of an earlier frame and no snapshot")
        before = snap if snap is not None else self._host[self._host_prev]
        at = torch.from_numpy(rows).to(before.device)
        self._write_rows(rows, lambda name, shape, dt: torch.zeros(shape, dtype=dt) if name == "overflow"
                         else self._field(before, name)[at].cpu())

    def put_rows(self, rows, state: dict) -> None:
        """Rows ``rows`` of the state := ``state`` (field -> host array of len(rows) rows; fields not named are reset to a fresh
        tracker's: zeros, slot_src -1), on the device and in the host mirror marked good, if there is one."""
        self._write_rows(np.asarray(rows, dtype=np.int64).reshape(-1), lambda name, shape, dt:
                         torch.as_tensor(np.ascontiguousarray(state[name])).to(dt).reshape(shape) if name in state
                         else torch.full(shape, -1 if name == "slot_src" else 0, dtype=dt))

    def state_rows(self, rows) -> dict:
        """Rows ``rows`` of the device state (every field of _STATE) as host arrays (synchronises)."""
        idx = torch.as_tensor(np.asarray(rows, dtype=np.int64).reshape(-1)).to(self._flat.device)
        return {name: getattr(self, name)[idx].cpu().numpy() for name in self._STATE}

    def _resized(self, t_max: int) -> "ChainTracker":
        """A tracker of t_max tracklet slots (no rigs) holding this one's state, as many slots of it as both have."""
        r = ChainTracker(self.hp, self.B, self.P, t_max, nfev_cold=self.nfev_cold, nfev_warm=self.nfev_warm)
        T = min(self.T, t_max)
        for name in ("params", "joints", "meta", "slot_src"):
            getattr(r, name)[:, :T] = getattr(self, name)[:, :T]
        for name in ("n_tracks", "next_id", "n_dead"):
            getattr(r, name).copy_(getattr(self, name))
        r.frame_idx = self.frame_idx
        return r

    def widened(self, t_max: int) -> "ChainTracker":
        """A tracker with t_max tracklet slots (> the present number) holding this tracker's state."""
        return self._resized(t_max)

    def narrowed(self, t_max: int) -> "ChainTracker":
        """The inverse of widened(): a tracker with t_max slots holding this one's first t_max (no chain may have more live tracklets
        than that) -- back on the tables the chain kernel runs on once a crowded scene has thinned out."""
        if int(self.n_tracks.max()) > t_max:      # (live tracklets occupy the first n_tracks slots: track_commit compacts the table)
            raise ValueError(f"ChainTracker.narrowed: a chain has more than {t_max} live tracklets")
        return self._resized(t_max)

    @property
    def fused_ok(self) -> bool:
        """Whether this tracker's padded sizes fit the chain kernel (include/mvmc.h: mvmc_chain_run)."""
        N = self.C * self.P
        small = N <= 40 and self.T + N <= 48 and self.T <= 8
        big = N <= 64 and self.T + N <= 80 and self.T <= T_WIDE
        return (small or big) and self.P <= 8 and self.C <= 16 and self.T + self.K <= 64


def run_chains(hp: HotPath, kps: torch.Tensor, counts: Optional[torch.Tensor], chain_len: int, t_max=8,
               nfev_cold=50, nfev_warm=5, events=None, want_info=False, n_groups=1, als_events=None, k_max: Optional[int] = None,
               v_max: Optional[int] = None):
    """Whole shard: frames [c*L, (c+1)*L) form chain c (F must be a multiple of L).  Returns per-frame
    tracklet tables: params (F,T,68), joints (F,T,18,3), meta (F,T,4), n_tracks (F).

    n_groups > 1 splits the chains into that many groups, each advanced on its own HIP stream: inside a chain the
    stages of a frame are strictly sequential (association -> assignment -> IK -> commit -> next frame), and the
    association solver is a long dependent chain on few waves, so one group's association runs in the shadow of
    another group's IK launch.  Results do not depend on n_groups (chains are independent)."""
    F, C, P = kps.shape[:3]
    L = chain_len
    if F % L:
        raise ValueError("run_chains: the frame count must be a multiple of the chain length")
    B = F // L
    G = max(1, min(int(n_groups), B))
    kps17, cnt = dev.ingest(kps, counts)
    k4 = kps17.view(B, L, C, P, 17, 3)
    c4 = cnt.view(B, L, C)
    d = kps.device
    out_p = torch.empty((B, L, t_max, 68), dtype=torch.float64, device=d)
    out_j = torch.empty((B, L, t_max, 18, 3), dtype=torch.float64, device=d)
    out_m = torch.empty((B, L, t_max, 4), dtype=torch.int32, device=d)
    out_n = torch.empty((B, L), dtype=torch.int32, device=d)
    n_dead = torch.empty((B,), dtype=torch.int32, device=d)
    next_id = torch.empty((B,), dtype=torch.int32, device=d)
    overflow = torch.empty((B,), dtype=torch.int32, device=d)
    bounds = [B * g // G for g in range(G + 1)]
    main = torch.cuda.current_stream(d)
    streams = [main] if G == 1 else [torch.cuda.Stream(device=d) for _ in range(G)]
    ready = torch.cuda.Event()
    ready.record(main)
    trackers, infos = [], [[] for _ in range(G)]
    for g in range(G):
        with torch.cuda.stream(streams[g]):
            streams[g].wait_event(ready)
            tr = ChainTracker(hp, bounds[g + 1] - bounds[g], P, t_max, k_max=k_max, v_max=v_max, nfev_cold=nfev_cold, nfev_warm=nfev_warm)
            tr.events = events
            tr.als_events = als_events
            trackers.append(tr)
    # stagger: group g starts once group g-1 has finished the association of its first frame, so that from then on
    # the association launches of one group and the IK launches of another alternate instead of colliding
    stagger = [torch.cuda.Event() for _ in range(G - 1)]
    for g in range(G - 1):
        trackers[g].assoc_done = stagger[g]
    for t in range(L):
        for g in range(G):
            b0, b1 = bounds[g], bounds[g + 1]
            with torch.cuda.stream(streams[g]):
                tr = trackers[g]
                if t == 0 and g > 0:
                    streams[g].wait_event(stagger[g - 1])
                o = tr.step(k4[b0:b1, t].contiguous(), c4[b0:b1, t].contiguous())
                if want_info:
                    infos[g].append(o["ik_info"])
                out_p[b0:b1, t], out_j[b0:b1, t], out_m[b0:b1, t], out_n[b0:b1, t] = tr.params, tr.joints, tr.meta, tr.n_tracks
    for g in range(G):
        with torch.cuda.stream(streams[g]):
            n_dead[bounds[g]:bounds[g + 1]] = trackers[g].n_dead
            next_id[bounds[g]:bounds[g + 1]] = trackers[g].next_id
            overflow[bounds[g]:bounds[g + 1]] = trackers[g].overflow
        if streams[g] is not main:
            main.wait_stream(streams[g])
    res = dict(params=out_p.view(F, t_max, 68), joints=out_j.view(F, t_max, 18, 3), meta=out_m.view(F, t_max, 4),
               n_tracks=out_n.view(F), n_dead=n_dead, next_id=next_id, overflow=overflow)
    if want_info:
        res["ik_info"] = torch.cat([torch.stack(i, 1) for i in infos], 0)
    return res


def run_chains_fused(hp: HotPath, kps: torch.Tensor, counts: Optional[torch.Tensor], chain_len: int, t_max: Optional[int] = None,
                     nfev_cold=50, nfev_warm=5, want_info=False, k_max: Optional[int] = None, v_max: Optional[int] = None,
                     parts: Optional[int] = None, kernel_events: Optional[list] = None, force_big: bool = False,
                     hand_over: Optional[str] = None, rigs: Optional[Sequence[HotPath]] = None, rig_of_chain=None):
    """run_chains in ONE launch (mvmc_chain_run): a persistent workgroup per chain runs graph -> ALS -> assignment ->
    IK -> commit for the chain's frames, so every chain advances at its own pace instead of waiting, stage by stage,
    for the slowest member of every launch.  Same device code and the same results as run_chains.
    parts > 1 (a divisor of chain_len): every chain is run by that many workgroups, one frame range after the other
    (hand-over through device flags), which lets the hardware dispatcher even out the load when the number of chains is
    not a multiple of the number of workgroup slots.  check_chain_flags(res) tells whether the run is valid.
    kernel_events: a list that receives the (start, end) torch.cuda.Event pair recorded right around the kernel launch.
    hand_over: "ticket" (default: a workgroup draws a ticket when it starts, ticket = part * n_chains + chain; a part's predecessor
    holds a lower ticket, so it has started: no assumption about the order of dispatch), "static" (the same mapping by block index:
    relies on in-order dispatch, bounded wait) or "queue" (ready queue: a freed slot goes to the chain that has been ready longest;
    no assumption either, ~3 % slower).  Same results bit for bit.
    rigs / rig_of_chain: a calibration per chain (mvmc_chain_run_rigs) -- ``rigs`` is a sequence of HotPath, one per rig, all with the
    cameras of ``kps``; chain b uses rigs[rig_of_chain[b]] (a host integer array of length B, checked here).  ``hp`` still supplies the
    skeleton.  With rigs=None the call is exactly the one-rig launch (mvmc_chain_run)."""
    F, Cn, P = kps.shape[:3]
    L = chain_len
    if F % L:
        raise ValueError("run_chains_fused: the frame count must be a multiple of the chain length")
    B = F // L
    if rigs is None and rig_of_chain is not None:
        raise ValueError("run_chains_fused: rig_of_chain needs rigs")
    roc = None if rigs is None else check_rig_of_chain(rig_of_chain, B, len(rigs))
    if parts is None:
        parts = L   # one workgroup per chain-frame: the finest hand-over, the best balance
    if parts > 1 and L % parts:
        raise ValueError("run_chains_fused: parts must divide the chain length")
    if hand_over is None:
        hand_over = "ticket"
    if hand_over not in ("static", "queue", "ticket"):
        raise ValueError("run_chains_fused: hand_over must be 'ticket', 'static' or 'queue'")
    # tracklet slots: 8 on the SMALL layout (views x people <= 40: its association variants hold rank 16), 16 on the BIG one (C8 P8),
    # whose workgroup takes a frame with a ninth tracklet (rank 18, 73 nodes) through its generic association variant in place
    T = t_max if t_max is not None else (T_WIDE if Cn * P > 40 else 8)
    k_def, v_def = default_caps(Cn, P)
    K = k_max or k_def
    V = v_max or v_def
    kps17, cnt = dev.ingest(kps, counts)
    d = kps.device
    if rigs is None:
        Pm, Fm, F2 = hp.P, hp.F, dev.fmats_from_projections(hp.P)
    else:
        Pm, Fm, F2 = stack_rigs(rigs, Cn)
    f64, i32 = torch.float64, torch.int32
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=d)
    t = dict(chain_workspace(B, F, Cn, P, T, K, V, d, want_info, ChainFlags.length(B, parts)),
             kps17=kps17, counts=cnt, Pmats=Pm, Fmats=Fm, F2=F2,
             params=z((B, T, 68), f64), joints=z((B, T, 18, 3), f64), meta=z((B, T, 4), i32), n_tracks=z((B,), i32),
             next_id=z((B,), i32), n_dead=z((B,), i32), slot_src=torch.full((B, T), -1, dtype=i32, device=d))
    ints = dict(n_chains=B, chain_len=L, n_views=Cn, p_max=P, t_max=T, k_max=K, v_max=V, max_nfev_cold=nfev_cold,
                max_nfev_warm=nfev_warm, n_inits=3, seed_len=t["seed_table"].numel(), n_parts=parts, force_big=int(force_big),
                hand_over={"static": 0, "queue": 1, "ticket": 2}[hand_over])
    buf = fill_chain_buffers(ints, t)
    rig_dev = None if roc is None else torch.from_numpy(roc).to(d)
    if kernel_events is not None:
        k0, k1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        k0.record()
    launch_chain(hp.skeleton, buf, d, rig_dev, 1 if rigs is None else len(rigs))
    if kernel_events is not None:
        k1.record()
        kernel_events.append((k0, k1))
    # void_words: {a hand-over time-out, a graph too large for the layout's association, a capacity exceeded} -- non-zero = the step is
    # void unless repair_chains clears it; parallel.run_sharded sends them along, so every rank learns of a void step from the gathered
    # messages instead of each rank reading its own words back before the collective
    fl = ChainFlags(t["flags"], B)
    res = dict(params=t["out_params"], joints=t["out_joints"], meta=t["out_meta"], n_tracks=t["out_n_tracks"],
               n_dead=t["n_dead"], next_id=t["next_id"], flags=t["flags"], void=fl.void, void_words=fl.status, n_chains=B,
               chain_len=L, _keepalive=dict(t, rig_of_chain=rig_dev))
    if rigs is not None:
        res["rigs"], res["rig_of_chain"] = list(rigs), roc
    if want_info:
        res["ik_info"] = t["out_info"].view(B, L, T + K, 8)
        res["als_iters"] = t["out_als_iters"].view(B, L)
        res["phase_cycles"] = t["out_phase_cycles"]
    return res


def check_rig_of_chain(rig_of_chain, n_chains: int, n_rigs: int) -> np.ndarray:
    """rig_of_chain as the int32 array mvmc_chain_run_rigs reads, checked on the host: length n_chains, every index in [0, n_rigs)."""
    if n_rigs < 1:
        raise ValueError("rigs: at least one rig")
    if rig_of_chain is None:
        if n_rigs != 1:
            raise ValueError("rig_of_chain: needed with more than one rig")
        return np.zeros(n_chains, dtype=np.int32)
    if isinstance(rig_of_chain, torch.Tensor):
        rig_of_chain = rig_of_chain.cpu().numpy()
    a = np.asarray(rig_of_chain)
    if a.ndim != 1 or a.shape[0] != n_chains:
        raise ValueError(f"rig_of_chain: {a.shape} for {n_chains} chains")
    if a.size and not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"rig_of_chain: integer indices, not {a.dtype}")
    if a.size and (a.min() < 0 or a.max() >= n_rigs):
        raise ValueError(f"rig_of_chain: indices in [{a.min()}, {a.max()}], the call has {n_rigs} rig(s)")
    return np.ascontiguousarray(a, dtype=np.int32)


def stack_rigs(rigs: Sequence[HotPath], n_views: int):
    """(P (R,C,3,4) f64, F (R,C,C,3,3) f32, F2 (R,C,C,3,3) f64) of R HotPaths of n_views cameras each: mvmc_chain_run_rigs' tables."""
    if len(rigs) == 0:
        raise ValueError("rigs: at least one rig")
    for r, h in enumerate(rigs):
        if h.P.shape[0] != n_views:
            raise ValueError(f"rigs[{r}] has {h.P.shape[0]} cameras, the keypoints {n_views} views")
    Pm = torch.stack([h.P for h in rigs]).contiguous()
    Fm = torch.stack([h.F for h in rigs]).contiguous()
    F2 = torch.stack([dev.fmats_from_projections(h.P) for h in rigs]).contiguous()
    return Pm, Fm, F2


def check_chain_flags(res) -> None:
    """Raise if a run_chains_fused / run_chains result is void (synchronises), as void_verdict says: a hand-over time-out, a frame's
    graph larger than the chain kernel's association variant holds, or a capacity (t_max; k_max / v_max when the caller passed smaller
    ones than default_caps) exceeded.  repair_chains re-runs the chains concerned with wider tables."""
    if "flags" not in res:      # run_chains: per-chain words of the same bits (CLUSTER, TRACKS, GRAPH), no hand-over
        _raise_if_void(0, res["overflow"].cpu().numpy(), "run_chains")
        return
    fl = ChainFlags(res["flags"], res["n_chains"]).host()
    _raise_if_void(fl.timeout, fl.void, "mvmc_chain_run")


def repair_chains(hp: HotPath, kps: torch.Tensor, counts: Optional[torch.Tensor], res, nfev_cold=50, nfev_warm=5,
                  t_wide: int = T_WIDE, big_first: bool = True) -> int:
    """What the reference does where the chain kernel's fixed tables end (it has no caps at all): the chains whose void word is set --
    more live tracklets than t_max, a graph beyond the layout's association variant -- are run again through the per-stage entry
    points with t_wide tracklet slots (association on up to 80 nodes, rank 32), and their rows of ``res`` (run_chains_fused's result,
    same kps / counts) are replaced; the per-frame tables are widened to the slots the repaired chains need.  Synchronises (it reads
    the void words); returns the number of chains repaired.  Raises after a hand-over time-out or if a chain exceeds the repair tier too.
    big_first: chains voided by the SMALL layout go through the chain kernel's BIG layout first (one launch), see below.
    A result of several rigs (run_chains_fused(..., rigs, rig_of_chain)) is repaired with each chain's own calibration; a chain whose
    rig index was out of range (void bit RIG) has nothing to repair: raises."""
    B, L = res["n_chains"], res["chain_len"]
    fl = ChainFlags(res["flags"], B)
    host = fl.host()
    _raise_if_void(host.timeout, host.void & ~ChainFlags.REPAIRABLE, "repair_chains")     # (what wider tables do not mend)
    idx = torch.from_numpy(np.nonzero(host.void)[0]).to(res["flags"].device)
    n = int(idx.numel())
    if n == 0:
        return 0
    rigs = res.get("rigs")
    roc = None if rigs is None else res["rig_of_chain"][idx.cpu().numpy()]
    C, P = kps.shape[1:3]
    k5 = kps.view(B, L, *kps.shape[1:])[idx].reshape(n * L, *kps.shape[1:]).contiguous()
    c5 = None if counts is None else counts.view(B, L, C)[idx].reshape(n * L, C).contiguous()
    sub = None
    if big_first and os.environ.get("MVMC_REPAIR_BIG_FIRST", "1") != "0" and C * P <= 40 and t_wide <= T_WIDE and res["params"].shape[1] <= 8:
        # The chains came from the SMALL layout (views x people <= 40: graphs of <= 32 nodes, 8 tracklet slots, <= 6 views per cluster).
        # What voids there -- a crowded frame of 5 x 6 or 7 x 5, a ninth tracklet -- is inside the BIG layout's tables (80 nodes,
        # 16 slots, 8 views): the same persistent kernel in its 512-thread form takes all of them in ONE launch (bit-identical to the
        # per-stage path, tests/test_gpu_chain_fused.py), which matters when a geometry voids EVERY chain (C5 P6 with everybody in view:
        # measured in tests/test_gpu_capacity_flags.py).  What is beyond that too falls through to the per-stage entry points below.
        big = run_chains_fused(hp, k5, c5, L, t_max=t_wide, nfev_cold=nfev_cold, nfev_warm=nfev_warm, force_big=True, rigs=rigs,
                               rig_of_chain=roc)
        bh = ChainFlags(big["flags"], n).host()
        if _verdict_of(bh.timeout, bh.void, "repair_chains") is None:
            sub = dict(params=big["params"], joints=big["joints"], meta=big["meta"], n_tracks=big["n_tracks"], n_dead=big["n_dead"],
                       next_id=big["next_id"])
    if sub is None:
        if rigs is None:
            sub = run_chains(hp, k5, c5, L, t_max=t_wide, nfev_cold=nfev_cold, nfev_warm=nfev_warm)
        else:
            sub = _run_chains_by_rig(rigs, roc, k5, c5, L, t_wide, nfev_cold, nfev_warm)
        _raise_if_void(0, sub["overflow"].cpu().numpy(), f"repair_chains: the repair tier (t_max = {t_wide}) as well")
    T = res["params"].shape[1]
    need = int(sub["n_tracks"].max())
    if need > T:   # widen the per-frame tables (rare: the repaired chains hold more tracklets than the tables have slots)
        F = B * L
        for k, tail in (("params", (68,)), ("joints", (18, 3)), ("meta", (4,))):
            wide = torch.zeros((F, t_wide) + tail, dtype=res[k].dtype, device=res[k].device)
            wide[:, :T] = res[k]
            res[k] = wide
        T = t_wide
    for k in ("params", "joints", "meta"):
        tail = res[k].shape[2:]
        res[k].view(B, L, T, *tail)[idx] = sub[k].view(n, L, t_wide, *tail)[:, :, :T]
    res["n_tracks"].view(B, L)[idx] = sub["n_tracks"].view(n, L)
    res["n_dead"][idx] = sub["n_dead"]
    res["next_id"][idx] = sub["next_id"]
    fl.void[idx] = 0
    fl.status[1:] = 0      # (graph and capacity: mended)
    res["repaired"] = idx
    return n


def _run_chains_by_rig(rigs, roc: np.ndarray, kps: torch.Tensor, counts: Optional[torch.Tensor], L: int, t_max: int, nfev_cold, nfev_warm):
    """run_chains over chains of several rigs: the chains of each rig as one group with that rig's HotPath, the results in chain order."""
    n = len(roc)
    C = kps.shape[1]
    k4 = kps.view(n, L, *kps.shape[1:])
    c4 = None if counts is None else counts.view(n, L, C)
    out = None
    for r in np.unique(roc):
        sel = np.nonzero(roc == r)[0]
        at = torch.from_numpy(sel).to(kps.device)
        m = len(sel)
        part = run_chains(rigs[int(r)], k4[at].reshape(m * L, *kps.shape[1:]).contiguous(),
                          None if c4 is None else c4[at].reshape(m * L, C).contiguous(), L, t_max=t_max, nfev_cold=nfev_cold,
                          nfev_warm=nfev_warm)
        if out is None:
            out = {k: torch.empty((n * (L if k in _PER_FRAME else 1),) + v.shape[1:], dtype=v.dtype, device=v.device)
                   for k, v in part.items()}
        for k, v in part.items():
            if k in _PER_FRAME:
                out[k].view(n, L, *v.shape[1:])[at] = v.view(m, L, *v.shape[1:])
            else:
                out[k][at] = v
    return out


_PER_FRAME = ("params", "joints", "meta", "n_tracks")
