"""CPU checks of the multi-rig sequence API (sequences.py, tracker.run_chains_fused's rigs / rig_of_chain, include/mvmc.h:
mvmc_chain_run_rigs): the launch layout of a batch of sequences, the stitched tables -> MvTracklet conversion against a per-frame
restatement of update_4d's rule, the host-side argument checks, and the new C entry point."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT


def _calibs(C, seed=0):
    from multiview_motion_capture_amd import synth
    from multiview_motion_capture_amd.common import Calib
    K, Rt, _ = synth.make_cameras(C, np.random.default_rng(seed))
    return [Calib.from_k_rt(K[c], Rt[c]) for c in range(C)]


def _seq(F, C, P, seed=0, fill=1.0):
    kps = np.full((F, C, P, 25, 3), fill, dtype=np.float32)
    counts = np.full((F, C), P, dtype=np.int32)
    return kps, counts, _calibs(C, seed)


# ---- layout -------------------------------------------------------------------------------------------------------------------
def test_groups_by_camera_count_pad_to_chains_and_lay_chains_end_to_end():
    from multiview_motion_capture_amd.sequences import check_sequences, pack_group, plan_groups
    seqs = [_seq(33, 5, 3, fill=1.0), _seq(16, 4, 2, fill=2.0), _seq(1, 5, 4, fill=3.0), _seq(40, 4, 5, fill=4.0), _seq(16, 5, 2, fill=5.0)]
    shapes = check_sequences(seqs)
    assert shapes == [(33, 5, 3), (16, 4, 2), (1, 5, 4), (40, 4, 5), (16, 5, 2)]
    groups = plan_groups(shapes, 16)
    assert [g.n_views for g in groups] == [5, 4]                     # in the order of each count's first sequence
    g5, g4 = groups
    assert g5.seq_ids == [0, 2, 4] and g4.seq_ids == [1, 3]
    assert g5.p_max == 4 and g4.p_max == 5                            # the group's largest P_s
    assert g5.n_chains == [3, 1, 1] and g5.chain_lo == [0, 3, 4] and g5.total_chains == 5
    assert g4.n_chains == [1, 3] and g4.chain_lo == [0, 1] and g4.total_chains == 4
    assert g5.rig_of_chain.dtype == np.int32
    assert g5.rig_of_chain.tolist() == [0, 0, 0, 1, 2] and g4.rig_of_chain.tolist() == [0, 1, 1, 1]
    kps, counts = pack_group(g5, seqs, 16)
    assert kps.shape == (5 * 16, 5, 4, 25, 3) and counts.shape == (80, 5) and kps.dtype == np.float32
    # sequence 0: frames [0, 33) real, [33, 48) empty; its people in slots [0, 3), slot 3 empty
    assert (counts[:33] == 3).all() and (counts[33:48] == 0).all()
    assert (kps[:33, :, :3] == 1.0).all() and (kps[:33, :, 3] == 0).all() and (kps[33:48] == 0).all()
    # sequence 2: one real frame at chain 3, then 15 empty ones; sequence 4 fills chain 4
    assert (counts[48] == 4).all() and (counts[49:64] == 0).all() and (kps[48] == 3.0).all()
    assert (counts[64:80] == 2).all() and (kps[64:80, :, :2] == 5.0).all() and (kps[64:80, :, 2:] == 0).all()


def test_chain_multiples_are_not_padded_further():
    from multiview_motion_capture_amd.sequences import plan_groups
    g, = plan_groups([(32, 5, 4), (48, 5, 4)], 16)
    assert g.n_chains == [2, 3] and g.chain_lo == [0, 2] and g.rig_of_chain.tolist() == [0, 0, 1, 1, 1]
    g, = plan_groups([(7, 3, 1)], 1)
    assert g.n_chains == [7] and g.rig_of_chain.tolist() == [0] * 7


# ---- tables -> MvTracklet ---------------------------------------------------------------------------------------------------------
def _restated(meta, n_tracks, params, joints, gid, L, n_real, frame_idx0):
    """MvTracker.update_4d's bookkeeping (motion_capture.py, update_4d) frame by frame, with update_4d's tracklet id = (chain, local id)
    and the record it feeds = the stitch's global identity of that pair."""
    from multiview_motion_capture_amd.motion_capture import TrackState
    recs, by_local, alive = {}, {}, set()
    for f in range(n_real):
        live = set()
        for s in range(int(n_tracks[f])):
            tid, state, hits, _ = (int(v) for v in meta[f, s])
            key = (f // L, tid)
            g = int(gid[f // L, tid])
            r = recs.setdefault(g, dict(frames=[], rows=[], state=None, last=None, since=0))
            if key not in by_local or hits > by_local[key]:
                r["frames"].append(frame_idx0 + f)
                r["rows"].append((f, s))
                r["since"] = 0
            by_local[key] = hits
            r["state"], r["last"] = state, f
            live.add(g)
        for g in alive | live:
            if g in live and recs[g]["rows"][-1][0] != f:
                recs[g]["since"] += 1
        for g in alive - live:
            if recs[g]["last"] == f - 1:           # noticed missing in this frame: Dead, one more frame since its update
                recs[g]["since"] += 1
                recs[g]["state"] = TrackState.Dead.value
        alive = live
    return recs


def _hand_tables():
    """Two chains of four frames (T = 3), one padded frame at the end: a person carried across the boundary (local 0 -> local 1), one
    who dies inside chain 0, one born in chain 1 whose hits stall for a frame, and a local id the stitch maps to an earlier identity."""
    L, T = 4, 3
    F = 2 * L
    meta = np.zeros((F, T, 4), np.int32)
    n = np.zeros(F, np.int32)
    rows = {   # frame: [(local id, state, hits)]
        0: [(0, 1, 1), (1, 1, 1)],
        1: [(0, 1, 2), (1, 1, 2)],
        2: [(0, 2, 3)],
        3: [(0, 2, 4)],
        4: [(0, 1, 1), (1, 1, 1)],
        5: [(0, 1, 2), (1, 1, 1)],        # local 1 of chain 1: hits did not grow
        6: [(1, 1, 2), (0, 2, 3)],        # (slot order need not follow the id)
        7: [(1, 2, 3)],                   # frame 7 is padding (n_real = 7): dropped
    }
    for f, rr in rows.items():
        n[f] = len(rr)
        for s, (i, st, h) in enumerate(rr):
            meta[f, s] = (i, st, h, h)
    rng = np.random.default_rng(3)
    params = rng.normal(size=(F, T, 68))
    joints = rng.normal(size=(F, T, 18, 3))
    gid = np.full((2, 16), -1, np.int32)
    gid[0, :2] = [0, 1]
    gid[1, :2] = [2, 0]                   # chain 1: local 1 continues identity 0 of chain 0, local 0 is new (identity 2)
    return meta, n, params, joints, gid, L, 7


def test_tables_to_tracklets_matches_the_per_frame_restatement():
    from multiview_motion_capture_amd.motion_capture import MvTracklet, TrackState
    from multiview_motion_capture_amd.sequences import tables_to_tracklets
    meta, n, params, joints, gid, L, n_real = _hand_tables()
    tl = tables_to_tracklets(meta, n, params, joints, gid, L, n_real, frame_idx0=1)
    exp = _restated(meta, n, params, joints, gid, L, n_real, 1)
    assert sorted(t.track_id for t in tl) == sorted(exp) == [0, 1, 2]
    assert [len(t) for t in tl] == sorted((len(t) for t in tl), reverse=True)          # longest first
    for t in tl:
        e = exp[t.track_id]
        assert isinstance(t, MvTracklet)
        assert t.frame_idxs == e["frames"]
        assert t.hits == len(e["frames"])
        assert t.state == TrackState(e["state"])
        assert t.time_since_update == e["since"]
        assert [p[0] for p in t.poses] == e["frames"]
        for (fi, pp, pose), (f, s) in zip(t.poses, e["rows"]):
            x = params[f, s]
            assert np.array_equal(pp.root, x[:3]) and np.array_equal(pp.euler_angles, x[3:57].reshape(18, 3))
            assert np.array_equal(pp.bone_lens, x[57:]) and np.array_equal(pose.keypoints, joints[f, s])
        assert t.last_pose_3d is t.poses[-1][-1]
    by = {t.track_id: t for t in tl}
    # identity 0: frames 0..3 of chain 0, then chain 1's local 1 from its first frame; frame 5 (hits stalled) and the padded frame 7 are
    # not appended; alive in the last real frame (6)
    assert by[0].frame_idxs == [1, 2, 3, 4, 5, 7] and by[0].state == TrackState.Tentative
    # identity 1 dies after frame 1: Dead, one frame since its update
    assert by[1].frame_idxs == [1, 2] and by[1].state == TrackState.Dead and by[1].time_since_update == 1
    assert by[2].frame_idxs == [5, 6, 7] and by[2].state == TrackState.Confirmed


def test_tables_to_tracklets_on_random_tables():
    """Random tables -- ids born and dying at random, hits that stall, identities carried across chain boundaries, a random number of
    padded frames -- give what the per-frame restatement gives."""
    from multiview_motion_capture_amd.sequences import tables_to_tracklets
    rng = np.random.default_rng(11)
    for trial in range(20):
        L, T, B = 5, 6, 4
        F = B * L
        meta = np.zeros((F, T, 4), np.int32)
        n = np.zeros(F, np.int32)
        gid = np.full((B, 16), -1, np.int32)
        next_g = 0
        for b in range(B):
            live, nid = {}, 0
            for t in range(L):
                f = b * L + t
                for i in list(live):
                    if rng.uniform() < 0.15:
                        del live[i]
                    elif rng.uniform() < 0.8:
                        live[i] += 1
                while len(live) < T and rng.uniform() < 0.4 and nid < 16:
                    live[nid] = 1
                    nid += 1
                order = rng.permutation(list(live)) if live else []
                n[f] = len(order)
                for s, i in enumerate(order):
                    meta[f, s] = (i, 1 + int(live[i] >= 3), live[i], live[i])
            for i in range(nid):   # a third of the ids continue an identity of the previous chain
                if b and rng.uniform() < 0.33 and next_g:
                    gid[b, i] = rng.integers(0, next_g)
                else:
                    gid[b, i] = next_g
                    next_g += 1
        params = rng.normal(size=(F, T, 68))
        joints = rng.normal(size=(F, T, 18, 3))
        n_real = int(rng.integers(F - L + 1, F + 1))
        tl = tables_to_tracklets(meta, n, params, joints, gid, L, n_real)
        exp = _restated(meta, n, params, joints, gid, L, n_real, 0)
        assert {t.track_id for t in tl} == set(exp)
        for t in tl:
            e = exp[t.track_id]
            assert t.frame_idxs == e["frames"], trial
            assert t.hits == len(e["frames"])
            assert t.state.value == e["state"], trial
            assert t.time_since_update == e["since"], trial


def test_tables_to_tracklets_edge_cases():
    from multiview_motion_capture_amd.sequences import tables_to_tracklets
    meta, n, params, joints, gid, L, n_real = _hand_tables()
    assert tables_to_tracklets(meta, n * 0, params, joints, gid, L, n_real) == []
    assert tables_to_tracklets(meta, n, params, joints, gid, L, 0) == []
    bad = gid.copy()
    bad[1, 1] = -1
    with pytest.raises(ValueError, match="global identity"):
        tables_to_tracklets(meta, n, params, joints, bad, L, n_real)


# ---- host validation ---------------------------------------------------------------------------------------------------------------
def test_sequence_checks():
    from multiview_motion_capture_amd.sequences import check_sequences, track_sequences
    with pytest.raises(ValueError, match="no sequences"):
        track_sequences([])
    kps, counts, calibs = _seq(4, 5, 2)
    with pytest.raises(ValueError, match="calibrations for 5 cameras"):
        check_sequences([(kps, counts, calibs[:4])])
    with pytest.raises(ValueError, match="counts must be"):
        check_sequences([(kps, counts[:, :4], calibs)])
    with pytest.raises(ValueError, match="counts outside"):
        check_sequences([(kps, counts + 1, calibs)])
    with pytest.raises(ValueError, match=r"\(F,C,P,25,3\)"):
        check_sequences([(kps[..., :2], counts, calibs)])


def test_rig_of_chain_checks():
    from multiview_motion_capture_amd.tracker import check_rig_of_chain
    assert check_rig_of_chain([0, 1, 1, 2], 4, 3).dtype == np.int32
    assert check_rig_of_chain(None, 3, 1).tolist() == [0, 0, 0]
    with pytest.raises(ValueError, match="needed"):
        check_rig_of_chain(None, 3, 2)
    with pytest.raises(ValueError, match="for 4 chains"):
        check_rig_of_chain([0, 1, 1], 4, 3)
    with pytest.raises(ValueError, match="for 4 chains"):
        check_rig_of_chain(np.zeros((2, 2), int), 4, 3)
    with pytest.raises(ValueError, match="has 3 rig"):
        check_rig_of_chain([0, 1, 3, 2], 4, 3)
    with pytest.raises(ValueError, match="has 3 rig"):
        check_rig_of_chain([0, -1, 1, 2], 4, 3)
    with pytest.raises(ValueError, match="integer"):
        check_rig_of_chain([0.0, 1.0], 2, 3)
    with pytest.raises(ValueError, match="at least one rig"):
        check_rig_of_chain([], 0, 0)


def test_stack_rigs_checks_camera_counts():
    from types import SimpleNamespace
    from multiview_motion_capture_amd.tracker import stack_rigs
    with pytest.raises(ValueError, match="at least one rig"):
        stack_rigs([], 5)
    fake = SimpleNamespace(P=np.zeros((4, 3, 4)))
    with pytest.raises(ValueError, match="4 cameras"):
        stack_rigs([fake], 5)


def test_run_chains_fused_rejects_rig_errors_before_any_launch():
    """The checks run on the host before the first device call: no GPU is needed to see them."""
    import torch
    from multiview_motion_capture_amd.tracker import run_chains_fused
    kps = torch.zeros((32, 5, 2, 25, 3), dtype=torch.float32)
    with pytest.raises(ValueError, match="rig_of_chain needs rigs"):
        run_chains_fused(None, kps, None, 16, rig_of_chain=[0, 0])
    with pytest.raises(ValueError, match="for 2 chains"):
        run_chains_fused(None, kps, None, 16, rigs=[None, None], rig_of_chain=[0, 1, 1])
    with pytest.raises(ValueError, match="has 2 rig"):
        run_chains_fused(None, kps, None, 16, rigs=[None, None], rig_of_chain=[0, 2])


# ---- the C entry point -------------------------------------------------------------------------------------------------------------
def test_chain_run_rigs_is_declared_and_bound():
    import ctypes
    from multiview_motion_capture_amd import _cabi
    header = open(os.path.join(ROOT, "include", "mvmc.h")).read()
    m = re.search(r"int\s+mvmc_chain_run_rigs\s*\(([^)]*)\)", header)
    assert m, "mvmc_chain_run_rigs is not declared in include/mvmc.h"
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1)).split(",")]
    assert len(args) == 5 and "int32_t*" in args[2].replace(" ", "") and args[3].startswith("int ")
    assert "mvmc_chain_run_rigs" in _cabi.SYMBOLS
    lib = _cabi.load()
    fn = lib.mvmc_chain_run_rigs
    assert fn.argtypes[2] is ctypes.c_void_p and fn.argtypes[3] is ctypes.c_int and fn.restype is ctypes.c_int
    # argument errors are reported before anything touches the device
    sk, buf = _cabi.MvmcSkeleton(), _cabi.MvmcChainBuffers()
    assert fn(ctypes.byref(sk), ctypes.byref(buf), None, 0, None) == 1       # n_rigs < 1
    assert fn(ctypes.byref(sk), ctypes.byref(buf), None, 2, None) == 1       # no rig_of_chain with two rigs
    assert fn(None, ctypes.byref(buf), None, 1, None) == 1
