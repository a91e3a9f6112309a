"""GPU: a calibration per chain in the chain kernel (include/mvmc.h: mvmc_chain_run_rigs), run_chains_fused(..., rigs, rig_of_chain),
repair_chains on a mixed batch, and the sequence API on top (sequences.track_sequences, motion_capture.run_main_batched)."""
import pickle

import numpy as np
import pytest
import torch


pytestmark = pytest.mark.gpu

L = 16
D = torch.device("cuda:0")


def _scene(F, C, P, seed):
    """A walk="scene" sequence whose cameras come from ``seed``: a rig of its own."""
    from multiview_motion_capture_amd import synth
    from multiview_motion_capture_amd.common import Calib
    data = synth.generate(F, C, P, seed, walk="scene")
    calibs = [Calib.from_k_rt(data["K"][c], data["Rt"][c]) for c in range(C)]
    return data, (data["kps25"], data["counts"], calibs)


def _launch(seqs):
    """The launch layout of `seqs` (one camera count): HotPaths, device keypoints / counts, the layout."""
    from multiview_motion_capture_amd.pipeline import HotPath
    from multiview_motion_capture_amd.sequences import check_sequences, pack_group, plan_groups
    lay, = plan_groups(check_sequences(seqs), L)
    rigs = [HotPath(np.array([c.K for c in seqs[i][2]]), np.array([c.Rt for c in seqs[i][2]]), device=D) for i in lay.seq_ids]
    k, c = pack_group(lay, seqs, L)
    return rigs, torch.from_numpy(k).to(D), torch.from_numpy(c).to(D), lay


def _rows(res, f0, f1):
    return {k: res[k][f0:f1].cpu().numpy() for k in ("params", "joints", "meta", "n_tracks")}


def _same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in ("params", "joints", "meta", "n_tracks"))


def _alone(rig, kps, cnt, lay, r, **kw):
    from multiview_motion_capture_amd.tracker import run_chains_fused
    f0, f1 = lay.chain_lo[r] * L, (lay.chain_lo[r] + lay.n_chains[r]) * L
    return run_chains_fused(rig, kps[f0:f1].contiguous(), cnt[f0:f1].contiguous(), L, **kw), f0, f1


@pytest.mark.parametrize("case", ["latency", "throughput", "big"])
def test_each_sequence_of_a_multi_rig_launch_equals_the_sequence_alone(case):
    """Three rigs (C5), sequences of different lengths and people counts (p_max padding), one launch: every sequence's rows are those
    of the same sequence run alone with its own HotPath (the one-rig entry point) at the same p_max and t_max, bit for bit.
    latency: 32 chains x 16 parts <= 2 x 256 CUs (the 256-VGPR build); throughput: 48 chains; big: the BIG layout (force_big)."""
    from multiview_motion_capture_amd.tracker import check_chain_flags, run_chains_fused
    lens = (300, 200, 250) if case == "throughput" else (160, 96, 250)
    seqs = [_scene(n, 5, p, 20270101 + 7 * i)[1] for i, (n, p) in enumerate(zip(lens, (4, 3, 4)))]
    rigs, kps, cnt, lay = _launch(seqs)
    assert lay.p_max == 4 and lay.total_chains == (48 if case == "throughput" else 32)
    kw = dict(t_max=8, force_big=case == "big")
    res = run_chains_fused(rigs[0], kps, cnt, L, rigs=rigs, rig_of_chain=lay.rig_of_chain, **kw)
    torch.cuda.synchronize()
    check_chain_flags(res)
    for r in range(3):
        one, f0, f1 = _alone(rigs[r], kps, cnt, lay, r, **kw)
        torch.cuda.synchronize()
        check_chain_flags(one)
        assert _same(_rows(res, f0, f1), _rows(one, 0, f1 - f0)), f"{case}: sequence {r} differs from its own run"
        assert int(one["n_tracks"].max()) > 0
    # the calibration is really per chain: every chain on rig 0 changes the other rigs' sequences
    wrong = run_chains_fused(rigs[0], kps, cnt, L, rigs=rigs, rig_of_chain=np.zeros_like(lay.rig_of_chain), **kw)
    torch.cuda.synchronize()
    for r in (1, 2):
        f0, f1 = lay.chain_lo[r] * L, (lay.chain_lo[r] + lay.n_chains[r]) * L
        assert not _same(_rows(res, f0, f1), _rows(wrong, f0, f1)), f"{case}: rig {r} made no difference"
    f1 = lay.n_chains[0] * L
    assert _same(_rows(res, 0, f1), _rows(wrong, 0, f1))


def test_default_entry_point_and_null_rigs_give_the_same_bits(monkeypatch):
    """mvmc_chain_run, mvmc_chain_run_rigs(..., NULL, 1) and mvmc_chain_run_rigs with every chain on rig 0 of one: the same results on a
    config-4-shaped batch (C5 P4, chains of 16, 320 chains: the throughput build)."""
    from multiview_motion_capture_amd import _cabi, synth
    from multiview_motion_capture_amd.pipeline import HotPath
    from multiview_motion_capture_amd.tracker import check_chain_flags, run_chains_fused
    data = synth.generate(320 * L, 5, 4, 20260103, chain_len=L)
    hp = HotPath(data["K"], data["Rt"], device=D)
    kps, cnt = torch.from_numpy(data["kps25"]).to(D), torch.from_numpy(data["counts"]).to(D)
    base = run_chains_fused(hp, kps, cnt, L)
    via_rig0 = run_chains_fused(hp, kps, cnt, L, rigs=[hp], rig_of_chain=np.zeros(320, np.int32))
    lib = _cabi.load()
    rigs_fn = lib.mvmc_chain_run_rigs
    monkeypatch.setattr(lib, "mvmc_chain_run", lambda sk, buf, st: rigs_fn(sk, buf, None, 1, st))
    via_null = run_chains_fused(hp, kps, cnt, L)
    torch.cuda.synchronize()
    check_chain_flags(base)
    F = 320 * L
    for other in (via_rig0, via_null):
        assert _same(_rows(base, 0, F), _rows(other, 0, F))
        assert torch.equal(base["next_id"], other["next_id"]) and torch.equal(base["n_dead"], other["n_dead"])


@pytest.mark.parametrize("big_first", [True, False])
def test_a_sequence_that_voids_the_small_layout_is_repaired_with_its_own_rig(big_first):
    """The crowded geometry of test_gpu_capacity_flags.py (C5 P6, everybody in view: every chain of the SMALL layout is void) next to an
    ordinary sequence of another rig.  After repair_chains -- through the BIG layout, or the per-stage path grouped by rig -- each
    sequence's live rows equal the same sequence alone, repaired."""
    from multiview_motion_capture_amd import synth
    from multiview_motion_capture_amd.common import Calib
    from multiview_motion_capture_amd.tracker import check_chain_flags, repair_chains, run_chains_fused
    n_frames = 3 * L if big_first else 2 * L
    crowd = synth.generate(n_frames, 5, 6, 20260119, chain_len=L)
    seqs = [_scene(n_frames, 5, 4, 20270303)[1],
            (crowd["kps25"], crowd["counts"], [Calib.from_k_rt(crowd["K"][c], crowd["Rt"][c]) for c in range(5)])]
    rigs, kps, cnt, lay = _launch(seqs)
    res = run_chains_fused(rigs[0], kps, cnt, L, rigs=rigs, rig_of_chain=lay.rig_of_chain)
    torch.cuda.synchronize()
    void = res["void"].cpu().numpy()
    assert (void[lay.chain_lo[1]:] != 0).all() and (void[:lay.chain_lo[1]] == 0).all()
    assert repair_chains(rigs[0], kps, cnt, res, big_first=big_first) == lay.n_chains[1]
    check_chain_flags(res)
    for r in range(2):
        one, f0, f1 = _alone(rigs[r], kps, cnt, lay, r)
        repair_chains(rigs[r], kps[f0:f1].contiguous(), cnt[f0:f1].contiguous(), one, big_first=big_first)
        check_chain_flags(one)
        a, b = _rows(res, f0, f1), _rows(one, 0, f1 - f0)
        assert np.array_equal(a["n_tracks"], b["n_tracks"])
        for f in range(f1 - f0):
            n = a["n_tracks"][f]
            for k in ("params", "joints", "meta"):
                assert np.array_equal(a[k][f, :n], b[k][f, :n], equal_nan=True), (r, f, k)


def test_track_sequences_identities():
    """Three walk="scene" sequences of three rigs through track_sequences: every identity the stitch carries across a chain boundary
    is the same ground-truth person on both sides (bench.carries_against_ground_truth, per sequence); each sequence's identities are
    those parallel.run_sharded gives for it alone at world 1; no identity leaves its sequence."""
    import bench
    from multiview_motion_capture_amd import parallel
    from multiview_motion_capture_amd.sequences import track_sequences
    from multiview_motion_capture_amd.tracker import check_chain_flags, repair_chains
    datas, seqs = zip(*[_scene(n, 5, 4, 20270505 + 11 * i) for i, n in enumerate((200, 150, 250))])
    tables = []
    out = track_sequences(list(seqs), chain_len=L, tables=tables)
    rigs, kps, cnt, lay = _launch(list(seqs))
    total_carried = 0
    for r, (data, tl, tb) in enumerate(zip(datas, out, tables)):
        n_ch = lay.n_chains[r]
        assert tb["gid"].shape[0] == n_ch and tb["n_frames"] == len(data["counts"])
        wrap = dict(stitch=dict(gid=torch.from_numpy(tb["gid"])), meta=torch.from_numpy(tb["meta"]), n_tracks=torch.from_numpy(tb["n_tracks"]),
                    joints=torch.from_numpy(tb["joints"]))
        c = bench.carries_against_ground_truth(wrap, data, L, 4)
        assert c["identities_carried"] == c["carried_to_the_right_person"] and c["identities_carried"] > 0, c
        total_carried += c["identities_carried"]
        # the same sequence alone, through the benchmark's sharded path at world 1
        one, f0, f1 = _alone(rigs[r], kps, cnt, lay, r)
        repair_chains(rigs[r], kps[f0:f1].contiguous(), cnt[f0:f1].contiguous(), one)
        check_chain_flags(one)
        T = one["params"].shape[1]
        sh = parallel.run_sharded(lambda: one, L, n_ch, 0, 1, rows_per_frame=T)
        parallel.check_stitch_info(sh)
        assert np.array_equal(tb["gid"], sh["gid"].cpu().numpy()), f"sequence {r}: identities differ from its own stitch"
        assert (tb["match"][0] == -1).all()                 # nothing is matched into a sequence's first chain
        # the records: one per identity that has a live row in a real frame, frames inside the sequence
        live = {int(tb["gid"][f // L, tb["meta"][f, s, 0]]) for f in range(tb["n_frames"]) for s in range(tb["n_tracks"][f])}
        assert sorted(t.track_id for t in tl) == sorted(live)
        assert all(0 <= fi < tb["n_frames"] for t in tl for fi in t.frame_idxs)
    assert total_carried > 0


def test_out_of_range_rig_index_voids_only_its_chain(monkeypatch):
    """The Python layer refuses a bad index before any launch, so the kernel's own guard is reached through the C entry point: n_rigs
    = 2 and an index of 3, with calibration allocated for FOUR rigs (were the guard missing, the read would still be inside the
    allocation).  The chain gets void bit 4 and empty tables, the other chains are intact, and check_chain_flags / repair_chains
    raise."""
    from multiview_motion_capture_amd import _cabi
    from multiview_motion_capture_amd.tracker import check_chain_flags, repair_chains, run_chains_fused
    seqs = [_scene(3 * L, 5, 4, 20270707 + 5 * i)[1] for i in range(4)]
    rigs, kps, cnt, lay = _launch(seqs)
    roc = lay.rig_of_chain.copy()
    roc[roc >= 2] -= 2                       # chains on rigs 0 and 1 only ...
    bad = 4
    roc[bad] = 3                             # ... but one: index 3
    good = run_chains_fused(rigs[0], kps, cnt, L, rigs=rigs, rig_of_chain=np.where(np.arange(len(roc)) == bad, 0, roc))
    lib = _cabi.load()
    fn = lib.mvmc_chain_run_rigs
    seen = []
    monkeypatch.setattr(lib, "mvmc_chain_run_rigs", lambda sk, buf, rig, n, st: seen.append(n) or fn(sk, buf, rig, 2, st))
    res = run_chains_fused(rigs[0], kps, cnt, L, rigs=rigs, rig_of_chain=roc)
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert seen == [4]
    void = res["void"].cpu().numpy()
    assert void[bad] & 16 and (np.delete(void, bad) == 0).all()
    assert int(res["flags"][len(roc) + 2]) & 16
    n_t = res["n_tracks"].cpu().numpy().reshape(-1, L)
    assert (n_t[bad] == 0).all()
    F = len(roc) * L
    keep = np.repeat(np.arange(len(roc)) != bad, L)
    a, b = _rows(res, 0, F), _rows(good, 0, F)
    assert all(np.array_equal(a[k][keep], b[k][keep], equal_nan=True) for k in a)
    with pytest.raises(ValueError, match="rig index"):
        check_chain_flags(res)
    with pytest.raises(ValueError, match="rig index"):
        repair_chains(rigs[0], kps, cnt, res)


def _shelf_pickles(tmp_path, g):
    from multiview_motion_capture_amd.common import Calib
    from multiview_motion_capture_amd.motion_capture import frame_data_from_batch
    calibs = [Calib.from_k_rt(g["K"][c], g["Rt"][c]) for c in range(g["K"].shape[0])]
    pose_dir = tmp_path / "poses"
    pose_dir.mkdir()
    for f in range(g["kps25"].shape[0]):
        with open(pose_dir / f"{f}.pkl", "wb") as fh:
            pickle.dump(frame_data_from_batch(f, g["kps25"][f], g["counts"][f], calibs), fh)
    return pose_dir


def test_shelf_through_run_main_batched(tmp_path, shelf_inputs):
    """The 301 Shelf frames as per-frame FrameData pickles, passed twice to run_main_batched (one launch, two sequences): both
    tracklets.pkl files load, are identical, and hold MvTracklet records; against run_main (update_4d frame by frame) on the same
    frames, every tracklet of >= 100 frames has a batched identity that lies on it at a small joint distance, and the batched identities
    together cover nearly all of its frames.
    Measured on one MI355X, for run_main's four tracklets of >= 100 frames (300, 300, 156, 105 frames): the best batched identity covers
    1.0, 0.32, 0.891, 0.714 of the frames at a mean joint distance of 1.2, 3.7, 8.4, 4.9 mm; all batched identities together 1.0, 0.99,
    0.987, 0.981.  (The second person is split into several identities: a chain that starts while that person is seen by too few views
    cold-starts without them, and the stitch has nothing to carry across that boundary -- the batched semantics, INTEGRATION.md C.)
    Gate, with margin: best coverage >= 0.25, mean distance <= 2 cm, together >= 0.95."""
    from multiview_motion_capture_amd.motion_capture import MvTracklet, TrackState, run_main, run_main_batched
    pose_dir = _shelf_pickles(tmp_path, shelf_inputs)
    outs = [tmp_path / "a", tmp_path / "b"]
    res = run_main_batched([pose_dir, pose_dir], outs, n_test=300)
    blobs = [open(o / "tracklets.pkl", "rb").read() for o in outs]
    assert blobs[0] == blobs[1]
    tl = pickle.loads(blobs[0])["tracklets"]
    assert len(tl) == len(res[0]) > 0
    for t in tl:
        assert isinstance(t, MvTracklet) and isinstance(t.state, TrackState)
        for name in ("track_id", "frame_idxs", "poses", "state", "hits", "time_since_update"):
            assert hasattr(t, name), name
        assert len(t.frame_idxs) == len(t.poses) == t.hits and all(1 <= f <= 300 for f in t.frame_idxs)
    assert [len(t) for t in tl] == sorted((len(t) for t in tl), reverse=True)
    ref = run_main(None, pose_dir, tmp_path / "ref", n_test=300)
    long_ref = [t for t in ref if len(t) >= 100]
    assert long_ref
    report = []
    for t in long_ref:
        # the batched identity that lies on this tracklet in the most frames (mean joint distance < 0.2 m): its coverage of the
        # tracklet's frames, and the mean joint distance over the frames they share
        # (and the frames of the tracklet that SOME batched identity lies on: where the batched identities of one person split)
        rj = {f: p[2].keypoints for f, p in zip(t.frame_idxs, t.poses)}
        best, near = (0, 0.0, np.inf), set()
        for b in tl:
            fr = [f for f in b.frame_idxs if f in rj]
            dist = np.array([np.linalg.norm(p[2].keypoints - rj[f], axis=-1).mean() for f, p in zip(b.frame_idxs, b.poses) if f in rj])
            near |= {f for f, d in zip(fr, dist) if d < 0.2}
            if dist.size and int((dist < 0.2).sum()) > best[0]:
                best = (int((dist < 0.2).sum()), int((dist < 0.2).sum()) / len(t), float(dist.mean()))
        report.append((len(t), round(best[1], 4), round(best[2], 5), round(len(near) / len(t), 4)))
    print("shelf run_main_batched vs run_main (frames, coverage, mean joint distance m, covered by any identity):", report)
    for n, cov, dist, union in report:
        assert cov >= 0.25 and dist <= 0.02 and union >= 0.95, report
