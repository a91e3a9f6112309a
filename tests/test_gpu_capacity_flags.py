"""GPU: the reference has no capacities (motion_capture.py:417-446, :763-808: any cluster size, any number of clusters and tracklets).
Clusters per frame and members per cluster are covered by construction (tracker.default_caps + the IK phase's view pool), so they can
only be exceeded by a caller that passes smaller ones -- then they are REPORTED, as is the one table that remains, t_max tracklet
slots; tracker.repair_chains re-runs the chains concerned with the widest tables the kernels hold."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _data(P=4, F=8, L=4, **kw):
    from multiview_motion_capture_amd import synth
    from multiview_motion_capture_amd.pipeline import HotPath
    data = synth.generate(F, 5, P, 20260107, chain_len=L, **kw)
    d = torch.device("cuda:0")
    return HotPath(data["K"], data["Rt"], device=d), torch.from_numpy(data["kps25"]).to(d), torch.from_numpy(data["counts"]).to(d), L


def test_tracklet_table_overflow_is_reported_and_repaired():
    from multiview_motion_capture_amd.tracker import check_chain_flags, repair_chains, run_chains, run_chains_fused
    hp, kps, cnt, L = _data(P=4)
    for runner in (run_chains, run_chains_fused):
        ok = runner(hp, kps, cnt, L, t_max=8)
        torch.cuda.synchronize()
        check_chain_flags(ok)                                   # four people fit eight slots
        small = runner(hp, kps, cnt, L, t_max=2)                # ... but not two
        torch.cuda.synchronize()
        with pytest.raises(ValueError, match="capacity"):
            check_chain_flags(small)
    # the repair tier: both chains are run again with 16 slots, the tables are widened, and the result is that of a run with room
    assert small["void"].cpu().tolist() == [2, 2]
    assert repair_chains(hp, kps, cnt, small) == 2
    check_chain_flags(small)
    assert small["params"].shape[1] == 16 and small["repaired"].cpu().tolist() == [0, 1]
    n = ok["n_tracks"].cpu().numpy()
    assert np.array_equal(small["n_tracks"].cpu().numpy(), n) and torch.equal(small["next_id"], ok["next_id"])
    for f in range(len(n)):
        assert torch.equal(small["meta"][f, :n[f]], ok["meta"][f, :n[f]])
        # (same device code for the solves; the association runs the generic variant, whose iteration count may differ by one or two)
        assert (small["joints"][f, :n[f]] - ok["joints"][f, :n[f]]).abs().max() < 2e-2
    assert repair_chains(hp, kps, cnt, ok) == 0


def test_a_geometry_that_voids_every_chain_of_the_small_layout_is_repaired_in_one_launch_of_the_big_one():
    """5 views x 6 people with everybody in view: 30 nodes + 6 tracklets = 36 > the 32 nodes the SMALL layout's association holds, so
    EVERY chain's void word is set.  repair_chains takes them through the chain kernel's BIG layout (80 nodes, 16 slots) in one launch
    before it falls back to the per-stage entry points: the same rows bit for bit, an order of magnitude sooner."""
    import time
    from multiview_motion_capture_amd import synth
    from multiview_motion_capture_amd.pipeline import HotPath
    from multiview_motion_capture_amd.tracker import check_chain_flags, repair_chains, run_chains_fused
    L, B = 16, 96
    data = synth.generate(B * L, 5, 6, 20260119, chain_len=L)
    d = torch.device("cuda:0")
    hp, kps, cnt = HotPath(data["K"], data["Rt"], device=d), torch.from_numpy(data["kps25"]).to(d), torch.from_numpy(data["counts"]).to(d)
    res, took = {}, {}
    # (an untimed pass of both paths first: allocations, hipFuncSetAttribute and the first launch of the BIG kernel are one-off costs)
    for big_first in (True, False, True, False):
        r = run_chains_fused(hp, kps, cnt, L)
        torch.cuda.synchronize()
        assert int((r["void"] != 0).sum()) == B and int(r["void"].max()) == 4          # every chain: a graph beyond the layout
        t0 = time.perf_counter()
        assert repair_chains(hp, kps, cnt, r, big_first=big_first) == B
        torch.cuda.synchronize()
        took[big_first] = time.perf_counter() - t0
        check_chain_flags(r)
        res[big_first] = r
    a, b = res[True], res[False]
    assert torch.equal(a["n_tracks"], b["n_tracks"]) and torch.equal(a["next_id"], b["next_id"]) and torch.equal(a["n_dead"], b["n_dead"])
    assert int(a["n_tracks"].min()) == 6
    n = a["n_tracks"].cpu().numpy()
    live = torch.arange(a["meta"].shape[1], device=d)[None, :] < a["n_tracks"][:, None]
    assert torch.equal(a["meta"][live], b["meta"][live])
    assert torch.equal(a["params"][live], b["params"][live]) and torch.equal(a["joints"][live], b["joints"][live])
    print(f"\n{B} chains of {L} frames, C5 P6, all void on the SMALL layout: repair through the BIG layout {took[True] * 1e3:.0f} ms, "
          f"through the per-stage entry points {took[False] * 1e3:.0f} ms; rows bit-identical")
    assert took[True] < 1.5 * took[False]      # (wall clock of a shared box: the claim is 'not slower', the measured ratio is ~ 1 : 3)


def test_smaller_caps_than_the_frame_allows_are_reported():
    from multiview_motion_capture_amd.tracker import check_chain_flags, default_caps, run_chains_fused
    hp, kps, cnt, L = _data(P=4)
    assert default_caps(5, 4) == (10, 20) and default_caps(8, 8) == (32, 64)
    out = run_chains_fused(hp, kps, cnt, L, t_max=8, k_max=2)   # four new people per chain head, room for two clusters
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="capacity"):
        check_chain_flags(out)
    assert (out["void"] == 1).all()
    out = run_chains_fused(hp, kps, cnt, L, t_max=8, v_max=3)   # five views per person, room for three
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="capacity"):
        check_chain_flags(out)


def test_per_frame_tracker_reports_per_call_and_can_be_restored():
    from multiview_motion_capture_amd.tracker import ChainTracker
    from multiview_motion_capture_amd import device as dev
    hp, kps, cnt, L = _data(P=4)
    k17, c = dev.ingest(kps[:2].contiguous(), cnt[:2].contiguous())
    tr = ChainTracker(hp, 1, 4, t_max=2)
    snap = tr.snapshot()
    tr.step(k17[:1], c[:1])
    with pytest.raises(ValueError, match="t_max"):
        tr.check()
    tr.check()                          # the report is per call: the word was cleared
    tr.restore(snap)
    assert int(tr.n_tracks[0]) == 0
    wide = tr.widened(8)
    wide.step(k17[:1], c[:1])
    wide.check()
    assert int(wide.n_tracks[0]) == 4
    tr2 = ChainTracker(hp, 1, 4, t_max=8)
    tr2.step(k17[:1], c[:1])
    tr2.check()
    assert int(tr2.n_tracks[0]) == 4 and torch.equal(tr2.joints, wide.joints)
    with pytest.raises(ValueError):
        ChainTracker(hp, 1, 9)          # rank 18 > 16: refused at construction


def test_update_4d_keeps_tracking_beyond_t_max():
    """MvTracker.update_4d with a table of two slots and four people: the frame is redone with the wide table (the reference has none)."""
    from multiview_motion_capture_amd import motion_capture as mc, synth
    from multiview_motion_capture_amd.common import Calib
    from multiview_motion_capture_amd.pose_def import KpsFormat, Pose
    data = synth.generate(4, 5, 4, 20260107, chain_len=4)
    from helpers import oracle_ingest
    k17, cnt = oracle_ingest(data["kps25"].astype(np.float64), data["counts"])
    calibs = [Calib.from_k_rt(data["K"][c], data["Rt"][c]) for c in range(5)]
    import tracker_np as tk
    import trf_np as t
    trk = mc.MvTracker(p_max=4, t_max=2)
    ref = mc.MvTracker(p_max=4, t_max=8)
    # the noise-free oracle tracker (no capacities) is the reference for both; the gates are those of the Shelf chain test
    orc = tk.OracleTracker(data["K"], data["Rt"], data["P"], solver=lambda poses, projs, init: t.pose_solver_solve_clean(poses, projs, init))
    diffs, between = [], 0.0
    for f in range(3):
        frames = [mc.FrameData(f, {p: Pose(KpsFormat.COCO, k17[f, c, p, :, :2].copy(), k17[f, c, p, :, 2:3].copy(), None)
                                   for p in range(cnt[f, c])}, calibs[c], None) for c in range(5)]
        trk.update_4d(f, frames)
        ref.update_4d(f, frames)
        orc.update(f, [[k17[f, c, p] for p in range(cnt[f, c])] for c in range(5)])
        exp = [(o.tid, o.state, o.hits, o.length) for o in orc.tracklets]
        assert len(exp) == 4
        for tr in (trk, ref):
            assert [(a.track_id, a.state.value, a.hits, len(a)) for a in tr.tracklets] == exp, f
            assert len(tr.dead_tracklets) == orc.n_dead and len(tr._by_id) == orc.next_id
            for a, o in zip(tr.tracklets, orc.tracklets):
                diffs.append(np.abs(a.last_pose_3d.keypoints - o.joints).max())
        for a, b in zip(trk.tracklets, ref.tracklets):
            between = max(between, float(np.abs(a.last_pose_3d.keypoints - b.last_pose_3d.keypoints).max()))
    dd = np.array(diffs)
    print(f"\nupdate_4d beyond t_max: joints vs oracle p90 {np.percentile(dd, 90):.1e} max {dd.max():.1e}; t_max 2 vs 8: {between:.1e}")
    assert np.percentile(dd, 90) < 1e-6 and (dd > 1e-6).mean() < 0.05 and dd.max() < 5e-3
    assert between == 0.0       # (the widened per-stage replay and the eight-slot launch: the same arithmetic, bit for bit)


def test_a_cluster_larger_than_the_number_of_views_is_solved_with_all_its_members():
    """match_spatial keeps every member of a cluster (motion_capture.py:618-626): when match_als merges two people, the new tracklet's
    cold solve sees two poses per view.  Ten members of five views: the solver's cost at the start point and at convergence against
    the oracle's residual over the same ten observations."""
    import oracle_np as o
    from conftest import load_golden
    from multiview_motion_capture_amd import device as dev
    g = load_golden("ik_cases.npz")
    Pshelf = load_golden("shelf_inputs.npz")["P"]
    i = next(i for i in range(len(g["frame"])) if int(g["n_views"][i]) == 5 and not g["cold"][i])
    rng = np.random.default_rng(5)
    kps = np.zeros((1, 5, 2, 17, 3))
    obs_poses, projs, mem = [], [], []
    for rep in range(2):
        for s in range(5):
            cam = int(np.argmin([np.abs(Pshelf[c] - g["projs"][i, s]).max() for c in range(5)]))
            pose = g["poses"][i, s].copy()
            if rep:
                pose[:, :2] += rng.normal(0, 3.0, size=(17, 2))
            kps[0, cam, rep] = pose
            obs_poses.append(pose); projs.append(Pshelf[cam]); mem.append(cam * 2 + rep)
    d = torch.device("cuda:0")
    init = np.concatenate([g["init_root"][i], g["init_euler"][i].ravel(), g["init_blens"][i]])[None]
    members = torch.tensor([mem + [-1] * 10], dtype=torch.int32, device=d)        # v_max = 20 columns, ten used
    args = (torch.from_numpy(kps).to(d), torch.from_numpy(Pshelf).to(d), members, torch.from_numpy(init).to(d),
            torch.zeros(1, dtype=torch.uint8, device=d))
    obs = np.array([o.add_mid_spine(p) for p in obs_poses])[:, o.IK_OBS_IDX, :]
    bd, _ = o.skeleton_constants()
    p1, _, i1 = dev.ik_solve(*args, 1, 1)
    f0 = o.ik_residual(init[0, :3], init[0, 3:57], init[0, 57:], obs, np.array(projs), bd)
    c0 = 0.5 * f0.dot(f0)
    assert abs(float(i1[0, 0]) - c0) <= 1e-12 * c0
    p2, j2, i2 = dev.ik_solve(*args, 400, 400)
    r, e, res1 = o.ik_stage1(obs, np.array(projs), init[0, :3], init[0, 3:57].reshape(18, 3), init[0, 57:], 400, bd)
    _, _, _, res2 = o.ik_stage2(obs, np.array(projs), r, e, init[0, 57:], 400, bd)
    assert res2.status > 0 and float(i2[0, 5]) > 0
    assert float(i2[0, 3]) <= res2.cost * (1 + 1e-4), (float(i2[0, 3]), res2.cost)
    # holes in the member row are allowed on this entry point: the same ten members spread over the row give the same solve
    spread = -torch.ones((1, 20), dtype=torch.int32, device=d)
    spread[0, ::2] = members[0, :10]
    p3, _, i3 = dev.ik_solve(args[0], args[1], spread, args[3], args[4], 400, 400)
    assert torch.equal(p2, p3)


def test_occluded_workload_runs_births_deaths_and_single_view_tracklets_at_scale():
    """A generator with whole-pose occlusion and false detections (ragged counts): the chain kernel's birth / death / one-view paths
    run at benchmark scale, bit-identical to the launch-per-stage path, on both layouts.  With views missing the reference's match_als
    now and then merges two people into one cluster of 9-11 poses at a chain head (oracle: max 11 on this workload): the view pool
    holds them, NO chain raises a word."""
    from multiview_motion_capture_amd import synth
    from multiview_motion_capture_amd.pipeline import HotPath
    from multiview_motion_capture_amd.tracker import check_chain_flags, run_chains, run_chains_fused
    F, L = 1600, 16
    data = synth.generate(F, 5, 4, 20260108, chain_len=L, occlusion=0.25, spurious=0.02)
    d = torch.device("cuda:0")
    hp = HotPath(data["K"], data["Rt"], device=d)
    kps, cnt = torch.from_numpy(data["kps25"]).to(d), torch.from_numpy(data["counts"]).to(d)
    assert data["counts"].min() <= 1 and data["counts"].max() == 4
    a = run_chains_fused(hp, kps, cnt, L)
    big = run_chains_fused(hp, kps, cnt, L, force_big=True)     # the BIG layout on these 20-node graphs
    b = run_chains(hp, kps, cnt, L, want_info=True)
    torch.cuda.synchronize()
    ov = b["overflow"].cpu().numpy()
    assert not ov.any()
    check_chain_flags(a)
    check_chain_flags(big)
    assert int(a["void"].max()) == 0
    for k in ("n_tracks", "meta", "n_dead"):
        assert torch.equal(a[k], big[k])
    assert torch.equal(a["n_tracks"], b["n_tracks"]) and torch.equal(a["meta"], b["meta"]) and torch.equal(a["n_dead"], b["n_dead"])
    n = a["n_tracks"].cpu().numpy()
    ja, jb = a["joints"].cpu().numpy(), b["joints"].cpu().numpy()
    assert all(np.array_equal(ja[f, :n[f]], jb[f, :n[f]]) for f in range(F))
    meta = a["meta"].cpu().numpy()
    good = np.repeat(ov == 0, L)
    births, deaths = int(a["next_id"].cpu().numpy()[ov == 0].sum()), int(a["n_dead"].cpu().numpy()[ov == 0].sum())
    n_good = int((ov == 0).sum())
    print(f"occluded workload: {births} births and {deaths} deaths over {n_good} chains, tracks per frame min {n[good].min()} mean "
          f"{n[good].mean():.2f} max {n[good].max()}")
    assert births > 4.2 * n_good and deaths > 0.2 * n_good      # people re-born inside chains, tracklets dying
    assert n[good].min() < 4 <= n[good].max()
    gt = data["gt_joints"]
    errs = []
    for f in range(0, F, 7):
        if good[f]:
            for s in range(n[f]):
                if meta[f, s, 1] == 2:      # confirmed tracklets follow a real person
                    errs.append(np.linalg.norm(gt[f] - ja[f, s][None], axis=-1).mean(axis=-1).min())
    print("confirmed tracklets: median joint error vs ground truth %.3f m over %d samples" % (np.median(errs), len(errs)))
    assert np.median(errs) < 0.03
