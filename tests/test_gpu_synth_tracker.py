"""GPU: the persistent chain kernel (mvmc_chain_run, the benchmark's default path) against the REFERENCE tracker on the benchmark's
workloads: tests/golden/synth_c4_tracker.npz and synth_c5_tracker.npz hold MvTracker.update_4d (motion_capture.py:873-963) run by the
reference itself over 64-frame subsets of synthetic config 4 (seed 20260103, C5 P4: the SMALL layout) and config 5 (seed 20260104,
C8 P8: the BIG layout, als5) made by the random-walk generator, chains of 16 (oracle/gen_golden_ikconv.py, oracle/gen_golden_c5.py) --
SURVEY.md section 8c.  synth_c4_scene_tracker.npz and synth_c5_scene_tracker.npz hold the same on selected chains of the steps
bench.py times (--walk continuous: one bounded scene, tests/helpers.bench_step_data; oracle/gen_golden_scene.py), where some pairs of
people stay close for a whole step: those tests run the whole step in one launch, as the benchmark does."""
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden
from helpers import bench_step_data, closest_pair_root, oracle_chain_job

pytestmark = pytest.mark.gpu


def check_against_reference(g, L, P, n_t, meta, joints, n_dead, info, gt):
    """The device's tables of the fixture's frames (n_t, meta, joints, info: one row per fixture frame; n_dead: one per chain; gt: the
    ground-truth joints of those frames) against the reference's recorded run."""
    F = len(n_t)
    # ---- association + tracker state machine: exact ----
    assert np.array_equal(n_t, g["n_tracks"])
    for f in range(F):
        k = int(g["n_tracks"][f])
        assert np.array_equal(meta[f, :k], g["meta"][f, :k]), (f, meta[f, :k], g["meta"][f, :k])
    assert np.array_equal(n_dead, g["n_dead"][L - 1::L])
    solved = ~np.isnan(info[:, :, 1])
    assert np.array_equal(solved.sum(axis=1), g["n_solves"])
    # ---- 3-D output: cold chain heads are converged solves (tight); warm frames are 5 + 5-evaluation truncated solves ----
    dj = np.full((F, P), np.nan)
    for f in range(F):
        for s in range(int(g["n_tracks"][f])):
            dj[f, s] = np.abs(joints[f, s] - g["joints"][f, s]).max()
    head = dj[0::L].ravel()
    warm = np.concatenate([dj[b * L + 1:(b + 1) * L].ravel() for b in range(F // L)])
    print("chain heads (cold, 50 + 50): joint diff median %.2e max %.2e | warm frames (5 + 5): median %.2e p90 %.2e max %.2e" %
          (np.nanmedian(head), np.nanmax(head), np.nanmedian(warm), np.nanquantile(warm, 0.9), np.nanmax(warm)))
    e_dev, e_ref = [], []
    for f in range(F):
        for s in range(int(g["n_tracks"][f])):
            pj = np.linalg.norm(gt[f] - g["joints"][f, s][None], axis=-1).mean(axis=-1)
            e_ref.append(pj.min())
            e_dev.append(np.linalg.norm(gt[f, int(pj.argmin())] - joints[f, s], axis=-1).mean())
    print("mean joint error vs ground truth: device %.4f m, reference %.4f m" % (np.mean(e_dev), np.mean(e_ref)))
    assert np.nanmax(head) < 1e-5          # converged solves (observed: 9.5e-7 on config 4)
    assert np.nanmedian(warm) < 5e-3 and np.nanquantile(warm, 0.9) < 1.6e-2     # the reference's own rounding band (tests/test_gpu_ik.py)
    assert np.mean(e_dev) < 1.1 * np.mean(e_ref) + 1e-3


@pytest.mark.parametrize("fixture", ["synth_c4_tracker.npz", "synth_c5_tracker.npz"])
def test_chain_kernel_reproduces_the_reference_tracker_on_the_synthetic_workload(fixture):
    from multiview_motion_capture_amd import synth
    from multiview_motion_capture_amd.pipeline import HotPath
    from multiview_motion_capture_amd.tracker import check_chain_flags, run_chains_fused
    g = load_golden(fixture)
    F, L, C, P = int(g["n_frames"]), int(g["chain_len"]), int(g["n_views"]), int(g["n_people"])
    data = synth.generate(F, C, P, int(g["seed"]), chain_len=L)
    assert float(np.abs(data["kps25"].astype(np.float64)).sum()) == float(g["kps25_checksum"])   # same inputs as the reference saw
    d = torch.device("cuda:0")
    hp = HotPath(data["K"], data["Rt"], device=d)
    out = run_chains_fused(hp, torch.from_numpy(data["kps25"]).to(d), torch.from_numpy(data["counts"]).to(d), L, want_info=True)
    torch.cuda.synchronize()
    check_chain_flags(out)
    n_t, meta, joints = out["n_tracks"].cpu().numpy(), out["meta"].cpu().numpy(), out["joints"].cpu().numpy()
    info = out["ik_info"].cpu().numpy().reshape(F, -1, 8)
    check_against_reference(g, L, P, n_t, meta, joints, out["n_dead"].cpu().numpy(), info, data["gt_joints"])


@pytest.mark.parametrize("C,P,seed,n_chains", [(5, 4, 20260103, 3), (8, 8, 20260104, 1)])
def test_chain_kernel_equals_the_noise_free_oracle_tracker_on_every_frame(C, P, seed, n_chains):
    """The same workloads against the DETERMINISTIC oracle (tracker_np.OracleTracker driving trf_np.pose_solver_solve_clean: the
    reference's tracker with its two least_squares calls freed of LAPACK's noise, tests/test_gpu_tracker.py): the warm frames, which
    the comparison with the reference's recorded results above can only hold to a band, must agree like the chain heads -- tracker
    tables on every frame, joints to 1e-8."""
    import oracle_np as o
    import tracker_np as tk
    import trf_np as t
    from multiview_motion_capture_amd import synth
    from multiview_motion_capture_amd.pipeline import HotPath
    from multiview_motion_capture_amd.tracker import check_chain_flags, run_chains_fused
    L = 16
    F = n_chains * L
    data = synth.generate(F, C, P, seed, chain_len=L)
    d = torch.device("cuda:0")
    hp = HotPath(data["K"], data["Rt"], device=d)
    out = run_chains_fused(hp, torch.from_numpy(data["kps25"]).to(d), torch.from_numpy(data["counts"]).to(d), L)
    torch.cuda.synchronize()
    check_chain_flags(out)
    n_t, meta, joints = out["n_tracks"].cpu().numpy(), out["meta"].cpu().numpy(), out["joints"].cpu().numpy()
    kps25 = data["kps25"].astype(np.float64)
    dd = []
    for b in range(n_chains):
        orc = tk.OracleTracker(data["K"], data["Rt"], data["P"], solver=lambda poses, projs, init: t.pose_solver_solve_clean(poses, projs, init))
        for tt in range(L):
            f = b * L + tt
            views = []
            for c in range(C):
                poses = [o.openpose25_to_coco17(kps25[f, c, p]) for p in range(int(data["counts"][f, c]))]
                views.append([q for q in poses if o.pose_is_good(q)])
            orc.update(tt, views)
            exp = np.array([[x.tid, x.state, x.hits, x.length] for x in orc.tracklets], dtype=np.int32).reshape(-1, 4)
            assert n_t[f] == len(exp) and np.array_equal(meta[f, :len(exp)], exp), (f, meta[f, :n_t[f]], exp)
            dd += [float(np.abs(joints[f, s] - x.joints).max()) for s, x in enumerate(orc.tracklets)]
        assert orc.n_dead == int(out["n_dead"][b]) and orc.next_id == int(out["next_id"][b])
    dd = np.array(dd)
    print(f"\nC{C} P{P}: {n_chains} chain(s) of {L} frames against the noise-free oracle tracker: tables equal on every frame; {len(dd)} "
          f"tracklet-frames, joint difference median {np.median(dd):.1e} p90 {np.percentile(dd, 90):.1e} max {dd.max():.1e} m")
    # observed: 1.2e-13 m (config 4), 5.3e-11 m (config 5) at worst -- every observation is seen by all views here, no weak models
    assert dd.max() < 1e-8


SCENE_FIXTURES = ["synth_c4_scene_tracker.npz", "synth_c5_scene_tracker.npz"]
ORACLE_EXTRA = {"synth_c4_scene_tracker.npz": 6, "synth_c5_scene_tracker.npz": 0}   # more close-pair chains for the oracle test
# Tracklet-frames of the scene chains whose joints are held to their measured level instead of 1e-8: (segment, chain, frame, tracklet
# id) -> bar.  Config 4's closest-pair chain 45 (roots 6.8 cm apart at its head), frame 7, tracklet 1: one limb angle (parameter 17)
# differs from the oracle by 1.2e-3 rad and moves the joints by only 2.3e-7 m -- a weak-eigenvalue direction of that solve, where a
# different rounding of the last bits lands elsewhere along a nearly flat valley (tests/test_gpu_update_4d.py has the same for
# Shelf's occluded person).  Its other 15 frames, and the chain's other tracklets, are at 1e-14.
WEAK = {("synth_c4_scene_tracker.npz", 0, 45, 7, 1): 3e-7}
OUT_KEYS = ("params", "joints", "meta", "n_tracks")


@functools.lru_cache(maxsize=2)
def scene_run(fixture):
    """The fixture's steps, each run WHOLE by the chain kernel (625 or 1,563 chains co-resident: the benchmark's launch); -> the rows
    of the fixture's chains and of ORACLE_EXTRA more chains whose heads have the next smallest closest-pair root distance."""
    from multiview_motion_capture_amd.pipeline import HotPath
    from multiview_motion_capture_amd.tracker import check_chain_flags, run_chains_fused
    g = load_golden(fixture)
    F, L, C, P, seed = (int(g[k]) for k in ("n_frames", "chain_len", "n_views", "n_people", "seed"))
    d = torch.device("cuda:0")
    segs = list(dict.fromkeys(int(s) for s in g["segments"]))
    chains, cams = {}, {}
    for i, seg in enumerate(segs):
        data = bench_step_data(F, C, P, seed, seg, L)
        assert float(np.abs(data["kps25"].astype(np.float64)).sum()) == float(g["step_checksum"][i])   # the frames the reference saw
        mine = [int(b) for s, b in zip(g["segments"], g["chains"]) if int(s) == seg]
        head = closest_pair_root(data["gt_joints"][0::L])
        extra = [int(b) for b in np.argsort(head, kind="stable") if int(b) not in mine][:ORACLE_EXTRA[fixture]]
        hp = HotPath(data["K"], data["Rt"], device=d)
        out = run_chains_fused(hp, torch.from_numpy(data["kps25"]).to(d), torch.from_numpy(data["counts"]).to(d), L, want_info=True)
        torch.cuda.synchronize()
        check_chain_flags(out)
        assert out["n_chains"] == F // L
        for b in mine + extra:
            sl = slice(b * L, (b + 1) * L)
            r = {k: out[k][sl].cpu().numpy() for k in OUT_KEYS}
            r.update(ik_info=out["ik_info"][b].cpu().numpy(), als_iters=out["als_iters"][b].cpu().numpy(), n_dead=int(out["n_dead"][b]),
                     next_id=int(out["next_id"][b]), kps25=data["kps25"][sl].copy(), counts=data["counts"][sl].copy(),
                     gt=data["gt_joints"][sl].copy(), head=float(head[b]), fixture=b in mine)
            chains[(seg, b)] = r
        cams[seg] = (data["K"], data["Rt"], data["P"])
        del data, out
    return chains, cams


@pytest.mark.parametrize("fixture", SCENE_FIXTURES)
def test_chain_kernel_reproduces_the_reference_tracker_on_the_benchmark_scene(fixture):
    """The reference's tables on the benchmark's own frames, with the bars of the random-walk fixtures above, plus every frame's ALS
    iteration count; and each selected chain run ALONE is bit-identical to the same chain inside the whole step's launch."""
    from multiview_motion_capture_amd.pipeline import HotPath
    from multiview_motion_capture_amd.tracker import check_chain_flags, run_chains_fused
    g = load_golden(fixture)
    L, P = int(g["chain_len"]), int(g["n_people"])
    chains, cams = scene_run(fixture)
    sel = [chains[(int(s), int(b))] for s, b in zip(g["segments"], g["chains"])]
    heads = np.array([r["head"] for r in sel])
    print(f"\n{fixture}: chains {g['chains'].tolist()} of segments {g['segments'].tolist()}, closest-pair root distance at their heads "
          f"{np.round(heads, 4).tolist()} m")
    assert heads.min() < 0.2                              # the close-pair regime is covered
    assert np.allclose(heads, g["head_closest_pair"], rtol=0, atol=1e-12)
    cat = lambda k: np.concatenate([r[k] for r in sel])
    check_against_reference(g, L, P, cat("n_tracks"), cat("meta"), cat("joints"), np.array([r["n_dead"] for r in sel]),
                            cat("ik_info"), cat("gt"))
    # ---- ALS: the same iteration count as the reference's match_als at every chain head below the cap of 1,000.  A head's graph is
    # built from the detections alone; a warm frame's also from the tracklets' joints, which agree with the reference's only to its
    # rounding band above, so its affinity -- and the iteration count -- differs in the last bits (measured: 27 of 120 warm frames
    # equal).  Warm frames are held to the noise-free oracle instead, which the device matches to 1e-13 m (the test below). ----
    it_dev, it_ref = cat("als_iters"), g["als_iters"]
    h_dev, h_ref = it_dev[0::L], it_ref[0::L]
    free = (h_ref < 1000) & (h_dev < 1000)
    print(f"ALS iterations: chain heads {h_ref.tolist()} (reference), equal on {int((h_dev == h_ref).sum())} of {len(h_ref)}, "
          f"{int((~free).sum())} at the cap; warm frames equal on {int((it_dev == it_ref).sum() - (h_dev == h_ref).sum())} of "
          f"{len(it_ref) - len(h_ref)}")
    assert np.array_equal(h_dev[free], h_ref[free]), (h_dev.tolist(), h_ref.tolist())
    assert np.array_equal(h_dev >= 1000, h_ref >= 1000)
    # ---- a chain alone == the same chain among all the step's chains, bit for bit ----
    d = torch.device("cuda:0")
    for s, b in zip(g["segments"], g["chains"]):
        r = chains[(int(s), int(b))]
        K, Rt, _ = cams[int(s)]
        one = run_chains_fused(HotPath(K, Rt, device=d), torch.from_numpy(r["kps25"]).to(d), torch.from_numpy(r["counts"]).to(d), L,
                               want_info=True)
        torch.cuda.synchronize()
        check_chain_flags(one)
        for k in OUT_KEYS:
            assert np.array_equal(np.nan_to_num(one[k].cpu().numpy()), np.nan_to_num(r[k])), (int(s), int(b), k)
        assert np.array_equal(np.nan_to_num(one["ik_info"][0].cpu().numpy()), np.nan_to_num(r["ik_info"])), (int(s), int(b), "ik_info")
        assert np.array_equal(one["als_iters"][0].cpu().numpy(), r["als_iters"])
        assert (int(one["n_dead"][0]), int(one["next_id"][0])) == (r["n_dead"], r["next_id"])


@pytest.mark.parametrize("fixture", SCENE_FIXTURES)
def test_chain_kernel_equals_the_noise_free_oracle_tracker_on_the_benchmark_scene(fixture):
    """The fixture's chains of the benchmark's steps and, on config 4, six more chains whose heads have the next smallest closest-pair
    root distance, against the noise-free oracle tracker: tables on every frame and n_dead / next_id exact, the ALS iteration count on
    every frame below the cap, joints to 1e-8 -- the bar of the random-walk workloads above -- except the weak solves named in WEAK.
    Measured: 10 config-4 chains, joints within 1.1e-13 m but for the one WEAK tracklet-frame (2.3e-7 m); 4 config-5 chains, 1.3e-14 m;
    ALS counts equal on all 224 frames.  The oracle runs in spawned worker processes (NumPy only, one chain each)."""
    import multiprocessing as mp
    chains, cams = scene_run(fixture)
    keys = list(chains)
    with mp.get_context("spawn").Pool(min(8, len(keys))) as pool:
        done = pool.map(oracle_chain_job, [(chains[k]["kps25"], chains[k]["counts"], cams[k[0]]) for k in keys], chunksize=1)
    dd, per, als_diff, n_frames, weak = [], [], [], 0, []
    for k, (rows, n_dead, next_id) in zip(keys, done):
        r = chains[k]
        dk = []
        for tt, (exp, jts, it_o) in enumerate(rows):
            n = int(r["n_tracks"][tt])
            assert n == len(exp) and np.array_equal(r["meta"][tt, :n], exp), (k, tt, r["meta"][tt, :n], exp)
            for s, j in enumerate(jts):
                dj = float(np.abs(r["joints"][tt, s] - j).max())
                bar = WEAK.get((fixture, k[0], k[1], tt, int(exp[s][0])))
                if bar is None:
                    dk.append(dj)
                else:
                    weak.append(dj)
                    assert dj < bar, (k, tt, exp[s].tolist(), dj)
                if dj > 1e-8:
                    print(f"  above 1e-8: segment {k[0]} chain {k[1]} frame {tt} slot {s} meta {exp[s].tolist()}: {dj:.2e} m")
            if int(r["als_iters"][tt]) != it_o:
                als_diff.append((k, tt, int(r["als_iters"][tt]), it_o))
            n_frames += 1
        assert (n_dead, next_id) == (r["n_dead"], r["next_id"]), k
        per.append((k, r["head"], max(dk)))
        dd += dk
    dd = np.array(dd)
    print(f"ALS iterations equal to the oracle's on {n_frames - len(als_diff)} of {n_frames} frames; the others: {als_diff[:8]}")
    heads = np.array([p[1] for p in per])
    print(f"\n{fixture}: {len(keys)} chains against the noise-free oracle tracker, closest-pair root distance at their heads "
          f"{np.round(heads, 4).tolist()} m: tables equal on every frame; {len(dd)} tracklet-frames, joint difference median "
          f"{np.median(dd):.1e} p90 {np.percentile(dd, 90):.1e} max {dd.max():.1e} m; worst per chain "
          f"{[(int(p[0][1]), float('%.1e' % p[2])) for p in per]}; the weak solves gated apart: {['%.1e' % w for w in weak]}")
    assert heads.min() < 0.2                              # the close-pair regime is covered
    assert len(weak) == len([w for w in WEAK if w[0] == fixture])
    assert not [a for a in als_diff if max(a[2], a[3]) < 1000], als_diff[:8]       # every frame below the cap
    assert dd.max() < 1e-8
