"""Device gates of the exchange repair (multiview_motion_capture_amd/exchanges.py, csrc/mvmc_exchange.hip) against the restatement
tests/exchange_np.py: the hand-built cases of tests/exchange_cases.py, the apply kernel against the host permutation, batch
independence, a clean scene against mvmc_body_observe, and the stage end to end through the real tracker."""
import numpy as np
import pytest

import exchange_cases as ec
import exchange_np as ex

CASES = ec.all_cases()
IDS = [c["name"].replace(" ", "_").replace(",", "") for c in CASES]

pytestmark = pytest.mark.gpu


def _calibs(K, Rt):
    from multiview_motion_capture_amd.common import Calib
    return [Calib.from_k_rt(K[c], Rt[c]) for c in range(len(K))]


def _close(got, want, tol=1e-9):
    """Equal to tol px, with the same NaNs and infinities."""
    got, want = np.asarray(got), np.asarray(want)
    fin = np.isfinite(want)
    return np.array_equal(fin, np.isfinite(got)) and np.array_equal(np.isnan(want), np.isnan(got)) and \
        np.array_equal(want[~fin & ~np.isnan(want)], got[~fin & ~np.isnan(got)]) and np.all(np.abs(got[fin] - want[fin]) <= tol)


@pytest.mark.parametrize("cs", CASES, ids=IDS)
def test_device_equals_the_restatement_on_the_hand_built_cases(cs):
    import torch

    from multiview_motion_capture_amd import device as dev, exchanges
    from multiview_motion_capture_amd.sequences import check_records, plan_groups, problem_tables, stack_group
    seqs = [(k, n, _calibs(K, Rt)) for k, n, _, K, Rt in cs["seqs"]]
    before = [k.copy() for k, _, _ in seqs]
    recs = ec.as_records(cs["records"])
    # the entry itself, on the shared front end's tables: members and flags exactly, dist and cost to 1e-9 px
    shapes, arrs = check_records(seqs, recs, "test")
    T = dev.uploader(torch.device("cuda:0"))
    for lay in plan_groups(shapes, 1):
        grp = stack_group(lay, seqs)
        sel = problem_tables(grp, arrs)
        k17, c17 = dev.ingest(T(grp.kps), T(grp.cnt))
        mem, dist, flags, cost = dev.exchange_observe(k17, c17, T(grp.Pm), T(sel.frame_of), T(sel.rig_of), T(sel.joints), T(sel.order),
                                                      T(sel.lo), T(sel.hi), T(sel.rank), exchanges.MAX_DIST, exchanges.MIN_SCORE,
                                                      cs["params"]["margin_px"], cs["params"]["ratio"])
        mem, dist, flags, cost = (x.cpu().numpy() for x in (mem, dist, flags, cost))
        np_seqs = [(cs["seqs"][i][0], cs["seqs"][i][1], cs["seqs"][i][2]) for i in lay.seq_ids]
        _, problems, (sel_np, dist_np, flags_np, cost_np) = ex.repair(np_seqs, [cs["records"][i] for i in lay.seq_ids], **cs["params"])
        assert len(problems) == mem.shape[0]
        C, Pg = grp.n_views, grp.Pg
        q_want = (sel.frame_of.astype(np.int64)[:, None] * C + np.arange(C)[None, :]) * Pg + sel_np
        assert np.array_equal(mem, np.where(sel_np >= 0, q_want, -1)), cs["name"]
        assert np.array_equal(flags, flags_np), cs["name"]
        assert _close(dist, dist_np) and _close(cost, cost_np), cs["name"]
    # the stage: the truth of the case, the restatement's report and its repaired bytes
    want, _, _ = ex.repair([(k, n, P) for k, n, P, _, _ in cs["seqs"]], cs["records"], **cs["params"])
    tm = {}
    repaired, report = exchanges.repair_sequences(seqs, recs, timings=tm, **cs["params"])
    assert set(tm) == {"pack", "observe", "report", "apply", "read_back"}
    for s, ((k, n, cal), rep) in enumerate(zip(repaired, report)):
        assert np.array_equal(rep["flags"], cs["flags"][s]) and np.array_equal(rep["record"], cs["record"][s]), (cs["name"], s)
        assert np.array_equal(rep["flags"], want[s]["flags"]) and _close(rep["cost"], want[s]["cost"])
        assert rep["flags"].dtype == np.uint8 and rep["record"].dtype == np.int32 and rep["cost"].dtype == np.float64
        assert rep["exchanged"] == {g: int(np.count_nonzero(cs["flags"][s] & (1 << b))) for b, g in enumerate(("arms", "legs", "face"))}
        assert k.dtype == before[s].dtype and k.shape == before[s].shape and k.tobytes() == want[s]["kps"].tobytes()
        assert n is seqs[s][1] and cal is seqs[s][2] and k is not seqs[s][0]
        assert seqs[s][0].tobytes() == before[s].tobytes()                    # the input is untouched
    if len(seqs) == 1:
        one, rep_one = exchanges.repair_tracklets(recs[0], *seqs[0], **cs["params"])
        assert one[0].tobytes() == repaired[0][0].tobytes() and np.array_equal(rep_one["flags"], report[0]["flags"])


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("J", [17, 25])
def test_apply_equals_the_host_permutation_bit_for_bit(dtype, J):
    """Odd sizes, more than one workgroup, and more triples than the grid has lanes (2048 x 256: the grid-stride path)."""
    import torch

    from multiview_motion_capture_amd import device as dev, exchanges
    rng = np.random.default_rng(J)
    for shape in ((1, 1, 1), (7, 3, 5), (31, 5, -(-2048 * 256 // (J * 31 * 5)) + 1)):
        kps = rng.normal(300.0, 200.0, shape + (J, 3)).astype(dtype)
        kps[rng.random(kps.shape) < 0.01] = np.nan
        kps[rng.random(shape) < 0.1] = 0.0
        flags = rng.integers(0, 8, shape).astype(np.uint8)
        flags[rng.random(shape) < 0.5] = 0
        got = dev.exchange_apply(torch.from_numpy(kps).cuda(), torch.from_numpy(flags).cuda())
        assert got.dtype == torch.from_numpy(kps).dtype and tuple(got.shape) == kps.shape
        want = exchanges.apply_flags(kps, flags)
        assert got.cpu().numpy().tobytes() == want.tobytes(), shape
        if np.prod(shape) <= 105:
            assert ex.apply(kps, flags).tobytes() == want.tobytes()
    assert shape[0] * shape[1] * shape[2] * J > 2048 * 256


def _scene_with_records(seed, C, P, n_frames=30, exchanged=True):
    from multiview_motion_capture_amd import synth
    g = synth.generate(n_frames, C, P, seed, walk="scene")
    kps = ec.draw_exchanges(g["kps25"], 900 + seed)[0] if exchanged else g["kps25"]
    rng = np.random.default_rng(seed)
    recs = [ec.Record(np.arange(n_frames), g["gt_joints"][:, p] + rng.normal(0.0, 0.01, (n_frames, 18, 3)), p) for p in range(P)]
    return (kps, g["counts"], _calibs(g["K"], g["Rt"])), recs


def test_a_sequence_gives_the_same_bits_alone_and_among_the_others_and_from_run_to_run():
    from multiview_motion_capture_amd import exchanges
    made = [_scene_with_records(seed, C, P) for seed, (C, P) in zip((11, 12, 13, 14), ((5, 4), (4, 3), (5, 2), (5, 4)))]
    made[3] = ((made[3][0][0].astype(np.float64),) + made[3][0][1:], made[3][1][:2])      # a float64 sequence with fewer records
    seqs, recs = [m[0] for m in made], [m[1] for m in made]
    rep_all, info_all = exchanges.repair_sequences(seqs, recs)
    rep_again, info_again = exchanges.repair_sequences(seqs, recs)
    assert sum(sum(r["exchanged"].values()) for r in info_all) > 100
    for s in range(len(seqs)):
        one, info = exchanges.repair_sequences([seqs[s]], [recs[s]])
        for other, oinfo in ((rep_all[s], info_all[s]), (rep_again[s], info_again[s])):
            assert one[0][0].dtype == seqs[s][0].dtype and one[0][0].tobytes() == other[0].tobytes()
            assert info[0]["exchanged"] == oinfo["exchanged"]
            for k in ("flags", "record", "cost"):
                assert info[0][k].tobytes() == oinfo[k].tobytes(), (s, k)


def test_on_a_clean_scene_the_selection_is_body_observes_and_no_flag_is_set():
    from multiview_motion_capture_amd import device as dev, exchanges, synth
    from multiview_motion_capture_amd.sequences import check_records, plan_groups, select_views, stack_group, track_sequences
    import torch
    g = synth.generate(60, 5, 3, 41, walk="scene")
    seqs = [(g["kps25"], g["counts"], _calibs(g["K"], g["Rt"]))]
    recs = track_sequences(seqs, chain_len=16)
    shapes, arrs = check_records(seqs, recs, "test")
    d = torch.device("cuda:0")
    T = dev.uploader(d)
    lay, = plan_groups(shapes, 1)
    sel = select_views(stack_group(lay, seqs), arrs, d, exchanges.MAX_DIST, exchanges.MIN_SCORE)
    mem, dist, flags, cost = dev.exchange_observe(sel.k17, sel.c17, sel.Pm_d, T(sel.frame_of), sel.rig_d, T(sel.joints), T(sel.order),
                                                  T(sel.lo), T(sel.hi), T(sel.rank), exchanges.MAX_DIST, exchanges.MIN_SCORE)
    assert sel.members.shape[0] >= 100 and int((sel.members >= 0).sum()) >= 300
    assert torch.equal(mem, sel.members)
    assert int(flags.sum()) == 0
    repaired, report = exchanges.repair_sequences(seqs, recs)
    assert repaired[0][0].tobytes() == g["kps25"].tobytes() and not report[0]["flags"].any()


def _mpjpe(records, g, min_len=10):
    """Mean joint error of the records against the generator's people (a record follows the person its joints are nearest to)."""
    err = []
    for t in records:
        if len(t) < min_len:
            continue
        J = np.array([q[2].keypoints for q in t.poses])
        e = np.linalg.norm(J[:, None] - g["gt_joints"][np.array(t.frame_idxs)], axis=-1).mean(-1)       # (n, people)
        err.append(e[:, e.mean(0).argmin()])
    return float(np.mean(np.concatenate(err))), int(sum(len(e) for e in err))


def test_end_to_end_the_second_track_is_nearer_the_truth_on_every_seed():
    """60 frames, 5 cameras, 3 people, seeds 51, 52, 53 (scene walks), 20 % of the detections with the arms or the legs exchanged (the
    robust probe's draw): track_sequences -> fit_sequences -> smooth_sequences(loss="cauchy") -> repair_sequences -> track_sequences on
    the repaired keypoints.  Gate: the re-tracked records' MPJPE against the generator's joints is strictly below the first track's,
    on every seed.  Printed beside it: the clean input's MPJPE, and precision and recall of the flags against the drawn exchanges.
    Measured on one MI355X (records of 10 frames or more; precision counts a face flag as wrong, the draw exchanges no face):
      seed 51: 184 exchanges, 181 flagged, 150 correct (precision 0.829, recall 0.815); MPJPE first track 34.01 mm, re-tracked 11.86 mm,
               clean input 8.46 mm
      seed 52: 187 exchanges, 164 flagged, 156 correct (precision 0.951, recall 0.834); 36.36 mm -> 8.46 mm, clean 8.26 mm
      seed 53: 204 exchanges, 183 flagged, 182 correct (precision 0.995, recall 0.892); 35.03 mm -> 10.69 mm, clean 9.67 mm
    No recall is gated: it is the Cauchy smoother's records that decide it."""
    from multiview_motion_capture_amd import exchanges, synth
    from multiview_motion_capture_amd.body_fit import fit_sequences
    from multiview_motion_capture_amd.sequences import track_sequences
    from multiview_motion_capture_amd.smoothing import smooth_sequences
    seeds = (51, 52, 53)
    gts = [synth.generate(60, 5, 3, s, walk="scene") for s in seeds]
    cal = [_calibs(g["K"], g["Rt"]) for g in gts]
    drawn = [ec.draw_exchanges(g["kps25"], 900 + i) for i, g in enumerate(gts)]
    clean = [(g["kps25"], g["counts"], c) for g, c in zip(gts, cal)]
    dirty = [(k, g["counts"], c) for (k, _), g, c in zip(drawn, gts, cal)]

    def track(seqs):
        for chain_len in (16, 8):            # (the stitch may refuse contaminated chains of 16 frames: the robust probe's fall-back)
            try:
                return track_sequences(seqs, chain_len=chain_len)
            except RuntimeError:
                if chain_len == 8:
                    raise
    first = track(dirty)
    smoothed = smooth_sequences(dirty, fit_sequences(dirty, first), loss="cauchy")
    repaired, report = exchanges.repair_sequences(dirty, smoothed)
    second = track(repaired)
    ref = track(clean)
    for i, (g, (_, truth)) in enumerate(zip(gts, drawn)):
        present = (np.arange(3)[None, None, :] < g["counts"][:, :, None]) & (g["gt_order"] >= 0)
        truth = np.where(present, truth, 0).astype(np.uint8)
        fl = report[i]["flags"]
        tp = sum(int(np.count_nonzero(truth & fl & b)) for b in (1, 2))
        n_true = sum(int(np.count_nonzero(truth & b)) for b in (1, 2))
        n_flag = sum(int(np.count_nonzero(fl & b)) for b in (1, 2, 4))
        e1, n1 = _mpjpe(first[i], g)
        e2, n2 = _mpjpe(second[i], g)
        e0, n0 = _mpjpe(ref[i], g)
        print(f"\nseed {seeds[i]}: exchanges {n_true}, flagged {n_flag}, correct {tp}: precision {tp / max(n_flag, 1):.3f}, recall "
              f"{tp / max(n_true, 1):.3f}; MPJPE mm first track {1e3 * e1:.2f} ({n1} poses), re-tracked {1e3 * e2:.2f} ({n2}), clean input "
              f"{1e3 * e0:.2f} ({n0})")
        assert n_true > 100 and n1 > 100 and n2 > 100
        assert e2 < e1, (seeds[i], e1, e2)
