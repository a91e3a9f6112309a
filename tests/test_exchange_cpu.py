"""CPU gates of the exchange repair (multiview_motion_capture_amd/exchanges.py): the restatement tests/exchange_np.py on the hand-built
cases of tests/exchange_cases.py, the host-side apply, the argument checks (no device), and the rule's statistics on a synthetic scene."""
import numpy as np
import pytest

import exchange_cases as ec
import exchange_np as ex

CASES = ec.all_cases()
IDS = [c["name"].replace(" ", "_").replace(",", "") for c in CASES]


def _np_seqs(cs):
    return [(k, n, P) for k, n, P, _, _ in cs["seqs"]]


@pytest.mark.parametrize("cs", CASES, ids=IDS)
def test_the_restatement_gives_the_built_in_truth(cs):
    out, problems, (sel, dist, flags, cost) = ex.repair(_np_seqs(cs), cs["records"], **cs["params"])
    assert len(problems) <= 8
    for s, res in enumerate(out):
        assert np.array_equal(res["flags"], cs["flags"][s]), (cs["name"], s)
        assert np.array_equal(res["record"], cs["record"][s]), (cs["name"], s)
        chosen = res["record"] >= 0
        assert np.all(np.isnan(res["cost"][~chosen])) and not np.any(res["flags"][~chosen])
        for g in range(3):                                          # an exchanged group has its two costs, and e1 < e0
            hit = (res["flags"] >> g & 1) == 1
            assert np.all(res["cost"][hit][:, g, 1] < res["cost"][hit][:, g, 0])
    for s, f, c, p, g in cs["nan_cost"]:
        assert out[s]["record"][f, c, p] >= 0 and np.all(np.isnan(out[s]["cost"][f, c, p, g]))
        assert np.all(np.isfinite(np.delete(out[s]["cost"][f, c, p], g, axis=0)))
    assert np.all(np.isinf(dist[sel < 0]) | (dist[sel < 0] < ex.D_MAX))        # a loser keeps the distance it lost with


def test_a_whole_body_flip_lies_beyond_max_dist_as_it_is_and_the_tie_is_exact():
    import body_fit_np as bf
    cs = next(c for c in CASES if c["name"].startswith("whole body flip"))
    kps, _, P, _, _ = cs["seqs"][0]
    n = 0
    for f, c, p in np.argwhere(cs["flags"][0] == 7):
        person = int(cs["record"][0][f, c, p])
        d = bf.reproj_dist(cs["J"][0][f, person], np.asarray(kps[f, c, p], np.float64), P[c])
        assert d > ex.D_MAX, d                                      # body_observe selects nothing here
        n += 1
    assert n == 2
    cs = next(c for c in CASES if c["name"].startswith("exact tie"))
    out, _, _ = ex.repair(_np_seqs(cs), cs["records"], **cs["params"])
    cost = out[0]["cost"][0, 0, 0, 2]
    assert cost[0] == cost[1] and cost[0] > 10.0, cost              # e0 == e1 bit for bit, and nothing is exchanged
    assert out[0]["flags"][0, 0, 0] == 0


@pytest.mark.parametrize("cs", CASES, ids=IDS)
def test_host_apply_is_a_pure_permutation_and_the_repaired_arrays_flag_nothing(cs):
    from multiview_motion_capture_amd import exchanges
    out, _, _ = ex.repair(_np_seqs(cs), cs["records"], **cs["params"])
    again, _, _ = ex.repair([(res["kps"], n, P) for res, (_, n, P) in zip(out, _np_seqs(cs))], cs["records"], **cs["params"])
    for s, (kps, _, _) in enumerate(_np_seqs(cs)):
        got = exchanges.apply_flags(kps, out[s]["flags"])
        assert got.dtype == kps.dtype and got.shape == kps.shape
        assert got.tobytes() == out[s]["kps"].tobytes()             # the package's host apply is the restatement's, bit for bit
        hit = out[s]["flags"] != 0
        assert np.array_equal(got[~hit], kps[~hit], equal_nan=True)
        a, b = (np.nan_to_num(x[hit].astype(np.float64), nan=-1e9) for x in (got, kps))
        key = lambda x: np.array([sorted(map(tuple, pose)) for pose in x])
        assert np.array_equal(key(a), key(b))                       # the same triples, under other names
        assert hit.sum() == 0 or not np.array_equal(a, b)
        # idempotent where the thresholds are the defaults (a threshold case sits on its own boundary by construction)
        assert not again[s]["flags"].any(), (cs["name"], np.argwhere(again[s]["flags"]))
        assert np.array_equal(exchanges.apply_flags(got, out[s]["flags"]), kps, equal_nan=True)      # an exchange is its own inverse


def test_group_rows_and_ingest_slots_are_the_restatements():
    from multiview_motion_capture_amd import exchanges
    for J in (17, 25):
        for flag in range(8):
            want = sorted(ex.swap_rows(J, flag))
            got = sorted(p for b, pairs in exchanges.group_pairs(J).items() if flag & b for p in pairs)
            assert got == want == sorted(ec.rows_of(J, flag)), (J, flag)
    rng = np.random.default_rng(3)
    for J in (17, 25):
        kps = rng.uniform(0, 600, (6, 3, 5, J, 3))
        kps[..., 2] = rng.uniform(0, 1, kps.shape[:-1]) * (rng.random(kps.shape[:-1]) < 0.6)
        kps[rng.random((6, 3, 5)) < 0.3] *= np.array([1e-3, 1e-3, 1.0])        # tiny boxes: filter_bad_pose drops them
        kps[rng.random((6, 3, 5)) < 0.2, :, 2] = 0.0                           # nobody there
        kps[0, 0, 0, 3, 0] = np.nan
        counts = rng.integers(0, 6, (6, 3)).astype(np.int32)
        got = exchanges.ingest_slots(kps.astype(np.float32), counts)
        want = ex.ingest_slots(kps.astype(np.float32), counts)
        n_kept = 0
        for f in range(6):
            for c in range(3):
                g = want[f][c]
                assert got[f, c, :len(g)].tolist() == g and np.all(got[f, c, len(g):] == -1)
                n_kept += len(g)
        assert 10 < n_kept < counts.sum()


def test_argument_checks_run_before_any_device_call(monkeypatch):
    from multiview_motion_capture_amd import _cabi, device as dev, exchanges
    from multiview_motion_capture_amd.common import Calib

    def boom(*a, **k):
        raise AssertionError("device called")
    for name in ("ingest", "exchange_observe", "exchange_apply", "body_observe", "uploader"):
        monkeypatch.setattr(dev, name, boom)
    monkeypatch.setattr(_cabi, "load", boom)
    cs = CASES[1]
    kps, cnt, _, K, Rt = cs["seqs"][0]
    cal = [Calib.from_k_rt(K[c], Rt[c]) for c in range(len(K))]
    recs = ec.as_records(cs["records"])[0]
    bad = [dict(margin_px=-1.0), dict(margin_px=np.nan), dict(margin_px=np.inf), dict(margin_px=-np.inf), dict(margin_px="4"),
           dict(margin_px=None), dict(margin_px=True)]
    for kw in bad:
        with pytest.raises(ValueError, match="margin_px"):
            exchanges.repair_sequences([(kps, cnt, cal)], [recs], **kw)
        with pytest.raises(ValueError, match="margin_px"):
            exchanges.repair_tracklets(recs, kps, cnt, cal, **kw)
    for kw in [dict(ratio=0.0), dict(ratio=-0.5), dict(ratio=1.0 + 1e-12), dict(ratio=np.nan), dict(ratio=np.inf), dict(ratio=None)]:
        with pytest.raises(ValueError, match="ratio"):
            exchanges.repair_sequences([(kps, cnt, cal)], [recs], **kw)
    # the records' usual faults, as the other record stages report them
    with pytest.raises(ValueError, match="record lists"):
        exchanges.repair_sequences([(kps, cnt, cal)], [recs, recs])
    with pytest.raises(ValueError, match="records without sequences"):
        exchanges.repair_sequences([], [recs])
    with pytest.raises(ValueError, match="outside the 2 frames"):
        exchanges.repair_sequences([(kps, cnt, cal)], [[ec.Record([0, 2], np.zeros((2, 18, 3)))]])
    with pytest.raises(ValueError, match="appears twice"):
        exchanges.repair_sequences([(kps, cnt, cal)], [[ec.Record([1, 1], np.zeros((2, 18, 3)))]])
    with pytest.raises(ValueError, match="poses must be"):
        exchanges.repair_sequences([(kps, cnt, cal)], [[ec.Record([0, 1], np.zeros((2, 17, 3)))]])
    with pytest.raises(ValueError, match="kps25 must be"):
        exchanges.repair_sequences([(kps[..., :2], cnt, cal)], [recs])
    # a calibration that still carries a lens: refused as by every stage that reads pinhole pixels
    from multiview_motion_capture_amd import lens
    lensed = list(cal)
    lensed[1] = Calib.from_k_rt(K[1], Rt[1], lens=lens.Lens(_cabi.LENS_BROWN, (0.1,) + (0.0,) * 7))
    with pytest.raises(ValueError, match="repair_sequences: sequence 0: camera 1 has a lens model"):
        exchanges.repair_sequences([(kps, cnt, lensed)], [recs])
    # an empty call returns empty lists; the defaults are the documented ones
    assert exchanges.repair_sequences([], []) == ([], [])
    assert (exchanges.MARGIN_PX, exchanges.RATIO) == (4.0, 0.7) == (ex.MARGIN_PX, ex.RATIO)
    assert exchanges.MAX_DIST == ex.D_MAX and exchanges.MIN_SCORE == ex.MIN_SCORE


def test_the_entries_refuse_bad_arguments_before_any_hip_call():
    """mvmc_exchange_observe and mvmc_exchange_apply with nothing to do (0 problems / 0 slots, no GPU needed)."""
    from multiview_motion_capture_amd import _cabi
    lib = _cabi.load()
    observe = lambda margin, ratio, n=0, c=3: lib.mvmc_exchange_observe(None, None, 2, c, 2, None, 1, None, None, None, None, None, None, None,
                                                                        n, 0.1, 36.0, margin, ratio, None, None, None, None, None)
    for margin, ratio in ((4.0, 0.7), (0.0, 1.0), (1e300, 1e-300)):
        assert observe(margin, ratio) == _cabi.MVMC_OK
    for margin, ratio in ((-1.0, 0.7), (float("nan"), 0.7), (float("inf"), 0.7), (4.0, 0.0), (4.0, 1.5), (4.0, float("nan")), (4.0, -0.1)):
        assert observe(margin, ratio) == 1, (margin, ratio)
    assert observe(4.0, 0.7, n=-1) == 1 and observe(4.0, 0.7, c=0) == 1
    assert observe(4.0, 0.7, n=5) == 1                                  # work to do and no buffers
    apply = lambda dtype, n, J: lib.mvmc_exchange_apply(None, dtype, n, J, None, None, None)
    assert apply(_cabi.MVMC_F32, 0, 25) == apply(_cabi.MVMC_F64, 0, 17) == _cabi.MVMC_OK
    assert apply(2, 0, 25) == 1 and apply(_cabi.MVMC_F32, 0, 18) == 1 and apply(_cabi.MVMC_F32, -1, 17) == 1
    assert apply(_cabi.MVMC_F32, 4, 17) == 1


def test_recall_and_false_decisions_on_a_synthetic_scene_with_good_joints():
    """synth.generate(100, 5, 4, 20280101, walk="scene"), 20 % of the detections with the arms or the legs exchanged (the robust
    probe's draw, seed 900), one record per person from the ground-truth joints + N(0, 1 cm) (seed 1), the default margin_px = 4 and
    ratio = 0.7, through this restatement (its own exchange-aware selection).  An exchange counts where the slot holds a detection of
    a real person.  Gates: recall >= 0.98, false decisions (a group flagged that was not exchanged, any of the three) <= 2 % of the
    true exchanges.  Measured: 377 exchanges, 375 found (recall 0.9947), no false decision; 1,998 of the 2,000 detections are selected
    by a record -- the two exchanges missed are the two detections no record selects (an experiment that took the selection from the
    generator's order found 377 of 377 and 2 false decisions)."""
    from multiview_motion_capture_amd import synth
    g = synth.generate(100, 5, 4, 20280101, walk="scene")
    kps, drawn = ec.draw_exchanges(g["kps25"], 900)
    present = (np.arange(4)[None, None, :] < g["counts"][:, :, None]) & (g["gt_order"] >= 0)
    truth = np.where(present, drawn, 0).astype(np.uint8)
    rng = np.random.default_rng(1)
    records = [dict(frames=np.arange(100), joints=g["gt_joints"][:, p] + rng.normal(0.0, 0.01, (100, 18, 3))) for p in range(4)]
    out, _, _ = ex.repair([(kps, g["counts"], g["P"])], [records])
    flags = out[0]["flags"]
    n_true = int(np.count_nonzero(truth & 1) + np.count_nonzero(truth & 2))
    found = int(np.count_nonzero(truth & flags & 1) + np.count_nonzero(truth & flags & 2))
    false = int(sum(np.count_nonzero(flags & ~truth & b) for b in (1, 2, 4)))
    print(f"\nexchanges {n_true}, found {found} (recall {found / n_true:.4f}), false decisions {false} ({100.0 * false / n_true:.2f} % of "
          f"the true ones), detections {int(present.sum())}, selected {int((out[0]['record'] >= 0).sum())}")
    assert n_true > 300
    assert found >= 0.98 * n_true
    assert false <= 0.02 * n_true
    # and the repaired keypoints are the generator's, where a real person was decided
    fixed = out[0]["kps"]
    decided = present & (out[0]["record"] >= 0) & (flags == truth)
    assert np.array_equal(fixed[decided][:, :19], g["kps25"][decided][:, :19])
