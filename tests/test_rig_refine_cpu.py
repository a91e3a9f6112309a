"""Rig refinement without a GPU: the NumPy restatement (tests/rig_refine_np.py) against synthetic ground truth, its invariants, and
the host side of multiview_motion_capture_amd/rig_refine.py (input checks, packing)."""
import numpy as np
import pytest

import rig_refine_np as rr

PIX_SIGMA = 2.0
RMS_EXPECTED = 2.34       # sqrt(2) sigma sqrt(1 - unknowns / residuals) for 4,080 points, 19,418 observations, 4 free cameras


@pytest.fixture(scope="module")
def scene():
    from multiview_motion_capture_amd import synth
    d = synth.generate(300, 5, 4, seed=7, walk="scene", shuffle=False)
    return d, rr.gt_candidates(d, frame_step=5)


def test_recovery_on_the_prototype_scene(scene):
    """5 x 4 scene walk, ground-truth association, every 5th frame, cameras 1-4 perturbed by N(0, 1 deg) / N(0, 3 cm).  After the
    similarity alignment of the centres every camera's centre and rotation error is <= 0.2 x the RMS of the errors before (measured:
    0.6 - 0.9 mm and 0.009 - 0.023 deg against 55 mm and 0.8 deg, about 0.02), rms_after <= sqrt(2) pix_sigma, rms_before > 2 x 2.34."""
    d, cand = scene
    Rt0 = rr.perturb_rig(d["Rt"], 11)
    out = rr.refine(cand, d["K"], Rt0)
    ce0, re0 = rr.rig_errors(Rt0, d["Rt"])
    ce, re = rr.rig_errors(out["Rt"], d["Rt"])
    print(f"\n{out['n_points']} points, {out['n_obs']} observations, rms {out['rms_before']:.2f} -> {out['rms_after']:.3f} px, trials "
          f"{out['trials']}, stop {out['stop']}\n  centres mm {np.round(1e3 * ce0, 1)} -> {np.round(1e3 * ce, 2)}\n  rotations deg "
          f"{np.round(np.rad2deg(re0), 3)} -> {np.round(np.rad2deg(re), 4)}")
    assert (out["n_points"], out["n_obs"]) == (4080, 19418)
    assert np.all(ce <= 0.2 * np.sqrt(np.mean(ce0 ** 2))) and np.all(re <= 0.2 * np.sqrt(np.mean(re0 ** 2)))
    assert out["rms_after"] <= np.sqrt(2.0) * PIX_SIGMA
    assert out["rms_before"] > 2.0 * RMS_EXPECTED
    assert out["stop"] in ("ftol", "xtol") and len(out["trials"]) <= 6


def test_the_true_rig_in(scene):
    """No camera moves by more than the noise floor.  The restatement's floor on this input: centres 0.57 - 0.88 mm, rotations
    0.0091 - 0.0233 deg (the prototype's: 0.6 - 0.9 mm, 0.01 - 0.02 deg); gates at twice the largest: 1.77 mm and 0.047 deg.  E must
    not increase (2.611 -> 2.344 px rms: the DLT points are not the reprojection optimum)."""
    d, cand = scene
    out = rr.refine(cand, d["K"], d["Rt"])
    ce, re = rr.rig_errors(out["Rt"], d["Rt"])
    print(f"\ncentres mm {np.round(1e3 * ce, 3)}, rotations deg {np.round(np.rad2deg(re), 4)}, rms {out['rms_before']:.3f} -> {out['rms_after']:.3f}")
    assert ce.max() <= 2 * 0.883e-3 and np.rad2deg(re.max()) <= 2 * 0.0234
    assert out["cost"][-1] <= out["cost"][0]


def test_invariants(scene):
    from multiview_motion_capture_amd.common import Calib
    d, cand = scene
    Rt0 = rr.perturb_rig(d["Rt"], 12)
    out = rr.refine(cand, d["K"], Rt0)
    assert np.array_equal(out["Rt"][0], Rt0[0])                                   # camera 0: bit for bit
    c_in, c_out = rr.centres(Rt0), rr.centres(out["Rt"])
    L0, L1 = np.linalg.norm(c_in[1] - c_in[0]), np.linalg.norm(c_out[1] - c_out[0])
    assert abs(L1 - L0) <= 1e-12 * L0
    assert out["gauge"] and max(out["gauge"]) <= 1e-12                            # the rescale leaves E unchanged
    acc = [c for c, t in zip(out["cost"][1:], out["trials"]) if t]
    assert np.all(np.diff([out["cost"][0]] + acc) < 0) and np.all(np.diff(out["cost"]) <= 0)
    for c in range(5):
        cal = Calib.from_k_rt(d["K"][c], out["Rt"][c])
        assert np.array_equal(cal.P, cal.K @ cal.Rt)
        assert np.abs(cal.Kr_inv @ (cal.K @ cal.Rt[:, :3]) - np.eye(3)).max() < 1e-12
        R = out["Rt"][c, :, :3]
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and np.linalg.det(R) > 0


def test_held_cameras_and_degenerate_input(scene):
    d, cand = scene
    Rt0 = rr.perturb_rig(d["Rt"], 13)
    few = cand.copy()
    few[50:, 3, 2] = 0.0                       # camera 3 sees 50 candidates only: held, its observations leave the problem
    out = rr.refine(few, d["K"], Rt0)
    assert list(out["held"]) == [True, False, False, True, False] and out["obs_per_camera"][3] == 0
    assert np.array_equal(out["Rt"][3], Rt0[3]) and np.array_equal(out["Rt"][0], Rt0[0])
    assert out["stop"] in ("ftol", "xtol") and out["rms_after"] <= np.sqrt(2.0) * PIX_SIGMA
    out = rr.refine(cand, d["K"], Rt0, min_cam_obs=10 ** 6)
    assert out["stop"] == "few_cameras" and np.array_equal(out["Rt"], Rt0) and out["trials"] == []
    out = rr.refine(cand[:2], d["K"], Rt0, min_cam_obs=0)
    assert out["stop"] == "few_points" and np.array_equal(out["Rt"], Rt0)


def _record(frames):
    import oracle_np as o
    from multiview_motion_capture_amd.inverse_kinematics import PoseShapeParam
    from multiview_motion_capture_amd.motion_capture import MvTracklet
    from multiview_motion_capture_amd.pose_def import KpsFormat, Pose
    _, ref = o.skeleton_constants()
    x = np.concatenate([[0.0, 0.0, 1.0], np.zeros(54), ref])
    J = o.forward_kinematics(x[:3], x[3:57], x[57:])[0]
    mk = lambda: (PoseShapeParam(x[:3].copy(), x[3:57].reshape(18, 3).copy(), x[57:].copy()), Pose(KpsFormat.BASIC_18, J.copy(), np.ones((18, 1)), None))
    p0 = mk()
    t = MvTracklet(1, frames[0], p0[0], p0[1])
    t.frame_idxs = list(frames)
    t.poses = [(f,) + mk() for f in frames]
    return t


def test_checks_raise_before_any_device_work(scene):
    from multiview_motion_capture_amd import rig_refine as rg
    from multiview_motion_capture_amd.common import Calib
    d, _ = scene
    cal = [Calib.from_k_rt(d["K"][c], d["Rt"][c]) for c in range(5)]
    row = (d["kps25"][:10], d["counts"][:10], cal)
    ok = dict(max_iter=10, max_px=97.0, min_score=0.1, min_views=2, min_cam_obs=100, frame_step=1)
    shapes, recs = rg.check_refine([row], [[_record([2, 3])]], **ok)
    assert shapes == [(10, 5, 4)] and recs[0][0][0].tolist() == [2, 3]
    bad = [
        (([row], [[], []]), {}),                                         # record lists and sequences differ in number
        (([row], [[_record([2, 10])]]), {}),                             # a frame outside kps
        (([row], [[]]), dict(min_views=1)),
        (([row], [[]]), dict(frame_step=0)),
        (([row], [[]]), dict(max_iter=rg.MAX_ITER_CAP + 1)),
        (([(row[0][:, :1], row[1][:, :1], cal[:1])], [[]]), {}),          # fewer than 2 cameras
    ]
    for args, kw in bad:
        with pytest.raises(ValueError):
            rg.check_refine(*args, **{**ok, **kw})
    with pytest.raises(ValueError):
        rg.refine_rigs([row], [[], []])
    with pytest.raises(ValueError):
        rg.refine_rigs([row], [[]], min_views=1)


def test_packing_against_hand_made_cases():
    from multiview_motion_capture_amd import rig_refine as rg
    # two sequences of three cameras; min_views 2, min_cam_obs 2, max_px 10
    valid = np.array([[1, 1, 1], [1, 1, 0], [1, 1, 1], [1, 0, 1], [1, 1, 1],      # sequence 0
                      [1, 1, 1], [1, 1, 1], [1, 1, 1]], bool)                     # sequence 1
    dist = np.ones((8, 3))
    dist[0, 2] = 11.0          # an observation beyond the gate: dropped, the point keeps two views
    dist[3, 2] = 50.0          # ... and here the point falls below min_views
    dist[1, 1] = np.nan        # a NaN distance drops the observation (and here the point)
    x_ok = np.ones(8, bool)
    x_ok[7] = False            # a NaN start value drops the point
    seq_of = np.array([0, 0, 0, 0, 0, 1, 1, 1])
    obs, held, stop = rg.pack_problems(valid, dist, x_ok, seq_of, 2, 10.0, 2, 2)
    assert obs.astype(int).tolist() == [[1, 1, 0], [0, 0, 0], [1, 1, 1], [0, 0, 0], [1, 1, 1], [1, 1, 1], [1, 1, 1], [0, 0, 0]]
    assert held.tolist() == [[True, False, False], [True, False, False]] and stop.tolist() == [0, 4]   # sequence 1: two points
    # camera 2 below min_cam_obs = 3 in sequence 0: held, its observations leave; sequence 0 is left with one free camera
    obs, held, stop = rg.pack_problems(valid, dist, x_ok, seq_of, 2, 10.0, 2, 3)
    assert held.tolist() == [[True, False, True], [True, True, True]]
    assert obs[:5].astype(int).tolist() == [[1, 1, 0], [0, 0, 0], [1, 1, 0], [0, 0, 0], [1, 1, 0]] and not obs[5:].any()
    assert stop.tolist() == [3, 3]
    # tiles are cut from each sequence's own points
    tile, seq = rg.tile_tables([130, 0, 64])
    assert tile.tolist() == [[0, 0, 64, 0], [0, 64, 64, 0], [0, 128, 2, 0], [2, 130, 64, 0]]
    assert seq.tolist() == [[0, 3, 0, 130], [3, 0, 130, 0], [3, 1, 130, 64]]
    # the packing equals the restatement's on a real candidate table
    from multiview_motion_capture_amd import synth
    d = synth.generate(60, 5, 3, seed=9, walk="scene", shuffle=False, occlusion=0.3)
    cand = rr.gt_candidates(d)
    cand = cand[(cand[:, :, 2] > 0.1).sum(axis=1) >= 2]
    Rt0 = rr.perturb_rig(d["Rt"], 3, rot_deg=3.0, trans_m=0.09)
    prob = rr.build_problem(cand, d["K"], Rt0, 20.0, 0.1, 3, 700)
    v = cand[:, :, 2] > 0.1
    X = rr.dlt_points(np.einsum("cij,cjk->cik", d["K"], Rt0), cand, v)
    dd = np.linalg.norm(rr.project(d["K"], Rt0[:, :, :3], Rt0[:, :, 3], X) - cand[:, :, :2], axis=-1)
    obs, held, stop = rg.pack_problems(v, np.where(v, dd, np.nan), np.isfinite(X).all(axis=1), np.zeros(len(cand), int), 1, 20.0, 3, 700)
    assert np.array_equal(held[0], prob["held"]) and np.array_equal(np.flatnonzero(obs.any(axis=1)), prob["rows"])
    assert np.array_equal(obs[obs.any(axis=1)], ~np.isnan(prob["uv"][:, :, 0])) and (~obs).any() and held[0, 1:].any()


# ---- the hand-made cases of the kernel tests (tests/rig_cases.py), proven on the restatement alone ----
import rig_cases as rc


@pytest.mark.parametrize("name", list(rc.CASES))
def test_case_precondition(name):
    """Every point has at least two observations among the cameras of the problem (a point without any makes V = 0 and NaN of its
    whole tile: include/mvmc.h), a held camera other than camera 0 has none, and every free camera but the deliberately empty one has."""
    mk = rc.CASES[name][0]
    c = rc.case(name)
    prob = c["prob"]
    obs = ~np.isnan(prob["uv"][:, :, 0])
    assert prob["X"].shape == (mk["N"], 3) and np.isfinite(prob["X"]).all() and prob["uv"].shape == (mk["N"], mk["C"], 2)
    assert np.array_equal(np.isnan(prob["uv"][:, :, 0]), np.isnan(prob["uv"][:, :, 1]))
    assert obs.sum(axis=1).min() >= 2
    held_extra = sorted(mk.get("held_extra", ()))
    assert np.flatnonzero(prob["held"]).tolist() == [0] + held_extra and prob["stop"] is None
    per_cam = obs.sum(axis=0)
    for k in range(mk["C"]):
        if k in held_extra or k == mk.get("empty"):
            assert per_cam[k] == 0
        else:
            assert per_cam[k] >= 20
    assert not np.array_equal(c["Rt"][1:], c["Rt_true"][1:]) and np.array_equal(c["Rt"][0], c["Rt_true"][0])


@pytest.mark.parametrize("name", list(rc.CASES))
def test_case_margins(name):
    """Every decision the device has to reproduce is clear of its threshold (rig_cases.margin_violations): |Et - E| / E >= 1e-6 at
    every trial, |d|_inf outside [xtol / 10, 10 xtol], pred / E and the accepted reductions outside [ftol / 10, 10 ftol].  Device and
    restatement agree to ~1e-13 on these, so the equalities of trials and stop in tests/test_gpu_rig_kernels.py cannot fail for
    rounding reasons.  A case that violates a margin gets another seed, not another margin."""
    out, trace = rc.reference(name)
    for t in trace:
        if not t["bad"]:
            print(f"  E {t['E']:.6g} mu {t['mu']:.0e} |d|_inf {t['dmax']:.2e} pred / E {t['pred'] / t['E']:.2e} (E - Et) / E {(t['E'] - t['Et']) / t['E']:.2e}")
    assert rc.margin_violations(name) == []
    # the restatement's own error on the reduced matrix (V*^-1 by np.linalg.inv: what it is off by shows as asymmetry) is orders below
    # the 1e-10 the device is gated at: no point's V* is ill-conditioned enough to matter
    for t in trace:
        S = t["terms"]["S"]
        assert np.abs(S - S.T).max() <= 1e-13 * np.abs(S).max() and np.linalg.cond(t["terms"]["Vd"]).max() < 1e5
    # one look per trial, and one more where the stop came before a trial (xtol, or ftol on the prediction)
    assert len(trace) in (len(out["trials"]), len(out["trials"]) + 1)
    if out["stop"] == "max_iter":
        assert len(trace) == len(out["trials"]) == rc.params(name)["max_iter"]


def test_cases_take_their_branches():
    ref = {n: rc.reference(n) for n in rc.CASES}
    trials = {n: ref[n][0]["trials"] for n in rc.CASES}
    stop = {n: ref[n][0]["stop"] for n in rc.CASES}
    print("\n", {n: ("".join(map(str, trials[n])), stop[n]) for n in rc.CASES})
    # the shapes: tiles and blocks as the table says
    shape = {n: (rc.CASES[n][0]["C"], rc.CASES[n][0]["N"]) for n in rc.CASES}
    assert [shape[n] for n in ("c2", "c3_full", "c4_held_mid", "c5_65", "c6", "c7", "c8")] == \
        [(2, 70), (3, 64), (4, 100), (5, 65), (6, 61), (7, 199), (8, 130)]
    for n in ("c2", "c3_full", "c4_held_mid", "c5_65", "c6", "c7", "c8", "maxit_cap"):
        o = ref[n][0]
        assert stop[n] in ("ftol", "xtol") and sum(trials[n]) >= 2 and o["cost"][-1] < 0.2 * o["cost"][0]
        print(f"  {n}: rms {o['rms_before']:.2f} -> {o['rms_after']:.2f} px")
        assert o["rms_after"] <= np.sqrt(2.0) * PIX_SIGMA                            # down to the 2 px noise of the observations
    assert rc.case("c4_held_mid")["prob"]["held"].tolist() == [True, False, True, False]
    assert np.array_equal(ref["c4_held_mid"][0]["Rt"][2], rc.case("c4_held_mid")["Rt"][2])
    # a rejected trial followed by an accepted one, the first trial rejected (the one-trial tests read a rejection there)
    s = "".join(map(str, trials["reject"]))
    assert "01" in s and s[0] == "0" and 6 <= rc.params("reject")["max_iter"] <= 10 and rc.params("reject")["mu0"] == 1e-6
    acc = np.array(trials["reject"], bool)
    cost = np.array(ref["reject"][0]["cost"])
    assert np.all(np.diff(cost)[acc] < 0) and np.all(np.diff(cost)[~acc] == 0)
    assert all(t["Et"] >= 1.006 * t["E"] for t, a in zip(ref["reject"][1], acc) if not a)
    # the matrix is not positive definite at every trial: nothing moves
    o, tr = ref["bad"]
    c = rc.case("bad")
    assert trials["bad"] == [0] * rc.params("bad")["max_iter"] and stop["bad"] == "max_iter" and all(t["bad"] for t in tr)
    assert np.array_equal(o["Rt"], c["Rt"]) and np.array_equal(o["X"], c["prob"]["X"]) and len(set(o["cost"])) == 1
    mu = rr.LM_MU0
    for t in tr:                                                     # mu x 10 at every one of them, exactly
        assert t["mu"] == mu
        mu *= 10.0
    e = rc.CASES["bad"][0]["empty"]
    S = tr[0]["terms"]["S"]
    q = list(tr[0]["terms"]["free"]).index(e)
    assert not c["prob"]["held"][e] and np.all(S[6 * q:6 * q + 6] == 0.0)
    # the three stop rules, each after two accepted trials
    assert (trials["xtol"], stop["xtol"]) == ([1, 1], "xtol") and rc.params("xtol")["xtol"] == 1e-3
    assert (trials["ftol"], stop["ftol"]) == ([1, 1], "ftol") and rc.params("ftol")["ftol"] == 1e-4
    assert (trials["maxit"], stop["maxit"]) == ([1, 1], "max_iter") and rc.params("maxit")["max_iter"] == 2
    assert (trials["maxit0"], stop["maxit0"], len(ref["maxit0"][0]["cost"])) == ([], "max_iter", 1)
    assert rc.params("maxit_cap")["max_iter"] == rc.MAX_ITER_CAP and len(trials["maxit_cap"]) < rc.MAX_ITER_CAP


def test_trial_is_one_step_of_solve():
    """solve() with a trace is solve() without, and its first look is trial() at the start values."""
    c, p = rc.case("c4_held_mid"), rc.params("c4_held_mid")
    a = rr.solve(c["prob"], c["K"], c["Rt"], **p)
    b, trace = rc.reference("c4_held_mid")
    assert np.array_equal(a["Rt"], b["Rt"]) and np.array_equal(a["X"], b["X"]) and a["cost"] == b["cost"] and a["trials"] == b["trials"]
    t = rr.trial(c["prob"]["X"], c["prob"]["uv"], c["K"], c["Rt"][:, :, :3], c["Rt"][:, :, 3], c["prob"]["held"], p["mu0"])
    for k in ("dc", "dp", "R", "t", "X"):
        assert np.array_equal(t[k], trace[0][k])
    assert (t["Et"], t["pred"], t["dmax"], t["dg"], t["dDd"]) == tuple(trace[0][k] for k in ("Et", "pred", "dmax", "dg", "dDd"))
    assert t["Et"] == rr.cost(t["X"], c["prob"]["uv"], c["K"], t["R"], t["t"]) and t["pred"] == 0.5 * (t["mu"] * t["dDd"] - t["dg"])
    assert not t["bad"]
