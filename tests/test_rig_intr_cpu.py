"""The restatement of the rig refinement with intrinsic unknowns (tests/rig_intr_np.py) on its own, no GPU: that without intrinsics it is
the restatements it builds on, that its Jacobian columns and its prior are derivatives, what the geometry leaves unobservable (the
null spaces the two refusals of refine_rigs come from), that every case of tests/rig_intr_cases.py takes the branch it is named for
with every decision clear of its threshold, and what it recovers on the ground-truth scene of tests/test_rig_refine_cpu.py."""
import numpy as np
import pytest

import rig_cases as rc
import rig_intr_cases as rci
import rig_intr_np as ri
import rig_refine_np as rr
import rig_robust_np as rb

# the ground-truth scene, measured with this restatement: every camera's centre and rotation error after intrinsics="focal" (after
# the similarity that aligns the centres).  Worse than the 0.6 - 0.9 mm / 0.009 - 0.023 deg of a known K: the focal / depth correlation
SCENE_CENTRE_MM, SCENE_ROTATION_DEG = 2.40, 0.0257        # the largest of 0.63 - 2.40 mm and 0.010 - 0.026 deg
SCENE_GATE = (2.0 * SCENE_CENTRE_MM * 1e-3, 2.0 * SCENE_ROTATION_DEG)


def _same(a, b):
    for k in a:
        if isinstance(a[k], (np.ndarray, list, float)):
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k
        elif a[k] is None or isinstance(a[k], (str, int)):
            assert a[k] == b[k], k


@pytest.mark.parametrize("name", list(rc.CASES))
def test_without_intrinsics_it_is_the_restatements_it_builds_on(name):
    """intrinsics=None: every entry of rig_refine_np.solve's result and, with a loss, of rig_robust_np.solve's, bit for bit, on every
    case of tests/rig_cases.py."""
    c, p = rc.case(name), rc.params(name)
    _same(rr.solve(c["prob"], c["K"], c["Rt"], **p), ri.solve(c["prob"], c["K"], c["Rt"], **p))
    for loss in ("huber", "cauchy"):
        _same(rb.solve(c["prob"], c["K"], c["Rt"], loss=loss, **p), ri.solve(c["prob"], c["K"], c["Rt"], loss=loss, **p))


def _residuals(X, uv, K, R, t, sw):
    r = rr.project(K, R, t, X) - uv
    return np.nan_to_num(r) * sw[..., None]


@pytest.mark.parametrize("loss", [None, "huber", "cauchy"])
def test_intrinsic_columns_are_central_differences(loss):
    """d(u, v)/dphi = (u - cx, v - cy), d/dcx = (1, 0), d/dcy = (0, 1) of every observation against central differences of the
    projection with K moved as the trial moves it, through sqrt(w) (the weights of the linearisation point, as the reweighted
    iteration takes them); the residual rows likewise."""
    c = rci.case("cauchy")
    p, K, Rt = c["prob"], c["K"], c["Rt"]
    R, t = Rt[:, :, :3], Rt[:, :, 3]
    J = ri.jacobian(p["X"], p["uv"], K, R, t, 3, loss, 3.0)
    w = rb.weights(p["X"], p["uv"], K, R, t, loss, 3.0)
    sw = np.sqrt(np.nan_to_num(w))
    assert (np.sqrt(w[~np.isnan(w)]) < 0.9).any() == (loss is not None)
    r0 = _residuals(p["X"], p["uv"], K, R, t, sw)
    assert np.abs(r0[..., 0] - J["ru"]).max() <= 1e-12 and np.abs(r0[..., 1] - J["rv"]).max() <= 1e-12
    cam, row = np.arange(4), np.full(4, 0)
    for k, h in ((0, 1e-6), (1, 1e-3), (2, 1e-3)):
        d = []
        for s in (+h, -h):
            Kk = ri.apply_step(K, R, t, np.full(4, s), cam, row + 6 + k)[0]
            d.append(_residuals(p["X"], p["uv"], Kk, R, t, sw))
        fd = (d[0] - d[1]) / (2.0 * h)
        err = max(np.abs(fd[..., 0] - J["ju"][..., 6 + k]).max(), np.abs(fd[..., 1] - J["jv"][..., 6 + k]).max())
        print(f"{loss} column {k}: {err:.2e} of {np.abs(J['ju'][..., 6 + k]).max():.1f}")
        assert err <= 1e-6 * max(1.0, np.abs(J["ju"][..., 6 + k]).max())


def test_the_prior_agrees_with_its_finite_difference_gradient():
    """The prior's part of the camera gradient (terms with the prior minus terms without) against central differences of E_prior
    along every intrinsic column, at a K away from the prior's centre; its diagonal term is 1 / sigma^2."""
    c = rci.case("fc_c7")
    p, K, Rt, K0 = c["prob"], c["K"], c["Rt"], c["K_true"]
    R, t, held = Rt[:, :, :3], Rt[:, :, 3], p["held"]
    ifree = ri.free_intrinsics(held, 3, (2,))
    sf, sc = 0.02, 15.0
    A = ri.terms(p["X"], p["uv"], K, R, t, held, 1e-3, ifree, 3, K0, sf, sc)
    B = ri.terms(p["X"], p["uv"], K, R, t, held, 1e-3, ifree, 3, K0)
    cam, row = A["cam"], A["row"]
    assert not ((cam == 2) & (row >= 6)).any() and ((cam == 0) & (row >= 6)).sum() == 3 and not ((cam == 0) & (row < 6)).any()
    for i in np.flatnonzero(row >= 6):
        h = 1e-6 if row[i] == 6 else 1e-4
        e = [ri.prior(ri.apply_step(K, R, t, np.eye(cam.size)[i] * s, cam, row)[0], K0, ifree, 3, sf, sc) for s in (+h, -h)]
        fd = (e[0] - e[1]) / (2.0 * h)
        g = A["gc"][i] - B["gc"][i]
        assert abs(fd - g) <= 1e-7 * max(1.0, abs(g)), (i, fd, g)
        assert abs((A["dU"][i] - B["dU"][i]) - 1.0 / (sf if row[i] == 6 else sc) ** 2) <= 1e-9 * A["dU"][i]
    assert np.array_equal(A["gc"][row < 6], B["gc"][row < 6]) and A["E"] > B["E"]
    assert abs(A["E"] - B["E"] - ri.prior(K, K0, ifree, 3, sf, sc)) <= 1e-12 * A["E"]


def test_sigma_inf_is_no_prior_and_a_tiny_sigma_keeps_k():
    """sigma = +inf equals no prior to 1e-13; focal_sigma = 1e-9 returns the input K to 1e-8 (and still refines the poses)."""
    c, p = rci.case("sigma_inf"), rci.params("sigma_inf")
    a = ri.solve(c["prob"], c["K"], c["Rt"], **p)
    b = ri.solve(c["prob"], c["K"], c["Rt"], **{**p, "focal_sigma": None})
    assert a["trials"] == b["trials"] and a["stop"] == b["stop"]
    for k in ("K", "Rt", "X", "cost"):
        assert np.abs(np.asarray(a[k]) - np.asarray(b[k])).max() <= 1e-13 * np.abs(np.asarray(b[k])).max(), k
    t = ri.solve(c["prob"], c["K"], c["Rt"], **{**p, "focal_sigma": 1e-9})
    assert np.abs(t["K"] - c["K"]).max() <= 1e-8 * 1000.0 and np.abs(t["k_moved"]).max() <= 1e-8
    assert t["rms_after"] < 0.5 * t["rms_before"] and a["rms_after"] < t["rms_after"]
    fe = lambda K: np.abs(np.log(K[:, 0, 0] / c["K_true"][:, 0, 0])).max()
    tight, _ = rci.reference("tight")
    print(f"worst focal error: input {fe(c['K']):.4f}, sigma 1e-4 {fe(tight['K']):.4f}, no prior {fe(a['K']):.4f}")
    assert abs(fe(tight["K"]) - fe(c["K"])) <= 1e-3 * fe(c["K"]) and fe(a["K"]) < 0.75 * fe(c["K"])     # a tight prior decides the result


@pytest.mark.parametrize("name", ["f_c8", "fc_c8", "reject", "cauchy", "tight"])
def test_the_gauge_rescale_leaves_e_unchanged(name):
    """E, prior included, before and after the rescale of every accepted trial: 1e-12 relative.  The rescale moves no intrinsic."""
    out, _ = rci.reference(name)
    assert len(out["gauge"]) == sum(out["trials"]) >= 2
    print(name, max(out["gauge"]))
    assert max(out["gauge"]) <= 1e-12


def _null_dim(C, NI, sf=np.inf, sc=np.inf):
    """The null space of the reduced camera matrix at the true ring rig (150 points in the 2 x 2 x 1.8 m box, 2 px noise, occlusion
    0.3, camera 0's pose held, no damping): columns scaled to a unit diagonal, eigenvalues below 1e-8 counted -> (count, the gap:
    the smallest eigenvalue above 1e-8)."""
    c = rc.make(C=C, N=150, seed=100 + C, rot_deg=0.0, trans_m=0.0)
    p, held = c["prob"], c["prob"]["held"]
    T = ri.terms(p["X"], p["uv"], c["K"], c["Rt"][:, :, :3], c["Rt"][:, :, 3], held, 0.0, ri.free_intrinsics(held, NI), NI, c["K"], sf, sc)
    d = 1.0 / np.sqrt(np.diag(T["S"]))
    w = np.linalg.eigvalsh(T["S"] * d[:, None] * d[None])
    return int((w < 1e-8).sum()), float(w[w >= 1e-8].min())


def test_what_the_geometry_leaves_unobservable():
    """The null spaces behind the two refusals, on rig_cases.ring_rig (cameras that fixate one point, as most tripod rigs do).  Focal
    only: the scale gauge alone at C = 3, 5, 8, one more direction at C = 2.  Focal + principal point without a prior: three more at
    C = 5.  With centre_sigma_px the matrix is positive definite up to the gauge.  Every count is separated from the spectrum by more
    than three orders of magnitude."""
    got = {("focal", C): _null_dim(C, 1) for C in (2, 3, 5, 8)}
    got[("focal+centre", 5)] = _null_dim(5, 3)
    got[("focal+centre, centre_sigma_px 20", 5)] = _null_dim(5, 3, sc=20.0)
    got[("focal+centre, both priors", 2)] = _null_dim(2, 3, sf=0.05, sc=20.0)
    for k, v in got.items():
        print(k, v)
    assert [got[("focal", C)][0] for C in (2, 3, 5, 8)] == [2, 1, 1, 1]
    assert got[("focal+centre", 5)][0] == 4 and got[("focal+centre, centre_sigma_px 20", 5)][0] == 1
    assert got[("focal+centre, both priors", 2)][0] == 1
    assert min(v[1] for v in got.values()) >= 1e-5
    for kw in (dict(intrinsics="focal+centre"), dict(intrinsics="focal+centre", centre_sigma_px=np.inf)):
        with pytest.raises(ValueError):
            ri.check(C=5, focal_sigma=None, **{"centre_sigma_px": None, **kw})
    with pytest.raises(ValueError):
        ri.check("focal", None, None, 2)
    assert ri.check("focal", 0.05, None, 2) == (1, 0.05, np.inf) and ri.check("focal", None, None, 3)[0] == 1


@pytest.mark.parametrize("name", list(rci.CASES))
def test_case_precondition(name):
    """Every point has at least two observations among the cameras of the problem, a pose-held camera other than camera 0 has none,
    and every free camera but the deliberately empty one has."""
    mk = rci.CASES[name][0]
    p = rci.case(name)["prob"]
    obs = ~np.isnan(p["uv"][:, :, 0])
    assert (obs.sum(axis=1) >= 2).all() and np.isfinite(p["X"]).all()
    for c in range(obs.shape[1]):
        if c and p["held"][c]:
            assert not obs[:, c].any()
        elif c != mk.get("empty"):
            assert obs[:, c].sum() >= 10
    assert 61 <= p["X"].shape[0] <= 199


@pytest.mark.parametrize("name", list(rci.CASES))
def test_case_margins(name):
    """Every decision the device has to reproduce is a factor 10 clear of its threshold (rig_cases.margin_violations' rule)."""
    assert rci.margin_violations(name) == []


def test_cases_take_their_branches():
    ref = {n: rci.reference(n) for n in rci.CASES}
    trials = {n: ref[n][0]["trials"] for n in rci.CASES}
    stop = {n: ref[n][0]["stop"] for n in rci.CASES}
    cols = lambda n: ref[n][1][0]["terms"]["cam"].size
    assert cols("f_c3") == 15 and cols("f_c8") == 50 and cols("fc_c8") == 66 and cols("fc_c7") == 57 and cols("fc_c2") == 12
    assert rci.case("f_c5_65")["prob"]["X"].shape[0] == 65 and rci.case("fc_c8")["prob"]["X"].shape[0] == 130
    t = ref["k_held_mid"][1][0]["terms"]                        # a camera between the others with its pose columns alone
    assert [int(((t["cam"] == c) & (t["row"] >= 6)).sum()) for c in range(5)] == [1, 1, 0, 1, 1] and cols("k_held_mid") == 28
    t = ref["k_held_0"][1][0]["terms"]                          # camera 0 without any column
    assert not (t["cam"] == 0).any() and cols("k_held_0") == 27
    t = ref["pose_held"][1][0]["terms"]                         # the camera whose observations left has no column at all
    assert not (t["cam"] == 2).any() and cols("pose_held") == 22
    for n in ("k_held_mid", "k_held_0"):
        out, c = ref[n][0], rci.case(n)
        assert np.array_equal(out["K"][~out["ifree"]], c["K"][~out["ifree"]]) and (out["K"][out["ifree"]] != c["K"][out["ifree"]]).any()
    assert 0 in trials["reject"] and 1 in trials["reject"][trials["reject"].index(0):] and trials["reject"][0] == 1
    assert trials["bad"] == [0] * 6 and all(t["bad"] for t in ref["bad"][1])
    assert stop["xtol"] == "xtol" and stop["ftol"] == "ftol" and stop["maxit"] == "max_iter" and trials["maxit"] == [1, 1]
    assert trials["maxit0"] == [] and stop["maxit0"] == "max_iter"
    assert ref["tight"][0]["cost_prior"] > 0 and ref["fc_c8"][0]["cost_prior"] > 0 and ref["sigma_inf"][0]["cost_prior"] == 0.0
    for n in ("huber", "cauchy"):
        assert (ref[n][0]["weights"] < 0.9).sum() > 10 and ref[n][0]["loss"] == n
    for n in rci.CASES:                                         # the refinement does what it is for, where nothing is in its way
        if n not in ("bad", "maxit0", "tight", "reject"):
            assert ref[n][0]["rms_after"] < 0.4 * ref[n][0]["rms_before"], n


def test_trial_is_one_step_of_solve():
    """solve() with a trace is solve() without, and its first look is trial() at the start values with the prior about the input K."""
    c, p = rci.case("fc_c7"), rci.params("fc_c7")
    a = ri.solve(c["prob"], c["K"], c["Rt"], **p)
    b, trace = rci.reference("fc_c7")
    assert np.array_equal(a["K"], b["K"]) and np.array_equal(a["Rt"], b["Rt"]) and a["trials"] == b["trials"]
    held = c["prob"]["held"]
    t = ri.trial(c["prob"]["X"], c["prob"]["uv"], c["K"], c["Rt"][:, :, :3], c["Rt"][:, :, 3], held, p["mu0"], ri.free_intrinsics(held, 3), 3,
                 c["K"], np.inf, p["centre_sigma_px"])
    assert np.array_equal(t["dc"], trace[0]["dc"]) and t["Et"] == trace[0]["Et"] == b["cost"][1]


@pytest.fixture(scope="module")
def scene():
    """tests/test_rig_refine_cpu.py's scene: a 5 x 4 scene walk, ground-truth association, every 5th frame (4,080 points), cameras 1 - 4
    perturbed by N(0, 1 deg) / N(0, 3 cm); and every camera's focal length off by a seeded U(-5 %, +5 %)."""
    from multiview_motion_capture_amd import synth
    d = synth.generate(300, 5, 4, seed=7, walk="scene", shuffle=False)
    Kt = np.asarray(d["K"], np.float64)
    K = Kt.copy()
    f = np.exp(np.random.default_rng(711).uniform(-0.05, 0.05, 5))
    K[:, 0, 0] *= f
    K[:, 1, 1] *= f
    return d, rr.gt_candidates(d, frame_step=5), K, Kt, rr.perturb_rig(d["Rt"], 11)


def test_ground_truth_on_the_prototype_scene(scene):
    """intrinsics="focal" on the ground-truth scene.  The worst focal error afterwards is at most 0.25 x the worst before (measured:
    4.34 % -> 0.09 %; the noise floor of 4,080 points); the plain rms ends within 2 % of sqrt(2) sigma sqrt(1 - unknowns / residuals)
    (measured 2.344 against 2.340 px; without intrinsics the same input ends at 2.62 px, with centre errors of 23 - 122 mm); after the
    similarity that aligns the centres, every camera's centre error is within 2 x the measured 2.40 mm and its rotation error within
    2 x the measured 0.0257 deg (0.63 - 2.40 mm, 0.010 - 0.026 deg: worse than the 0.6 - 0.9 mm of a known K, the price of the
    focal / depth correlation)."""
    d, cand, K, Kt, Rt0 = scene
    out = ri.refine(cand, K, Rt0, intrinsics="focal")
    fe0, fe1 = (np.abs(np.log(k[:, 0, 0] / Kt[:, 0, 0])) for k in (K, out["K"]))
    ce, re = rr.rig_errors(out["Rt"], d["Rt"])
    unknowns = 3 * out["n_points"] + 6 * 4 + 5 - 1            # (the scale gauge is no unknown)
    expect = np.sqrt(2.0) * 2.0 * np.sqrt(1.0 - unknowns / (2.0 * out["n_obs"]))
    print(f"{out['n_points']} points, trials {out['trials']}, stop {out['stop']}; focal error {100 * fe0.max():.2f} % -> {100 * fe1.max():.3f} % "
          f"({np.round(100 * fe1, 3)}); rms {out['rms_before']:.2f} -> {out['rms_after']:.3f} px, expected {expect:.3f}; centres "
          f"{np.round(1e3 * ce, 2)} mm, rotations {np.round(np.degrees(re), 4)} deg")
    assert out["n_points"] == 4080 and out["stop"] in ("ftol", "xtol")
    assert fe1.max() <= 0.25 * fe0.max()
    assert abs(out["rms_after"] - expect) <= 0.02 * expect
    assert ce.max() <= SCENE_GATE[0] and np.degrees(re.max()) <= SCENE_GATE[1]
    assert np.array_equal(out["K"][:, :2, 2], K[:, :2, 2]) and np.array_equal(out["Rt"][0], Rt0[0])
    plain = ri.refine(cand, K, Rt0)
    assert plain["rms_after"] > 1.05 * out["rms_after"]
