"""The robust loss of the rig refinement on its NumPy restatement (tests/rig_robust_np.py) alone: that without a loss it IS
tests/rig_refine_np.py, the loss's analytic properties, that every case of tests/rig_robust_cases.py takes the branch it is named for
with every decision far from its threshold (so that tests/test_gpu_rig_robust.py can ask the device for the same decisions), and what
the loss is for: the rig calibration's polish on walks whose detections exchange left and right."""
import numpy as np
import pytest

import rig_cases as rc
import rig_init_cases as ric
import rig_init_np as ri
import rig_refine_np as rr
import rig_robust_cases as rcs
import rig_robust_np as rb
from test_rig_init_cpu import RIG_GATE

# the worst camera's centre and rotation error with a loss at 6 px over those of the plain polish, on the contaminated walks
CENTRE_RATIO, ROTATION_RATIO = 0.75, 0.5


@pytest.mark.parametrize("name", list(rc.CASES))
def test_without_a_loss_it_is_the_plain_restatement(name):
    """loss=None: solve returns rig_refine_np.solve's result exactly -- every array and number of it -- on every case of
    tests/rig_cases.py, and so do terms, trial and cost at the start."""
    c, p = rc.case(name), rc.params(name)
    tra, trb = [], []
    a = rr.solve(c["prob"], c["K"], c["Rt"], trace=tra, **p)
    b = rb.solve(c["prob"], c["K"], c["Rt"], trace=trb, loss=None, **p)
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], str) or a[k] is None:
            assert a[k] == b[k], k
        else:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k
    assert len(tra) == len(trb)
    for x, y in zip(tra, trb):
        assert x["bad"] == y["bad"]
        for k in ("dc", "dp", "pred", "dmax", "Et", "E"):
            if not x["bad"]:
                assert np.array_equal(x[k], y[k]), k
        for k in ("E", "S", "g", "gp", "Vd"):
            assert np.array_equal(x["terms"][k], y["terms"][k]), k


@pytest.mark.parametrize("loss", rcs.LOSSES)
def test_loss_is_continuous_and_w_is_its_derivative(loss):
    """rho and w continuous at s = delta (Huber's two branches meet there; Cauchy is smooth): one-sided values within 1e-12
    relative; w = rho'(s) / s against a central difference on both sides of delta and far from it (h = 1e-5 s: the difference's own
    error is h^2 rho''' / 6 ~ 1e-10 relative, its rounding eps / h ~ 1e-11; gate 1e-8)."""
    for d in (0.5, 6.0, 40.0):
        lo, hi = np.nextafter(d, 0.0), np.nextafter(d, np.inf)
        for f in (0, 1):
            a, b, m = (rb.rho_w(np.array(x * x), loss, d)[f] for x in (lo, hi, d))
            assert abs(a - m) <= 1e-12 * abs(m) and abs(b - m) <= 1e-12 * abs(m)
        s = d * np.array([1e-3, 0.3, 0.999, 1.001, 1.5, 3.0, 30.0])
        h = 1e-5 * s
        num = (rb.rho_w((s + h) ** 2, loss, d)[0] - rb.rho_w((s - h) ** 2, loss, d)[0]) / (2.0 * h) / s
        w = rb.rho_w(s * s, loss, d)[1]
        assert np.abs(num / w - 1.0).max() <= 1e-8, (d, num, w)
        assert np.all(w > 0.0) and np.all(w <= 1.0) and np.all(rb.rho_w(s * s, loss, d)[0] <= 0.5 * s * s * (1 + 1e-15))
    assert np.all(rb.rho_w(np.array([0.0, 1e-300]), loss, 6.0)[1] == 1.0)           # no 0 / 0 at a residual of zero


@pytest.mark.parametrize("name", ["c2", "c4_held_mid", "c8", "far"])
def test_huber_at_1e30_is_the_plain_cost_and_terms(name):
    """Huber with delta = 1e30 has w = 1 and rho = 1/2 s^2 for every residual: cost and every array of terms within 1e-13 relative (to
    the largest entry) of rig_refine_np's on the contaminated problem."""
    c = rcs.case(name)
    prob, K, R, t = c["prob"], c["K"], c["Rt"][:, :, :3], c["Rt"][:, :, 3]
    a = rr.terms(prob["X"], prob["uv"], K, R, t, prob["held"], 1e-3)
    b = rb.terms(prob["X"], prob["uv"], K, R, t, prob["held"], 1e-3, "huber", 1e30)
    for k in ("E", "S", "g", "Wf", "Vd", "Vi", "gp", "gc", "dU", "dV"):
        assert np.abs(np.asarray(a[k]) - np.asarray(b[k])).max() <= 1e-13 * np.abs(a[k]).max(), k
    ea, eb = rr.cost(prob["X"], prob["uv"], K, R, t), rb.cost(prob["X"], prob["uv"], K, R, t, "huber", 1e30)
    assert abs(ea - eb) <= 1e-13 * ea
    w = rb.weights(prob["X"], prob["uv"], K, R, t, "huber", 1e30)
    assert np.all(w[~np.isnan(w)] == 1.0) and np.array_equal(np.isnan(w), np.isnan(prob["uv"][:, :, 0]))


@pytest.mark.parametrize("name,loss", rcs.PAIRS)
def test_gauge_rescale_leaves_the_robust_cost_unchanged(name, loss):
    """The rescale after an accepted trial moves no residual: the robust E at the rescaled state equals the trial's to 1e-12
    relative, at every accepted trial of every case."""
    out, _ = rcs.reference(name, loss)
    assert len(out["gauge"]) == sum(out["trials"])
    assert all(g <= 1e-12 for g in out["gauge"]), max(out["gauge"])


@pytest.mark.parametrize("name,loss", rcs.PAIRS)
def test_case_margins(name, loss):
    """Every decision of the case's reference solve is clear of its threshold (rig_robust_cases.violations: zero allowed), so the
    device, which agrees with the restatement to ~1e-13 on these quantities, cannot decide otherwise for rounding reasons; no
    reduced matrix fails its Cholesky factorisation; and every step is finite (the largest, 129 m on a point of a rejected trial of a
    rig 14 degrees off, is no overflow hazard)."""
    out, trace = rcs.reference(name, loss)
    assert rcs.margin_violations(name, loss) == []
    assert not any(t["bad"] for t in trace) and all(t["dmax"] < 1e3 for t in trace)
    assert len(trace) in (len(out["trials"]), len(out["trials"]) + 1)
    assert np.isfinite(out["Rt"]).all() and np.isfinite(out["weights"][~np.isnan(out["weights"])]).all()


def test_cases_take_their_branches():
    """What each case is in the table for."""
    ref = {(n, l): rcs.reference(n, l) for n, l in rcs.PAIRS}
    res = {k: ("".join(map(str, v[0]["trials"])), v[0]["stop"], len(v[1])) for k, v in ref.items()}
    print()
    for k, v in res.items():
        print(f"  {k[0]:14s} {k[1]:7s} trials {v[0] or '-':9s} stop {v[1]:8s} looks {v[2]}")
    for n in ("c2", "c3_full", "c4_held_mid", "c5_65", "c8", "far", "delta_small"):
        for l in rcs.LOSSES:
            assert res[n, l][:2] == ("111111", "max_iter") and ref[n, l][0]["cost"][-1] < 0.7 * ref[n, l][0]["cost"][0]
    assert rcs.case("c4_held_mid")["prob"]["held"].tolist() == [True, False, True, False]
    assert [rcs.case(n)["prob"]["X"].shape[0] for n in ("c2", "c3_full", "c5_65", "c8")] == [70, 64, 65, 130]
    for l in rcs.LOSSES:
        # every observation of the far points lies beyond delta at the start: all their weights < 1; delta = 1e30: all 1; 0.5: nearly all < 1
        def w0(n):
            c = rcs.case(n)
            return c, rb.weights(c["prob"]["X"], c["prob"]["uv"], c["K"], c["Rt"][:, :, :3], c["Rt"][:, :, 3], l, rcs.params(n)["loss_px"])
        c, w = w0("far")
        assert c["far"].size == 8 and np.nanmax(w[c["far"]]) < 0.7 and np.all((~np.isnan(w[c["far"]])).sum(axis=1) >= 3)
        _, w = w0("delta_inf")
        assert np.all(w[~np.isnan(w)] == 1.0) and res["delta_inf", l][:2] == ("111", "max_iter")
        _, w = w0("delta_small")
        assert np.mean(w[~np.isnan(w)] < 1.0) > 0.95
        assert np.mean(ref["delta_small", l][0]["weights"][~np.isnan(w)] < 1.0) > 0.7          # ... and most still at the end (a point of two views ends on both)
        assert res["maxit0", l] == ("", "max_iter", 0) and len(ref["maxit0", l][0]["cost"]) == 1
    # rejected, then accepted trials
    assert res["reject", "huber"][0] == "11011111" and res["reject_c", "cauchy"][0] == "11001111"
    # the stop rules: xtol and ftol on the prediction come before a trial (one more look than trials), ftol after a trial does not
    for n, l in (("xtol", "huber"), ("xtol_c", "cauchy")):
        assert res[n, l] == ("11", "xtol", 3)
    for n, l in (("ftol_before", "huber"), ("ftol_before_c", "cauchy"), ("maxit_cap", "huber"), ("maxit_cap_c", "cauchy")):
        assert res[n, l] == ("11", "ftol", 3)
    assert rcs.params("maxit_cap")["max_iter"] == rcs.params("maxit_cap_c")["max_iter"] == rc.MAX_ITER_CAP
    assert res["ftol_after", "huber"] == ("1", "ftol", 1) and res["ftol_after_c", "cauchy"] == ("1001", "ftol", 4)
    # the cases of the tolerance rules do reweight: some Huber weights below 1 at the start, every Cauchy weight
    c = rcs.case("xtol")
    wh = rb.weights(c["prob"]["X"], c["prob"]["uv"], c["K"], c["Rt"][:, :, :3], c["Rt"][:, :, 3], "huber", rcs.params("xtol")["loss_px"])
    assert 0 < np.sum(wh[~np.isnan(wh)] < 1.0)


def _polish(name, loss):
    """The polish of rig_init_np.calibrate on the walk, from the same pose-graph rig and with the same gates, through the robust
    restatement -> (worst centre error m, worst rotation error degrees, the solve's dict)."""
    out, det = ric.reference(name)
    w, _ = ric.case(name)
    pol = rb.refine(ri.candidates(det["px"]), w["K"], out["Rt_tree"], max_iter=10, max_px=ri.POLISH_PX, min_score=0.1, min_views=2,
                    min_cam_obs=100, loss=loss, loss_px=6.0)
    ce, re = rr.rig_errors(pol["Rt"], w["Rt"])
    return float(ce.max()), float(np.degrees(re.max())), pol


@pytest.mark.parametrize("name", ["dirty_11", "dirty_12", "clean_11", "clean_12"])
def test_polish_against_ground_truth(name):
    """The four walks of tests/rig_init_cases.py (5 views x 120 frames; the dirty ones with 20 % of the detections' left and right
    exchanged and 10 % moved by up to 150 px), polished from the pose-graph rig with max_iter = 10 and the default tolerances.  On the
    dirty walks each loss at 6 px ends with the worst camera's centre error <= 0.75 x and rotation error <= 0.5 x the plain polish's
    (rig_init_cases.reference, computed here); on the clean walks each loss stays inside the clean gate of tests/test_rig_init_cpu.py.
    Measured (worst camera; plain -> Huber, Cauchy; ratios in brackets):
      dirty_11   8.08 mm, 0.245 deg -> 4.07 mm, 0.070 deg (0.50, 0.28); 2.68 mm, 0.047 deg (0.33, 0.19)
      dirty_12  13.48 mm, 0.309 deg -> 5.72 mm, 0.096 deg (0.42, 0.31); 3.26 mm, 0.053 deg (0.24, 0.17)
      clean_11   0.70 mm, 0.017 deg -> 0.69 mm, 0.017 deg; 1.01 mm, 0.018 deg
      clean_12   1.46 mm, 0.027 deg -> 1.44 mm, 0.027 deg; 1.27 mm, 0.027 deg
    -- the ratios the gates were set beside (0.50 / 0.42 and 0.29 / 0.31 for Huber, 0.33 / 0.24 and 0.19 / 0.17 for Cauchy), so the
    gates are those: 0.75 and 0.5.  Every robust solve runs its ten trials (the plain ones stop on ftol after 3 - 5); 13 - 18 % of a
    camera's observations end with w < 0.5 on the dirty walks, at most 1 % on the clean ones."""
    out, _ = ric.reference(name)
    w, _ = ric.case(name)
    ce0, re0 = (float(v.max()) for v in rr.rig_errors(out["Rt"], w["Rt"]))
    re0 = float(np.degrees(re0))
    plain = _polish(name, None)
    assert abs(plain[0] - ce0) <= 1e-12 and abs(plain[1] - re0) <= 1e-10          # the same polish through the robust restatement
    for loss in rcs.LOSSES:
        ce, re, pol = _polish(name, loss)
        print(f"\n{name} {loss}: centre {1e3 * ce0:.2f} -> {1e3 * ce:.2f} mm ({ce / ce0:.2f}), rotation {re0:.3f} -> {re:.3f} deg ({re / re0:.2f}); "
              f"trials {len(pol['trials'])}, stop {pol['stop']}, rms {pol['rms_before']:.2f} -> {pol['rms_after']:.2f} px, downweighted "
              f"{np.round(pol['downweighted'], 3)}")
        if name.startswith("dirty"):
            assert ce <= CENTRE_RATIO * ce0 and re <= ROTATION_RATIO * re0
            assert 0.08 <= pol["downweighted"].min() and pol["downweighted"].max() <= 0.3
        else:
            assert ce <= RIG_GATE["clean"][0] and re <= RIG_GATE["clean"][1]
            assert pol["downweighted"].max() <= 0.02
        assert np.all(np.diff(pol["cost"]) <= 0) and pol["cost"][0] < out["polish"]["cost"][0]
