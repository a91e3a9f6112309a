"""The robust loss of the rig refinement on the device (csrc/mvmc_rigfit.hip: mvmc_rig_accumulate_robust, mvmc_rig_step_robust,
mvmc_rig_weights; rig_refine.refine_rigs(loss=...), rig_init.calibrate_rigs(polish_loss=...)) against its NumPy restatement
(tests/rig_robust_np.py) on the small contaminated problems of tests/rig_robust_cases.py, against the entries without a loss, and
against synthetic ground truth.  tests/test_rig_robust_cpu.py proves on the restatement alone that every decision of a case is far
from its threshold."""
import functools

import numpy as np
import pytest
import torch

import rig_cases as rc
import rig_init_cases as ric
import rig_refine_np as rr
import rig_robust_cases as rcs
import rig_robust_np as rb
from test_rig_init_cpu import RIG_GATE
from test_rig_robust_cpu import CENTRE_RATIO, ROTATION_RATIO

pytestmark = pytest.mark.gpu

MAX_ITER = rc.MAX_ITER_CAP
TRIALS, COSTS = 8, 8 + MAX_ITER
STOP_XTOL, STOP_FTOL, STOP_FEW_CAMERAS, STOP_MAX_ITER = 1, 2, 3, 5
STOP_NAME = {STOP_XTOL: "xtol", STOP_FTOL: "ftol", STOP_MAX_ITER: "max_iter"}
CODE = {None: 0, "huber": 1, "cauchy": 2}
PAIRS = [(n, l) for n in rcs.CASES for l in rcs.CASES[n][2]]
KEYS = ("X", "X_trial", "cams", "cams_trial", "info", "ctl", "red", "w")


def device_solve(problems, K, Rts, max_iter, mu0, ftol, xtol, loss=None, loss_px=6.0, variant=1, steps=None, step=True, stop0=None,
                 plain=False):
    """test_gpu_rig_kernels.device_solve through the _robust entries (plain=True: through the entries without a loss, which take no
    loss): one or several packed problems of equal C, each with its own rig, packed as refine_rigs packs them.  -> dict of NumPy
    arrays: X, X_trial, cams, cams_trial, cams_in, info, ctl, red, part2, w0 and w (the weights at the start and at the end), p_lo."""
    from multiview_motion_capture_amd import device as dev
    from multiview_motion_capture_amd import rig_refine as rg
    d = torch.device("cuda:0")
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(d)
    S, C = len(problems), problems[0]["uv"].shape[1]
    stop0 = np.zeros(S, np.int32) if stop0 is None else np.asarray(stop0, np.int32)
    run = stop0 == 0
    n_pts = np.array([p["X"].shape[0] if r else 0 for p, r in zip(problems, run)])
    tile, seq = rg.tile_tables(n_pts)
    held = np.array([p["held"] for p in problems])
    slot = np.where(held, -1, np.cumsum(~held, axis=1) - 1).astype(np.int32)
    Rts = np.asarray(Rts, np.float64)
    cams = np.concatenate([np.broadcast_to(K.reshape(1, C, 9), (S, C, 9)), Rts[:, :, :, :3].reshape(S, C, 9), Rts[:, :, :, 3]], axis=2)
    info = np.zeros((S, 64))
    info[:, TRIALS:TRIALS + MAX_ITER] = -1.0
    ctl = np.zeros((S, 4), np.int32)
    ctl[:, 0] = stop0
    X = np.concatenate([p["X"] for p, r in zip(problems, run) if r] + [np.zeros((0, 3))])
    uv = np.concatenate([p["uv"] for p, r in zip(problems, run) if r] + [np.zeros((0, C, 2))])
    X_d, uv_d, tile_d, seq_d, slot_d, cams_d, info_d, ctl_d = T(X), T(uv), T(tile), T(seq), T(slot), T(cams), T(info), T(ctl)
    Xt_d, camt_d = X_d.clone(), cams_d.clone()
    part, part2, red = dev.rig_work(tile.shape[0], S, C, d)
    part2.zero_()
    code = CODE[loss]
    w0 = dev.rig_weights(X_d, uv_d, tile_d, cams_d, code, loss_px)
    for _ in range(max(int(max_iter), 1) if steps is None else steps):
        if plain:
            dev.rig_accumulate(X_d, uv_d, tile_d, seq_d, slot_d, cams_d, camt_d, ctl_d, info_d, max_iter, mu0, part, red, variant)
        else:
            dev.rig_accumulate_robust(X_d, uv_d, tile_d, seq_d, slot_d, cams_d, camt_d, ctl_d, info_d, max_iter, mu0, part, red, variant,
                                      code, loss_px)
        if int(max_iter) and step:
            if plain:
                dev.rig_step(X_d, Xt_d, uv_d, tile_d, seq_d, slot_d, cams_d, camt_d, ctl_d, info_d, red, max_iter, ftol, xtol, part2)
            else:
                dev.rig_step_robust(X_d, Xt_d, uv_d, tile_d, seq_d, slot_d, cams_d, camt_d, ctl_d, info_d, red, max_iter, ftol, xtol, part2,
                                    code, loss_px)
    w = dev.rig_weights(X_d, uv_d, tile_d, cams_d, code, loss_px)
    torch.cuda.synchronize()
    N = lambda t: t.cpu().numpy()
    return dict(X=N(X_d), X_trial=N(Xt_d), cams=N(cams_d), cams_trial=N(camt_d), cams_in=cams, info=N(info_d), ctl=N(ctl_d), red=N(red),
                part2=N(part2), w0=N(w0), w=N(w), p_lo=np.concatenate([[0], np.cumsum(n_pts)]))


def _case_solve(name, loss, **kw):
    c, p = rcs.case(name), dict(rcs.params(name))
    return device_solve([c["prob"]], c["K"], [c["Rt"]], loss=loss, **{**p, **kw})


def _rt(cams):
    return np.concatenate([cams[:, 9:18].reshape(-1, 3, 3), cams[:, 18:21, None]], axis=2)


def _rel(a, b):
    """max |a - b| relative to the largest entry of b."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def _unpack(out, s=0):
    n_t = int(out["ctl"][s, 1])
    return [int(v) for v in out["info"][s, TRIALS:TRIALS + n_t]], out["info"][s, COSTS:COSTS + n_t + 1].copy(), STOP_NAME.get(int(out["ctl"][s, 0]))


# ---- a. one trial ----
@pytest.mark.parametrize("name,loss", PAIRS)
def test_one_trial_against_the_restatement(name, loss):
    """ONE trial of every case at its mu0, on the matrix cores and as FMAs: E, the reduced gradient, the reduced matrix, the camera
    step, the point steps, the predicted reduction, the trial cost and the weights at the start, each within 1e-10 of the
    restatement's relative to its largest entry (the existing kernels' gate).  It prints what it measures."""
    c, p = rcs.case(name), rcs.params(name)
    prob, K, Rt = c["prob"], c["K"], c["Rt"]
    C, held = K.shape[0], prob["held"]
    if p["max_iter"] == 0:
        p = {**p, "max_iter": 1}
    t = rb.trial(prob["X"], prob["uv"], K, Rt[:, :, :3], Rt[:, :, 3], held, p["mu0"], loss, p["loss_px"])
    assert not t["bad"]
    w_np = rb.weights(prob["X"], prob["uv"], K, Rt[:, :, :3], Rt[:, :, 3], loss, p["loss_px"])
    M, m = 6 * (C - 1), 6 * int((~held).sum())
    for variant in (1, 0):
        out = device_solve([prob], K, [Rt], loss=loss, variant=variant, steps=1, **p)
        r = out["red"][0]
        S, g, d = r[:M * M].reshape(M, M)[:m, :m], r[M * M:M * M + m], r[M * M + M:M * M + M + m]
        e = dict(E=abs(out["info"][0, 0] - t["terms"]["E"]) / t["terms"]["E"], g=_rel(g, t["terms"]["g"]), S=_rel(S, t["terms"]["S"]),
                 dc=_rel(d, t["dc"]), dp=_rel(out["X_trial"] - prob["X"], t["dp"]), pred=abs(out["info"][0, 7] - t["pred"]) / abs(t["pred"]),
                 Et=abs(out["part2"][:, 0].sum() - t["Et"]) / t["Et"])
        assert np.array_equal(np.isnan(out["w0"]), np.isnan(w_np))
        e["w"] = float(np.nanmax(np.abs(out["w0"] - w_np)))
        print(f"\n{name} {loss} variant {variant}: " + ", ".join(f"{k} {v:.1e}" for k, v in e.items()))
        assert max(e.values()) <= 1e-10, e
        assert out["ctl"][0, 1] == 1 and out["ctl"][0, 3] == 0


# ---- b. whole solves ----
@pytest.mark.parametrize("name,loss", PAIRS)
def test_whole_solves_against_the_restatement(name, loss):
    """The trial list, the stop reason and the number of trials equal the restatement's (its decisions are clear of their thresholds:
    test_rig_robust_cpu.py::test_case_margins); camera centres within 1e-6 m, rotations within 1e-6 rad (the existing gates); the
    final robust cost within 1e-10 relative; the final weights within 1e-6 (they are read at the final cameras); both variants."""
    c, p = rcs.case(name), rcs.params(name)
    exp, _ = rcs.reference(name, loss)
    for variant in (1, 0):
        out = _case_solve(name, loss, variant=variant)
        trials, cost, stop = _unpack(out)
        assert trials == exp["trials"], (trials, exp["trials"])
        assert stop == exp["stop"], (stop, exp["stop"])
        assert out["ctl"][0, 1] == len(exp["trials"]) and out["ctl"][0, 2] == sum(exp["trials"])
        got = _rt(out["cams"][0])
        dc = np.linalg.norm(rr.centres(got) - rr.centres(exp["Rt"]), axis=1).max()
        dr = max(rr.rot_angle(got[k, :, :3] @ np.linalg.inv(exp["Rt"][k, :, :3])) for k in range(got.shape[0]))
        dE = abs(cost[-1] - exp["cost"][-1]) / exp["cost"][-1]
        dw = float(np.nanmax(np.abs(out["w"] - exp["weights"])))
        print(f"\n{name} {loss} variant {variant}: centres {dc:.2e} m, rotations {dr:.2e} rad, final cost {dE:.2e} relative, weights {dw:.2e}; "
              f"trials {trials}, stop {stop}")
        assert dc <= 1e-6 and dr <= 1e-6 and dE <= 1e-10 and dw <= 1e-6
        assert len(cost) == len(exp["cost"]) and out["info"][0, 0] == cost[0] and out["info"][0, 1] == cost[-1]
        assert np.array_equal(out["cams"][0, c["prob"]["held"]], out["cams_in"][0, c["prob"]["held"]])


# ---- c. the loss that is none: delta = 1e30, and loss 0 ----
@pytest.mark.parametrize("loss", rcs.LOSSES)
def test_delta_1e30_equals_the_entries_without_a_loss(loss):
    """delta = 1e30 makes every weight 1 and rho = 1/2 s^2: a whole solve through the _robust entries agrees with the same solve
    through the entries without a loss to 1e-13 relative (to the largest entry) in everything read back."""
    c, p = rcs.case("delta_inf"), rcs.params("delta_inf")
    assert p["loss_px"] == 1e30
    a = device_solve([c["prob"]], c["K"], [c["Rt"]], loss=loss, **p)
    b = device_solve([c["prob"]], c["K"], [c["Rt"]], loss=None, plain=True, **p)
    assert np.array_equal(a["ctl"], b["ctl"]) and a["ctl"][0, 1] >= 2
    e = {k: _rel(np.nan_to_num(a[k]), np.nan_to_num(b[k])) for k in ("X", "X_trial", "cams", "cams_trial", "info", "red", "part2")}
    print(f"\ndelta 1e30 {loss}: " + ", ".join(f"{k} {v:.1e}" for k, v in e.items()))
    assert max(e.values()) <= 1e-13, e
    assert np.all(a["w"][~np.isnan(a["w"])] == 1.0) and np.array_equal(np.isnan(a["w"]), np.isnan(c["prob"]["uv"][:, :, 0]))


@pytest.mark.parametrize("name", ["reject", "c8", "bad"])
def test_loss_none_is_bit_identical_to_the_entries_without_a_loss(name):
    """MVMC_RIG_LOSS_NONE through the _robust entries runs the instantiation the entries without a loss run: whole solves of three of
    tests/rig_cases.py's problems (rejected trials, six row blocks, a matrix that is not positive definite), both variants, every
    array bit-identical.  (loss_px is not read: it is passed as NaN.)"""
    c, p = rc.case(name), rc.params(name)
    for variant in (1, 0):
        a = device_solve([c["prob"]], c["K"], [c["Rt"]], loss=None, loss_px=float("nan"), variant=variant, **p)
        b = device_solve([c["prob"]], c["K"], [c["Rt"]], loss=None, plain=True, variant=variant, **p)
        for k in KEYS + ("part2",):
            assert np.array_equal(a[k], b[k], equal_nan=True), (variant, k)
        assert a["ctl"][0, 1] >= 2


# ---- d. several sequences in one launch ----
def test_several_sequences_in_one_launch():
    """Five 5-camera sequences in one launch -- a rejected-then-accepted solve, one stopped at entry, a tile of one point, a solve that
    stops early on xtol and one with delta = 0.5 -- and two 8-camera sequences in another: cameras, points, costs, trials, control words
    and weights of every sequence are bit-identical alone, together and in a second run."""
    for loss in rcs.LOSSES:
        for names, kw in ((["reject", "stopped", "c5_65", "xtol", "delta_small"], dict(max_iter=8, mu0=1e-4, ftol=1e-12, xtol=rcs.params("xtol")["xtol"])),
                          (["c8", "c8_b"], dict(max_iter=5, mu0=1e-3, ftol=1e-12, xtol=1e-10))):
            cs = [rcs.case({"stopped": "c5_65", "c8_b": "c8"}.get(n, n)) for n in names]
            Rts = [c["Rt"] if n != "c8_b" else rr.perturb_rig(c["Rt_true"], 99) for n, c in zip(names, cs)]
            K = cs[0]["K"]
            stop0 = [STOP_FEW_CAMERAS if n == "stopped" else 0 for n in names]
            a, b = [device_solve([c["prob"] for c in cs], K, Rts, loss=loss, stop0=stop0, **kw) for _ in range(2)]
            for k in KEYS:
                assert np.array_equal(a[k], b[k], equal_nan=True), k
            print("\n", loss, [(n, _unpack(a, s)[0], int(a["ctl"][s, 0])) for s, n in enumerate(names)])
            for s, n in enumerate(names):
                if n == "stopped":
                    assert a["ctl"][s].tolist() == [STOP_FEW_CAMERAS, 0, 0, 0] and np.array_equal(a["cams"][s], a["cams_in"][s])
                    continue
                one = device_solve([cs[s]["prob"]], K, [Rts[s]], loss=loss, **kw)
                lo, hi = a["p_lo"][s], a["p_lo"][s + 1]
                assert np.array_equal(one["cams"][0], a["cams"][s]) and np.array_equal(one["X"], a["X"][lo:hi]), n
                assert np.array_equal(one["info"][0], a["info"][s]) and np.array_equal(one["ctl"][0], a["ctl"][s]), n
                assert np.array_equal(one["w"], a["w"][lo:hi], equal_nan=True), n
            if "xtol" in names:
                s = names.index("xtol")
                assert a["ctl"][s, 0] == STOP_XTOL and a["ctl"][s, 1] < 8 and a["ctl"][names.index("reject"), 1] > a["ctl"][s, 1]


# ---- e. the argument checks ----
def test_argument_checks_launch_nothing():
    from multiview_motion_capture_amd import device as dev
    from multiview_motion_capture_amd import rig_refine as rg
    d = torch.device("cuda:0")
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(d)
    c = rcs.case("c3_full")
    prob, K, Rt = c["prob"], c["K"], c["Rt"]
    C = 3
    tile, seq = rg.tile_tables([prob["X"].shape[0]])
    slot = np.array([[-1, 0, 1]], np.int32)
    cams = np.concatenate([K.reshape(1, C, 9), Rt[:, :, :3].reshape(1, C, 9), Rt[:, :, 3][None]], axis=2)
    info = np.zeros((1, 64))
    info[:, TRIALS:TRIALS + MAX_ITER] = -1.0
    X_d, Xt_d, uv_d, cams_d, camt_d = T(prob["X"]), T(prob["X"]), T(prob["uv"]), T(cams), T(cams)
    info_d, ctl_d = T(info), torch.zeros((1, 4), dtype=torch.int32, device=d)
    part, part2, red = dev.rig_work(1, 1, C, d)
    acc = lambda loss, px, max_iter=10, variant=1: dev.rig_accumulate_robust(X_d, uv_d, T(tile), T(seq), T(slot), cams_d, camt_d, ctl_d, info_d,
                                                                             max_iter, 1e-3, part, red, variant, loss, px)
    stp = lambda loss, px, max_iter=10: dev.rig_step_robust(X_d, Xt_d, uv_d, T(tile), T(seq), T(slot), cams_d, camt_d, ctl_d, info_d, red,
                                                            max_iter, 1e-6, 1e-10, part2, loss, px)
    wts = lambda loss, px: dev.rig_weights(X_d, uv_d, T(tile), cams_d, loss, px)
    bad = [(3, 6.0), (-1, 6.0), (1, 0.0), (2, 0.0), (1, -1.0), (2, float("nan")), (1, float("inf")), (2, float("-inf"))]
    for fn in (acc, stp, wts):
        for loss, px in bad:
            with pytest.raises(ValueError, match="mvmc_rig_"):
                fn(loss, px)
    for call in (lambda: acc(1, 6.0, MAX_ITER + 1), lambda: acc(1, 6.0, 10, 2), lambda: stp(2, 6.0, -1)):
        with pytest.raises(ValueError, match="mvmc_rig_"):
            call()
    torch.cuda.synchronize()
    assert np.array_equal(info_d.cpu().numpy(), info) and not ctl_d.cpu().numpy().any() and not red.cpu().numpy().any()
    assert np.array_equal(cams_d.cpu().numpy(), cams) and np.array_equal(camt_d.cpu().numpy(), cams) and np.array_equal(X_d.cpu().numpy(), prob["X"])
    acc(0, float("nan"))                                               # without a loss loss_px is not read
    acc(2, 6.0, MAX_ITER)
    torch.cuda.synchronize()
    assert info_d.cpu().numpy()[0, 0] > 0 and red.cpu().numpy().any()


# ---- f. refine_rigs ----
@functools.lru_cache(maxsize=None)
def _tracked():
    """The smallest whole solve of tests/test_gpu_rig_refine.py: a 5 x 2 scene of 120 frames on a rig perturbed by 1 degree / 3 cm,
    tracked on the perturbed rig -> (generator dict, perturbed Rt, sequence row, records)."""
    from multiview_motion_capture_amd.sequences import track_sequences
    from test_gpu_rig_refine import _scene
    g, Rt, row = _scene(47, 5, 2, F=120)
    return g, Rt, row, track_sequences([row], chain_len=16)[0]


def _bits(r):
    return (np.array([c.Rt for c in r.calibs]).tobytes(), np.asarray(r.cost).tobytes(), tuple(r.trials), r.stop, r.rms_before, r.rms_after)


def test_refine_rigs_without_a_loss_is_untouched():
    """loss=None, spelled out with the other new arguments at their defaults, is bit-identical to a call without them, and fills none
    of the loss's fields; the new arguments are checked before any device work."""
    from multiview_motion_capture_amd.rig_refine import refine_rig, refine_rigs
    _, _, row, recs = _tracked()
    a = refine_rigs([row], [recs])[0]
    b = refine_rigs([row], [recs], loss=None, loss_px=6.0, ftol=None, xtol=None, return_weights=False)[0]
    assert _bits(a) == _bits(b) == _bits(refine_rig(recs, *row)) and len(a.trials) >= 2
    assert b.loss is None and b.loss_px is None and b.downweighted is None and b.weights is None
    for kw in (dict(loss="l1"), dict(loss="huber", loss_px=0.0), dict(loss="cauchy", loss_px=float("nan")), dict(loss="huber", ftol=-1.0),
               dict(xtol=float("inf"))):
        with pytest.raises(ValueError):
            refine_rigs([row], [recs], **kw)


@pytest.mark.parametrize("loss", rcs.LOSSES)
def test_refine_rigs_with_a_loss_against_the_restatement(loss):
    """A whole call with a loss against the restatement fed the same selection: the same problem, trial list and stop; centres within
    1e-6 m and rotations within 1e-6 rad (the gates of tests/test_gpu_rig_refine.py); the robust cost list, the plain rms before and
    after, the weights and the downweighted shares.  Four trials: on this clean scene the reweighted iteration is still far from any
    tolerance there, so the decisions are clear."""
    from multiview_motion_capture_amd.rig_refine import refine_rigs
    from test_gpu_rig_refine import rr_max_px
    g, Rt, row, recs = _tracked()
    pr = []
    out = refine_rigs([row], [recs], problems=pr, max_iter=4, loss=loss, return_weights=True)[0]
    K = np.asarray(g["K"], np.float64)
    exp = rb.refine(pr[0]["cand"], K, Rt, max_iter=4, max_px=rr_max_px(), loss=loss)
    assert out.n_points == exp["n_points"] and out.n_obs == exp["n_obs"] and np.array_equal(out.held, exp["held"])
    assert out.trials == exp["trials"] and out.stop == exp["stop"], (out.trials, exp["trials"], out.stop, exp["stop"])
    got = np.array([c.Rt for c in out.calibs])
    dc = np.linalg.norm(rr.centres(got) - rr.centres(exp["Rt"]), axis=1).max()
    dr = max(rr.rot_angle(got[c, :, :3] @ np.linalg.inv(exp["Rt"][c, :, :3])) for c in range(5))
    dE = _rel(out.cost, exp["cost"])
    dw = float(np.nanmax(np.abs(out.weights - exp["weights"])))
    print(f"\n{loss}: {out.n_points} points, centres {dc:.2e} m, rotations {dr:.2e} rad, cost {dE:.2e}, weights {dw:.2e}; trials {out.trials}, "
          f"stop {out.stop}; rms {out.rms_before:.3f} -> {out.rms_after:.3f} px, downweighted {np.round(out.downweighted, 4)}")
    assert dc <= 1e-6 and dr <= 1e-6 and dE <= 1e-6 and dw <= 1e-6
    assert out.loss == loss and out.loss_px == 6.0 and out.weights.shape == (out.n_points, 5)
    assert abs(out.rms_before - exp["rms_before"]) <= 1e-6 * exp["rms_before"] and abs(out.rms_after - exp["rms_after"]) <= 1e-6 * exp["rms_after"]
    assert np.allclose(out.downweighted, exp["downweighted"], atol=2.0 / out.n_points)
    plain = refine_rigs([row], [recs], max_iter=4)[0]
    assert abs(out.rms_before - plain.rms_before) <= 1e-9 * plain.rms_before           # the plain rms of the same problem at the same start
    assert out.cost[0] < plain.cost[0]                                                 # ... while the cost is the robust E


# ---- g. calibrate_rigs ----
@functools.lru_cache(maxsize=None)
def _calibrated(name, loss):
    from multiview_motion_capture_amd.rig_init import calibrate_rig
    w, _ = ric.case(name)
    r = calibrate_rig(w["kps25"], w["counts"], [(w["K"][c], (1032, 776)) for c in range(5)], polish_loss=loss)
    ce, re = rr.rig_errors(np.array([c.Rt for c in r.calibs]), w["Rt"])
    return r, float(ce.max()), float(np.degrees(re.max()))


@pytest.mark.parametrize("loss", rcs.LOSSES)
@pytest.mark.parametrize("name", ["dirty_11", "dirty_12", "clean_11"])
def test_calibrate_rigs_with_a_loss_against_ground_truth(name, loss):
    """What the loss is for, on the device: on the contaminated walks the polish with a loss at 6 px ends with the worst camera's
    centre error at or below 0.75 x and its rotation error at or below 0.5 x those of the polish_loss=None call of the same test; on
    the clean walk it stays inside the clean gate of tests/test_rig_init_cpu.py.  It prints what it measures."""
    r0, ce0, re0 = _calibrated(name, None)
    r, ce, re = _calibrated(name, loss)
    assert r.stop == "ok" and r0.polish.loss is None and r.polish.loss == loss and r.polish.loss_px == 6.0
    print(f"\n{name} {loss}: centre {1e3 * ce0:.2f} -> {1e3 * ce:.2f} mm ({ce / ce0:.2f}), rotation {re0:.3f} -> {re:.3f} deg ({re / re0:.2f}); "
          f"trials {len(r0.polish.trials)} -> {len(r.polish.trials)}, stop {r.polish.stop}, rms {r0.rms_px:.2f} -> {r.rms_px:.2f} px, "
          f"downweighted {np.round(r.polish.downweighted, 3)}")
    if name.startswith("dirty"):
        assert ce <= CENTRE_RATIO * ce0 and re <= ROTATION_RATIO * re0
        assert r.rms_px >= r0.rms_px                                   # the plain rms: the least-squares polish minimises it
    else:
        assert ce <= RIG_GATE["clean"][0] and re <= RIG_GATE["clean"][1]
    assert len(r.polish.cost) == len(r.polish.trials) + 1 and r.polish.cost[0] < r0.polish.cost[0]
