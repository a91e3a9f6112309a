"""The intrinsic unknowns of the rig refinement on the device (csrc/mvmc_rigfit.hip: mvmc_rig_accumulate_intr, mvmc_rig_step_intr;
rig_refine.refine_rigs(intrinsics=...), rig_init.calibrate_rigs(polish_intrinsics=...)) against their NumPy restatement
(tests/rig_intr_np.py) on the small problems of tests/rig_intr_cases.py, against the entries without intrinsics, and against
synthetic ground truth.  tests/test_rig_intr_cpu.py proves on the restatement alone that every decision of a case is far from its
threshold."""
import functools

import numpy as np
import pytest
import torch

import rig_cases as rc
import rig_init_cases as ric
import rig_intr_cases as rci
import rig_intr_np as ri
import rig_refine_np as rr

pytestmark = pytest.mark.gpu

MAX_ITER = rc.MAX_ITER_CAP
TRIALS, COSTS = 8, 8 + MAX_ITER
STOP_XTOL, STOP_FTOL, STOP_FEW_CAMERAS, STOP_MAX_ITER = 1, 2, 3, 5
STOP_NAME = {STOP_XTOL: "xtol", STOP_FTOL: "ftol", STOP_MAX_ITER: "max_iter"}
CODE = {None: 0, "huber": 1, "cauchy": 2}
KEYS = ("X", "X_trial", "cams", "cams_trial", "info", "ctl", "red")


def device_solve(problems, Ks, Rts, max_iter, mu0, ftol, xtol, intrinsics, focal_sigma=None, centre_sigma_px=None, intrinsics_held=(),
                 loss=None, loss_px=6.0, steps=None, step=True, stop0=None, K0s=None):
    """One or several packed problems of equal C, each with its own K and rig, through the _intr entries, packed as refine_rigs packs
    them.  K0s: the centre of the prior (default: Ks, as in refine_rigs).  -> dict of NumPy arrays: X, X_trial, cams, cams_trial,
    cams_in, info, ctl, red, part2, islot, p_lo."""
    from multiview_motion_capture_amd import device as dev
    from multiview_motion_capture_amd import rig_refine as rg
    d = torch.device("cuda:0")
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(d)
    S, C = len(problems), problems[0]["uv"].shape[1]
    n_intr = ri.MODES[intrinsics]
    sf, sc = (np.inf if v is None else float(v) for v in (focal_sigma, centre_sigma_px))
    stop0 = np.zeros(S, np.int32) if stop0 is None else np.asarray(stop0, np.int32)
    run = stop0 == 0
    n_pts = np.array([p["X"].shape[0] if r else 0 for p, r in zip(problems, run)])
    tile, seq = rg.tile_tables(n_pts)
    held = np.array([p["held"] for p in problems])
    slot = np.where(held, -1, np.cumsum(~held, axis=1) - 1).astype(np.int32)
    islot = rg.intrinsic_slots(held, n_intr, intrinsics_held)
    Ks, Rts = np.asarray(Ks, np.float64), np.asarray(Rts, np.float64)
    K0s = Ks if K0s is None else np.asarray(K0s, np.float64)
    cams = np.concatenate([Ks.reshape(S, C, 9), Rts[:, :, :, :3].reshape(S, C, 9), Rts[:, :, :, 3]], axis=2)
    info = np.zeros((S, 64))
    info[:, TRIALS:TRIALS + MAX_ITER] = -1.0
    ctl = np.zeros((S, 4), np.int32)
    ctl[:, 0] = stop0
    X = np.concatenate([p["X"] for p, r in zip(problems, run) if r] + [np.zeros((0, 3))])
    uv = np.concatenate([p["uv"] for p, r in zip(problems, run) if r] + [np.zeros((0, C, 2))])
    X_d, uv_d, tile_d, seq_d, slot_d, cams_d, info_d, ctl_d = T(X), T(uv), T(tile), T(seq), T(slot), T(cams), T(info), T(ctl)
    islot_d, K0_d = T(islot), T(K0s[:, :, [0, 0, 1], [0, 2, 2]])
    Xt_d, camt_d = X_d.clone(), cams_d.clone()
    part, part2, red = dev.rig_work_intr(tile.shape[0], S, C, n_intr, d)
    part2.zero_()
    code = CODE[loss]
    for _ in range(max(int(max_iter), 1) if steps is None else steps):
        dev.rig_accumulate_intr(X_d, uv_d, tile_d, seq_d, slot_d, cams_d, camt_d, ctl_d, info_d, max_iter, mu0, part, red, n_intr, islot_d,
                                K0_d, sf, sc, 1, code, loss_px)
        if int(max_iter) and step:
            dev.rig_step_intr(X_d, Xt_d, uv_d, tile_d, seq_d, slot_d, cams_d, camt_d, ctl_d, info_d, red, max_iter, ftol, xtol, part2,
                              n_intr, islot_d, K0_d, sf, sc, code, loss_px)
    torch.cuda.synchronize()
    N = lambda t: t.cpu().numpy()
    return dict(X=N(X_d), X_trial=N(Xt_d), cams=N(cams_d), cams_trial=N(camt_d), cams_in=cams, info=N(info_d), ctl=N(ctl_d), red=N(red),
                part2=N(part2), islot=islot, p_lo=np.concatenate([[0], np.cumsum(n_pts)]))


def _rt(cams):
    return np.concatenate([cams[:, 9:18].reshape(-1, 3, 3), cams[:, 18:21, None]], axis=2)


def _k(cams):
    return cams[:, :9].reshape(-1, 3, 3)


def _rel(a, b):
    """max |a - b| relative to the largest entry of b."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def _unpack(out, s=0):
    n_t = int(out["ctl"][s, 1])
    return [int(v) for v in out["info"][s, TRIALS:TRIALS + n_t]], out["info"][s, COSTS:COSTS + n_t + 1].copy(), STOP_NAME.get(int(out["ctl"][s, 0]))


# ---- a. one trial ----
@pytest.mark.parametrize("name", list(rci.CASES))
def test_one_trial_against_the_restatement(name):
    """ONE trial of every case at its mu0 with the prior centred on the TRUE K (so that its gradient is not zero at the start): E
    including the prior, the reduced gradient, the reduced matrix entry for entry in the device's layout (identity past the
    sequence's own columns), the camera step including the intrinsic entries, the point steps, the predicted reduction, the trial
    cameras including the trial K, and the trial cost, each within 1e-10 of the restatement's relative to its largest entry.  Each
    is read before a second trial could hide it.  It prints what it measures."""
    c, p = rci.case(name), dict(rci.params(name))
    prob, K, Rt, K0 = c["prob"], c["K"], c["Rt"], c["K_true"]
    C, held = K.shape[0], prob["held"]
    if p["max_iter"] == 0:
        p["max_iter"] = 1
    NI, sf, sc = ri.check(p["intrinsics"], p["focal_sigma"], p["centre_sigma_px"], C)
    ifree = ri.free_intrinsics(held, NI, p["intrinsics_held"])
    t = ri.trial(prob["X"], prob["uv"], K, Rt[:, :, :3], Rt[:, :, 3], held, p["mu0"], ifree, NI, K0, sf, sc, p["loss"], p["loss_px"])
    M, m = 6 * (C - 1) + NI * C, t["terms"]["cam"].size
    out = device_solve([prob], [K], [Rt], steps=1, K0s=[K0], **p)
    r = out["red"][0]
    S, g, d = r[:M * M].reshape(M, M), r[M * M:M * M + M], r[M * M + M:]
    assert np.array_equal(S[m:, m:], np.eye(M - m)) and not S[:m, m:].any() and not S[m:, :m].any() and not g[m:].any() and not d[m:].any()
    e = dict(E=abs(out["info"][0, 0] - t["terms"]["E"]) / t["terms"]["E"], g=_rel(g[:m], t["terms"]["g"]), S=_rel(S[:m, :m], t["terms"]["S"]))
    assert out["ctl"][0, 3] == int(t["bad"])
    if not t["bad"]:
        Kt, Rtt = _k(out["cams_trial"][0]), _rt(out["cams_trial"][0])
        e.update(dc=_rel(d[:m], t["dc"]), dp=_rel(out["X_trial"] - prob["X"], t["dp"]), pred=abs(out["info"][0, 7] - t["pred"]) / abs(t["pred"]),
                 K=_rel(Kt, t["K"]), R=_rel(Rtt[:, :, :3], t["R"]), t=_rel(Rtt[:, :, 3], t["t"]),
                 Et=abs(out["part2"][:, 0].sum() + ri.prior(Kt, K0, ifree, NI, sf, sc) - t["Et"]) / t["Et"])
        acc = t["Et"] < t["terms"]["E"]
        assert out["info"][0, TRIALS] == float(acc)
        if acc:
            e["Et_info"] = abs(out["info"][0, 1] - t["Et"]) / t["Et"]
            assert np.array_equal(_k(out["cams"][0]), Kt)                     # the trial K is taken over
        assert np.array_equal(Kt[~ifree], K[~ifree])
    print(f"\n{name}: " + ", ".join(f"{k} {v:.1e}" for k, v in e.items()))
    assert max(e.values()) <= 1e-10, e
    assert out["ctl"][0, 1] == 1


# ---- b. whole solves ----
@pytest.mark.parametrize("name", list(rci.CASES))
def test_whole_solves_against_the_restatement(name):
    """The trial list, the stop reason and the number of trials equal the restatement's (its decisions are clear of their thresholds:
    test_rig_intr_cpu.py::test_case_margins); camera centres within 1e-6 m, rotations within 1e-6 rad, phi within 1e-9, the
    principal points within 1e-6 px, the final cost within 1e-10 relative."""
    c, p = rci.case(name), rci.params(name)
    exp, _ = rci.reference(name)
    out = device_solve([c["prob"]], [c["K"]], [c["Rt"]], **p)
    trials, cost, stop = _unpack(out)
    assert trials == exp["trials"], (trials, exp["trials"])
    assert stop == exp["stop"], (stop, exp["stop"])
    assert out["ctl"][0, 1] == len(exp["trials"]) and out["ctl"][0, 2] == sum(exp["trials"])
    got, Kg = _rt(out["cams"][0]), _k(out["cams"][0])
    dc = np.linalg.norm(rr.centres(got) - rr.centres(exp["Rt"]), axis=1).max()
    dr = max(rr.rot_angle(got[k, :, :3] @ np.linalg.inv(exp["Rt"][k, :, :3])) for k in range(got.shape[0]))
    dk = np.abs(ri.deltas(Kg, c["K"]) - ri.deltas(exp["K"], c["K"]))
    dE = abs(cost[-1] - exp["cost"][-1]) / exp["cost"][-1] if len(cost) else 0.0
    print(f"\n{name}: centres {dc:.2e} m, rotations {dr:.2e} rad, phi {dk[:, 0].max():.2e}, principal point {dk[:, 1:].max():.2e} px, "
          f"final cost {dE:.2e} relative; trials {trials}, stop {stop}")
    assert dc <= 1e-6 and dr <= 1e-6 and dk[:, 0].max() <= 1e-9 and dk[:, 1:].max() <= 1e-6 and dE <= 1e-10
    assert len(cost) == len(exp["cost"]) and out["info"][0, 0] == cost[0] and out["info"][0, 1] == cost[-1]
    held, ifree = c["prob"]["held"], exp["ifree"]
    assert np.array_equal(out["cams"][0, held, 9:], out["cams_in"][0, held, 9:])            # a held pose is not moved
    assert np.array_equal(out["cams"][0, ~ifree, :9], out["cams_in"][0, ~ifree, :9])        # a held K neither
    assert np.array_equal(Kg[:, 2], c["K"][:, 2]) and np.array_equal(Kg[:, 1, 0], c["K"][:, 1, 0])
    if p["intrinsics"] == "focal":
        assert np.array_equal(Kg[:, :2, 2], c["K"][:, :2, 2])


# ---- c. several sequences in one launch ----
def test_several_sequences_in_one_launch():
    """Five 5-camera sequences in one launch -- rejected-then-accepted trials, one stopped at entry, a tile of one point, a solve that
    stops early on xtol and one with a camera between the others whose K is another problem's -- in both modes: cameras, points,
    costs, trials and control words of every sequence are bit-identical alone, together and in a second run."""
    names = ["reject", "stopped", "f_c5_65", "xtol", "tight"]
    cs = [rci.case({"stopped": "f_c5_65"}.get(n, n)) for n in names]
    stop0 = [STOP_FEW_CAMERAS if n == "stopped" else 0 for n in names]
    for mode in (dict(intrinsics="focal", focal_sigma=0.05), dict(intrinsics="focal+centre", focal_sigma=0.05, centre_sigma_px=10.0)):
        kw = dict(mode, max_iter=6, mu0=1e-4, ftol=1e-12, xtol=rci.params("xtol")["xtol"])
        a, b = [device_solve([c["prob"] for c in cs], [c["K"] for c in cs], [c["Rt"] for c in cs], stop0=stop0, **kw) for _ in range(2)]
        for k in KEYS:
            assert np.array_equal(a[k], b[k], equal_nan=True), k
        print("\n", mode["intrinsics"], [(n, _unpack(a, s)[0], int(a["ctl"][s, 0])) for s, n in enumerate(names)])
        for s, n in enumerate(names):
            if n == "stopped":
                assert a["ctl"][s].tolist() == [STOP_FEW_CAMERAS, 0, 0, 0] and np.array_equal(a["cams"][s], a["cams_in"][s])
                continue
            one = device_solve([cs[s]["prob"]], [cs[s]["K"]], [cs[s]["Rt"]], **kw)
            lo, hi = a["p_lo"][s], a["p_lo"][s + 1]
            assert np.array_equal(one["cams"][0], a["cams"][s]) and np.array_equal(one["X"], a["X"][lo:hi]), n
            assert np.array_equal(one["info"][0], a["info"][s]) and np.array_equal(one["ctl"][0], a["ctl"][s]), n
            assert np.array_equal(one["red"][0], a["red"][s]), n
            assert a["ctl"][s, 1] >= 2
        s = names.index("xtol")
        assert a["ctl"][s, 0] == STOP_XTOL and a["ctl"][s, 1] < 6


# ---- c2. the entries without intrinsics are the case without intrinsic columns ----
@pytest.mark.parametrize("n_intr", [1, 3])
@pytest.mark.parametrize("name", ["c2", "c4_held_mid", "c8"])
def test_pose_only_is_the_case_without_intrinsic_columns(name, n_intr):
    """tests/rig_cases.py's problems through the _intr entries with every islot = -1 (K0 the input K, finite sigmas, no loss) against
    mvmc_rig_accumulate / mvmc_rig_step with the case's own parameters, after one trial and after the whole solve: X, cams, cams_trial,
    ctl, info and part2 bit-identical; the leading 6 n_free rows and columns of S and entries of g and d bit-identical; the rest of red
    exactly the identity, with zeros in g and d."""
    from test_gpu_rig_kernels import device_solve as plain_solve
    c, p = rc.case(name), rc.params(name)
    prob, K, Rt = c["prob"], c["K"], c["Rt"]
    C = K.shape[0]
    mode = {1: dict(intrinsics="focal", focal_sigma=0.05), 3: dict(intrinsics="focal+centre", focal_sigma=0.05, centre_sigma_px=10.0)}[n_intr]
    M0, M, m = 6 * (C - 1), 6 * (C - 1) + n_intr * C, 6 * int((~prob["held"]).sum())
    for steps in (1, None):
        a = plain_solve([prob], K, [Rt], steps=steps, **p)
        b = device_solve([prob], [K], [Rt], steps=steps, intrinsics_held=tuple(range(C)), **mode, **p)
        assert (b["islot"] == -1).all()
        for k in ("X", "cams", "cams_trial", "ctl", "info", "part2"):
            assert np.array_equal(a[k], b[k], equal_nan=True), (k, steps)
        ra, rb = a["red"][0], b["red"][0]
        Sa, ga, da = ra[:M0 * M0].reshape(M0, M0), ra[M0 * M0:M0 * M0 + M0], ra[M0 * M0 + M0:]
        Sb, gb, db = rb[:M * M].reshape(M, M), rb[M * M:M * M + M], rb[M * M + M:]
        assert np.array_equal(Sa[:m, :m], Sb[:m, :m]) and np.array_equal(ga[:m], gb[:m]) and np.array_equal(da[:m], db[:m]), steps
        assert np.array_equal(Sb[m:, m:], np.eye(M - m)) and not Sb[:m, m:].any() and not Sb[m:, :m].any(), steps
        assert not gb[m:].any() and not db[m:].any(), steps
        assert a["ctl"][0, 1] >= 1


# ---- d. the argument checks ----
def test_argument_checks_launch_nothing():
    """n_intr outside {1, 3}, a sigma that is <= 0 or NaN and variant 0 (refused on these entries: the stacked product runs on the
    matrix cores) are MVMC_ERR_ARG on both entries, and nothing is launched or written."""
    from multiview_motion_capture_amd import device as dev
    from multiview_motion_capture_amd import rig_refine as rg
    d = torch.device("cuda:0")
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(d)
    c = rci.case("f_c3")
    prob, K, Rt = c["prob"], c["K"], c["Rt"]
    C = 3
    tile, seq = rg.tile_tables([prob["X"].shape[0]])
    slot, islot = np.array([[-1, 0, 1]], np.int32), np.array([[0, 1, 2]], np.int32)
    cams = np.concatenate([K.reshape(1, C, 9), Rt[:, :, :3].reshape(1, C, 9), Rt[:, :, 3][None]], axis=2)
    info = np.zeros((1, 64))
    info[:, TRIALS:TRIALS + MAX_ITER] = -1.0
    X_d, Xt_d, uv_d, cams_d, camt_d = T(prob["X"]), T(prob["X"]), T(prob["uv"]), T(cams), T(cams)
    info_d, ctl_d, K0_d = T(info), torch.zeros((1, 4), dtype=torch.int32, device=d), T(K[None, :, [0, 0, 1], [0, 2, 2]])
    part, part2, red = dev.rig_work_intr(tile.shape[0], 1, C, 3, d)        # (the widest: every n_intr below fits)
    part1, _, red1 = dev.rig_work_intr(tile.shape[0], 1, C, 1, d)
    rd, pt = lambda n: red1 if n == 1 else red, lambda n: part1 if n == 1 else part
    acc = lambda n, sf, sc, variant=1, max_iter=10: dev.rig_accumulate_intr(X_d, uv_d, T(tile), T(seq), T(slot), cams_d, camt_d, ctl_d, info_d,
                                                                            max_iter, 1e-3, pt(n), rd(n), n, T(islot), K0_d, sf, sc, variant)
    stp = lambda n, sf, sc, max_iter=10: dev.rig_step_intr(X_d, Xt_d, uv_d, T(tile), T(seq), T(slot), cams_d, camt_d, ctl_d, info_d, rd(n),
                                                           max_iter, 1e-6, 1e-10, part2, n, T(islot), K0_d, sf, sc)
    inf, nan = float("inf"), float("nan")
    bad = [(0, inf, inf), (2, inf, inf), (4, inf, inf), (1, 0.0, inf), (1, -0.05, inf), (1, nan, inf), (3, 0.05, 0.0), (3, 0.05, -1.0),
           (3, 0.05, nan), (3, -inf, 10.0)]
    for fn in (acc, stp):
        for n, sf, sc in bad:
            with pytest.raises(ValueError, match="mvmc_rig_"):
                fn(n, sf, sc)
    for call in (lambda: acc(1, inf, inf, 0), lambda: acc(3, inf, 10.0, 0), lambda: acc(1, inf, inf, 1, MAX_ITER + 1), lambda: stp(3, inf, 10.0, -1)):
        with pytest.raises(ValueError, match="mvmc_rig_"):
            call()
    assert dev._cabi.load().mvmc_rig_part_doubles_intr(C, 2) == -1 and dev._cabi.load().mvmc_rig_red_doubles_intr(9, 1) == -1
    torch.cuda.synchronize()
    assert np.array_equal(info_d.cpu().numpy(), info) and not ctl_d.cpu().numpy().any() and not red.cpu().numpy().any()
    assert not red1.cpu().numpy().any()
    assert np.array_equal(cams_d.cpu().numpy(), cams) and np.array_equal(camt_d.cpu().numpy(), cams) and np.array_equal(X_d.cpu().numpy(), prob["X"])
    acc(1, inf, inf)                                                       # +inf is no term, not an error
    torch.cuda.synchronize()
    assert info_d.cpu().numpy()[0, 0] > 0 and red1.cpu().numpy().any()


def test_the_two_refusals_before_any_device_work():
    """"focal+centre" without a finite centre_sigma_px, and intrinsics on a two-camera sequence without a finite focal_sigma, raise
    ValueError before anything is read from the sequences; so do the malformed arguments."""
    from multiview_motion_capture_amd.common import Calib
    from multiview_motion_capture_amd.rig_init import calibrate_rigs
    from multiview_motion_capture_amd.rig_refine import refine_rigs
    K, Rt = rc.ring_rig(3)
    cal = [Calib.from_k_rt(K[c], Rt[c]) for c in range(3)]
    row3 = (np.zeros((2, 3, 1, 25, 3), np.float32), np.zeros((2, 3), np.int32), cal)
    row2 = (np.zeros((2, 2, 1, 25, 3), np.float32), np.zeros((2, 2), np.int32), cal[:2])
    for row, kw in ((row3, dict(intrinsics="focal+centre")), (row3, dict(intrinsics="focal+centre", centre_sigma_px=float("inf"))),
                    (row2, dict(intrinsics="focal")), (row2, dict(intrinsics="focal+centre", centre_sigma_px=10.0)),
                    (row3, dict(intrinsics="zoom")), (row3, dict(intrinsics="focal", focal_sigma=0.0)),
                    (row3, dict(intrinsics="focal", focal_sigma=float("nan"))), (row3, dict(intrinsics="focal", intrinsics_held=(3,)))):
        with pytest.raises(ValueError, match="refine_rigs"):
            refine_rigs([row], [[]], **kw)
    assert refine_rigs([row2], [[]], intrinsics="focal", focal_sigma=0.05)[0].stop == "few_cameras"
    for kw in (dict(polish_intrinsics="focal+centre"), dict(polish_intrinsics="f"), dict(polish_intrinsics="focal", polish_focal_sigma=-1.0)):
        with pytest.raises(ValueError, match="calibrate_rigs"):
            calibrate_rigs([(row3[0], row3[1], [(K[c], (1280, 720)) for c in range(3)])], **kw)


# ---- e. refine_rigs ----
@functools.lru_cache(maxsize=None)
def _tracked():
    """The smallest whole solve of tests/test_gpu_rig_refine.py: a 5 x 2 scene of 120 frames on a rig perturbed by 1 degree / 3 cm
    whose focal lengths are off by a seeded U(-3 %, +3 %), tracked on that rig -> (generator dict, input K, input Rt, row, records)."""
    from multiview_motion_capture_amd.sequences import track_sequences
    from test_gpu_rig_refine import _calibs, _scene
    g, Rt, _ = _scene(47, 5, 2, F=120)
    K = np.array(g["K"], np.float64)
    f = np.exp(np.random.default_rng(4747).uniform(-0.03, 0.03, 5))
    K[:, 0, 0] *= f
    K[:, 1, 1] *= f
    row = (g["kps25"], g["counts"], _calibs(K, Rt))
    return g, K, Rt, row, track_sequences([row], chain_len=16)[0]


def _bits(r):
    return (np.array([c.Rt for c in r.calibs]).tobytes(), np.array([c.K for c in r.calibs]).tobytes(), np.asarray(r.cost).tobytes(),
            tuple(r.trials), r.stop, r.rms_before, r.rms_after)


def test_refine_rigs_without_intrinsics_is_untouched():
    """intrinsics=None, spelled out with the other new arguments at their defaults, is bit-identical to a call without them and fills
    none of the new fields; "focal" with every camera in intrinsics_held solves the same problem through the _intr entries: Rt within
    1e-10 of the call without intrinsics."""
    from multiview_motion_capture_amd.rig_refine import refine_rig, refine_rigs
    _, K, _, row, recs = _tracked()
    a = refine_rigs([row], [recs])[0]
    b = refine_rigs([row], [recs], intrinsics=None, focal_sigma=None, centre_sigma_px=None, intrinsics_held=())[0]
    assert _bits(a) == _bits(b) == _bits(refine_rig(recs, *row)) and len(a.trials) >= 2
    assert b.intrinsics is None and b.K_before is None and b.K_after is None and b.k_moved is None and b.cost_prior is None
    h = refine_rigs([row], [recs], intrinsics="focal", intrinsics_held=(0, 1, 2, 3, 4))[0]
    dRt = np.abs(np.array([c.Rt for c in h.calibs]) - np.array([c.Rt for c in a.calibs])).max()
    print(f"\nall K held against intrinsics=None: Rt {dRt:.2e}, trials {h.trials} / {a.trials}")
    assert dRt <= 1e-10 and h.trials == a.trials and h.stop == a.stop
    assert np.array_equal(h.K_after, K) and not h.k_moved.any() and h.cost_prior == 0.0 and h.intrinsics == "focal"


def test_refine_rigs_focal_against_the_restatement_and_ground_truth():
    """A whole call with intrinsics="focal" through the real tracker against the restatement fed the same selection: the same
    problem, trial list and stop; centres, rotations, phi, cost and the plain rms within 1e-6.  Against ground truth: the worst focal
    error afterwards is at most 0.25 x the worst before.  Downstream: the MPJPE of a re-track on the refined calibs is below that of a
    re-track after the intrinsics=None refinement of the same input -- each after the similarity that aligns its rig's centres to the
    true ones, the measure of tests/test_gpu_rig_refine.py (the refinement fixes the world's frame and scale by the input rig: camera
    0's pose and its distance to the first free camera, 3 cm off here).  It prints what it measures."""
    from multiview_motion_capture_amd.rig_refine import refine_rigs
    from multiview_motion_capture_amd.sequences import track_sequences
    from test_gpu_rig_refine import _calibs, _mpjpe, rr_max_px
    g, K, Rt, row, recs = _tracked()
    pr = []
    out = refine_rigs([row], [recs], problems=pr, intrinsics="focal")[0]
    exp = ri.refine(pr[0]["cand"], K, Rt, max_px=rr_max_px(), intrinsics="focal")
    assert out.n_points == exp["n_points"] and out.n_obs == exp["n_obs"] and np.array_equal(out.held, exp["held"])
    assert out.trials == exp["trials"] and out.stop == exp["stop"], (out.trials, exp["trials"], out.stop, exp["stop"])
    got = np.array([c.Rt for c in out.calibs])
    dc = np.linalg.norm(rr.centres(got) - rr.centres(exp["Rt"]), axis=1).max()
    dr = max(rr.rot_angle(got[c, :, :3] @ np.linalg.inv(exp["Rt"][c, :, :3])) for c in range(5))
    dk = np.abs(out.k_moved - exp["k_moved"]).max()
    dE = _rel(out.cost, exp["cost"])
    Kt = np.asarray(g["K"], np.float64)
    fe0, fe1 = (np.abs(np.log(k[:, 0, 0] / Kt[:, 0, 0])).max() for k in (K, out.K_after))
    print(f"\nfocal: {out.n_points} points, centres {dc:.2e} m, rotations {dr:.2e} rad, k_moved {dk:.2e}, cost {dE:.2e}; trials {out.trials}, "
          f"stop {out.stop}; rms {out.rms_before:.3f} -> {out.rms_after:.3f} px; worst focal error {100 * fe0:.2f} % -> {100 * fe1:.2f} %")
    assert dc <= 1e-6 and dr <= 1e-6 and dk <= 1e-6 and dE <= 1e-6
    assert abs(out.rms_before - exp["rms_before"]) <= 1e-6 * exp["rms_before"] and abs(out.rms_after - exp["rms_after"]) <= 1e-6 * exp["rms_after"]
    assert np.array_equal(out.K_before, K) and np.array_equal(np.array([c.K for c in out.calibs]), out.K_after)
    assert abs(out.cost_prior) == 0.0 and out.intrinsics == "focal"
    assert fe1 <= 0.25 * fe0
    plain = refine_rigs([row], [recs])[0]
    m = {}
    Rt_true = np.asarray(g["Rt"], np.float64)
    for name, cal in (("intrinsics=None", plain.calibs), ("focal", out.calibs), ("true rig", _calibs(Kt, Rt_true))):
        sim = None if name == "true rig" else rr.similarity(rr.centres(np.array([c.Rt for c in cal])), rr.centres(Rt_true))
        m[name] = _mpjpe(track_sequences([(row[0], row[1], cal)], chain_len=16)[0], g, sim)
    print("MPJPE of a re-track (mm): " + ", ".join(f"{k} {1e3 * v:.2f}" for k, v in m.items()))
    assert m["focal"] < m["intrinsics=None"]


def test_batching_is_bit_identical():
    """A sequence refined alone, among others of another camera count and another K, and twice: bit-identical."""
    from multiview_motion_capture_amd.rig_refine import refine_rigs
    from multiview_motion_capture_amd.sequences import track_sequences
    from test_gpu_rig_refine import _scene
    _, _, _, row, recs = _tracked()
    _, _, row8 = _scene(23, 8, 2, F=40)
    recs8 = track_sequences([row8], chain_len=16)[0]
    kw = dict(intrinsics="focal+centre", focal_sigma=0.05, centre_sigma_px=10.0, max_iter=4, min_cam_obs=50)
    one = refine_rigs([row], [recs], **kw)[0]
    for _ in range(2):
        many = refine_rigs([row8, row, row], [recs8, recs, recs], **kw)
        assert _bits(many[1]) == _bits(one) == _bits(many[2]) and np.array_equal(many[1].k_moved, one.k_moved)
    assert len(one.trials) >= 2 and many[0].K_after.shape == (8, 3, 3) and many[0].stop != "few_cameras"


# ---- f. calibrate_rigs ----
def test_calibrate_rigs_polishes_the_focal_lengths():
    """One of tests/rig_init_cases.py's clean 5 x 120 walks given a K whose focal lengths are off by a seeded U(-3 %, +3 %):
    polish_intrinsics="focal" returns the same tree and stop as the plain polish on the same input, a lower rms_px, and a worst focal
    error of at most 0.5 x the input's.  It prints what it measures."""
    from multiview_motion_capture_amd.rig_init import calibrate_rig
    w, _ = ric.case("clean_11")
    K = np.array(w["K"], np.float64)
    f = np.exp(np.random.default_rng(1111).uniform(-0.03, 0.03, 5))
    K[:, 0, 0] *= f
    K[:, 1, 1] *= f
    cams = [(K[c], (1032, 776)) for c in range(5)]
    r0 = calibrate_rig(w["kps25"], w["counts"], cams)
    r1 = calibrate_rig(w["kps25"], w["counts"], cams, polish_intrinsics="focal")
    Kt = np.asarray(w["K"], np.float64)
    fe0, fe1 = (np.abs(np.log(k[:, 0, 0] / Kt[:, 0, 0])).max() for k in (K, np.array([c.K for c in r1.calibs])))
    print(f"\nclean_11, focal lengths off: rms {r0.rms_px:.2f} -> {r1.rms_px:.2f} px, worst focal error {100 * fe0:.2f} % -> {100 * fe1:.2f} %, "
          f"polish trials {len(r0.polish.trials)} / {len(r1.polish.trials)}, stop {r1.polish.stop}")
    assert r0.stop == r1.stop == "ok" and r0.tree == r1.tree
    assert r1.polish.intrinsics == "focal" and r0.polish.intrinsics is None
    assert np.array_equal(np.array([c.K for c in r0.calibs]), K)
    assert r1.rms_px < r0.rms_px and fe1 <= 0.5 * fe0
