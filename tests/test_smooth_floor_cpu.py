"""CPU: the floor under the trajectory smoother's foot contacts -- its NumPy restatement (tests/smooth_floor_np.py: gradient, levels
and projection, energy over the rounds, what the floor buys on walks whose footholds lie on one plane), the floor-bound planted walk
(synth.planted_walk(floor_normal=...)), smoothing.estimate_floor, and the argument checks of smoothing.smooth_sequences(floor=...)
(before any device call)."""
import functools

import numpy as np
import pytest

import oracle_np as o
import smooth_contact_np as ct
import smooth_floor_np as fl
import smooth_np as sm
import smooth_robust_np as rb
from test_body_fit_cpu import _cameras, _coco, _Rec
from test_smooth_contact_cpu import EFFECT_SEEDS, WC, _labels, mpjpe, skate
from test_smooth_cpu import W, _fk, _problem

NORMAL = fl.unit([0.1, -0.05, 1.0])
# Gate of the effect test: the planted ankles' height std with the floor <= R x the contacts-only std.  The geometric mean of 1 and
# the worst ratio measured with this restatement on the three scenes (test_what_the_floor_buys_on_floor_walks' docstring).
R_STD = 0.93
RATIO = 1.05                # conditions of the change, not measurements: the floor must not cost accuracy or skate


def test_gradient_with_the_floor_term_matches_central_differences():
    x0, filled, obs, prs = _problem()
    c = _labels(filled)
    J = np.array([_fk(p) for p in x0])
    wf = 10.0 * WC
    anc, h = fl.anchors(J, c, NORMAL)
    anc = anc + 0.01                        # off the plane and off the means: the gradient is not zero at x0
    with fl.floor(c, anc, WC, NORMAL, wf):
        Ed, Et, H, gd = sm.data_terms(x0, obs, prs)
        Ep, gp = sm.prior(x0[:, sm.COLS], W)[:2]
        g = gd + gp
        num = np.zeros_like(g)
        hh = 1e-6
        for r in range(x0.shape[0]):
            for q, col in enumerate(sm.COLS):
                xp, xm = x0.copy(), x0.copy()
                xp[r, col] += hh
                xm[r, col] -= hh
                num[r, q] = (sum(sm.energy(xp, obs, prs, W)) - sum(sm.energy(xm, obs, prs, W))) / (2 * hh)
    plain = sm.data_terms(x0, obs, prs)
    err = np.abs(num - g).max() / np.abs(g).max()
    print(f"\nrelative gradient error {err:.3e}; E_data + E_contact {Ed:.1f} against {plain[0]:.1f} plain")
    assert err < 1e-6
    assert sm.data_terms is rb._plain_data_terms                      # the binding is undone
    assert np.any(H[3] != 0) and np.array_equal(H[6], plain[2][6]) and Et[6] == plain[1][6]
    assert abs((Ed - plain[0]) - fl.floor_energy(J, c, anc, WC, NORMAL, wf)) <= 1e-9 * Ed
    # floor_weight = contact_weight is the contact term at the same anchors
    with ct.contact(c, anc, WC):
        con = sm.data_terms(x0, obs, prs)
    with fl.floor(c, anc, WC, NORMAL, WC):
        same = sm.data_terms(x0, obs, prs)
    assert np.abs(same[2] - con[2]).max() <= 1e-12 * np.abs(con[2]).max() and abs(same[0] - con[0]) <= 1e-12 * con[0]
    # the added Hessian is D^T (wc T + wf n n^T) D: along the normal wf acts, in the plane wc
    Wm = WC * np.eye(3) + (wf - WC) * np.outer(NORMAL, NORMAL)
    t = np.cross(NORMAL, [1.0, 0.0, 0.0])
    assert abs(NORMAL @ Wm @ NORMAL - wf) <= 1e-9 * wf and abs(t @ Wm @ t - WC * (t @ t)) <= 1e-9 * WC


def test_levels_and_projection_on_hand_built_joints():
    m = 10
    J = np.random.default_rng(3).normal(0, 1.0, (m, 18, 3))
    c = np.zeros((m, 2), bool)
    c[0:4, 0] = True
    c[6:7, 0] = True
    c[2:10, 1] = True
    A, h = fl.anchors(J, c, NORMAL)
    mean = ct.anchors(J, c)
    assert np.array_equal(np.isnan(A[:, :, 0]), ~c)
    # n . a == h to 4 ulp of the coordinates; the in-plane part is the run mean's
    T = np.eye(3) - np.outer(NORMAL, NORMAL)
    tol = 4 * np.finfo(float).eps * np.abs(mean[c]).max()
    assert np.abs(A[c] @ NORMAL - h).max() <= tol
    assert np.abs(A[c] @ T - mean[c] @ T).max() <= tol
    # h is the mean of n . X over the labelled pairs, both feet
    ank = J[:, list(ct.FEET)]
    assert abs(h - (ank[c] @ NORMAL).mean()) <= 4 * np.finfo(float).eps * np.abs(ank[c]).max()
    assert np.array_equal(fl.project(mean, c, NORMAL, h), A, equal_nan=True)
    # ... and minimises E_contact: 1 mm either way costs
    wf = 10.0 * WC
    E0 = fl.energy_at_level(J, c, NORMAL, h, WC, wf)
    for d in (1e-3, -1e-3):
        assert fl.energy_at_level(J, c, NORMAL, h + d, WC, wf) > E0
    # the two forms of E_contact agree: with the run means and a level, and with the anchors on the plane
    assert abs(fl.floor_energy(J, c, A, WC, NORMAL, wf) - E0) <= 1e-12 * E0
    # no label: NaN level, NaN anchors
    A0, h0 = fl.anchors(J, np.zeros((m, 2), bool), NORMAL)
    assert np.isnan(h0) and np.all(np.isnan(A0))


def floor_scene(seed, n_frames=24, stance=8, holes=(10, 11, 12), normal=NORMAL):
    """test_smooth_contact_cpu.effect_scene on the floor-bound walk: -> views, Ps, rec, true params (F,68), true labels (F,2)."""
    from multiview_motion_capture_amd import synth
    rng = np.random.default_rng(seed)
    Ps = _cameras()
    _, ref = o.skeleton_constants()
    root, ang, lab = synth.planted_walk(n_frames, 1, seed, stance=stance, side_lens=ref, start=np.array([0.0, 0.0, 1.0]), floor_normal=normal)
    p = np.concatenate([root[:, 0], ang[:, 0].reshape(n_frames, 54), np.tile(ref, (n_frames, 1))], axis=1)
    views = []
    for f in range(n_frames):
        J = _fk(p[f])
        row = []
        for c in range(4):
            k = _coco(J, Ps[c], [5, 6, 11, 12][c])
            k[:, :2] += rng.normal(0, 2.0, (17, 2))
            row.append(k[None])
        views.append(row)
    keep = [f for f in range(n_frames) if f not in holes]
    noisy = p.copy()
    noisy[:, :57] += rng.normal(0, 0.01, (n_frames, 57))
    rec = dict(frames=np.array(keep), params=noisy[keep], joints=np.array([_fk(q) for q in noisy[keep]]))
    return views, Ps, rec, p, lab[:, 0]


def heights(joints, labels, level, normal=NORMAL):
    """(std, rms about ``level``) of the planted ankles' heights along the normal, metres."""
    hgt = (np.asarray(joints)[:, list(ct.FEET)] @ normal)[labels]
    return float(hgt.std()), float(np.sqrt(np.mean((hgt - level) ** 2)))


def floor_figures(seed, run):
    """run(views, Ps, rec, labels, floor) -> joints (m,18,3) of the smoothed record; -> check_floor_effect's dict."""
    views, Ps, rec, p, lab = floor_scene(seed)
    J_true = np.array([_fk(q) for q in p])
    hs = (J_true[:, list(ct.FEET)] @ NORMAL)[lab]
    assert np.ptp(hs) <= 1e-9                                  # the true planted ankles lie on one plane
    f = {}
    for name, floor in (("contacts", None), ("floor", NORMAL)):
        J = run(views, Ps, rec, lab, floor)
        f["std_" + name], f["rms_" + name] = heights(J, lab, hs.mean())
        f["skate_" + name], f["mpjpe_" + name] = skate(J, lab), mpjpe(J, J_true)
    return f


def check_floor_effect(fig):
    for s in EFFECT_SEEDS:
        f = fig[s]
        print(f"\nseed {s}: planted-ankle height std contacts {1e3 * f['std_contacts']:.2f} mm, floor {1e3 * f['std_floor']:.2f} "
              f"({f['std_floor'] / f['std_contacts']:.2f} x); rms about the true level {1e3 * f['rms_contacts']:.2f} / "
              f"{1e3 * f['rms_floor']:.2f} mm; skate {1e3 * f['skate_contacts']:.2f} / {1e3 * f['skate_floor']:.2f} mm; MPJPE "
              f"{1e3 * f['mpjpe_contacts']:.2f} / {1e3 * f['mpjpe_floor']:.2f} mm")
    for s in EFFECT_SEEDS:
        f = fig[s]
        assert f["std_floor"] <= R_STD * f["std_contacts"], (s, f)
        assert f["mpjpe_floor"] <= RATIO * f["mpjpe_contacts"] and f["skate_floor"] <= RATIO * f["skate_contacts"], (s, f)


def _run_np(views, Ps, rec, lab, floor):
    return fl.smooth([views], [Ps], [[rec]], W, contacts=[[lab]], floor_normals=[floor], contact_weight=WC)[0][0]["joints"]


@functools.lru_cache(maxsize=None)
def restatement_floor_effect():
    return {s: floor_figures(s, _run_np) for s in EFFECT_SEEDS}


def test_what_the_floor_buys_on_floor_walks():
    """Scenes of seeds 5, 6, 7: test_smooth_contact_cpu.effect_scene (24 frames, stance 8, 4 cameras, 2 px noise, records without
    frames 10-12) on synth.planted_walk(floor_normal ~ (0.1, -0.05, 1)); default prior weights, 10 trials, the true labels, contact
    weight 1e6, floor weight = contact weight, the true normal, one round.  Gates: the std of the planted ankles' heights along the
    normal with the floor <= R_STD x the contacts-only std (the geometric mean of 1 and the worst measured ratio below); MPJPE and
    skate <= 1.05 x the contacts-only values.  Measured with this restatement (seeds 5 / 6 / 7), contacts only -> with the floor:
      height std (mm)        1.37 / 1.00 / 1.23 -> 0.91 / 0.87 / 0.98 (0.66 / 0.87 / 0.80 x)     -> R_STD = sqrt(0.870) = 0.93
      rms about truth (mm)   2.06 / 1.37 / 2.62 -> 1.79 / 1.27 / 2.52
      skate (mm)             1.69 / 1.44 / 2.21 -> 1.69 / 1.45 / 2.22
      MPJPE (mm)             8.55 / 12.11 / 9.43 -> 8.54 / 12.12 / 9.43
    At floor weight = contact weight the term is isotropic about anchors that share one level: what acts is the tie between the
    stances alone, and a 24-frame record has three of them.  Measured too, not gated: floor weight 10 x gives a height std of
    0.13 / 0.13 / 0.13 mm (0.09 / 0.13 / 0.10 x), rms 1.58 / 0.92 / 2.21, skate 1.18 / 1.18 / 1.90, MPJPE 8.54 / 12.12 / 9.44;
    100 x a std of 0.014 mm, rms 1.58 / 0.91 / 2.19, MPJPE 8.54 / 12.11 / 9.53: the heights lock, the level itself stays as good
    as the data makes it."""
    check_floor_effect(restatement_floor_effect())


def test_round_0_is_the_smoother_and_the_energy_never_increases_with_a_floor():
    views, Ps, rec, p, lab = floor_scene(6)
    plain = sm.smooth([views], [Ps], [[rec]], W)[0][0]
    res = fl.smooth([views], [Ps], [[rec]], W, contacts=[[lab]], floor_normals=[NORMAL], floor_weight=10.0 * WC, contact_weight=WC,
                    contact_rounds=3)[0][0]
    r0 = res["round0"]
    assert np.array_equal(r0["params"], plain["params"]) and np.array_equal(r0["cost"], plain["cost"]) and r0["trace"] == plain["trace"]
    h = np.array(res["history_contact"])
    print("\njoint energy over the rounds' trials:", h, "trials per round", res["round_trials"], "E_contact", res["contact_cost"],
          "level", res["floor_level"])
    assert len(res["round_trials"]) == 4 and res["round_trials"][0] == len(plain["trace"]) and res["round_trials"][1] >= 1
    assert np.all(np.diff(h) <= 0)                       # over the trials and across the rounds: anchors and level only lower it
    assert res["contact_cost"][1] < res["contact_cost"][0]
    on = res["contact"]
    assert np.abs(res["anchor"][on] @ NORMAL - res["floor_level"]).max() <= 4 * np.finfo(float).eps * np.abs(res["anchor"][on]).max()
    # a floor entry of None is the contacts-only result, exactly
    con = ct.smooth([views], [Ps], [[rec]], W, contacts=[[lab]], contact_weight=WC, contact_rounds=3)[0][0]
    none = fl.smooth([views], [Ps], [[rec]], W, contacts=[[lab]], floor_normals=[None], floor_weight=10.0 * WC, contact_weight=WC,
                     contact_rounds=3)[0][0]
    assert np.array_equal(none["params"], con["params"]) and none["trace"] == con["trace"] and np.isnan(none["floor_level"])
    assert np.array_equal(none["anchor"], con["anchor"], equal_nan=True) and np.array_equal(none["contact_cost"], con["contact_cost"])
    assert not np.array_equal(res["params"], con["params"])
    # no labelled row: the identity is not solved again
    off = fl.smooth([views], [Ps], [[rec]], W, contacts=[[np.zeros_like(lab)]], floor_normals=[NORMAL], contact_weight=WC)[0][0]
    assert np.array_equal(off["params"], plain["params"]) and off["round_trials"][1:] == [0] and np.isnan(off["floor_level"])


def test_planted_walk_on_a_floor():
    from multiview_motion_capture_amd import synth
    lens = np.broadcast_to(synth.skeleton_arrays()[1], (60, 3, 11))
    for seed, stance, normal in ((3, 8, NORMAL), (5, 5, fl.unit([0.0, 0.0, 1.0])), (6, 8, fl.unit([0.3, 0.2, 1.0]))):
        root, ang, lab = synth.planted_walk(60, 3, seed, stance=stance, floor_normal=3.0 * normal)       # (normalised inside)
        r0, a0, l0 = synth.planted_walk(60, 3, seed, stance=stance)
        assert np.array_equal(lab, l0) and np.array_equal(ang[:, :, 1:], a0[:, :, 1:]) and not np.array_equal(ang[:, :, 0], a0[:, :, 0])
        A = synth.batched_fk(root, ang, lens)[:, :, list(ct.FEET)]
        A0 = synth.batched_fk(r0, a0, lens)[:, :, list(ct.FEET)]
        d = np.linalg.norm(np.diff(A, axis=0), axis=-1)
        pair = lab[1:] & lab[:-1]
        hgt = [(A[:, p] @ normal)[lab[:, p]] for p in range(3)]
        plain = [(A0[:, p] @ normal)[lab[:, p]] for p in range(3)]
        print(f"\nseed {seed}, stance {stance}: anchors coplanar to {max(np.ptp(v) for v in hgt):.1e} m (the plain walk's differ by "
              f"{min(np.ptp(v) for v in plain):.2f} - {max(np.ptp(v) for v in plain):.2f} m), planted ankles move {d[pair].max():.1e} m")
        assert max(np.ptp(v) for v in hgt) <= 1e-12                    # every anchor of a person on one plane
        assert d[pair].max() <= 1e-12                                  # planted ankles stay
        assert lab.any(-1).all()                                       # a foot is down on every frame
        assert min(np.ptp(v) for v in plain) > 0.01
    # floor_normal=None is today's walk, bit for bit
    for a, b in zip(synth.planted_walk(30, 2, 4, floor_normal=None), synth.planted_walk(30, 2, 4)):
        assert np.array_equal(a, b)
    g0, g1 = synth.generate(20, 4, 2, 9, walk="planted"), synth.generate(20, 4, 2, 9, walk="planted", floor_normal=None)
    assert all(np.array_equal(g0[k], g1[k]) for k in g0)
    g = synth.generate(20, 4, 2, 9, walk="planted", floor_normal=NORMAL)
    for p in range(2):
        assert np.ptp((g["gt_joints"][:, p][:, list(ct.FEET)] @ NORMAL)[g["gt_contact"][:, p]]) <= 1e-12
    for bad in (np.zeros(3), np.array([0.0, np.nan, 1.0]), np.ones(2)):
        with pytest.raises(ValueError, match="floor_normal"):
            synth.planted_walk(10, 1, 0, floor_normal=bad)
    with pytest.raises(ValueError, match="floor_normal"):
        synth.generate(4, 4, 2, 9, walk="scene", floor_normal=NORMAL)


class _Smoothed(_Rec):
    def __init__(self, frames, params, joints, labels, tid=0):
        super().__init__(frames, params, joints, tid)
        self.smooth_contact = labels


def _truth_records(F=60, P=3, seed=5):
    from multiview_motion_capture_amd import synth
    root, ang, lab = synth.planted_walk(F, P, seed, floor_normal=NORMAL)
    lens = synth.skeleton_arrays()[1]
    J = synth.batched_fk(root, ang, np.broadcast_to(lens, (F, P, 11)))
    par = np.concatenate([root, ang.reshape(F, P, 54), np.broadcast_to(lens, (F, P, 11))], axis=-1)
    return [_Smoothed(list(range(F)), par[:, p], J[:, p], lab[:, p], tid=p) for p in range(P)], J, lab


def test_estimate_floor_on_ground_truth():
    from multiview_motion_capture_amd import smoothing
    recs, J, lab = _truth_records()
    est = smoothing.estimate_floor([recs])
    assert len(est) == 1
    e = est[0]
    ang = float(np.arctan2(np.linalg.norm(np.cross(e["normal"], NORMAL)), e["normal"] @ NORMAL))
    print(f"\nangle to the true normal {ang:.2e} rad, spread {e['spread']}, rms {e['rms']:.2e} m, levels {e['levels']}, runs {e['n_runs']}")
    assert e["status"] == 0 and ang <= 1e-9 and abs(np.linalg.norm(e["normal"]) - 1.0) <= 1e-15
    true_levels = np.array([(J[:, p][:, list(ct.FEET)] @ NORMAL)[lab[:, p]].mean() for p in range(3)])
    assert np.abs(e["levels"] - true_levels).max() <= 1e-9
    assert e["spread"].shape == (3,) and e["spread"][1] >= 0.05 and e["rms"] == e["spread"][0] <= 1e-6
    assert e["n_runs"] == sum(len(ct.runs(lab[:, p, f])) for p in range(3) for f in range(2))
    # the restatement's arithmetic on plain arrays
    r = fl.estimate([np.arange(60)] * 3, [J[:, p][:, list(ct.FEET)] for p in range(3)], [J[:, p, 0] for p in range(3)],
                    [lab[:, p] for p in range(3)])
    assert np.abs(r["normal"] - e["normal"]).max() <= 1e-12 and r["status"] == 0 and r["n_runs"] == e["n_runs"]
    assert np.abs(r["levels"] - e["levels"]).max() <= 1e-12
    # the orientation: the body is above its feet, whichever way the eigenvector came out
    flipped = smoothing.estimate_floor([recs[::-1]])[0]
    assert flipped["normal"] @ NORMAL > 0 and np.abs(flipped["levels"][::-1] - e["levels"]).max() <= 1e-9
    # one identity with two runs: the footholds span no plane
    one = _Smoothed(list(range(12)), np.zeros((12, 68)), J[:12, 0], lab[:12, 0])
    assert sum(len(ct.runs(lab[:12, 0, f])) for f in range(2)) == 2
    e1 = smoothing.estimate_floor([[one]])[0]
    assert e1["status"] == 1 and e1["n_runs"] == 2 and np.all(np.isfinite(e1["normal"]))
    # a huge min_spread refuses the good walk too; a hole in frame_idxs cuts a run
    assert smoothing.estimate_floor([recs], min_spread=10.0)[0]["status"] == 1
    keep = [f for f in range(60) if f != 4]
    cut = _Smoothed(keep, np.zeros((59, 68)), J[keep, 0], lab[keep, 0])
    assert smoothing.estimate_floor([[cut] + recs[1:]])[0]["n_runs"] == e["n_runs"] + 1
    # no label at all
    none = _Smoothed(list(range(12)), np.zeros((12, 68)), J[:12, 0], np.zeros((12, 2), bool))
    e2 = smoothing.estimate_floor([[none], []])
    assert e2[0]["status"] == 2 and np.all(np.isnan(e2[0]["normal"])) and np.isnan(e2[0]["levels"]).all() and e2[0]["n_runs"] == 0
    assert e2[1]["status"] == 2 and e2[1]["levels"].shape == (0,)
    with pytest.raises(ValueError, match="smooth_contact"):
        smoothing.estimate_floor([[_Rec([0, 1], np.zeros((2, 68)), J[:2, 0])]])
    with pytest.raises(ValueError, match="min_spread"):
        smoothing.estimate_floor([recs], min_spread=np.nan)


def test_the_entries_refuse_bad_floor_arguments_before_any_hip_call():
    """mvmc_smooth_blocks_floor and mvmc_smooth_floor_anchors with nothing to do (0 rows / 0 identities, no GPU needed)."""
    import ctypes as C

    from multiview_motion_capture_amd import _cabi, device as dev
    lib, sk = _cabi.load(), dev.make_skeleton()
    blocks = lambda loss, px, wc, wf: lib.mvmc_smooth_blocks_floor(C.byref(sk), None, 4, 2, None, None, None, None, None, None, 0, None,
                                                                   loss, px, None, None, wc, None, wf, None)
    for loss, px, wc, wf in ((0, 0.0, 0.0, 0.0), (0, 0.0, 1e6, 1e7), (2, 6.0, 1e300, 1e300)):
        assert blocks(loss, px, wc, wf) == _cabi.MVMC_OK
    for loss, px, wc, wf in ((0, 0.0, 1e6, -1.0), (0, 0.0, 1e6, float("nan")), (0, 0.0, 1e6, float("inf")), (0, 0.0, -1.0, 1e6),
                             (3, 6.0, 1e6, 1e6), (1, 0.0, 1e6, 1e6)):
        assert blocks(loss, px, wc, wf) == 1
    anchors = lambda n_ids, n: lib.mvmc_smooth_floor_anchors(None, None, n_ids, n, None, None, None, None, None, None)
    assert anchors(0, 0) == _cabi.MVMC_OK and anchors(-1, 0) == 1 and anchors(0, -1) == 1
    assert anchors(1, 1) == 1                       # rows to do and no buffers: refused before the launch
    assert {"mvmc_smooth_blocks_floor", "mvmc_smooth_floor_anchors"} <= set(_cabi.SYMBOLS)


def test_floor_argument_checks_run_before_any_device_call(monkeypatch):
    from multiview_motion_capture_amd import _cabi, device as dev, smoothing
    from multiview_motion_capture_amd.common import Calib

    def boom(*a, **k):
        raise AssertionError("device called")
    for name in ("ingest", "body_observe", "smooth_blocks", "smooth_step", "smooth_contact_anchors", "smooth_floor_anchors", "fk",
                 "uploader"):
        monkeypatch.setattr(dev, name, boom)
    monkeypatch.setattr(_cabi, "load", boom)
    cal = [Calib.from_k_rt(np.eye(3), np.concatenate([np.eye(3), np.zeros((3, 1))], 1)) for _ in range(4)]
    kps = np.zeros((5, 4, 2, 25, 3))
    cnt = np.zeros((5, 4), np.int32)
    _, ref = o.skeleton_constants()
    p = np.concatenate([np.zeros(57), ref])
    good = _Rec([0, 2], [p, p], np.zeros((2, 18, 3)))
    ok = np.zeros((3, 2), bool)
    up = np.array([0.0, 0.0, 2.0])
    bad = [dict(floor=up), dict(floor=up, contacts=None), dict(contacts="auto", floor_weight=1e6),
           dict(contacts="auto", floor=np.zeros(3)), dict(contacts="auto", floor=np.array([0.0, np.nan, 1.0])),
           dict(contacts="auto", floor=np.array([0.0, np.inf, 1.0])), dict(contacts="auto", floor=np.ones(2)),
           dict(contacts="auto", floor=np.ones((1, 3))), dict(contacts="auto", floor="up"), dict(contacts="auto", floor=1.0),
           dict(contacts="auto", floor=[0.0, 0.0, 0.0]), dict(contacts="auto", floor=[up, up]),
           dict(contacts=[ok], floor=up, floor_weight=-1.0), dict(contacts=[ok], floor=up, floor_weight=np.nan),
           dict(contacts=[ok], floor=up, floor_weight=np.inf), dict(contacts=[ok], floor=up, floor_weight="1e6"),
           dict(contacts=[ok], floor=up, floor_weight=True)]
    for kw in bad:
        with pytest.raises(ValueError, match="floor"):
            smoothing.smooth_tracklets([good], kps, cnt, cal, **kw)
    seqs, recs = [(kps, cnt, cal), (kps, cnt, cal)], [[good], [good]]
    for fl_arg in ([up], [up, up, up], [up, np.zeros(3)], [up, "x"], [None, np.ones(4)], (up, [1.0, 2.0])):
        with pytest.raises(ValueError, match="floor"):
            smoothing.smooth_sequences(seqs, recs, contacts="auto", floor=fl_arg)
    # good arguments reach the device: the first device call is the uploader's
    for kw in (dict(contacts="auto", floor=up), dict(contacts=[ok], floor=[0, 0, 1], floor_weight=0), dict(contacts=[ok], floor=(1, 2, 3),
                                                                                                      floor_weight=np.float32(1e7))):
        with pytest.raises(AssertionError, match="device called"):
            smoothing.smooth_tracklets([good], kps, cnt, cal, **kw)
    for fl_arg in (up, [up, None], [None, None], [[0, 0, 1], up]):
        with pytest.raises(AssertionError, match="device called"):
            smoothing.smooth_sequences(seqs, recs, contacts="auto", floor=fl_arg)
    assert smoothing.smooth_sequences([], [], contacts="auto", floor=up) == []
    n, wf = smoothing._check_floor([up, None], None, "auto", 3e5, 2)
    assert np.array_equal(n[0], [0.0, 0.0, 1.0]) and n[1] is None and wf == 3e5
    import inspect
    for fn in (smoothing.smooth_sequences, smoothing.smooth_tracklets):
        sig = inspect.signature(fn).parameters
        assert sig["floor"].default is None and sig["floor_weight"].default is None
    assert inspect.signature(smoothing.estimate_floor).parameters["min_spread"].default == 0.05
