"""CPU: the foot contacts of the trajectory smoother -- their NumPy restatement (tests/smooth_contact_np.py: gradient, detection and
anchors on hand-built joints, energy over the rounds, what they buy on walks with planted feet), the planted-walk ground truth
(synth.planted_walk) and the argument checks of smoothing.smooth_sequences(contacts=...) (before any device call)."""
import functools

import numpy as np
import pytest

import oracle_np as o
import smooth_contact_np as ct
import smooth_np as sm
import smooth_robust_np as rb
from test_body_fit_cpu import _cameras, _coco, _Rec
from test_smooth_cpu import W, _fk, _problem

WC = 1e6                    # smoothing.CONTACT_WEIGHT
EFFECT_SEEDS = (5, 6, 7)
# Gates of the effect test: skate with contacts <= R x today's smoother's.  Each is the geometric mean of 1 and the worst ratio
# measured with this restatement on the three scenes (test_what_contacts_buy_on_planted_walks' docstring has the figures).
R_TRUE, R_AUTO = 0.50, 0.73
MPJPE_RATIO = 1.05          # a condition of the change, not a measurement: contacts must not cost accuracy


def _labels(filled):
    """Labels for test_smooth_cpu._problem(): both feet on row 1, the left foot over the filled rows 3 and 4, the right foot at the end."""
    c = np.zeros((len(filled), 2), bool)
    c[0:2, 0] = True
    c[1:3, 1] = True
    c[3:6, 0] = True
    c[7:9, 1] = True
    assert c[1].all() and filled[3] and c[3, 0]
    return c


def test_gradient_with_the_contact_term_matches_central_differences():
    x0, filled, obs, prs = _problem()
    c = _labels(filled)
    J = np.array([_fk(p) for p in x0])
    anc = ct.anchors(J, c) + 0.01          # off the means: the term's gradient is not zero at x0
    with ct.contact(c, anc, WC):
        Ed, Et, H, gd = sm.data_terms(x0, obs, prs)
        Ep, gp = sm.prior(x0[:, sm.COLS], W)[:2]
        g = gd + gp
        num = np.zeros_like(g)
        h = 1e-6
        for r in range(x0.shape[0]):
            for q, col in enumerate(sm.COLS):
                xp, xm = x0.copy(), x0.copy()
                xp[r, col] += h
                xm[r, col] -= h
                num[r, q] = (sum(sm.energy(xp, obs, prs, W)) - sum(sm.energy(xm, obs, prs, W))) / (2 * h)
    plain = sm.data_terms(x0, obs, prs)
    err = np.abs(num - g).max() / np.abs(g).max()
    print(f"\nrelative gradient error {err:.3e}; E_data + E_contact {Ed:.1f} against {plain[0]:.1f} plain")
    assert err < 1e-6
    assert sm.data_terms is rb._plain_data_terms                      # the binding is undone
    assert np.any(H[3] != 0) and np.any(gd[3] != 0)                   # the filled row carries its contact term ...
    assert np.array_equal(H[6], plain[2][6]) and np.array_equal(gd[6], plain[3][6]) and Et[6] == plain[1][6]   # ... an unlabelled row nothing
    assert abs((Ed - plain[0]) - ct.contact_energy(J, c, anc, WC)) <= 1e-9 * Ed
    # it stacks on the robust binding: the contact part is the same, outside the loss
    with rb.robust("cauchy", 6.0):
        rob = sm.data_terms(x0, obs, prs)
        with ct.contact(c, anc, WC):
            both = sm.data_terms(x0, obs, prs)
    assert np.abs((both[2] - rob[2]) - (H - plain[2])).max() <= 1e-9 * np.abs(H).max()
    assert sm.data_terms is rb._plain_data_terms


def _still(m, seed=0):
    """Joints (m,18,3) whose two ankles the tests place by hand; the other joints are arbitrary."""
    return np.random.default_rng(seed).normal(0, 1.0, (m, 18, 3))


def test_detection_on_hand_built_joints():
    m = 12
    J = _still(m)
    # left ankle: moves 1/64 m per frame along x up to row 5 (speed exactly 1/64 on rows 0..4), stands on rows 5..9, moves on
    x = np.array([0, 1, 2, 3, 4, 5, 5, 5, 5, 5, 9, 13]) / 64.0
    J[:, 3] = np.stack([x, np.full(m, 0.25), np.full(m, 0.5)], -1)
    # right ankle: stands on rows 0..2 (a run touching the first row), jumps, stands on rows 9..11 (touching the last row), and stands
    # for two rows only in between (rows 5, 6)
    y = np.array([0, 0, 0, 8, 16, 24, 24, 32, 40, 48, 48, 48]) / 64.0
    J[:, 6] = np.stack([np.full(m, 1.0), y, np.full(m, 0.125)], -1)
    thr = 1.0 / 64.0
    c = ct.detect(J, thr, 3)
    # speeds of the left ankle: rows 0..4 exactly 1/64 (one-sided at row 0), row 5 1/128, rows 6..8 0: AT the threshold is no contact
    v = [abs(x[min(t + 1, m - 1)] - x[max(t - 1, 0)]) / (2.0 if 0 < t < m - 1 else 1.0) for t in range(m)]
    assert v[0] == thr and v[1] == thr and v[4] == thr and v[5] == thr / 2 and v[6] == 0.0
    assert c[:, 0].tolist() == [vt < thr for vt in v] == [False] * 5 + [True] * 4 + [False] * 3
    assert ct.detect(J, np.nextafter(thr, 1.0), 3)[0:5, 0].all()        # one ulp above: rows 0..4 are contacts
    # right ankle: rows 0, 1 stand (row 2's central difference sees the jump), so the run at the start has 2 rows -- dropped at min_run 3,
    # kept at 2; rows 5, 6 move by central differences; the run at the end is rows 10, 11
    sp = [abs(y[min(t + 1, m - 1)] - y[max(t - 1, 0)]) / (2.0 if 0 < t < m - 1 else 1.0) for t in range(m)]
    raw = [s < thr for s in sp]
    assert raw == [True, True] + [False] * 8 + [True, True]
    assert not c[:, 1].any()                                            # runs of min_run - 1 = 2 rows are dropped
    c2 = ct.detect(J, thr, 2)
    assert c2[:, 1].tolist() == raw and c2[0, 1] and c2[m - 1, 1]       # runs touching the first and the last row
    assert ct.runs(c2[:, 1]) == [(0, 2), (10, 12)]
    # the ground gate: the plane z = 0, height 0.25: the left ankle (z = 0.5) is out, the right one (z = 0.125) in; exactly AT the height is out
    g = (np.array([0.0, 0.0, 1.0]), 0.0)
    cg = ct.detect(J, thr, 2, g, 0.25)
    assert not cg[:, 0].any() and np.array_equal(cg[:, 1], c2[:, 1])
    assert not ct.detect(J, thr, 2, g, 0.125)[:, 1].any() and ct.detect(J, thr, 2, (g[0], -0.25), 0.5)[:, 1].any()
    assert not ct.detect(J[:1], thr, 1).any()                           # one row: no speed, no contact


def test_anchors_are_the_run_means_and_given_labels_pass_through():
    m = 10
    J = _still(m, 3)
    c = np.zeros((m, 2), bool)
    c[0:4, 0] = True
    c[6:7, 0] = True           # a given run of one row stays: min_run prunes detections only
    c[2:10, 1] = True
    A = ct.anchors(J, c)
    assert np.array_equal(np.isnan(A[:, :, 0]), ~c)
    for f, K in enumerate(ct.FEET):
        for a, b in ct.runs(c[:, f]):
            assert np.abs(A[a:b, f] - J[a:b, K].mean(0)).max() <= 4 * np.finfo(float).eps * np.abs(J[a:b, K]).max()
            assert np.all(A[a:b, f] == A[a, f])
    # the mean minimises E_contact over the anchor
    E0 = ct.contact_energy(J, c, A, WC)
    for d in (1e-3, -1e-3):
        assert ct.contact_energy(J, c, A + d, WC) > E0
    # given labels go through the rounds untouched
    x0, filled, obs, prs = _problem()
    lab = _labels(filled)
    x, info = ct.rounds(x0, obs, prs, W, lab, WC, n_rounds=1, max_iter=2)
    assert np.array_equal(info["contact"], lab) and np.array_equal(np.isnan(info["anchor"][:, :, 0]), ~lab)


def effect_scene(seed, n_frames=24, stance=8, holes=(10, 11, 12)):
    """A planted walk of one person in test_body_fit_cpu._cameras(): 2 px noise, records without the frames ``holes`` and with 0.01
    noise on root and angles (test_smooth_cpu._scene's) -> views, Ps, rec, true params (F,68), true labels (F,2)."""
    from multiview_motion_capture_amd import synth
    rng = np.random.default_rng(seed)
    Ps = _cameras()
    _, ref = o.skeleton_constants()
    root, ang, lab = synth.planted_walk(n_frames, 1, seed, stance=stance, side_lens=ref, start=np.array([0.0, 0.0, 1.0]))
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


def skate(joints, labels):
    """Mean ankle displacement per frame (m) over the pairs of consecutive rows on which ``labels`` (ground truth) has the foot down."""
    joints = np.asarray(joints)
    d = np.linalg.norm(np.diff(joints[:, list(ct.FEET)], axis=0), axis=-1)      # (m-1, 2)
    pair = labels[1:] & labels[:-1]
    return float(d[pair].mean())


def mpjpe(joints, J_true):
    return float(np.linalg.norm(np.asarray(joints) - J_true, axis=-1).mean())


def check_effect(fig):
    """fig[seed] = dict(skate0, skate_none, skate_true, skate_auto, mpjpe_none, mpjpe_true, mpjpe_auto, precision, recall)."""
    for s in EFFECT_SEEDS:
        f = fig[s]
        print(f"\nseed {s}: skate initial {1e3 * f['skate0']:.1f} mm, smoother {1e3 * f['skate_none']:.2f}, true labels "
              f"{1e3 * f['skate_true']:.2f} ({f['skate_true'] / f['skate_none']:.2f} x), auto {1e3 * f['skate_auto']:.2f} "
              f"({f['skate_auto'] / f['skate_none']:.2f} x); MPJPE {1e3 * f['mpjpe_none']:.2f} / {1e3 * f['mpjpe_true']:.2f} / "
              f"{1e3 * f['mpjpe_auto']:.2f} mm; detection precision {f['precision']:.2f} recall {f['recall']:.2f}")
    for s in EFFECT_SEEDS:
        f = fig[s]
        assert f["skate_true"] <= R_TRUE * f["skate_none"], (s, f)
        assert f["skate_auto"] <= R_AUTO * f["skate_none"], (s, f)
        assert f["mpjpe_true"] <= MPJPE_RATIO * f["mpjpe_none"] and f["mpjpe_auto"] <= MPJPE_RATIO * f["mpjpe_none"], (s, f)


def effect_figures(seed, run):
    """run(views, Ps, rec, contacts) -> (joints (m,18,3), labels (m,2) or None) of the smoothed record; -> check_effect's dict."""
    views, Ps, rec, p, lab = effect_scene(seed)
    J_true = np.array([_fk(q) for q in p])
    x0 = sm.init_traj(rec["frames"], rec["params"])[0]
    f = dict(skate0=skate([_fk(q) for q in x0], lab))
    for name, contacts in (("none", None), ("true", [[lab]]), ("auto", "auto")):
        J, c = run(views, Ps, rec, contacts)
        f["skate_" + name], f["mpjpe_" + name] = skate(J, lab), mpjpe(J, J_true)
        if name == "auto":
            f["precision"] = float((c & lab).sum() / max(c.sum(), 1))
            f["recall"] = float((c & lab).sum() / lab.sum())
    return f


def _run_np(views, Ps, rec, contacts):
    if contacts is None:
        return sm.smooth([views], [Ps], [[rec]], W)[0][0]["joints"], None
    res = ct.smooth([views], [Ps], [[rec]], W, contacts=contacts, contact_weight=WC)[0][0]
    return res["joints"], res["contact"]


@functools.lru_cache(maxsize=None)
def restatement_effect():
    return {s: effect_figures(s, _run_np) for s in EFFECT_SEEDS}


def test_what_contacts_buy_on_planted_walks():
    """Scenes of seeds 5, 6, 7: 24 frames of synth.planted_walk (stance 8), 4 cameras, 2 px noise, records without frames 10-12;
    default prior weights, 10 trials, contact weight 1e6, one round; skate = the mean ankle displacement per frame over the
    ground-truth contact pairs.  Gates: skate with the true labels <= R_TRUE x today's smoother's, with "auto" <= R_AUTO x (each the
    geometric mean of 1 and the worst measured ratio below), MPJPE <= 1.05 x today's.  Measured with this restatement (seeds 5 / 6 / 7):
      skate (mm)   initial 30.9 / 33.7 / 31.8   smoother 8.38 / 6.92 / 9.00   true labels 1.64 / 1.76 / 2.19 (0.20 / 0.25 / 0.24 x)
                   auto 2.63 / 3.74 / 3.86 (0.31 / 0.54 / 0.43 x)          -> R_TRUE = sqrt(0.254) = 0.50, R_AUTO = sqrt(0.541) = 0.73
      MPJPE (mm)   smoother 8.97 / 12.08 / 10.18   true labels 8.66 / 11.76 / 9.60   auto 8.74 / 11.88 / 9.77
      detection    precision 1.00 / 1.00 / 1.00, recall 0.81 / 0.77 / 0.73"""
    check_effect(restatement_effect())


def test_round_0_is_the_smoother_and_the_energy_never_increases():
    views, Ps, rec, p, lab = effect_scene(6)
    plain = sm.smooth([views], [Ps], [[rec]], W)[0][0]
    res = ct.smooth([views], [Ps], [[rec]], W, contacts=[[lab]], contact_weight=WC, contact_rounds=3)[0][0]
    r0 = res["round0"]
    assert np.array_equal(r0["params"], plain["params"]) and np.array_equal(r0["cost"], plain["cost"]) and r0["trace"] == plain["trace"]
    assert np.array_equal(res["cost"][:2], plain["cost"][:2])
    h = np.array(res["history_contact"])
    print("\njoint energy over the rounds' trials:", h, "trials per round", res["round_trials"], "E_contact", res["contact_cost"])
    assert len(res["round_trials"]) == 4 and res["round_trials"][0] == len(plain["trace"]) and res["round_trials"][1] >= 1
    assert sum(res["round_trials"]) == len(res["trace"]) and res["trace"][:len(plain["trace"])] == plain["trace"]
    assert np.all(np.diff(h) <= 0)                       # over the trials and across the rounds: the anchor step only lowers it
    assert res["contact_cost"][1] < res["contact_cost"][0]
    # labels without a contact: the identity is not solved again
    none = ct.smooth([views], [Ps], [[rec]], W, contacts=[[np.zeros_like(lab)]], contact_weight=WC)[0][0]
    assert np.array_equal(none["params"], plain["params"]) and none["trace"] == plain["trace"] and none["round_trials"][1:] == [0]
    assert np.array_equal(none["cost"], plain["cost"]) and not none["contact"].any() and np.all(none["contact_cost"] == 0)


def test_planted_walk_keeps_the_stance_ankle_where_it_is():
    from multiview_motion_capture_amd import synth
    for seed, stance, P in ((3, 8, 3), (4, 5, 1), (5, 2, 2)):
        root, ang, lab = synth.planted_walk(60, P, seed, stance=stance)
        assert root.shape == (60, P, 3) and ang.shape == (60, P, 18, 3) and lab.shape == (60, P, 2) and lab.dtype == bool
        J = synth.batched_fk(root, ang, np.broadcast_to(synth.skeleton_arrays()[1], (60, P, 11)))
        d = np.linalg.norm(np.diff(J[:, :, list(ct.FEET)], axis=0), axis=-1)
        pair = lab[1:] & lab[:-1]
        moving = d[~pair]
        print(f"\nseed {seed}, stance {stance}: planted ankles move {d[pair].max() if pair.any() else 0.0:.1e} m at most, the others "
              f"{moving.mean():.3f} m per frame on average")
        assert (d[pair].max() if pair.any() else 0.0) <= 1e-12
        assert lab.any(-1).all()                                       # a foot is down on every frame
        assert moving.mean() > 0.01
        both = lab.all(-1)
        assert both[stance::stance].all() and both.sum() == len(range(stance, 60, stance)) * P      # the double supports
        assert np.array_equal(ang, synth.scene_walk(60, P, seed)[1])
    g = synth.generate(20, 4, 2, 9, walk="planted")
    assert g["gt_contact"].shape == (20, 2, 2) and g["gt_contact"].any(-1).all()
    d = np.linalg.norm(np.diff(g["gt_joints"][:, :, list(ct.FEET)], axis=0), axis=-1)
    assert d[g["gt_contact"][1:] & g["gt_contact"][:-1]].max() <= 1e-12
    assert "gt_contact" not in synth.generate(4, 4, 2, 9, walk="scene") and "gt_contact" not in synth.generate(4, 4, 2, 9)
    with pytest.raises(ValueError):
        synth.planted_walk(10, 1, 0, stance=1)      # a change on every frame leaves no frame for the new anchor to hold


def test_the_entries_refuse_bad_contact_arguments_before_any_hip_call():
    """mvmc_smooth_blocks_contact and mvmc_smooth_contact_anchors with nothing to do (0 rows / 0 identities, no GPU needed)."""
    import ctypes as C

    from multiview_motion_capture_amd import _cabi, device as dev
    lib, sk = _cabi.load(), dev.make_skeleton()
    blocks = lambda loss, px, wc: lib.mvmc_smooth_blocks_contact(C.byref(sk), None, 4, 2, None, None, None, None, None, None, 0, None, loss,
                                                                 px, None, None, wc, None)
    for loss, px, wc in ((0, 0.0, 0.0), (0, 0.0, 1e6), (2, 6.0, 1e300)):
        assert blocks(loss, px, wc) == _cabi.MVMC_OK
    for loss, px, wc in ((0, 0.0, -1.0), (0, 0.0, float("nan")), (0, 0.0, float("inf")), (3, 6.0, 1e6), (1, 0.0, 1e6)):
        assert blocks(loss, px, wc) == 1
    anchors = lambda detect, speed, min_run, use_g, g, h: lib.mvmc_smooth_contact_anchors(None, None, 0, 0, detect, speed, min_run, use_g,
                                                                                          g, h, None, None, None, None)
    plane = (C.c_double * 4)(0.0, 0.0, 1.0, 0.0)
    assert anchors(0, float("nan"), 0, 0, None, 0.0) == _cabi.MVMC_OK and anchors(1, 0.01, 3, 1, plane, 0.15) == _cabi.MVMC_OK
    assert anchors(1, float("nan"), 3, 0, None, 0.0) == 1 and anchors(1, 0.01, 0, 0, None, 0.0) == 1 and anchors(1, 0.01, 3, 1, None, 0.1) == 1
    assert (_cabi.SMOOTH_FOOT_L, _cabi.SMOOTH_FOOT_R) == ct.FEET
    assert [int(o.IK_SKEL_IDX[k]) for k in range(16)].count(3) == 1 and [int(o.IK_SKEL_IDX[k]) for k in range(16)].count(6) == 1


def test_contact_argument_checks_run_before_any_device_call(monkeypatch):
    from multiview_motion_capture_amd import _cabi, device as dev, smoothing
    from multiview_motion_capture_amd.common import Calib

    def boom(*a, **k):
        raise AssertionError("device called")
    for name in ("ingest", "body_observe", "smooth_blocks", "smooth_step", "smooth_contact_anchors", "fk", "uploader"):
        monkeypatch.setattr(dev, name, boom)
    monkeypatch.setattr(_cabi, "load", boom)
    cal = [Calib.from_k_rt(np.eye(3), np.concatenate([np.eye(3), np.zeros((3, 1))], 1)) for _ in range(4)]
    kps = np.zeros((5, 4, 2, 25, 3))
    cnt = np.zeros((5, 4), np.int32)
    _, ref = o.skeleton_constants()
    p = np.concatenate([np.zeros(57), ref])
    good = _Rec([0, 2], [p, p], np.zeros((2, 18, 3)))        # rows 0..2: labels (3, 2)
    ok = np.zeros((3, 2), bool)
    plane = (np.array([0.0, 0.0, 1.0]), 0.0)
    bad = [dict(contacts="Auto"), dict(contacts=True), dict(contacts=1), dict(contacts=ok),
           dict(contacts=[ok, ok]), dict(contacts=[np.zeros((2, 2), bool)]), dict(contacts=[np.zeros((3, 2), np.int32)]),
           dict(contacts=[np.zeros((3,), bool)]), dict(contacts=["auto"]),
           dict(contacts="auto", contact_weight=-1.0), dict(contacts="auto", contact_weight=np.nan), dict(contacts="auto", contact_weight=np.inf),
           dict(contacts="auto", contact_weight="1e6"), dict(contacts="auto", contact_weight=True),
           dict(contacts="auto", contact_speed=np.nan), dict(contacts="auto", contact_speed=None),
           dict(contacts="auto", contact_min_frames=0), dict(contacts="auto", contact_min_frames=2.5),
           dict(contacts="auto", contact_rounds=0), dict(contacts="auto", contact_rounds=1.5), dict(contacts="auto", contact_rounds=True),
           dict(contacts="auto", contact_height=np.inf),
           dict(contacts="auto", ground=(np.zeros(2), 0.0)), dict(contacts="auto", ground=np.zeros(3)),
           dict(contacts="auto", ground=(np.array([0, 0, np.nan]), 0.0)), dict(contacts="auto", ground=(np.zeros(3), "0")),
           dict(contacts=[ok], ground=plane)]
    for kw in bad:
        with pytest.raises(ValueError, match="contact|ground"):
            smoothing.smooth_tracklets([good], kps, cnt, cal, **kw)
    with pytest.raises(ValueError, match="contacts"):
        smoothing.smooth_sequences([(kps, cnt, cal)], [[good]], contacts=[ok])               # per sequence a LIST of items
    with pytest.raises(ValueError, match="contacts"):
        smoothing.smooth_sequences([(kps, cnt, cal)], [[good]], contacts=[[ok], [ok]])
    # good arguments reach the device: the first device call is the uploader's
    for kw in (dict(contacts="auto"), dict(contacts=[ok]), dict(contacts=[None]), dict(contacts="auto", ground=plane, contact_rounds=2,
                                                                                      contact_weight=0, contact_speed=np.float32(0.02))):
        with pytest.raises(AssertionError, match="device called"):
            smoothing.smooth_tracklets([good], kps, cnt, cal, **kw)
    assert smoothing.smooth_sequences([], [], contacts="auto") == []
    assert (smoothing.CONTACT_WEIGHT, smoothing.CONTACT_MIN_FRAMES, smoothing.CONTACT_HEIGHT) == (WC, 3, 0.15)
    assert smoothing._FEET == ct.FEET
    # contacts=None sets no new attribute: the host's record builder is the one of a call without the argument
    import inspect
    sig = inspect.signature(smoothing.smooth_sequences).parameters
    assert sig["contacts"].default is None and sig["contact_rounds"].default == 1 and sig["ground"].default is None
    assert inspect.signature(smoothing.smooth_tracklets).parameters["contacts"].default is None
