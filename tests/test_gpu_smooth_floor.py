"""GPU: the floor under the trajectory smoother's foot contacts (smoothing.smooth_sequences(contacts=..., floor=...);
csrc/mvmc_smooth_row.h: sm_row_block<LOSS, CONTACT, FLOOR>, mvmc_smooth_blocks_floor; csrc/mvmc_smooth_contact.hip:
mvmc_smooth_floor_anchors) against its NumPy restatement (tests/smooth_floor_np.py) on test_gpu_smooth_small.py's 12 Shelf frames with
a tilted normal: the blocks launch per row, the floor-anchors launch on hand-built joints, the public path end to end (given labels,
"auto", a loss, the covariance), floor=None bit for bit, bit identity alone / in a batch of two normals / across partitions, and what
the floor buys on the CPU test's floor walks.  Tolerances against the restatement are tests/test_gpu_smooth_contact.py's."""
import numpy as np
import pytest

import smooth_contact_np as ct
import smooth_cov_np as sc
import smooth_floor_np as fl
import smooth_np as sm
import smooth_robust_np as rb
from test_body_fit_cpu import _cameras, _Rec
from test_gpu_smooth import _compare, _np_records, _same, _weights
from test_gpu_smooth_contact import CASES, LOSS_PX, _contact_same, _device_problem, _given, _unpack
from test_gpu_smooth_cov import TOL, _params
from test_gpu_smooth_small import _first, _shelf
from test_smooth_contact_cpu import EFFECT_SEEDS, WC
from test_smooth_floor_cpu import NORMAL, check_floor_effect, floor_figures

pytestmark = pytest.mark.gpu

WF = 10.0 * WC
OTHER = fl.unit([-0.2, 0.1, 1.0])


def _floor_same(a, b):
    _contact_same(a, b)
    for t, u in zip(a, b):
        assert np.array_equal(t.smooth_floor_normal, u.smooth_floor_normal, equal_nan=True)
        assert np.array_equal(t.smooth_floor_level, u.smooth_floor_level, equal_nan=True)


def _compare_floor(got, exp, wc, wf, what):
    """test_gpu_smooth_contact._compare_contacts with the floor's outputs: labels and trials per round exactly, anchors and level at
    the joints' gate (1e-8 m), n . anchor = level, E_contact within what that gate allows at the larger of the two weights."""
    worst = dict(anchor=0.0, level=0.0, cost=0.0, plane=0.0)
    for t, e in zip(got, exp):
        assert np.array_equal(t.smooth_contact, e["contact"]), (what, t.track_id, t.smooth_contact.T, e["contact"].T)
        assert t.smooth_round_trials == e["round_trials"], (what, t.smooth_round_trials, e["round_trials"])
        assert sum(t.smooth_round_trials) == len(t.smooth_trials)
        A, on = t.smooth_contact_anchor, t.smooth_contact
        assert A.shape == (len(t), 2, 3) and np.array_equal(np.isnan(A[:, :, 0]), ~on)
        n = t.smooth_floor_normal
        assert n.shape == (3,) and np.abs(n - e["floor_normal"]).max() <= 1e-15 and isinstance(t.smooth_floor_level, float)
        if on.any():
            worst["anchor"] = max(worst["anchor"], float(np.abs(A[on] - e["anchor"][on]).max()))
            worst["level"] = max(worst["level"], abs(t.smooth_floor_level - e["floor_level"]))
            worst["plane"] = max(worst["plane"], float(np.abs(A[on] @ n - t.smooth_floor_level).max()))
            J = np.array([q[2].keypoints for q in t.poses])[:, list(ct.FEET)]
            slack = max(wc, wf) * float(np.abs((J - A)[on]).sum()) * 2e-8
            for a, b in zip(t.smooth_contact_cost, e["contact_cost"]):
                assert abs(a - b) <= slack + 1e-9 * abs(b), (what, t.smooth_contact_cost, e["contact_cost"])
                worst["cost"] = max(worst["cost"], abs(a - b) / max(abs(b), 1e-300))
        else:
            assert np.all(t.smooth_contact_cost == 0.0) and np.isnan(t.smooth_floor_level) and np.isnan(e["floor_level"])
    print(f"{what}: floor outputs, worst differences from the restatement", worst)
    assert worst["anchor"] <= 1e-8 and worst["level"] <= 1e-8 and worst["plane"] <= 1e-12


@pytest.mark.parametrize("loss", [None, "cauchy"])
def test_the_floor_blocks_launch_per_row(loss):
    """test_gpu_smooth_contact's rows: 6 per identity, row 3 without data; labels per identity: row 0 left, row 1 right, row 2 both,
    row 3 (no data) left, rows 4 and 5 none; anchors 1 cm off the ankles.  Two rigs with the same cameras: identity 0 in rig 0 (the
    tilted normal), every other identity in rig 1 (a NaN normal).  Rows with a NaN normal or mask (0, 0) equal the contact launch
    bit for bit; the rows with the floor term are gated at 10 x the plain launch's worst relative deviation from the restatement."""
    import torch
    q = _device_problem()
    dev, T, d = q["dev"], q["T"], q["d"]
    x_h = np.concatenate(q["x0s"])
    N, n_id = x_h.shape[0], len(q["x0s"])
    x = T(x_h)
    mask = np.tile(np.array([[1, 0], [0, 1], [1, 1], [1, 0], [0, 0], [0, 0]], np.int32), (n_id, 1))
    J = np.array([ct._fk(p) for p in x_h])
    anc = J[:, list(ct.FEET)] + np.random.default_rng(2).choice([-0.01, 0.01], (N, 2, 3))
    anc[mask == 0] = np.nan
    m0 = int(q["m_of"][0])
    rig_h = np.ones(N, np.int32)
    rig_h[:m0] = 0
    rig = T(rig_h)
    Pm2 = torch.cat([q["Pm"], q["Pm"]]).contiguous()
    nrm = T(np.array([NORMAL, [np.nan] * 3]))
    ctl = torch.zeros((n_id, 4), dtype=torch.int32, device=d)
    ctl[:, 1] = 1                                             # -> buffer 0
    rob = dict(loss=loss, loss_px=LOSS_PX) if loss else {}
    ckw = dict(cmask=T(mask), anchors=T(anc), contact_weight=WC)
    blk_p, blk_c, blk_f = (torch.zeros((2, N, 820), dtype=torch.float64, device=d) for _ in range(3))
    dev.smooth_blocks(q["k17"], Pm2, rig, q["mem"], x, q["id_of"], ctl, blk_p, **rob)
    dev.smooth_blocks(q["k17"], Pm2, rig, q["mem"], x, q["id_of"], ctl, blk_c, **rob, **ckw)
    dev.smooth_blocks(q["k17"], Pm2, rig, q["mem"], x, q["id_of"], ctl, blk_f, **rob, **ckw, normals=nrm, floor_weight=WF)
    bp, bc, bf = blk_p[0].cpu().numpy(), blk_c[0].cpu().numpy(), blk_f[0].cpu().numpy()
    assert np.all(np.isfinite(bf)) and not np.any(blk_f[1].cpu().numpy())
    off = mask.sum(1) == 0
    assert n_id >= 2 and np.array_equal(bf[m0:], bc[m0:])                   # the NaN normal: the contact launch's blocks
    assert np.array_equal(bf[off], bc[off]) and np.array_equal(bf[off], bp[off])       # mask (0, 0): no term at all
    assert not np.array_equal(bf[:m0][~off[:m0]], bc[:m0][~off[:m0]])
    x0, (obs, prs) = q["x0s"][0], q["probs"][0]
    with rb.robust(loss, LOSS_PX):
        plain = sm.data_terms(x0, obs, prs)
        with fl.floor(mask[:m0] != 0, anc[:m0], WC, NORMAL, WF):
            flo = sm.data_terms(x0, obs, prs)
    base, worst = 0.0, 0.0
    for r in range(m0):
        for got, exp, is_floor in ((bp[r], plain, False), (bf[r], flo, True)):
            H, g, E = _unpack(got)
            He, ge, Ee = exp[2][r], exp[3][r], exp[1][r]
            if not np.any(He):
                assert not np.any(got)
                continue
            dev_ = max(np.abs(H - He).max() / np.abs(He).max(), np.abs(g - ge).max() / np.abs(ge).max(), abs(E - Ee) / abs(Ee))
            if is_floor and mask[r].any():
                worst = max(worst, dev_)
            elif not is_floor:
                base = max(base, dev_)
    assert np.any(flo[2][3]) and not np.any(plain[2][3]) and np.any(bf[3]) and not np.any(bp[3])   # no view: the term alone
    print(f"\nloss {loss}: worst relative deviation from the restatement, plain launch {base:.2e}, rows with the floor term {worst:.2e}")
    assert 0.0 < base and worst <= 10.0 * base


def test_the_floor_anchors_launch():
    """Hand-built joints, given labels.  Identity 0: 150 rows, runs of both feet across the 64-row chunks of the kernel's walk;
    identity 1: 5 rows, one run of one row; identity 2: 7 rows without a label; identity 3: 9 rows in the rig with a NaN normal;
    identity 4: 70 rows in a rig with another normal, the right foot alone.  Levels and anchors to 1e-12 of the restatement's;
    unlabelled rows stay NaN; identities 2 and 3 keep the contact launch's anchors bit for bit and get level NaN."""
    import torch

    from multiview_motion_capture_amd import device as dev
    d = torch.device("cuda:0")
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(d)
    rng = np.random.default_rng(8)
    m_of = np.array([150, 5, 7, 9, 70])
    lo = np.concatenate([[0], np.cumsum(m_of)])
    N = int(m_of.sum())
    Js = [rng.normal(0, 1.0, (m, 18, 3)) for m in m_of]
    masks = [np.zeros((m, 2), bool) for m in m_of]
    masks[0][3:70, 0] = True          # across the first chunk boundary
    masks[0][100:150, 0] = True       # across the second, to the last row
    masks[0][0:1, 1] = True           # a one-row run on the first row
    masks[0][60:131, 1] = True        # across both boundaries
    masks[1][2:3, 0] = True           # the identity's only label: one row
    masks[3][1:6, :] = True
    masks[4][10:69, 1] = True
    rigs = [0, 0, 0, 1, 2]
    normals = np.array([NORMAL, [np.nan] * 3, OTHER])
    joints, id_lo = T(np.concatenate(Js)), T(lo.astype(np.int32))
    cm = T(np.concatenate(masks).astype(np.int32))
    rig = T(np.repeat(np.array(rigs, np.int32), m_of))
    an = torch.zeros((N, 2, 3), dtype=torch.float64, device=d)
    ctl = torch.ones((len(Js), 4), dtype=torch.int32, device=d)
    dev.smooth_contact_anchors(joints, id_lo, cm, an, ctl, False, 0.0, 1)
    means = an.cpu().numpy()
    lev = torch.full((len(Js),), 7.0, dtype=torch.float64, device=d)      # every level is written
    dev.smooth_floor_anchors(joints, id_lo, rig, T(normals), cm, an, lev)
    got, lev_h = an.cpu().numpy(), lev.cpu().numpy()
    assert np.array_equal(cm.cpu().numpy() != 0, np.concatenate(masks))  # the labels are read only
    for s, (J, c) in enumerate(zip(Js, masks)):
        sl = slice(lo[s], lo[s + 1])
        assert np.array_equal(np.isnan(got[sl][:, :, 0]), ~c) and np.array_equal(np.isnan(got[sl]).any(-1), ~c)
        if s in (2, 3):
            assert np.isnan(lev_h[s]) and np.array_equal(got[sl], means[sl], equal_nan=True)
            continue
        A, h = fl.anchors(J, c, normals[rigs[s]])
        print(f"identity {s}: level {lev_h[s]:.6f}, differences from the restatement: level {abs(lev_h[s] - h):.1e}, anchors "
              f"{np.abs(got[sl][c] - A[c]).max():.1e}, n . a - h {np.abs(got[sl][c] @ normals[rigs[s]] - lev_h[s]).max():.1e}")
        assert abs(lev_h[s] - h) <= 1e-12 and np.abs(got[sl][c] - A[c]).max() <= 1e-12
        assert np.abs(got[sl][c] @ normals[rigs[s]] - lev_h[s]).max() <= 1e-12
    assert np.array_equal(ctl.cpu().numpy()[:, 0], [0, 0, 1, 0, 0])
    # an identity's numbers depend on nothing else in the launch: identity 0 alone
    an1 = torch.zeros((150, 2, 3), dtype=torch.float64, device=d)
    lev1 = torch.zeros((1,), dtype=torch.float64, device=d)
    ctl1 = torch.ones((1, 4), dtype=torch.int32, device=d)
    dev.smooth_contact_anchors(T(Js[0]), T(np.array([0, 150], np.int32)), T(masks[0].astype(np.int32)), an1, ctl1, False, 0.0, 1)
    dev.smooth_floor_anchors(T(Js[0]), T(np.array([0, 150], np.int32)), T(np.zeros(150, np.int32)), T(normals), T(masks[0].astype(np.int32)),
                             an1, lev1)
    assert np.array_equal(an1.cpu().numpy(), got[:150], equal_nan=True) and lev1.cpu().numpy()[0] == lev_h[0]


@pytest.mark.parametrize("contacts", ["given", "auto"])
@pytest.mark.parametrize("n,drop", CASES)
def test_device_equals_the_restatement_with_a_floor(n, drop, contacts):
    from multiview_motion_capture_amd.smoothing import smooth_tracklets
    si, kps, cnt, cal, fitted, views = _shelf()
    recs = _first(fitted, n, drop)
    kw = dict(contact_min_frames=2)
    lab = [_given(n) for _ in recs] if contacts == "given" else "auto"
    got = smooth_tracklets(recs, kps, cnt, cal, contacts=lab, floor=3.0 * NORMAL, floor_weight=WF, **kw)
    exp = fl.smooth([views], [si["P"]], [_np_records(recs)], _weights(), contacts=lab if contacts == "auto" else [lab],
                    floor_normals=[NORMAL], floor_weight=WF, contact_weight=WC, **kw)[0]
    for t in got:
        print(f"identity {t.track_id}: {len(t)} rows, E {np.array2string(t.smooth_cost, precision=3)}, E_contact "
              f"{np.array2string(t.smooth_contact_cost, precision=3)}, trials {t.smooth_round_trials}, labels {t.smooth_contact.sum(0)}, "
              f"level {t.smooth_floor_level:.4f}")
    what = f"floor, {contacts} labels, {n} rows" + ("" if drop is None else f", row {drop} without data")
    _compare(got, exp, what)
    _compare_floor(got, exp, WC, WF, what)
    assert any(t.smooth_contact.any() and t.smooth_round_trials[1] >= 1 for t in got)
    if contacts == "given":
        assert all(np.array_equal(t.smooth_contact, _given(n)) for t in got)


def test_device_equals_the_restatement_with_a_floor_a_loss_and_two_rounds():
    from multiview_motion_capture_amd.smoothing import smooth_tracklets
    si, kps, cnt, cal, fitted, views = _shelf()
    recs = _first(fitted, 11, 5)
    lab = [_given(11), None]                         # the second identity has no label: it is not solved again
    got = smooth_tracklets(recs, kps, cnt, cal, contacts=lab, loss="cauchy", contact_rounds=2, floor=NORMAL)     # floor_weight: wc
    with rb.robust("cauchy", LOSS_PX):
        exp = fl.smooth([views], [si["P"]], [_np_records(recs)], _weights(), contacts=[lab], floor_normals=[NORMAL], contact_weight=WC,
                        contact_rounds=2)[0]
        plain = sm.smooth([views], [si["P"]], [_np_records(recs)], _weights())[0]
    _compare(got, exp, "floor, cauchy, given labels, two rounds")
    _compare_floor(got, exp, WC, WC, "floor, cauchy, given labels, two rounds")
    assert len(got[0].smooth_round_trials) == 3 and got[1].smooth_round_trials[1:] == [0, 0] and not got[1].smooth_contact.any()
    assert np.isnan(got[1].smooth_floor_level) and np.array_equal(got[1].smooth_floor_normal, got[0].smooth_floor_normal)
    _compare(got[1:], plain[1:], "the identity without a label")


def test_floor_none_is_the_call_without_the_argument():
    from multiview_motion_capture_amd.smoothing import smooth_sequences, smooth_tracklets
    si, kps, cnt, cal, fitted, _ = _shelf()
    recs = _first(fitted, 11, 5)
    lab = [_given(11) for _ in recs]
    tm0, tm1 = {}, {}
    plain = smooth_tracklets(recs, kps, cnt, cal, contacts=lab, timings=tm0)
    none = smooth_tracklets(recs, kps, cnt, cal, contacts=lab, floor=None, floor_weight=None, timings=tm1)
    _same(plain, none)
    _contact_same(plain, none)
    assert set(tm0) == set(tm1)
    for t in plain + none:
        assert not hasattr(t, "smooth_floor_normal") and not hasattr(t, "smooth_floor_level")
    # a None entry: that sequence runs the contacts alone, beside one with a floor
    seq = (kps, cnt, cal)
    two = smooth_sequences([seq, seq], [recs, recs], contacts=[lab, lab], floor=[None, NORMAL], floor_weight=WF)
    _same(plain, two[0])
    _contact_same(plain, two[0])
    assert all(np.all(np.isnan(t.smooth_floor_normal)) and np.isnan(t.smooth_floor_level) for t in two[0])
    assert all(np.isfinite(t.smooth_floor_level) for t in two[1])
    allnone = smooth_sequences([seq], [recs], contacts=[lab], floor=[None])[0]
    _same(plain, allnone)
    _contact_same(plain, allnone)
    # fill_gaps=False and a one-frame record
    full = smooth_tracklets(recs, kps, cnt, cal, contacts=lab, floor=NORMAL)
    for t, u in zip(full, smooth_tracklets(recs, kps, cnt, cal, contacts=lab, floor=NORMAL, fill_gaps=False)):
        assert len(u) == 10 and np.array_equal(u.smooth_contact_anchor, t.smooth_contact_anchor[~t.smooth_filled], equal_nan=True)
        assert u.smooth_floor_level == t.smooth_floor_level
    one = smooth_tracklets(_first(fitted[:1], 1), kps, cnt, cal, contacts="auto", floor=NORMAL)[0]
    assert np.isnan(one.smooth_floor_level) and np.abs(one.smooth_floor_normal - NORMAL).max() <= 1e-15 and not one.smooth_contact.any()


def test_bit_identity_alone_in_a_batch_of_two_normals_and_across_partitions():
    from multiview_motion_capture_amd.smoothing import smooth_sequences, smooth_tracklets
    si, kps, cnt, cal, fitted, _ = _shelf()
    recs = _first(fitted, 11, 5)
    assert len(recs) >= 2
    seq = (kps, cnt, cal)
    for con in ("auto", [_given(11) for _ in recs]):
        per_seq = con if isinstance(con, str) else [con, con]
        kw = dict(contact_min_frames=2, floor_weight=WF)
        batch = smooth_sequences([seq, seq], [recs, recs], contacts=per_seq, floor=[NORMAL, OTHER], **kw)
        split = smooth_sequences([seq, seq], [recs, recs], contacts=per_seq, floor=[NORMAL, OTHER], max_work_bytes=12 * 48 * 1024, **kw)
        for s, n in enumerate((NORMAL, OTHER)):
            _same(batch[s], split[s])
            _floor_same(batch[s], split[s])
            whole = smooth_tracklets(recs, kps, cnt, cal, contacts=con, floor=n, **kw)
            _same(batch[s], whole)
            _floor_same(batch[s], whole)
            for k, t in enumerate(batch[s]):
                alone = smooth_tracklets([recs[k]], kps, cnt, cal, contacts=con if isinstance(con, str) else [con[k]], floor=n, **kw)
                assert np.array_equal(alone[0].smooth_select, t.smooth_select), "the selection of an identity alone differs: not this test's case"
                _same([t], alone)
                _floor_same([t], alone)
        assert any(t.smooth_contact.any() for t in batch[0])
        a, b = batch[0][0], batch[1][0]
        assert a.smooth_floor_level != b.smooth_floor_level and not np.array_equal(a.smooth_contact_anchor, b.smooth_contact_anchor)


def test_the_covariance_on_the_blocks_with_the_floor_term():
    """covariance="joints" with given labels and a floor on the 6-row problem with a row without data, against the restatement's
    DENSE inverse under the floor binding (the device's labels, anchors and normal) at the device's trajectory."""
    from multiview_motion_capture_amd.smoothing import smooth_tracklets
    si, kps, cnt, cal, fitted, views = _shelf()
    recs = _first(fitted, 6, 3)
    lab = [_given(6) for _ in recs]
    got = smooth_tracklets(recs, kps, cnt, cal, covariance="joints", contacts=lab, floor=NORMAL, floor_weight=WF)
    plain = smooth_tracklets(recs, kps, cnt, cal, contacts=lab, floor=NORMAL, floor_weight=WF)
    _same(got, plain)
    _floor_same(got, plain)
    probs = sc.problems(views, si["P"], _np_records(recs))
    for t, (obs, prs) in zip(got, probs):
        x = _params(t)
        assert t.smooth_cov_status == 0
        with fl.floor(t.smooth_contact, t.smooth_contact_anchor, WC, t.smooth_floor_normal, WF):
            e = sc.covariance(x, obs, prs, _weights(), blocks="dense")
        jc, pv = t.smooth_joint_cov, t.smooth_param_sigma ** 2
        d = dict(joint_cov=np.abs(jc - e["joint_cov"]).max() / np.abs(e["joint_cov"]).max(),
                 param_var=np.abs(pv - e["param_sigma"] ** 2).max() / np.abs(e["param_sigma"] ** 2).max(),
                 edof=abs(t.smooth_edof - e["edof"]) / e["edof"], noise_px=abs(t.smooth_noise_px - e["noise_px"]) / e["noise_px"])
        n = t.smooth_floor_normal
        along = float(np.sqrt(n @ jc[3, 3] @ n))
        print(f"\nidentity {t.track_id}: relative differences from the dense inverse " + ", ".join(f"{k} {v:.2e}" for k, v in d.items())
              + f"; left ankle on the filled row: sigma {1e3 * t.smooth_joint_sigma[3, 3]:.2f} mm, along the normal {1e3 * along:.2f} mm")
        assert t.smooth_nres == e["n_res"] and all(v <= TOL for v in d.values()), d


def _effect_run(views, Ps, rec, lab, floor):
    """test_smooth_floor_cpu.floor_scene through smooth_tracklets (test_gpu_smooth_contact._effect_run's way)."""
    from multiview_motion_capture_amd.common import Calib
    from multiview_motion_capture_amd.smoothing import smooth_tracklets
    kps = np.array([[v for v in row] for row in views])                    # (F, C, 1, 17, 3)
    K = np.array([[1000.0, 0, 500], [0, 1000.0, 400], [0, 0, 1.0]])
    assert np.array_equal(Ps, _cameras())
    cal = [Calib.from_k_rt(K, np.linalg.solve(K, P)) for P in Ps]
    r = _Rec(rec["frames"], rec["params"], rec["joints"])
    t = smooth_tracklets([r], kps, np.ones(kps.shape[:2], np.int32), cal, contacts=[lab], floor=floor)[0]
    return np.array([q[2].keypoints for q in t.poses])


def test_what_the_floor_buys_on_the_cpu_tests_scenes():
    """The gates of test_smooth_floor_cpu.test_what_the_floor_buys_on_floor_walks through smooth_tracklets, and its figures."""
    check_floor_effect({s: floor_figures(s, _effect_run) for s in EFFECT_SEEDS})
