"""GPU: the smoother's per-frame covariance (smoothing.smooth_sequences(covariance="joints"), csrc/mvmc_smooth_cov.hip) against the NumPy
restatement's dense inverse (tests/smooth_cov_np.py) at the row counts where a banded backward recursion goes wrong; nothing else
moves; bit identity of the new outputs; a singular factor; and the structure that theory fixes on synthetic scene walks with holes."""
import functools

import numpy as np
import pytest

import smooth_cov_np as sc
from test_gpu_body_fit import _raw_slot_maps
from test_gpu_smooth import _cut, _np_records, _person, _synth, _weights
from test_gpu_smooth_small import _first, _shelf

pytestmark = pytest.mark.gpu

# 10 x the worst banded-against-dense figure of tests/test_smooth_cov_cpu.py (9.1e-9: the margin because the device sums in another
# order); the bound may never be looser than 1e-6
TOL = 9.1e-8
assert TOL <= 1e-6

COV_FIELDS = ("smooth_joint_cov", "smooth_joint_sigma", "smooth_param_sigma", "smooth_noise_px", "smooth_edof", "smooth_nres",
              "smooth_cov_status")


def _params(t):
    return np.array([np.concatenate([q[1].root, np.ravel(q[1].euler_angles), q[1].bone_lens]) for q in t.poses])


@pytest.mark.parametrize("n,drop", [(2, None), (3, None), (4, None), (5, None), (6, None), (11, None), (6, 3), (11, 5)])
def test_device_equals_the_dense_inverse_on_few_rows(n, drop):
    """2 rows: no L2 at all; 3: the first Sigma_{t+2,t}; 4, 5, 6 and 11: the six block roles wrap once and twice; (6, drop 3) and
    (11, drop 5): a row with H_t = 0.  The restatement's DENSE inverse is built at the device's returned x."""
    from multiview_motion_capture_amd.smoothing import smooth_tracklets
    si, kps, cnt, cal, fitted, views = _shelf()
    recs = _first(fitted, n, drop)
    got = smooth_tracklets(recs, kps, cnt, cal, covariance="joints")
    probs = sc.problems(views, si["P"], _np_records(recs))
    assert len(got) == len(probs) >= 2
    for t, (obs, prs) in zip(got, probs):
        x = _params(t)
        assert x.shape == (n, 68) and t.smooth_cov_status == 0
        e = sc.covariance(x, obs, prs, _weights(), blocks="dense")
        jc, pv = t.smooth_joint_cov, t.smooth_param_sigma ** 2
        d = dict(joint_cov=np.abs(jc - e["joint_cov"]).max() / np.abs(e["joint_cov"]).max(),
                 param_var=np.abs(pv - e["param_sigma"] ** 2).max() / np.abs(e["param_sigma"] ** 2).max(),
                 edof=abs(t.smooth_edof - e["edof"]) / e["edof"], noise_px=abs(t.smooth_noise_px - e["noise_px"]) / e["noise_px"])
        print(f"\n{n} rows, drop {drop}, identity {t.track_id}: relative differences from the dense inverse "
              + ", ".join(f"{k} {v:.2e}" for k, v in d.items())
              + f"; edof {t.smooth_edof:.3f} of {39 * n}, n_res {t.smooth_nres}, noise {t.smooth_noise_px:.3f} px, "
              f"joint sigma {1e3 * t.smooth_joint_sigma.min():.2f} .. {1e3 * t.smooth_joint_sigma.max():.2f} mm")
        assert t.smooth_nres == e["n_res"]                                      # exact
        assert jc.shape == (n, 18, 3, 3) and np.array_equal(jc, jc.transpose(0, 1, 3, 2))
        assert t.smooth_joint_sigma.shape == (n, 18) and t.smooth_param_sigma.shape == (n, 39)
        assert all(v <= TOL for v in d.values()), d
        assert np.abs(t.smooth_joint_sigma - e["joint_sigma"]).max() <= TOL * e["joint_sigma"].max()
        assert 0.0 < t.smooth_edof < 39 * n
        if drop is not None:   # the row without data: e_t = 0 and n_t = 0 there (n_res and edof agree above), its sigma finite
            assert t.smooth_filled[drop] and e["e"][drop] == 0.0
            assert np.all(np.isfinite(t.smooth_joint_sigma[drop])) and np.all(t.smooth_joint_sigma[drop] > 0)


@functools.lru_cache(maxsize=None)
def _scene():
    """The synthetic scene walks of test_gpu_smooth._synth() (60 frames, rigs (5,4), (4,3), (5,2), occlusion 0.3), tracked, fitted,
    holes cut (test_gpu_smooth._synth_records' way), smoothed once with the covariance.  Nothing here is modified afterwards."""
    from multiview_motion_capture_amd.body_fit import fit_sequences
    from multiview_motion_capture_amd.sequences import track_sequences
    from multiview_motion_capture_amd.smoothing import smooth_sequences
    seqs, gts = _synth()
    fitted = fit_sequences(seqs, track_sequences(seqs, chain_len=16))
    rng = np.random.default_rng(5)
    cut = [_cut(r, rng) for r in fitted]
    return seqs, gts, fitted, cut, smooth_sequences(seqs, cut, covariance="joints")


def test_device_equals_the_dense_inverse_on_sixty_rows_with_a_hole():
    """A synthetic identity of about 60 rows with a 10-20-row hole: long enough that an error carried from row to row would show (the
    recursion without its symmetric step is off by 2.6e-4 of the largest entry after 60 rows, tests/test_smooth_cov_cpu.py)."""
    import smooth_np as sm
    seqs, gts, _, cut, out = _scene()
    s = 2
    k = max(range(len(cut[s])), key=lambda i: int(out[s][i].smooth_filled.sum()))
    t, g = out[s][k], gts[s]
    assert len(t) >= 50 and int(t.smooth_filled.sum()) >= 10 and t.smooth_cov_status == 0
    obs, prs = sc.problems(sm.bf.ingest_np(g["kps25"], g["counts"]), g["P"], _np_records(cut[s]))[k]
    e = sc.covariance(_params(t), obs, prs, _weights(), blocks="dense")
    d = dict(joint_cov=np.abs(t.smooth_joint_cov - e["joint_cov"]).max() / np.abs(e["joint_cov"]).max(),
             param_var=np.abs(t.smooth_param_sigma ** 2 - e["param_sigma"] ** 2).max() / np.abs(e["param_sigma"] ** 2).max(),
             edof=abs(t.smooth_edof - e["edof"]) / e["edof"], noise_px=abs(t.smooth_noise_px - e["noise_px"]) / e["noise_px"])
    print(f"\n{len(t)} rows, {int(t.smooth_filled.sum())} filled: relative differences from the dense inverse", d)
    assert t.smooth_nres == e["n_res"] and all(v <= TOL for v in d.values()), d


def _same_old_fields(a, b):
    assert len(a) == len(b)
    for t, u in zip(a, b):
        assert t.track_id == u.track_id and t.frame_idxs == u.frame_idxs and t.smooth_trials == u.smooth_trials
        assert np.array_equal(t.smooth_cost, u.smooth_cost) and np.array_equal(t.smooth_views, u.smooth_views)
        assert np.array_equal(t.smooth_select, u.smooth_select) and np.array_equal(t.smooth_filled, u.smooth_filled)
        for p, q in zip(t.poses, u.poses):
            assert p[0] == q[0] and np.array_equal(p[1].root, q[1].root) and np.array_equal(p[1].euler_angles, q[1].euler_angles)
            assert np.array_equal(p[1].bone_lens, q[1].bone_lens) and np.array_equal(p[2].keypoints, q[2].keypoints)


def test_nothing_else_moves():
    """poses, smooth_cost, smooth_trials, smooth_select and smooth_views with covariance="joints" are the bits of covariance=None,
    which sets none of the new attributes and times no "covariance" part."""
    from multiview_motion_capture_amd.smoothing import smooth_sequences, smooth_tracklets
    si, kps, cnt, cal, fitted, _ = _shelf()
    recs = _first(fitted, 11, 5)
    tm0, tm1 = {}, {}
    plain = smooth_tracklets(recs, kps, cnt, cal, timings=tm0)
    _same_old_fields(smooth_tracklets(recs, kps, cnt, cal, covariance="joints", timings=tm1), plain)
    assert "covariance" not in tm0 and tm1["covariance"] > 0.0 and set(tm1) == set(tm0) | {"covariance"}
    assert not any(hasattr(t, f) for t in plain for f in COV_FIELDS)
    seqs, _, _, cut, out = _scene()
    plain = smooth_sequences(seqs[1:2], cut[1:2])[0]
    assert sum(int(t.smooth_filled.sum()) for t in plain) >= 10
    _same_old_fields(out[1], plain)
    assert not any(hasattr(t, f) for t in plain for f in COV_FIELDS)


def _same_cov(a, b):
    assert len(a) == len(b)
    for t, u in zip(a, b):
        assert t.track_id == u.track_id
        for f in COV_FIELDS:
            assert np.array_equal(getattr(t, f), getattr(u, f), equal_nan=True), (t.track_id, f)


def test_bit_identity_of_the_covariance():
    """An identity alone (its sequence alone), among the others, and with a workspace cap that forces several launch partitions gives
    the same bits; so do two runs.  A one-frame record gets status 2 and NaN arrays of the right shapes."""
    from multiview_motion_capture_amd.smoothing import smooth_sequences
    seqs, _, _, cut, out = _scene()
    rows = sum(t.frame_idxs[-1] - t.frame_idxs[0] + 1 for r in cut for t in r)
    assert rows >= 300
    again = smooth_sequences(seqs, cut, covariance="joints")
    split = smooth_sequences(seqs, cut, covariance="joints", max_work_bytes=100 * 48 * 1024)    # ~100 rows a partition
    for s in range(len(seqs)):
        _same_cov(out[s], again[s])
        _same_cov(out[s], split[s])
        _same_cov(out[s], smooth_sequences([seqs[s]], [cut[s]], covariance="joints")[0])
    assert sum(len(r) for r in out) >= 6 and all(t.smooth_cov_status == 0 for r in out for t in r if len(t) >= 2)
    k = max(range(len(cut[0])), key=lambda i: int(out[0][i].smooth_filled.sum()))      # one identity with a hole, all alone
    _same_cov([out[0][k]], smooth_sequences(seqs[:1], [[cut[0][k]]], covariance="joints")[0])
    one = _first([cut[0][0]], 1)
    t = smooth_sequences(seqs[:1], [one], covariance="joints")[0][0]
    assert t.smooth_cov_status == 2 and t.smooth_nres == 0 and np.isnan(t.smooth_noise_px) and np.isnan(t.smooth_edof)
    assert t.smooth_joint_cov.shape == (1, 18, 3, 3) and t.smooth_joint_sigma.shape == (1, 18) and t.smooth_param_sigma.shape == (1, 39)
    assert np.all(np.isnan(t.smooth_joint_cov)) and np.all(np.isnan(t.smooth_joint_sigma)) and np.all(np.isnan(t.smooth_param_sigma))


def _launch(recs, sel, w, kps, cnt, cal):
    """The two covariance launches on the rows of ``recs`` (their interpolated start, selection ``sel``), driven as smooth_sequences
    drives them -> (jcov, pvar, cinfo) on the host."""
    import torch

    from multiview_motion_capture_amd import device as dev
    from multiview_motion_capture_amd import smoothing as S
    d = torch.device("cuda:0")
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(d)
    C, P = kps.shape[1], kps.shape[2]
    x0s, mems = [], []
    for r, s in zip(_np_records(recs), sel):
        x0, filled = S.initial_trajectory(r["frames"], r["params"])
        fr = np.arange(r["frames"][0], r["frames"][-1] + 1)
        assert np.all(s[filled] == -1)
        x0s.append(x0)
        mems.append(np.where(s >= 0, (fr[:, None] * C + np.arange(C)[None]) * P + s, -1).astype(np.int32))
    m_of = np.array([x.shape[0] for x in x0s])
    n_ids, n_rows = len(x0s), int(m_of.sum())
    x = T(np.concatenate(x0s))
    k17, _ = dev.ingest(T(kps), T(cnt))
    Pm = T(np.array([[np.asarray(c.P, np.float64).reshape(3, 4) for c in cal]]))
    ctl = torch.zeros((n_ids, 4), dtype=torch.int32, device=d)
    ctl[:, 1] = 1
    blk = torch.empty((2, n_rows, 820), dtype=torch.float64, device=d)
    work = torch.empty((n_rows, 3940), dtype=torch.float64, device=d)
    id_lo = T(np.concatenate([[0], np.cumsum(m_of)]).astype(np.int32))
    id_of = T(np.repeat(np.arange(n_ids, dtype=np.int32), m_of))
    rig = torch.zeros((n_rows,), dtype=torch.int32, device=d)
    mem = T(np.concatenate(mems))
    jcov = torch.zeros((n_rows, 18, 6), dtype=torch.float64, device=d)
    pvar = torch.zeros((n_rows, 39), dtype=torch.float64, device=d)
    cinfo = torch.zeros((n_ids, 8), dtype=torch.float64, device=d)
    dev.smooth_blocks(k17, Pm, rig, mem, x, id_of, ctl, blk)
    dev.smooth_cov(x, blk[0], id_lo, w, S.COV_MU, k17, Pm, rig, mem, work, jcov, pvar, cinfo)
    lo = np.concatenate([[0], np.cumsum(m_of)])
    sl = [slice(lo[i], lo[i + 1]) for i in range(n_ids)]
    return jcov.cpu().numpy(), pvar.cpu().numpy(), cinfo.cpu().numpy(), sl


def test_singular_factor_is_reported_as_status_1_with_nan_rows():
    """Six rows, row 3 without data.  (a) All four prior weights 0 (test_zero_pivot_block_is_reported_and_nothing_moves' system): row
    3's pivot block is exactly zero, the Cholesky reports it without dividing: status 1, every jcov / pvar row of the identity NaN,
    no fault.  With all four weights 0 EVERY identity is singular (no prior at all leaves the knees' Rz angles, which move no joint,
    without curvature in any row), so the identity that must stay finite is checked in (b): the root weights 0 and the angle weights
    at their defaults.  Row 3 of the identity without data there still has exactly zero pivots (its three root columns), status 1 and
    NaN rows; the complete identity beside it in the launch is solved, finite, and has the bits it has when launched alone."""
    from multiview_motion_capture_amd import smoothing as S
    si, kps, cnt, cal, fitted, views = _shelf()
    holed, whole = _first(fitted, 6, 3), _first(fitted, 6)
    sel_h = [t.smooth_select for t in S.smooth_tracklets(holed, kps, cnt, cal, max_iter=0)]
    sel_w = [t.smooth_select for t in S.smooth_tracklets(whole, kps, cnt, cal, max_iter=0)]
    # (a)
    jc, pv, ci, sl = _launch(holed, sel_h, (0.0, 0.0, 0.0, 0.0), kps, cnt, cal)
    print("\nall weights 0: cinfo", ci[:, :4])
    assert np.all(ci[:, 0] == 1.0) and np.all(np.isnan(jc)) and np.all(np.isnan(pv))
    assert np.all(np.isfinite(ci[:, 1])) and np.all(ci[:, 1] > 0) and np.all(ci[:, 4:] == 0.0)
    # (b)
    w = (0.0, 0.0, S.ANG_VEL, S.ANG_ACC)
    jc, pv, ci, sl = _launch([holed[0], whole[1]], [sel_h[0], sel_w[1]], w, kps, cnt, cal)
    print("root weights 0: cinfo", ci[:, :4])
    assert ci[0, 0] == 1.0 and np.all(np.isnan(jc[sl[0]])) and np.all(np.isnan(pv[sl[0]]))
    assert ci[1, 0] == 0.0 and np.all(np.isfinite(jc[sl[1]])) and np.all(np.isfinite(pv[sl[1]])) and np.all(pv[sl[1]] > 0)
    assert np.all(np.isfinite(ci[1])) and 0.0 < ci[1, 3] < 39 * 6 and ci[1, 2] > 0
    jc1, pv1, ci1, sl1 = _launch([whole[1]], [sel_w[1]], w, kps, cnt, cal)
    assert np.array_equal(jc[sl[1]], jc1) and np.array_equal(pv[sl[1]], pv1) and np.array_equal(ci[1], ci1[0])


def _holes(filled):
    """Runs of filled frames -> [(first, last)]."""
    out, k = [], 0
    while k < filled.size:
        if filled[k]:
            a = k
            while k + 1 < filled.size and filled[k + 1]:
                k += 1
            out.append((a, k))
        k += 1
    return out


def test_structure_that_theory_fixes_on_synthetic_scene_walks():
    """Inside a hole the prior alone carries the trajectory, a bridge pinned at both ends: the root's sigma at the middle frame is at
    least that at both frames next to data.  Per identity the median joint sigma of filled frames exceeds that of data frames.
    noise_px is a pure scale: 2 s doubles every sigma of s (s^2 x 4 and the square root are exact: the same bits x 2).  And sigma
    ranks the actual error against the generator's joints: a positive rank correlation over the pooled joints of the three rigs."""
    from scipy.stats import spearmanr

    from multiview_motion_capture_amd.smoothing import smooth_sequences
    seqs, gts, fitted, cut, out = _scene()
    n_holes = n_ids = 0
    for r in out:
        for t in r:
            if len(t) < 2:
                continue
            fl, sg = t.smooth_filled, t.smooth_joint_sigma
            assert np.all(np.isfinite(sg)) and np.all(sg > 0) and np.isfinite(t.smooth_noise_px) and t.smooth_noise_px > 0
            for a, b in _holes(fl):
                if b - a + 1 >= 3:
                    mid = (a + b) // 2
                    assert sg[mid, 0] >= sg[a, 0] and sg[mid, 0] >= sg[b, 0], (t.track_id, a, b, sg[a:b + 1, 0])
                    n_holes += 1
            if fl.any():
                assert np.median(sg[fl]) > np.median(sg[~fl]), (t.track_id, np.median(sg[fl]), np.median(sg[~fl]))
                n_ids += 1
    assert n_holes >= 3 and n_ids >= 3
    one = smooth_sequences(seqs, cut, covariance="joints", noise_px=1.5)
    two = smooth_sequences(seqs, cut, covariance="joints", noise_px=3.0)
    for r1, r2, r0 in zip(one, two, out):
        for t1, t2, t0 in zip(r1, r2, r0):
            assert t1.smooth_noise_px == 1.5 and t2.smooth_noise_px == 3.0
            if len(t1) < 2:
                continue
            for f in ("smooth_joint_sigma", "smooth_param_sigma"):
                a, b = getattr(t1, f), getattr(t2, f)
                assert np.all(np.abs(b - 2.0 * a) <= 2.0 ** -52 * np.abs(b)), (t1.track_id, f)
            assert np.all(np.abs(t2.smooth_joint_cov - 4.0 * t1.smooth_joint_cov) <= 2.0 ** -52 * np.abs(t2.smooth_joint_cov))
            assert t1.smooth_edof == t0.smooth_edof and t1.smooth_nres == t0.smooth_nres
    # sigma against the actual error, identities matched to the generator's people as test_ground_truth_of_synthetic_scene_walks does
    sig, err = [], []
    for s, g in enumerate(gts):
        maps = _raw_slot_maps(g)
        for t_fit, t in zip(fitted[s], out[s]):
            if len(t_fit) < 30 or len(t) < 2:
                continue
            person = _person(t_fit, g, maps, t_fit.fit_select)
            if person < 0:
                continue
            J = np.array([q[2].keypoints for q in t.poses])
            err.append(np.linalg.norm(J - g["gt_joints"][np.array(t.frame_idxs), person], axis=-1).ravel())
            sig.append(t.smooth_joint_sigma.ravel())
    sig, err = np.concatenate(sig), np.concatenate(err)
    rho = float(spearmanr(sig, err)[0])
    print(f"\n{sig.size} pooled joints: rank correlation of joint sigma with the actual error {rho:.3f}; median sigma "
          f"{1e3 * np.median(sig):.1f} mm, median error {1e3 * np.median(err):.1f} mm")
    assert sig.size >= 3 * 60 * 18 and rho > 0.0    # at least one whole identity per rig
