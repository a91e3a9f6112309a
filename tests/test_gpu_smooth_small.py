"""GPU: the offline trajectory smoother's block-banded sweep (csrc/mvmc_smooth_sweep.h through csrc/mvmc_smooth.hip) at the row counts
where a banded sweep goes wrong, against the NumPy restatement (tests/smooth_np.py): 2 rows (no second sub-diagonal), 3 (the first
L(t+2,t) block), 4, 5, 6 and 11 rows (the five rotating block roles wrapped once and twice), a row without data (the prior alone places
it), and a system whose pivot block is exactly zero (the Cholesky must report it: stop reason 5, no trial)."""
import functools

import numpy as np
import pytest

import smooth_np as sm
from conftest import load_golden
from test_gpu_smooth import _calibs, _compare, _np_records, _oracle_records, _weights

pytestmark = pytest.mark.gpu

N = 12   # Shelf frames 1..12: both people are tracked on every one of them


@functools.lru_cache(maxsize=None)
def _shelf():
    """Body-fitted records of the first N Shelf frames, once for the module (nothing here is modified afterwards)."""
    from multiview_motion_capture_amd.body_fit import fit_tracklets
    si, fx = load_golden("shelf_inputs.npz"), load_golden("shelf_clean_oracle_tracker.npz")
    kps, cnt = si["kps25"][:N + 1], si["counts"][:N + 1].astype(np.int32)
    cal = _calibs(si["K"], si["Rt"])
    fitted = fit_tracklets(_oracle_records(fx, N), kps, cnt, cal)
    assert len(fitted) >= 2 and all(len(t) >= 11 for t in fitted)
    return si, kps, cnt, cal, fitted, sm.bf.ingest_np(kps, cnt)


def _first(recs, n, drop=None):
    """Copies of the records cut to their first n record frames (test_gpu_smooth._cut's way of copying), without frame ``drop``."""
    out = []
    for t in recs:
        keep = [i for i in range(n) if i != drop]
        u = type(t).__new__(type(t))
        u.__dict__.update(t.__dict__)
        u.frame_idxs = [t.frame_idxs[i] for i in keep]
        u.poses = [t.poses[i] for i in keep]
        out.append(u)
    return out


@pytest.mark.parametrize("n,drop", [(2, None), (3, None), (4, None), (5, None), (6, None), (11, None), (6, 3), (11, 5)])
def test_device_equals_the_restatement_on_few_rows(n, drop):
    from multiview_motion_capture_amd.smoothing import smooth_tracklets
    si, kps, cnt, cal, fitted, views = _shelf()
    recs = _first(fitted, n, drop)
    got = smooth_tracklets(recs, kps, cnt, cal)
    exp = sm.smooth([views], [si["P"]], [_np_records(recs)], _weights())[0]
    for t in got:
        assert len(t) == n and int(t.smooth_filled.sum()) == (drop is not None)
        if drop is not None:   # the filled row: no member, no data term
            assert t.smooth_filled[drop] and t.smooth_views[drop] == 0 and np.all(t.smooth_select[drop] == -1)
        print(f"identity {t.track_id}: {len(t)} rows, E {np.array2string(t.smooth_cost, precision=3)}, trials {t.smooth_trials}")
    assert any(len(t.smooth_trials) >= 1 for t in got)
    _compare(got, exp, f"{n} rows" + ("" if drop is None else f", row {drop} without data"))


def test_zero_pivot_block_is_reported_and_nothing_moves():
    """Six rows, row 3 without data, all four prior weights 0: row 3's pivot block is exactly zero.  The restatement's first banded
    Cholesky fails (smooth_np.lm stops without a trial); the device must stop the same way, reason 5 in info, with x and E untouched.
    smoothing._check_weights refuses all-zero weights, so the two kernels are driven as smooth_sequences drives them."""
    import torch

    from multiview_motion_capture_amd import device as dev
    from multiview_motion_capture_amd import smoothing as S
    si, kps, cnt, cal, fitted, views = _shelf()
    recs = _first(fitted, 6, 3)
    nrec = _np_records(recs)
    w0 = (0.0, 0.0, 0.0, 0.0)
    solves = []
    solve = sm.banded_solve

    def spy(*a):
        out = solve(*a)
        solves.append(out[2])
        return out
    sm.banded_solve = spy
    try:
        exp = sm.smooth([views], [si["P"]], [nrec], w0)[0]
    finally:
        sm.banded_solve = solve
    assert solves == [False] * len(recs)                       # one solve per identity, and it fails
    for e in exp:
        assert e["trace"] == [] and np.array_equal(e["cost"][2:], e["cost"][:2]) and np.array_equal(e["params"], e["x0"])
    # the selection of the public path (default weights), then the same rows through the kernels with zero weights
    sel = [t.smooth_select for t in S.smooth_tracklets(recs, kps, cnt, cal, max_iter=0)]
    d = torch.device("cuda:0")
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(d)
    C, P = kps.shape[1], kps.shape[2]
    x0s, mems = [], []
    for r, e, s in zip(nrec, exp, sel):
        x0, filled = S.initial_trajectory(r["frames"], r["params"])
        assert np.array_equal(filled, e["filled"]) and np.abs(x0 - e["x0"]).max() <= 1e-12
        assert np.array_equal(s[~filled], e["sel"]) and np.all(s[filled] == -1)
        fr = np.arange(r["frames"][0], r["frames"][-1] + 1)
        x0s.append(x0)
        mems.append(np.where(s >= 0, (fr[:, None] * C + np.arange(C)[None]) * P + s, -1).astype(np.int32))
    m_of = np.array([x.shape[0] for x in x0s])
    n_ids, n_rows = len(x0s), int(m_of.sum())
    x_h = np.concatenate(x0s)
    x = T(x_h)
    xt = x.clone()
    k17, _ = dev.ingest(T(kps), T(cnt))
    Pm = T(np.array([[np.asarray(c.P, np.float64).reshape(3, 4) for c in cal]]))
    ctl = torch.zeros((n_ids, 4), dtype=torch.int32, device=d)
    ctl[:, 1] = 1
    info = torch.empty((n_ids, 32), dtype=torch.float64, device=d)
    blk = torch.empty((2, n_rows, 820), dtype=torch.float64, device=d)
    work = torch.empty((n_rows, 3940), dtype=torch.float64, device=d)
    id_lo = T(np.concatenate([[0], np.cumsum(m_of)]).astype(np.int32))
    id_of = T(np.repeat(np.arange(n_ids, dtype=np.int32), m_of))
    rig = torch.zeros((n_rows,), dtype=torch.int32, device=d)
    mem = T(np.concatenate(mems))
    for phase in range(10 + 1):
        dev.smooth_blocks(k17, Pm, rig, mem, x if phase == 0 else xt, id_of, ctl, blk)
        dev.smooth_step(x, xt, blk, id_lo, w0, S.LM_MU0, S.LM_FTOL, S.LM_XTOL, 10, phase, ctl, info, work)
    inf = info.cpu().numpy()
    print("\nzero pivot block: info", inf[:, :8])
    assert np.all(ctl[:, 0].cpu().numpy() == 1)
    assert np.all(inf[:, 7] == 5.0) and np.all(inf[:, 4] == 0.0) and np.all(inf[:, 5] == 0.0) and np.all(inf[:, 8:] == -1.0)
    assert np.array_equal(inf[:, 2:4], inf[:, 0:2])            # smooth_cost[2:] == smooth_cost[:2]
    assert np.array_equal(x.cpu().numpy(), x_h)                 # the interpolated start
    for a, e in enumerate(exp):
        assert inf[a, 1] == 0.0 and abs(inf[a, 0] - e["cost"][0]) <= 1e-9 * e["cost"][0]
