"""The restatement the temporal-layer kernels are compared with (tests/track_np.py) is itself pinned here, without a GPU: on the
first 24 golden Shelf frames its three functions must reproduce oracle/tracker_np.OracleTracker -- the reference's match_spatial_time
and MvTracker.update_4d restated, which tests/test_tracker_oracle_cpu.py holds bit-exact against the reference's own log -- frame by
frame, and the hand-built cases of tests/track_cases.py must reach every branch they are made for (check_coverage)."""
import numpy as np

import oracle_np as o
import track_cases as tc
import track_np as tn
import tracker_np as tk
from conftest import load_golden
from helpers import oracle_ingest

N_FRAMES, T, K, V = 24, 8, 6, 6


def make_standin_solver(period=5, lift=0.2):
    """A cheap deterministic solve: BASIC_18 joints from the DLT of the matched COCO joints (the joints reprojection_error reads;
    the rest at their mean), parameters that name the joints -- enough for the tracker to keep following people.  Every ``period``-th
    call returns its joints ``lift`` metres too high, so that the next frame's association loses that tracklet and a new one is born:
    the 24 frames then hold deaths and births, not two people tracked without an event."""
    calls = [0]

    def solve(poses, projs, init):
        calls[0] += 1
        X = o.triangulate_groups(np.asarray(projs), [np.asarray(p) for p in poses], 0.01)[:, :3]
        joints = np.tile(X[o.REPROJ_COCO_IDX].mean(axis=0), (18, 1))
        joints[o.REPROJ_SKEL_IDX] = X[o.REPROJ_COCO_IDX]
        if calls[0] % period == period - 1:
            joints = joints + np.array([0.0, 0.0, lift])
        root = joints[0] + (0.0 if init is None else 1e-3)
        return (root, joints * 0.5, joints[:11, 0].copy()), joints
    return solve


def _flat(param):
    return np.concatenate([param[0], np.asarray(param[1]).ravel(), param[2]])


def test_restatement_follows_the_oracle_tracker_on_shelf():
    si = load_golden("shelf_inputs.npz")
    k17, cnt = oracle_ingest(si["kps25"][:N_FRAMES + 1], si["counts"][:N_FRAMES + 1].astype(np.int32))
    C, P = k17.shape[1:3]
    tr = tk.OracleTracker(si["K"], si["Rt"], si["P"], solver=make_standin_solver())
    solver = make_standin_solver()            # the same solves in the same order (live tracklets by slot, then the new ones)
    tab = dict(params=np.zeros((1, T, 68)), joints=np.zeros((1, T, 18, 3)), meta=np.zeros((1, T, 4), np.int32),
               n_tracks=np.zeros(1, np.int32), next_id=np.zeros(1, np.int32), n_dead=np.zeros(1, np.int32))
    seen = dict(st=0, sp=0, status=set(), born=0)
    for fi in range(1, N_FRAMES + 1):
        views = [[k17[fi, c, p] for p in range(cnt[fi, c])] for c in range(C)]
        fidx = np.array([fi], np.int32)
        nt = len(tr.tracklets)
        assert nt == tab["n_tracks"][0]
        lab_sp, lab_st = -np.ones((1, C * P), np.int32), -np.ones((1, T + C * P), np.int32)
        ncl_sp, ncl_st = np.zeros(1, np.int32), np.zeros(1, np.int32)
        tm, nm = tk.associate(tr.tracklets, views, si["P"], si["K"], si["Rt"])
        if nt:
            D_o, dim = o.spatial_time_distance([t.joints for t in tr.tracklets], views, si["P"])
            _, S_o = o.spatial_time_affinity(D_o)
            n = dim[-1]
            W, D, gc = tn.st_affinity_np(k17, cnt, fidx, tab["joints"], tab["n_tracks"], si["P"])
            assert gc[0].tolist() == np.diff(dim).tolist()
            assert np.array_equal(D[0, :n, :n], D_o, equal_nan=True) and np.array_equal(W[0, :n, :n], S_o)
            assert not W[0, n:].any() and not W[0, :, n:].any() and not D[0, n:].any() and not D[0, :, n:].any()
            mm, _ = o.match_als(S_o, dim)
            lab = o.cluster_labels(mm, n)
            lab_st[0, :n], ncl_st[0] = lab, lab.max() + 1
            seen["st"] += 1
        else:
            pts = [p[:, :2] for v in views for p in v]
            dim = np.concatenate([[0], np.cumsum([len(v) for v in views])]).tolist()
            _, S = o.geometry_affinity(np.array(pts), o.pairwise_f_mats(si["K"], si["Rt"]), dim)
            mm, _ = o.match_als(S, dim)
            lab = o.cluster_labels(mm, dim[-1])
            lab_sp[0, :dim[-1]], ncl_sp[0] = lab, lab.max() + 1
            seen["sp"] += 1
        mem, cold, init, status, n_new, ovf = tn.assign_np(lab_sp, ncl_sp, lab_st, ncl_st, cnt, fidx, tab["n_tracks"], tab["params"],
                                                           P, K, V)
        val = lambda m: [(fi * C + v) * P + l for v, l in m]
        assert ovf[0] == 0 and np.array_equal(init[0], tab["params"][0] * (np.arange(T) < nt)[:, None])
        assert cold[0].tolist() == [0] * T + [1] * K
        for k in range(T):
            exp = tm.get(k, []) if k < nt else []
            assert status[0, k] == (2 if len(exp) >= 2 else 1 if len(exp) == 1 else 0), (fi, k)
            assert [q for q in mem[0, k] if q >= 0] == (val(exp) if len(exp) >= 2 else []), (fi, k)
            if k < nt:
                seen["status"].add(int(status[0, k]))
        new = [m for m in nm if len(m) >= 2]
        assert n_new[0] == len(new)
        for k in range(K):
            assert [q for q in mem[0, T + k] if q >= 0] == (val(new[k]) if k < len(new) else []), (fi, k)
        # the frame's solves, slot by slot, then the commit against the tracker's own update
        ikp, ikj = np.zeros((1, T + K, 68)), np.zeros((1, T + K, 18, 3))
        for s in [k for k in range(T) if status[0, k] == 2] + [T + k for k in range(int(n_new[0]))]:
            q = [int(x) for x in mem[0, s] if x >= 0]
            poses = [k17[fi, (x // P) % C, x % P] for x in q]
            param, joints = solver(poses, [si["P"][(x // P) % C] for x in q], None if s >= T else tr.tracklets[s].param)
            ikp[0, s], ikj[0, s] = _flat(param), joints
        tab = tn.commit_np(status, n_new, ikp, ikj, tab["params"], tab["joints"], tab["meta"], tab["n_tracks"], tab["next_id"],
                           tab["n_dead"], K, 3)
        tr.update(fi, views)
        n_after = len(tr.tracklets)
        exp_meta = np.array([[t.tid, t.state, t.hits, t.length] for t in tr.tracklets], np.int32).reshape(-1, 4)
        assert tab["n_tracks"][0] == n_after and np.array_equal(tab["meta"][0, :n_after], exp_meta), fi
        assert tab["n_dead"][0] == tr.n_dead and tab["next_id"][0] == tr.next_id and tab["overflow"][0] == 0, fi
        for s, t in enumerate(tr.tracklets):
            assert np.array_equal(tab["joints"][0, s], t.joints) and np.array_equal(tab["params"][0, s], _flat(t.param)), (fi, s)
        seen["born"] = int(tab["next_id"][0])
    # the sequence exercised both paths, updates, deaths and births (one-view matches: tests/track_cases.py)
    assert seen["sp"] >= 1 and seen["st"] >= N_FRAMES - 2 and seen["status"] >= {0, 2}, seen
    assert seen["born"] >= 5 and tr.n_dead >= 3, (seen, tr.n_dead)


def test_cases_reach_what_they_are_for():
    rep = tc.check_coverage()
    for k, v in rep.items():
        print(k, v)
