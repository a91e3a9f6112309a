"""NumPy restatement of the body fit (multiview_motion_capture_amd/body_fit.py, csrc/mvmc_bodyfit.hip): one side-length vector per
identity, every frame's pose re-solved against it.  The device is gated against this file.

Data model (host side, no MvTracklet objects):
  views    per sequence, per frame, per camera: (n, 17, 3) COCO-17 poses in ingest order (openpose25_to_coco17 + filter_bad_pose,
           compacted): the pose slots the tracker's graph sees;
  Ps       per sequence (C, 3, 4);
  records  per sequence: dicts(frames (n,), params (n, 68), joints (n, 18, 3)), in the caller's order.

Algorithm (one identity = one record):
  a. selection: per (problem, camera) the pose with the smallest reprojection_error (motion_capture.py:403-414, min score 0.1) to the
     record's joints among those with a finite distance below the affinity floor D_MAX; a pose claimed by two records of the same frame
     goes to the smaller distance (ties: the earlier record), the loser takes nothing in that camera; fewer than 2 views: frozen;
  b. l0 = per-slot median of the per-frame lengths over the non-frozen problems (all problems when every one is frozen);
  c. rounds of (length step: Levenberg-Marquardt on the free slots, poses fixed; pose step: stage 1 of PoseSolver, trf(ne_clean),
     max_nfev evaluations, warm from the current pose).
"""
import numpy as np

import oracle_np as o
import trf_np as t

MIN_SCORE = 0.1
D_MAX = 15.0 + 30.0 * np.log(999.0) / 5.0     # S = 1 / (1 + exp(5 (D - 15) / 30)) < 1e-3 is cut to 0 (mvmc_st_affinity)
N_SIDE = 11
LM_MU0 = 1e-3       # Marquardt's damping (H + mu diag(H)): mu is dimensionless
LM_FTOL = 1e-12
LM_XTOL = 1e-10


def ingest_np(kps, counts):
    """(F,C,P,25|17,3), (F,C) -> views[f][c] = (n,17,3) good poses in order (mvmc_ingest)."""
    kps = np.asarray(kps, np.float64)
    out = []
    for f in range(kps.shape[0]):
        row = []
        for c in range(kps.shape[1]):
            ps = [kps[f, c, p] for p in range(int(counts[f, c]))]
            ps = [o.openpose25_to_coco17(q) if q.shape[0] == 25 else q for q in ps]
            ps = [q for q in ps if o.pose_is_good(q)]
            row.append(np.array(ps).reshape(-1, 17, 3))
        out.append(row)
    return out


def reproj_dist(joints, kp17, P):
    """reprojection_error(joints, kp17[:, :2], kp17[:, 2], P, 0.1, nan), summed in joint order."""
    X = joints[o.REPROJ_SKEL_IDX]
    h = X @ P[:, :3].T + P[:, 3]
    u = h[:, 0] / (1e-5 + h[:, 2])
    v = h[:, 1] / (1e-5 + h[:, 2])
    k = kp17[o.REPROJ_COCO_IDX]
    m = k[:, 2] > MIN_SCORE
    if not m.any():
        return np.nan
    e = np.sqrt((u - k[:, 0]) ** 2 + (v - k[:, 1]) ** 2)[m]
    return np.cumsum(e)[-1] / m.sum()


def select(problems, views, Ps):
    """problems: list of (seq, frame, rec, joints (18,3)), rec = position of the record in its sequence's list.
    -> sel (B,C) slot in the camera's pose list or -1, dist (B,C) (inf where nothing was chosen), n_views (B,)."""
    B = len(problems)
    C = max((Ps[s].shape[0] for s, _, _, _ in problems), default=0)
    sel = -np.ones((B, C), np.int64)
    dist = np.full((B, C), np.inf)
    for b, (s, f, _, J) in enumerate(problems):
        for c in range(Ps[s].shape[0]):
            for p, q in enumerate(views[s][f][c]):
                d = reproj_dist(J, q, Ps[s][c])
                if np.isfinite(d) and d < D_MAX and d < dist[b, c]:
                    sel[b, c], dist[b, c] = p, d
    # conflicts inside one (sequence, frame): the smaller distance wins, ties the earlier record; the loser takes nothing
    won = sel.copy()
    for b, (s, f, r, _) in enumerate(problems):
        for c in range(C):
            if sel[b, c] < 0:
                continue
            for b2, (s2, f2, r2, _) in enumerate(problems):
                if b2 == b or s2 != s or f2 != f or sel[b2, c] != sel[b, c]:
                    continue
                if dist[b2, c] < dist[b, c] or (dist[b2, c] == dist[b, c] and r2 < r):
                    won[b, c] = -1
    return won, dist, (won >= 0).sum(axis=1)


def len_basis(params):
    """Joints of the IK rows as root + A l: (root (3,), A (16, 11, 3)) at the record's angles."""
    dirs, _ = o.skeleton_constants()
    _, G = o.forward_kinematics(params[:3], params[3:57], params[57:])
    Rg = G[:, :3, :3]
    A = np.zeros((16, N_SIDE, 3))
    for r, k in enumerate(o.IK_SKEL_IDX):
        j = k
        while j != 0:
            p = o.SKEL_PARENTS[j]
            A[r, o.SIDE_TO_FULL[j]] += Rg[p] @ dirs[j]
            j = p
    return params[:3].copy(), A


def len_terms(roots, As, pv_prob, pv_P, pv_obs, lens):
    """E = 1/2 sum r^2, H = J^T J, g = J^T r over the (problem, view) pairs, with respect to the 11 lengths."""
    X = roots[:, None, :] + np.einsum("nrsd,s->nrd", As, lens)
    Xv = X[pv_prob]
    h = np.einsum("mrd,med->mre", Xv, pv_P[:, :, :3]) + pv_P[:, None, :, 3]
    wd = h[..., 2] + 1e-5
    u, v = h[..., 0] / wd, h[..., 1] / wd
    w = pv_obs[..., 2]
    ru, rv = (u - pv_obs[..., 0]) * w, (v - pv_obs[..., 1]) * w
    E = 0.5 * (np.sum(ru * ru) + np.sum(rv * rv))
    Av = As[pv_prob]
    du = (pv_P[:, None, 0, :3] - u[..., None] * pv_P[:, None, 2, :3]) / wd[..., None]
    dv = (pv_P[:, None, 1, :3] - v[..., None] * pv_P[:, None, 2, :3]) / wd[..., None]
    Ju = (w[..., None] * np.einsum("mrd,mrsd->mrs", du, Av)).reshape(-1, N_SIDE)
    Jv = (w[..., None] * np.einsum("mrd,mrsd->mrs", dv, Av)).reshape(-1, N_SIDE)
    H = Ju.T @ Ju + Jv.T @ Jv
    g = Ju.T @ ru.ravel() + Jv.T @ rv.ravel()
    return E, H, g


def length_step(params, obs, projs, lens, free=None, max_iter=10, mu0=LM_MU0, ftol=LM_FTOL, xtol=LM_XTOL, log=None):
    """Levenberg-Marquardt on the free slots of the identity's lengths, every problem's root and angles fixed.
    params (n,68); obs / projs: per problem (V,16,3) / (V,3,4).  -> (lens, free, dict(E0, E, trace)); trace: 1 accepted, 0 rejected.
    log: a list that receives one dict per look at the system (E, dmax = |d|_inf, pred, stop: None / "xtol" / "pred" / "ftol", and for
    a look that made a trial Et and accepted): what the tests' decision margins are computed from."""
    lens = np.array(lens, np.float64)
    basis = [len_basis(p) for p in params]
    roots = np.array([b[0] for b in basis])
    As = np.array([b[1] for b in basis])
    pv_prob = np.concatenate([np.full(len(ob), i) for i, ob in enumerate(obs)]).astype(int)
    pv_P = np.concatenate(projs)
    pv_obs = np.concatenate(obs)
    E, H, g = len_terms(roots, As, pv_prob, pv_P, pv_obs, lens)
    E0 = E
    if free is None:
        free = np.diag(H) > 0
    trace = []
    if not free.any() or max_iter <= 0:
        return lens, free, dict(E0=E0, E=E, trace=trace)
    mu = mu0
    for _ in range(max_iter):
        Hf = H[np.ix_(free, free)]
        d = np.linalg.solve(Hf + mu * np.diag(np.diag(Hf)), -g[free])
        # (stops before a trial whose predicted reduction is below LM_FTOL E: such a trial's accept / reject is decided by rounding)
        dmax, pred = np.abs(d).max(), -(d @ g[free] + 0.5 * d @ Hf @ d)
        look = dict(E=E, dmax=dmax, pred=pred, stop="xtol" if dmax < xtol else "pred" if pred < ftol * E else None)
        if log is not None:
            log.append(look)
        if look["stop"]:
            break
        trial = lens.copy()
        trial[free] += d
        E2, H2, g2 = len_terms(roots, As, pv_prob, pv_P, pv_obs, trial)
        look.update(Et=E2, accepted=bool(E2 < E))
        if E2 < E:
            red = E - E2
            lens, E_old, E, H, g = trial, E, E2, H2, g2
            mu /= 10.0
            trace.append(1)
            if red < ftol * E_old:
                look["stop"] = "ftol"
                break
        else:
            mu *= 10.0
            trace.append(0)
    return lens, free, dict(E0=E0, E=E, trace=trace)


def length_margins(log, ftol=LM_FTOL, xtol=LM_XTOL):
    """The smallest relative distance of a length step's decisions from their thresholds (length_step's log): dict(trial = |Et - E| / E
    over the trials, pred = |pred / (ftol E) - 1| and dmax = |dmax / xtol - 1| over the looks, red = |(E - Et) / (ftol E) - 1| over the
    accepted trials); inf where there was no such decision."""
    m = dict(trial=np.inf, pred=np.inf, dmax=np.inf, red=np.inf)
    for k in log:
        m["dmax"] = min(m["dmax"], abs(k["dmax"] / xtol - 1.0))
        if k["stop"] != "xtol":                     # (the kernel's || evaluates pred either way; it decides only past the xtol test)
            m["pred"] = min(m["pred"], abs(k["pred"] / (ftol * k["E"]) - 1.0) if ftol * k["E"] > 0 else np.inf)
        if "Et" in k:
            m["trial"] = min(m["trial"], abs(k["Et"] - k["E"]) / k["E"])
            if k["accepted"]:
                m["red"] = min(m["red"], abs((k["E"] - k["Et"]) / (ftol * k["E"]) - 1.0) if ftol * k["E"] > 0 else np.inf)
    return m


def pose_step(param, ob, pr, lens, max_nfev=5, trace=None):
    """solve_pose_reproj with the identity's lengths, warm from the problem's pose -> (params (68,), cost).  trace: trf_np.trf's."""
    f1 = lambda x: o.ik_residual(x[:3], x[3:57], lens, ob, pr)
    j1 = lambda x, f: t.ik_jacobian(x[:3], x[3:57], lens, ob, pr, False)
    r = t.trf(f1, j1, param[:57].copy(), max_nfev, solver="ne_clean", trace=trace)
    return np.concatenate([r["x"], lens]), r["cost"]


def pose_margin(trace, ftol=1e-8, xtol=1e-8, gtol=1e-8):
    """The smallest relative distance of a pose step's trust-region decisions from their thresholds (trf_np.trf's trace): the trial's
    cost against the cost, the ratio against 0.25 and 0.75, the step against 0.95 Delta, the reduction against ftol cost, the step
    against xtol (xtol + |x|), the gradient against gtol; and the weakest eigenvalue of a model relative to its largest, where it lies
    between the null cluster (1e-13) and 1e-6 (tests/test_gpu_ik_whole_solves.py: such a model's step is not reproducible to 1e-8 m)."""
    m = np.inf
    for e in trace:
        if "model" in e:
            lam = e["lam"] / e["lam"][0]
            weak = lam[(lam > 1e-13) & (lam < 1e-6)]
            m = min([m, abs(e["g_inf"] / gtol - 1.0)] + ([0.0] if weak.size else []))
            continue
        red = e["cost"] - e["cost_new"]
        m = min(m, abs(red) / e["cost"], abs(e["ratio"] / 0.25 - 1.0), abs(e["ratio"] / 0.75 - 1.0),
                abs(e["step_norm"] / (0.95 * e["Delta"]) - 1.0), abs(red / (ftol * e["cost"]) - 1.0),
                abs(e["step_norm"] / (xtol * (xtol + np.linalg.norm(e["x"]))) - 1.0))
    return m


def select_padded(kps17, counts, Pmats, frame_of, rig_of, rank, joints, max_dist=D_MAX):
    """select() on the device's own tables (include/mvmc.h: mvmc_body_observe), which may hold what ingest would have filtered: kps17
    (F,C,P,17,3) read as given, counts (F,C) clamped to [0, P], Pmats (R,C,3,4); per problem frame_of (a row of kps17: two problems
    compete when they name the same row), rig_of, rank, joints (B,18,3).  A problem whose frame or rig is out of range chooses nothing.
    -> choice (B,C) pose index (f C + c) P + p before the conflicts or -1, dist (B,C), members (B,C), n_views (B,)."""
    F, C, Pmax = kps17.shape[:3]
    B = len(frame_of)
    choice = -np.ones((B, C), np.int64)
    dist = np.full((B, C), np.inf)
    for b in range(B):
        f, r = int(frame_of[b]), int(rig_of[b])
        if not (0 <= f < F and 0 <= r < Pmats.shape[0]):
            continue
        for c in range(C):
            for p in range(min(max(int(counts[f, c]), 0), Pmax)):
                d = reproj_dist(joints[b], kps17[f, c, p], Pmats[r, c])
                if d < max_dist and d < dist[b, c]:              # (NaN: never a candidate)
                    choice[b, c], dist[b, c] = (f * C + c) * Pmax + p, d
    members = choice.copy()
    for b in range(B):
        for c in range(C):
            for b2 in range(B):
                if choice[b, c] < 0 or b2 == b or frame_of[b2] != frame_of[b] or choice[b2, c] != choice[b, c]:
                    continue
                if dist[b2, c] < dist[b, c] or (dist[b2, c] == dist[b, c] and rank[b2] < rank[b]):
                    members[b, c] = -1
    return choice, dist, members, (members >= 0).sum(axis=1)


def observations(sel_row, views_f, P):
    """(V,16,3) IK observation rows and (V,3,4) projections of the selected poses."""
    obs, pr = [], []
    for c, p in enumerate(sel_row):
        if p >= 0:
            obs.append(o.add_mid_spine(views_f[c][p])[o.IK_OBS_IDX])
            pr.append(P[c])
    return np.array(obs).reshape(-1, 16, 3), np.array(pr).reshape(-1, 3, 4)


def fit(views, Ps, records, rounds=3, max_iter=10, max_nfev=5):
    """All sequences' records -> per sequence, per record: dict(lens, params, joints, views (n,), sel (n,C), cost [E0, len1, pose1, ...],
    traces [per round: LM accept / reject list])."""
    problems, owner = [], []
    for s, recs in enumerate(records):
        for r, rec in enumerate(recs):
            for k, f in enumerate(rec["frames"]):
                problems.append((s, int(f), r, np.asarray(rec["joints"][k], np.float64)))
                owner.append((s, r, k))
    sel, dist, nv = select(problems, views, Ps) if problems else (np.zeros((0, 0), int), None, np.zeros(0, int))
    out = [[None] * len(recs) for recs in records]
    at = 0
    for s, recs in enumerate(records):
        for r, rec in enumerate(recs):
            n = len(rec["frames"])
            rows = np.arange(at, at + n)
            at += n
            params = np.array(rec["params"], np.float64).copy()
            live = nv[rows] >= 2
            src = params[live] if live.any() else params
            lens = np.median(src[:, 57:], axis=0)
            lens[7] = params[0, 57 + 7]
            obs, prs = [], []
            for k in np.flatnonzero(live):
                ob, pr = observations(sel[rows[k]], views[s][int(rec["frames"][k])], Ps[s])
                obs.append(ob)
                prs.append(pr)
            cost, traces, free = [], [], None
            lp = np.flatnonzero(live)
            for rd in range(rounds):
                lens, free, info = length_step(params[lp], obs, prs, lens, free, max_iter) if lp.size else (lens, free, None)
                if rd == 0:
                    cost.append(info["E0"] if info else 0.0)
                cost.append(info["E"] if info else 0.0)
                traces.append(info["trace"] if info else [])
                e = 0.0
                for i, k in enumerate(lp):
                    params[k], c = pose_step(params[k], obs[i], prs[i], lens, max_nfev)
                    e += c
                cost.append(e)
            if rounds == 0:
                cost.append(length_step(params[lp], obs, prs, lens, None, 0)[2]["E0"] if lp.size else 0.0)
            params[:, 57:] = lens
            joints = np.array([o.forward_kinematics(p[:3], p[3:57], lens)[0] for p in params]).reshape(-1, 18, 3)
            out[s][r] = dict(lens=lens, params=params, joints=joints, views=nv[rows] * live, sel=sel[rows], cost=np.array(cost),
                             traces=traces, free=free)
    return out
