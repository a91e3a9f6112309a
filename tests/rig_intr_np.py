"""NumPy restatement of the rig refinement with intrinsic unknowns (rig_refine.refine_rigs(intrinsics=...),
rig_init.calibrate_rigs(polish_intrinsics=...), csrc/mvmc_rigfit.hip: mvmc_rig_accumulate_intr, mvmc_rig_step_intr).  Everything the
intrinsics do not touch is tests/rig_refine_np.py's and tests/rig_robust_np.py's: the problem, the loss, the gauge rescale, the
Levenberg-Marquardt rules.

Model.  intrinsics "focal" (NI = 1) gives every camera with free intrinsics a log-scale phi: K[0,0], K[0,1], K[1,1] <- e^phi x
themselves; "focal+centre" (NI = 3) adds dcx, dcy on K[0,2], K[1,2].  The rows of an observation are closed-form:
d(u, v)/dphi = (u - cx, v - cy), d/dcx = (1, 0), d/dcy = (0, 1), times sqrt(w) with a loss.  Camera 0's pose stays held, its
intrinsics are free; a camera held for too few observations keeps its K as well (its observations left); a camera named in
intrinsics_held keeps its K and stays in the problem with its pose free.

Prior.  E_prior = 1/2 sum (phi / focal_sigma)^2 + 1/2 sum (dcx^2 + dcy^2) / centre_sigma^2 about the INPUT K, with
phi = log(K[0,0] / K_in[0,0]) -- accumulated over the call, not per step.  It is part of E wherever a cost is read and of the
normal equations (diagonal and gradient of the intrinsic columns).  sigma None or +inf: no term.

Layout of the reduced system (the device's, so that red compares entry for entry): one contiguous block per camera in camera order,
its 6 pose columns if the pose is free, then its NI intrinsic columns if the intrinsics are free.

Stop rule.  In |d|_inf the intrinsic steps enter as phi and dc / fx: dimensionless and of the size of the rotation steps.

What the geometry allows (tests/test_rig_intr_cpu.py asserts it on rig_cases.ring_rig): with focal only the reduced matrix has the
scale gauge as its one null direction at C >= 3 and one more at C = 2, so two cameras need a finite focal_sigma; with the principal
point it has three more at any C on rigs that fixate one point, so "focal+centre" needs a finite centre_sigma_px.  Both are refused
with ValueError.
"""
import numpy as np

import rig_refine_np as rr
import rig_robust_np as rb

MODES = {None: 0, "focal": 1, "focal+centre": 3}
LOSS_PX = rb.LOSS_PX


def check(intrinsics, focal_sigma, centre_sigma_px, C):
    """The refusals -> (NI, sigma_f, sigma_c) with +inf for no term."""
    if intrinsics not in MODES:
        raise ValueError('intrinsics is None, "focal" or "focal+centre"')
    sf = np.inf if focal_sigma is None else float(focal_sigma)
    sc = np.inf if centre_sigma_px is None else float(centre_sigma_px)
    if not (sf > 0.0 and sc > 0.0):
        raise ValueError("focal_sigma and centre_sigma_px must be None or > 0")
    if intrinsics == "focal+centre" and not np.isfinite(sc):
        raise ValueError('"focal+centre" needs a finite centre_sigma_px: the principal points are not observable without a prior')
    if intrinsics is not None and C == 2 and not np.isfinite(sf):
        raise ValueError("two cameras need a finite focal_sigma: their focal lengths are not observable without a prior")
    return MODES[intrinsics], sf, sc


def free_intrinsics(held, NI, intrinsics_held=()):
    """(C,) bool: the cameras whose intrinsics are unknowns."""
    held = np.asarray(held, bool)
    f = np.full(held.shape[0], NI > 0)
    f[1:] &= ~held[1:]
    f[[int(c) for c in intrinsics_held]] = False
    return f


def columns(held, ifree, NI):
    """-> (cam (M,), row (M,)): the camera and its row 0 .. 5 (pose) or 6 .. 6 + NI - 1 (intrinsics) of every column."""
    cam, row = [], []
    for c in range(len(held)):
        if not held[c]:
            cam += [c] * 6
            row += list(range(6))
        if ifree[c]:
            cam += [c] * NI
            row += list(range(6, 6 + NI))
    return np.array(cam, np.int64), np.array(row, np.int64)


def deltas(K, K0):
    """(C, 3): phi, dcx, dcy of K about K0."""
    return np.stack([np.log(K[:, 0, 0] / K0[:, 0, 0]), K[:, 0, 2] - K0[:, 0, 2], K[:, 1, 2] - K0[:, 1, 2]], axis=1)


def prior(K, K0, ifree, NI, sf, sc):
    if NI == 0:
        return 0.0
    d = deltas(K, K0)[ifree]
    e = 0.5 * np.sum((d[:, 0] / sf) ** 2)
    if NI == 3:
        e = e + 0.5 * np.sum((d[:, 1] / sc) ** 2 + (d[:, 2] / sc) ** 2)
    return float(e)


def cost(X, uv, K, R, t, K0, ifree, NI, sf, sc, loss=None, loss_px=LOSS_PX):
    return rb.cost(X, uv, K, R, t, loss, loss_px) + prior(K, K0, ifree, NI, sf, sc)


def jacobian(X, uv, K, R, t, NI, loss=None, loss_px=LOSS_PX):
    """The rows of every observation at (X, cameras), zero where there is none -> dict(E (the data cost), ru, rv (n,C), a, b (n,C,3)
    point rows, ju, jv (n,C,6+NI) camera rows: rotation, translation, then phi, dcx, dcy)."""
    obs = ~np.isnan(uv[:, :, 0])
    y = np.einsum("cij,nj->nci", R, X)
    xc = y + t[None]
    p = np.einsum("cij,ncj->nci", K, xc)
    u, v = p[..., 0] / p[..., 2], p[..., 1] / p[..., 2]
    ru = np.where(obs, u - uv[..., 0], 0.0)
    rv = np.where(obs, v - uv[..., 1], 0.0)
    du = (K[None, :, 0, :] - u[..., None] * K[None, :, 2, :]) / p[..., 2:3]
    dv = (K[None, :, 1, :] - v[..., None] * K[None, :, 2, :]) / p[..., 2:3]
    du, dv = np.where(obs[..., None], du, 0.0), np.where(obs[..., None], dv, 0.0)
    sw = obs.astype(np.float64)
    if loss is None:
        E = 0.5 * (np.sum(ru * ru) + np.sum(rv * rv))
    else:
        rho, w = rb.rho_w(ru * ru + rv * rv, loss, loss_px)
        E = np.sum(np.where(obs, rho, 0.0))
        sw = np.where(obs, np.sqrt(w), 0.0)
        ru, rv, du, dv = sw * ru, sw * rv, sw[..., None] * du, sw[..., None] * dv
    a = np.einsum("cji,ncj->nci", R, du)
    b = np.einsum("cji,ncj->nci", R, dv)
    ju = [np.cross(y, du), du]
    jv = [np.cross(y, dv), dv]
    if NI >= 1:
        ju.append((sw * np.where(obs, u - K[None, :, 0, 2], 0.0))[..., None])
        jv.append((sw * np.where(obs, v - K[None, :, 1, 2], 0.0))[..., None])
    if NI == 3:
        z = np.zeros_like(sw)
        ju.append(np.stack([sw, z], axis=-1))
        jv.append(np.stack([z, sw], axis=-1))
    return dict(E=E, ru=ru, rv=rv, a=a, b=b, ju=np.concatenate(ju, axis=-1), jv=np.concatenate(jv, axis=-1))


def terms(X, uv, K, R, t, held, mu, ifree=None, NI=0, K0=None, sf=np.inf, sc=np.inf, loss=None, loss_px=LOSS_PX):
    """rig_robust_np.terms with the intrinsic columns and the prior: the same dict (E includes the prior), plus cam, row (M,) the
    layout and scale (M,) the columns' weights in |d|_inf."""
    N, C = uv.shape[:2]
    ifree = np.zeros(C, bool) if ifree is None else ifree
    K0 = K if K0 is None else K0
    cam, row = columns(held, ifree, NI)
    M = cam.size
    J = jacobian(X, uv, K, R, t, NI, loss, loss_px)
    ru, rv, a, b, ju, jv = J["ru"], J["rv"], J["a"], J["b"], J["ju"], J["jv"]
    V = np.einsum("nci,ncj->nij", a, a) + np.einsum("nci,ncj->nij", b, b)
    gp = np.einsum("nci,nc->ni", a, ru) + np.einsum("nci,nc->ni", b, rv)
    U = np.einsum("nci,ncj->cij", ju, ju) + np.einsum("nci,ncj->cij", jv, jv)
    gc = np.einsum("nci,nc->ci", ju, ru) + np.einsum("nci,nc->ci", jv, rv)
    W = np.einsum("nci,ncj->ncij", ju, a) + np.einsum("nci,ncj->ncij", jv, b)   # (n, C, 6 + NI, 3)
    if NI:
        # the prior's rows: residual delta / sigma, derivative 1 / sigma
        d = deltas(K, K0)
        sig = np.array([sf, sc, sc])
        for c in np.flatnonzero(ifree):
            for k in range(NI):
                U[c, 6 + k, 6 + k] += 1.0 / (sig[k] * sig[k])
                gc[c, 6 + k] += d[c, k] / sig[k] / sig[k]
    dV = np.einsum("nii->ni", V)
    Vd = V + mu * dV[:, :, None] * np.eye(3)[None]
    Vi = np.linalg.inv(Vd)
    Wf = np.ascontiguousarray(W[:, cam, row]).reshape(N, M, 3)
    S = -np.einsum("nik,nkl,njl->ij", Wf, Vi, Wf)
    gcf = gc[cam, row]
    g = gcf - np.einsum("nik,nkl,nl->i", Wf, Vi, gp)
    dU = U[cam, row, row]
    for c in range(C):
        m = np.flatnonzero(cam == c)
        if m.size:
            Uc = U[c][np.ix_(row[m], row[m])]
            S[m[0]:m[-1] + 1, m[0]:m[-1] + 1] += Uc + mu * np.diag(np.diag(Uc))
    scale = np.where(row >= 7, 1.0 / K[cam, 0, 0], 1.0) if M else np.ones(0)
    return dict(E=J["E"] + prior(K, K0, ifree, NI, sf, sc), S=S, g=g, free=np.flatnonzero(~held), Wf=Wf, Vd=Vd, Vi=Vi, gp=gp, gc=gcf,
                dU=dU, dV=dV, cam=cam, row=row, scale=scale)


def apply_step(K, R, t, dc, cam, row):
    """The trial cameras of the step dc in the layout (cam, row)."""
    Kn, Rn, tn = K.copy(), R.copy(), t.copy()
    for c in np.unique(cam):
        d = np.zeros(9)
        m = cam == c
        d[row[m]] = dc[m]
        if (row[m] < 6).any():
            Rn[c] = rr.rodrigues(d[:3]) @ R[c]
            tn[c] = t[c] + d[3:6]
        if (row[m] >= 6).any():
            e = np.exp(d[6])
            Kn[c, 0, 0], Kn[c, 0, 1], Kn[c, 1, 1] = K[c, 0, 0] * e, K[c, 0, 1] * e, K[c, 1, 1] * e
            Kn[c, 0, 2], Kn[c, 1, 2] = K[c, 0, 2] + d[7], K[c, 1, 2] + d[8]
    return Kn, Rn, tn


def trial(X, uv, K, R, t, held, mu, ifree=None, NI=0, K0=None, sf=np.inf, sc=np.inf, loss=None, loss_px=LOSS_PX):
    """rig_robust_np.trial with the intrinsic unknowns: also K, the trial intrinsics; Et includes their prior."""
    C = uv.shape[1]
    ifree = np.zeros(C, bool) if ifree is None else ifree
    K0 = K if K0 is None else K0
    T = terms(X, uv, K, R, t, held, mu, ifree, NI, K0, sf, sc, loss, loss_px)
    out = dict(terms=T, mu=mu, bad=False)
    try:
        Lc = np.linalg.cholesky(T["S"])
    except np.linalg.LinAlgError:
        out["bad"] = True
        return out
    dc = -np.linalg.solve(Lc.T, np.linalg.solve(Lc, T["g"]))
    dp = np.einsum("nkl,nl->nk", T["Vi"], -T["gp"] - np.einsum("nik,i->nk", T["Wf"], dc))
    dg = dc @ T["gc"] + np.sum(dp * T["gp"])
    dDd = np.sum(dc * dc * T["dU"]) + np.sum(dp * dp * T["dV"])
    pred = 0.5 * (mu * dDd - dg)
    dmax = max(np.abs(dc * T["scale"]).max(), np.abs(dp).max())
    Kn, Rn, tn = apply_step(K, R, t, dc, T["cam"], T["row"])
    Xn = X + dp
    out.update(dc=dc, dp=dp, dg=dg, dDd=dDd, pred=pred, dmax=dmax, K=Kn, R=Rn, t=tn, X=Xn,
               Et=cost(Xn, uv, Kn, Rn, tn, K0, ifree, NI, sf, sc, loss, loss_px))
    return out


def solve(prob, K, Rt, max_iter=10, mu0=rr.LM_MU0, ftol=rr.LM_FTOL, xtol=rr.LM_XTOL, trace=None, loss=None, loss_px=LOSS_PX,
          intrinsics=None, focal_sigma=None, centre_sigma_px=None, intrinsics_held=()):
    """rig_robust_np.solve with the intrinsic unknowns -> its dict (cost includes the prior; rms_before / rms_after stay the plain
    reprojection rms) and intrinsics, K (C,3,3) the refined intrinsics, k_moved (C,3) phi, dcx, dcy (zeros where held), cost_prior."""
    K, Rt = np.asarray(K, np.float64), np.asarray(Rt, np.float64)
    C = K.shape[0]
    NI, sf, sc = check(intrinsics, focal_sigma, centre_sigma_px, C)
    X, uv, held = prob["X"].copy(), prob["uv"], prob["held"]
    ifree = free_intrinsics(held, NI, intrinsics_held)
    K0, K = K, K.copy()
    R, t = Rt[:, :, :3].copy(), Rt[:, :, 3].copy()
    n_obs = int((~np.isnan(uv[:, :, 0])).sum())
    out = dict(Rt=Rt.copy(), X=X, cost=[], trials=[], stop=prob["stop"], n_points=X.shape[0], n_obs=n_obs, gauge=[],
               rms_before=float("nan"), rms_after=float("nan"), intrinsics=intrinsics, K=K.copy(), k_moved=np.zeros((C, 3)),
               cost_prior=0.0, ifree=ifree)
    if n_obs:
        E = cost(X, uv, K, R, t, K0, ifree, NI, sf, sc, loss, loss_px)
        out["cost"].append(E)
        out["rms_before"] = out["rms_after"] = float(np.sqrt(2.0 * rr.cost(X, uv, K, R, t) / n_obs))
    if prob["stop"] is not None:
        return out
    free = np.flatnonzero(~held)
    c_in = -np.einsum("cji,cj->ci", R, t)
    L0 = np.linalg.norm(c_in[free[0]] - c_in[0])
    mu, stop = mu0, "max_iter"
    for _ in range(int(max_iter)):
        tr = trial(X, uv, K, R, t, held, mu, ifree, NI, K0, sf, sc, loss, loss_px)
        tr["E"] = E
        if trace is not None:
            trace.append(tr)
        if tr["bad"]:
            out["trials"].append(0)
            out["cost"].append(E)
            mu *= 10.0
            continue
        if tr["dmax"] < xtol:
            stop = "xtol"
            break
        if tr["pred"] < ftol * E:
            stop = "ftol"
            break
        Kn, Rn, tn, Xn, Et = tr["K"], tr["R"], tr["t"], tr["X"], tr["Et"]
        acc = Et < E
        out["trials"].append(int(acc))
        if acc:
            X, t = rr.rescale(Xn, Rn, tn, held, L0)
            R, K = Rn, Kn
            out["gauge"].append(abs(cost(X, uv, K, R, t, K0, ifree, NI, sf, sc, loss, loss_px) - Et) / Et)
            small = E - Et < ftol * E
            E = Et
            out["cost"].append(E)
            mu /= 10.0
            if small:
                stop = "ftol"
                break
        else:
            out["cost"].append(E)
            mu *= 10.0
    E_plain = E if loss is None and NI == 0 else rr.cost(X, uv, K, R, t)
    out.update(Rt=np.concatenate([R, t[:, :, None]], axis=2), X=X, stop=stop, K=K, rms_after=float(np.sqrt(2.0 * E_plain / n_obs)),
               cost_prior=prior(K, K0, ifree, NI, sf, sc))
    if NI:
        out["k_moved"] = np.where(ifree[:, None], deltas(K, K0), 0.0) * np.array([1.0, NI == 3, NI == 3])
    if loss is not None:
        w = rb.weights(X, uv, K, R, t, loss, loss_px)
        with np.errstate(invalid="ignore", divide="ignore"):
            dw = (w < 0.5).sum(axis=0) / (~np.isnan(w)).sum(axis=0)
        out.update(loss=loss, loss_px=float(loss_px), weights=w, downweighted=dw)
    return out


def refine(cand, K, Rt, max_iter=10, max_px=97.88, min_score=0.1, min_views=2, min_cam_obs=100, ftol=rr.LM_FTOL, xtol=rr.LM_XTOL,
           loss=None, loss_px=LOSS_PX, intrinsics=None, focal_sigma=None, centre_sigma_px=None, intrinsics_held=()):
    """rig_robust_np.refine with the intrinsic unknowns: the problem is built on the input K, as it is without them."""
    prob = rr.build_problem(cand, K, Rt, max_px, min_score, min_views, min_cam_obs)
    out = solve(prob, K, Rt, max_iter, ftol=ftol, xtol=xtol, loss=loss, loss_px=loss_px, intrinsics=intrinsics, focal_sigma=focal_sigma,
                centre_sigma_px=centre_sigma_px, intrinsics_held=intrinsics_held)
    out.update(held=prob["held"], obs_per_camera=prob["obs_per_camera"], rows=prob["rows"])
    return out
