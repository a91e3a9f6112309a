"""NumPy restatement of the rig refinement with a robust loss (rig_refine.refine_rigs(loss=...), rig_init.calibrate_rigs(polish_loss=...),
csrc/mvmc_rigfit.hip: mvmc_rig_accumulate_robust, mvmc_rig_step_robust, mvmc_rig_weights).  Everything the loss does not touch is
tests/rig_refine_np.py's: the problem, the gauge rescale, the Levenberg-Marquardt rules.

The loss.  For an observation with residual (ru, rv): s^2 = ru^2 + rv^2, delta = loss_px > 0,
  huber   rho = 1/2 s^2, w = 1 for s <= delta; otherwise rho = delta (s - 1/2 delta), w = delta / s;
  cauchy  rho = 1/2 delta^2 log1p(s^2 / delta^2), w = 1 / (1 + s^2 / delta^2).
E = sum rho replaces 1/2 sum r^2 wherever the iteration reads a cost.  At every linearisation the observation's point rows a, b, its
camera rows ju, jv and its residual are multiplied by sqrt(w) (iteratively reweighted least squares, no second-order correction);
the normal equations, the Schur reduction, the step and the predicted reduction are then those of the weighted model.  Both weights
are strictly positive.  loss=None is rig_refine_np's arithmetic, operation for operation.
"""
import numpy as np

import rig_refine_np as rr

LOSSES = (None, "huber", "cauchy")
LOSS_PX = 6.0


def rho_w(s2, loss, loss_px):
    """s2: squared residual lengths -> (rho, w) of the loss, elementwise."""
    s2 = np.asarray(s2, np.float64)
    if loss is None:
        return 0.5 * s2, np.ones_like(s2)
    d = float(loss_px)
    if loss == "huber":
        s = np.sqrt(s2)
        inside = s <= d
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(inside, 0.5 * s2, d * (s - 0.5 * d)), np.where(inside, 1.0, d / s)
    if loss == "cauchy":
        q = s2 / (d * d)
        return 0.5 * d * d * np.log1p(q), 1.0 / (1.0 + q)
    raise ValueError(f"loss {loss!r}")


def _s2(X, uv, K, R, t):
    r = rr.project(K, R, t, X) - uv
    return r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]          # NaN where not observed


def cost(X, uv, K, R, t, loss=None, loss_px=LOSS_PX):
    if loss is None:
        return rr.cost(X, uv, K, R, t)
    return np.nansum(rho_w(_s2(X, uv, K, R, t), loss, loss_px)[0])


def weights(X, uv, K, R, t, loss=None, loss_px=LOSS_PX):
    """-> (N, C): w of every observation at (X, cameras), NaN where there is none."""
    s2 = _s2(X, uv, K, R, t)
    return np.where(np.isnan(s2), np.nan, rho_w(np.nan_to_num(s2), loss, loss_px)[1])


def terms(X, uv, K, R, t, held, mu, loss=None, loss_px=LOSS_PX):
    """rig_refine_np.terms of the weighted model: the same dict, E = sum rho."""
    N, C = uv.shape[:2]
    free = np.flatnonzero(~held)
    M = 6 * free.size
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
    if loss is None:
        E = 0.5 * (np.sum(ru * ru) + np.sum(rv * rv))
    else:
        rho, w = rho_w(ru * ru + rv * rv, loss, loss_px)
        E = np.sum(np.where(obs, rho, 0.0))
        sw = np.sqrt(w)
        ru, rv, du, dv = sw * ru, sw * rv, sw[..., None] * du, sw[..., None] * dv
    a = np.einsum("cji,ncj->nci", R, du)          # point rows of the Jacobian
    b = np.einsum("cji,ncj->nci", R, dv)
    ju = np.concatenate([np.cross(y, du), du], axis=-1)   # camera rows (n, C, 6)
    jv = np.concatenate([np.cross(y, dv), dv], axis=-1)
    V = np.einsum("nci,ncj->nij", a, a) + np.einsum("nci,ncj->nij", b, b)
    gp = np.einsum("nci,nc->ni", a, ru) + np.einsum("nci,nc->ni", b, rv)
    U = np.einsum("nci,ncj->cij", ju, ju) + np.einsum("nci,ncj->cij", jv, jv)
    gc = np.einsum("nci,nc->ci", ju, ru) + np.einsum("nci,nc->ci", jv, rv)
    W = np.einsum("nci,ncj->ncij", ju, a) + np.einsum("nci,ncj->ncij", jv, b)   # (n, C, 6, 3)
    dV = np.einsum("nii->ni", V)
    Vd = V + mu * dV[:, :, None] * np.eye(3)[None]
    Vi = np.linalg.inv(Vd)
    Wf = W[:, free].reshape(N, M, 3)
    S = -np.einsum("nik,nkl,njl->ij", Wf, Vi, Wf)
    g = gc[free].reshape(M) - np.einsum("nik,nkl,nl->i", Wf, Vi, gp)
    dU = np.zeros(M)
    for s, c in enumerate(free):
        S[6 * s:6 * s + 6, 6 * s:6 * s + 6] += U[c] + mu * np.diag(np.diag(U[c]))
        dU[6 * s:6 * s + 6] = np.diag(U[c])
    return dict(E=E, S=S, g=g, free=free, Wf=Wf, Vd=Vd, Vi=Vi, gp=gp, gc=gc[free].reshape(M), dU=dU, dV=dV)


def trial(X, uv, K, R, t, held, mu, loss=None, loss_px=LOSS_PX):
    """rig_refine_np.trial with the loss: the step of the weighted model, Et = the robust cost of the trial state."""
    T = terms(X, uv, K, R, t, held, mu, loss, loss_px)
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
    dmax = max(np.abs(dc).max(), np.abs(dp).max())
    Rn, tn = R.copy(), t.copy()
    for s, c in enumerate(T["free"]):
        Rn[c] = rr.rodrigues(dc[6 * s:6 * s + 3]) @ R[c]
        tn[c] = t[c] + dc[6 * s + 3:6 * s + 6]
    Xn = X + dp
    out.update(dc=dc, dp=dp, dg=dg, dDd=dDd, pred=pred, dmax=dmax, R=Rn, t=tn, X=Xn, Et=cost(Xn, uv, K, Rn, tn, loss, loss_px))
    return out


def solve(prob, K, Rt, max_iter=10, mu0=rr.LM_MU0, ftol=rr.LM_FTOL, xtol=rr.LM_XTOL, trace=None, loss=None, loss_px=LOSS_PX):
    """rig_refine_np.solve with the loss -> its dict; cost holds the robust E, rms_before / rms_after stay the PLAIN rms over the
    problem's observations, and with a loss the dict also carries loss, loss_px, weights (N, C) at the final state and downweighted
    (C,): the share of each camera's observations with w < 0.5 (NaN for a camera without any)."""
    K, Rt = np.asarray(K, np.float64), np.asarray(Rt, np.float64)
    X, uv, held = prob["X"].copy(), prob["uv"], prob["held"]
    R, t = Rt[:, :, :3].copy(), Rt[:, :, 3].copy()
    n_obs = int((~np.isnan(uv[:, :, 0])).sum())
    out = dict(Rt=Rt.copy(), X=X, cost=[], trials=[], stop=prob["stop"], n_points=X.shape[0], n_obs=n_obs, gauge=[],
               rms_before=float("nan"), rms_after=float("nan"))
    if n_obs:
        E = cost(X, uv, K, R, t, loss, loss_px)
        out["cost"].append(E)
        out["rms_before"] = out["rms_after"] = float(np.sqrt(2.0 * rr.cost(X, uv, K, R, t) / n_obs))
    if prob["stop"] is not None:
        return out
    free = np.flatnonzero(~held)
    c_in = -np.einsum("cji,cj->ci", R, t)
    L0 = np.linalg.norm(c_in[free[0]] - c_in[0])
    mu, stop = mu0, "max_iter"
    for _ in range(int(max_iter)):
        tr = trial(X, uv, K, R, t, held, mu, loss, loss_px)
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
        Rn, tn, Xn, Et = tr["R"], tr["t"], tr["X"], tr["Et"]
        acc = Et < E
        out["trials"].append(int(acc))
        if acc:
            X, t = rr.rescale(Xn, Rn, tn, held, L0)
            R = Rn
            out["gauge"].append(abs(cost(X, uv, K, R, t, loss, loss_px) - Et) / Et)
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
    E_plain = E if loss is None else rr.cost(X, uv, K, R, t)
    out.update(Rt=np.concatenate([R, t[:, :, None]], axis=2), X=X, stop=stop, rms_after=float(np.sqrt(2.0 * E_plain / n_obs)))
    if loss is not None:
        w = weights(X, uv, K, R, t, loss, loss_px)
        with np.errstate(invalid="ignore", divide="ignore"):
            dw = (w < 0.5).sum(axis=0) / (~np.isnan(w)).sum(axis=0)
        out.update(loss=loss, loss_px=float(loss_px), weights=w, downweighted=dw)
    return out


def refine(cand, K, Rt, max_iter=10, max_px=97.88, min_score=0.1, min_views=2, min_cam_obs=100, ftol=rr.LM_FTOL, xtol=rr.LM_XTOL,
           loss=None, loss_px=LOSS_PX):
    """rig_refine_np.refine with the loss: the two max_px gates stay in front, as they are."""
    prob = rr.build_problem(cand, K, Rt, max_px, min_score, min_views, min_cam_obs)
    out = solve(prob, K, Rt, max_iter, ftol=ftol, xtol=xtol, loss=loss, loss_px=loss_px)
    out.update(held=prob["held"], obs_per_camera=prob["obs_per_camera"], rows=prob["rows"])
    return out
