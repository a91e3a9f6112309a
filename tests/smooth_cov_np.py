"""NumPy restatement of the trajectory smoother's per-frame covariance (multiview_motion_capture_amd/smoothing.py: covariance="joints";
csrc/mvmc_smooth_cov.hip), on top of tests/smooth_np.py.  The device is gated against this file.

At the returned trajectory x the Laplace / Gauss-Newton covariance of E is sigma^2 A^-1, A = blockdiag(J_t^T J_t) + the exact prior
Hessian (smooth_np.data_terms / prior_mats / prior_weights: the matrix of smooth_np.banded_solve).  At mu = 0 that matrix is singular
on every identity: the Rz angles of the two knees are stage-1 columns (the knees are ancestors of the ankles) but turn the shin about
its own axis and move no joint, and the prior sees differences only, so their common mode over the frames has no curvature at all.
The covariance is therefore taken of A + MU diag A with a small MU, the damping the solver itself carries (smoothing.COV_MU): the
joints' covariances do not depend on it to first order, the two twist angles get a large, finite variance.  dense_A / dense_inverse
build and invert that matrix densely; banded_blocks is the kernel's algorithm: a block-banded Cholesky (39 x 39 blocks, two
sub-diagonals), then the backward recursion Sigma L = L^-T read column by column (Takahashi's selected inverse) for the diagonal blocks Sigma_tt alone.
Per row: C_K = D_K Sigma_tt D_K^T with D_K = d X_K / d x_t of all 18 joints (joint_jacobians), p = diag Sigma_tt,
e_t = tr(Sigma_tt J_t^T J_t); per identity edof = sum e_t, n_res = 2 x the (selected view, observed joint) pairs with a non-zero score,
noise_px = sqrt(2 E_data / (n_res - edof)); the e_t use the undamped J_t^T J_t.
"""
import numpy as np
from scipy.linalg import solve_triangular

import oracle_np as o
import smooth_np as sm

K = sm.K
MU = 1e-8          # multiview_motion_capture_amd/smoothing.py: COV_MU


def dense_A(H, w, mu=MU):
    """H (m,39,39) the rows' J^T J, w the four prior weights -> A + mu diag A (39 m, 39 m)."""
    m = H.shape[0]
    wv, wa = sm.prior_weights(w)
    Dv, Da = sm.prior_mats(m)
    A = np.kron(Dv.T @ Dv, np.diag(wv)) + np.kron(Da.T @ Da, np.diag(wa))
    for r in range(m):
        A[r * K:(r + 1) * K, r * K:(r + 1) * K] += H[r]
    A[np.diag_indices_from(A)] *= 1.0 + mu
    return A


def dense_inverse(H, w, mu=MU):
    """-> (Sigma (39 m, 39 m) = (A + mu diag A)^-1 by np.linalg.inv, its diagonal blocks (m,39,39))."""
    S = np.linalg.inv(dense_A(H, w, mu))
    m = H.shape[0]
    return S, np.array([S[r * K:(r + 1) * K, r * K:(r + 1) * K] for r in range(m)])


def banded_factor(H, w, mu=MU):
    """The block-banded Cholesky of A + mu diag A (mvmc_smooth_sweep.h) -> T (m,39,39) lower, L1, L2 (m,39,39) = L_{t+1,t}, L_{t+2,t}
    (zero beyond the last row), or None when a pivot block is not positive definite."""
    m = H.shape[0]
    wv, wa = sm.prior_weights(w)
    Dv, Da = sm.prior_mats(m)
    Hv, Ha = Dv.T @ Dv, Da.T @ Da
    blk = lambda i, j: np.diag(wv * Hv[i, j] + wa * Ha[i, j])
    T, L1, L2 = np.zeros((m, K, K)), np.zeros((m, K, K)), np.zeros((m, K, K))
    for t in range(m):
        S = H[t] + blk(t, t)
        S[np.diag_indices(K)] *= 1.0 + mu
        if t >= 1:
            S = S - L1[t - 1] @ L1[t - 1].T
        if t >= 2:
            S = S - L2[t - 2] @ L2[t - 2].T
        try:
            T[t] = np.linalg.cholesky(S)
        except np.linalg.LinAlgError:
            return None
        if t + 1 < m:
            N1 = blk(t + 1, t)
            if t >= 1:
                N1 = N1 - L2[t - 1] @ L1[t - 1].T
            L1[t] = solve_triangular(T[t], N1.T, lower=True).T          # N1 T^-T
        if t + 2 < m:
            L2[t] = solve_triangular(T[t], blk(t + 2, t).T, lower=True).T
    return T, L1, L2


def _right(G, T):
    """G T^-1, T lower triangular."""
    return solve_triangular(T, G.T, lower=True, trans="T").T


def banded_blocks(H, w, mu=MU):
    """The diagonal blocks Sigma_tt (m,39,39) of (A + mu diag A)^-1 by the kernel's backward recursion over the banded factor, or None."""
    f = banded_factor(H, w, mu)
    if f is None:
        return None
    T, L1, L2 = f
    m = H.shape[0]
    out = np.zeros((m, K, K))
    S11 = S21 = S22 = np.zeros((K, K))
    for t in range(m - 1, -1, -1):
        X1 = -_right(S11 @ L1[t] + S21.T @ L2[t], T[t])                   # Sigma_{t+1,t}
        X2 = -_right(S21 @ L1[t] + S22 @ L2[t], T[t])                     # Sigma_{t+2,t}
        Ti = _right(np.eye(K), T[t])
        St = _right(Ti.T - X1.T @ L1[t] - X2.T @ L2[t], T[t])
        out[t] = 0.5 * (St + St.T)       # the antisymmetric part of a rounding error grows from row to row (1.85 x per row measured)
        S11, S21, S22 = out[t], X1, S11
    return out


def fk(p):
    return o.forward_kinematics(p[:3], p[3:57], p[57:])[0]


def joint_jacobians(p):
    """One row's 68 parameters -> D (18,3,39) = d X_K / d x over the stage-1 columns: the identity for the root translation,
    cross(axis, X_K - X_a) for the Euler angles of every strict ancestor a of K (axes in the global frame: trf_np.ik_jacobian's)."""
    bone_dirs, _ = o.skeleton_constants()
    euler = np.asarray(p[3:57], float).reshape(18, 3)
    pos, G = o.forward_kinematics(p[:3], euler, p[57:], bone_dirs)
    Rg = G[:, :3, :3]
    par = o.SKEL_PARENTS
    full = np.zeros((18, 3, 57))
    for k in range(18):
        full[k, :, 0:3] = np.eye(3)
        j = k
        while j != 0:
            a = par[j]
            Rp = Rg[par[a]] if par[a] >= 0 else np.eye(3)
            ca, sa = np.cos(euler[a, 0]), np.sin(euler[a, 0])
            cb, sb = np.cos(euler[a, 1]), np.sin(euler[a, 1])
            axes = [Rp @ np.array([1.0, 0, 0]), Rp @ np.array([0, ca, sa]), Rp @ np.array([sb, -sa * cb, ca * cb])]
            for c in range(3):
                full[k, :, 3 + 3 * a + c] = np.cross(axes[c], pos[k] - pos[a])
            j = a
    return full[:, :, sm.COLS]


def n_residuals(obs):
    """obs per frame ((V,16,3) or None) -> 2 x the (view, joint) pairs whose score is not zero."""
    return 2 * sum(int(np.count_nonzero(ob[:, :, 2])) for ob in obs if ob is not None)


def covariance(x, obs, prs, w, noise_px=None, blocks=None, mu=MU):
    """x (m,68) the trajectory, obs / prs per frame (smooth_np.data_terms), w the four weights -> dict(sigma (m,39,39) the diagonal
    blocks of A^-1 (``blocks``: "dense" np.linalg.inv, default the banded recursion), jcov (m,18,3,3), pvar (m,39) at unit variance,
    e (m,), edof, n_res, E_data, noise_px, joint_cov (m,18,3,3) = noise_px^2 jcov, joint_sigma (m,18), param_sigma (m,39))."""
    Ed, _, H, _ = sm.data_terms(x, obs, prs)
    S = dense_inverse(H, w, mu)[1] if blocks == "dense" else banded_blocks(H, w, mu)
    m = x.shape[0]
    D = np.array([joint_jacobians(x[r]) for r in range(m)])                       # (m,18,3,39)
    jcov = np.einsum("mkap,mpq,mkbq->mkab", D, S, D)
    pvar = np.array([np.diag(S[r]) for r in range(m)])
    e = np.array([np.sum(S[r] * H[r]) for r in range(m)])
    edof, n_res = float(e.sum()), n_residuals(obs)
    if noise_px is None:
        noise_px = np.sqrt(2.0 * Ed / (n_res - edof)) if n_res - edof > 0 else np.nan
    s2 = noise_px * noise_px
    return dict(sigma=S, H=H, jcov=jcov, pvar=pvar, e=e, edof=edof, n_res=n_res, E_data=Ed, noise_px=float(noise_px),
                joint_cov=s2 * jcov, joint_sigma=np.sqrt(s2 * np.trace(jcov, axis1=-2, axis2=-1)), param_sigma=np.sqrt(s2 * pvar))


def problems(views, Ps, records):
    """The data model of smooth_np.smooth, one sequence: views[f][c] (n,17,3), Ps (C,3,4), records (dicts) -> per record with two
    frames or more (obs, prs) over its frames f0..f1 (None where the frame is missing or has no selected view), else None."""
    probs = [(0, int(f), r, np.asarray(rec["joints"][k], np.float64)) for r, rec in enumerate(records) for k, f in enumerate(rec["frames"])]
    sel, _, _ = sm.bf.select(probs, [views], [Ps])
    out, at = [], 0
    for rec in records:
        fr = np.asarray(rec["frames"])
        rows = np.arange(at, at + len(fr))
        at += len(fr)
        if len(fr) < 2:
            out.append(None)
            continue
        m = int(fr[-1] - fr[0] + 1)
        obs, prs = [None] * m, [None] * m
        for k, f in enumerate(fr):
            ob, pr = sm.bf.observations(sel[rows[k]], views[int(f)], Ps)
            if len(ob):
                obs[f - fr[0]], prs[f - fr[0]] = ob, pr
        out.append((obs, prs))
    return out
