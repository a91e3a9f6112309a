"""NumPy restatement of the live smoother's covariance (multiview_motion_capture_amd/live_smoothing.py: covariance="joints";
csrc/mvmc_smooth_window_cov.hip), on top of tests/live_smooth_np.py and tests/smooth_cov_np.py.  The device is gated against this file.

At the end of a tick an identity has n rows: the last m = min(W, n) free, the h = min(2, n - m) before them frozen.  A_w is the matrix
the window's LM step factors at the rows' final values: live_smooth_np.window_system's H (the free rows' J^T J; the weighted ones
inside smooth_robust_np.robust), Hv and Ha (the exact Hessian of every prior term whose stencil touches a free row, the history held
fixed, rows and columns of the free rows).  Sigma = (A_w + MU diag A_w)^-1, and the emitted free row e gets Sigma_ee: C_K = D_K Sigma_ee
D_K^T per skeleton joint (smooth_cov_np.joint_jacobians), p = diag Sigma_ee; edof = sum_t tr(Sigma_tt H_t) and n_res over the FREE rows,
noise_px = sqrt(2 E_data / (n_res - edof)).  This is the covariance CONDITIONAL on the frozen history.  dense_window_A / window_cov(
blocks="dense") build and invert the matrix densely; the default is the kernel's algorithm: the block-banded Cholesky of the window's
matrix, then smooth_cov_np's backward recursion from row m - 1, which may stop at row e.
"""
import numpy as np
from scipy.linalg import solve_triangular

import live_smooth_np as ls
import smooth_cov_np as sc

K = sc.K
MU = sc.MU


def dense_window_A(H, Hv, Ha, wv, wa, mu=MU):
    """H (m,39,39), Hv, Ha (m,m) of the free rows, wv, wa (39,) -> A_w + mu diag A_w (39 m, 39 m)."""
    m = H.shape[0]
    A = np.kron(Hv, np.diag(wv)) + np.kron(Ha, np.diag(wa))
    for r in range(m):
        A[r * K:(r + 1) * K, r * K:(r + 1) * K] += H[r]
    A[np.diag_indices_from(A)] *= 1.0 + mu
    return A


def window_factor(H, Hv, Ha, wv, wa, mu=MU):
    """smooth_cov_np.banded_factor on the window's matrix (the prior's coefficients are Hv, Ha of the free rows, which hold the
    history's share) -> T, L1, L2 (m,39,39), or None when a pivot block is not positive definite."""
    m = H.shape[0]
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
        if not np.all(np.isfinite(T[t])):
            return None
        if t + 1 < m:
            N1 = blk(t + 1, t)
            if t >= 1:
                N1 = N1 - L2[t - 1] @ L1[t - 1].T
            L1[t] = solve_triangular(T[t], N1.T, lower=True).T
        if t + 2 < m:
            L2[t] = solve_triangular(T[t], blk(t + 2, t).T, lower=True).T
    return T, L1, L2


def window_blocks(H, Hv, Ha, wv, wa, stop=0, mu=MU):
    """The diagonal blocks Sigma_tt, t = m - 1 .. stop, of (A_w + mu diag A_w)^-1 by smooth_cov_np.banded_blocks' recursion over the
    window's factor -> (m,39,39) with NaN in the rows below ``stop``, or None."""
    f = window_factor(H, Hv, Ha, wv, wa, mu)
    if f is None:
        return None
    T, L1, L2 = f
    m = H.shape[0]
    out = np.full((m, K, K), np.nan)
    S11 = S21 = S22 = np.zeros((K, K))
    for t in range(m - 1, stop - 1, -1):
        X1 = -sc._right(S11 @ L1[t] + S21.T @ L2[t], T[t])
        X2 = -sc._right(S21 @ L1[t] + S22 @ L2[t], T[t])
        Ti = sc._right(np.eye(K), T[t])
        St = sc._right(Ti.T - X1.T @ L1[t] - X2.T @ L2[t], T[t])
        out[t] = 0.5 * (St + St.T)
        S11, S21, S22 = out[t], X1, S11
    return out


def window_cov(x, h, obs, prs, w, e, noise_px=None, blocks=None, full=True, mu=MU):
    """x (h + m, 68) the window's rows at the end of the tick (the first h frozen), obs / prs per row (None for the history), w the
    four weights, e the emitted row's index among the free rows -> dict(status 0 / 1, sigma (39,39) = Sigma_ee, jcov (18,3,3), pvar
    (39,) at unit variance, edof, n_res (NaN without ``full``, as the device leaves them), E_data, noise_px, joint_cov (18,3,3),
    joint_sigma (18,), param_sigma (39,), m).  blocks="dense": np.linalg.inv of the whole matrix; default the banded recursion, down
    to row 0 when ``full`` and to row e otherwise."""
    Ed, _, H, _, Hv, Ha, wv, wa = ls.window_system(x, h, obs, prs, w)
    m = H.shape[0]
    if blocks == "dense":
        S = np.linalg.inv(dense_window_A(H, Hv, Ha, wv, wa, mu))
        S = np.array([S[r * K:(r + 1) * K, r * K:(r + 1) * K] for r in range(m)])
    else:
        S = window_blocks(H, Hv, Ha, wv, wa, 0 if full else e, mu)
    if S is None:
        nan = np.nan
        return dict(status=1, sigma=np.full((K, K), nan), jcov=np.full((18, 3, 3), nan), pvar=np.full(K, nan), edof=nan, n_res=nan,
                    E_data=Ed, noise_px=nan if noise_px is None else float(noise_px), joint_cov=np.full((18, 3, 3), nan),
                    joint_sigma=np.full(18, nan), param_sigma=np.full(K, nan), m=m)
    D = sc.joint_jacobians(x[h + e])                                        # (18,3,39)
    jcov = np.einsum("kap,pq,kbq->kab", D, S[e], D)
    pvar = np.diag(S[e]).copy()
    if full:
        edof, n_res = float(sum(np.sum(S[r] * H[r]) for r in range(m))), float(sc.n_residuals(obs[h:]))
    else:
        edof, n_res = np.nan, np.nan
    if noise_px is None:
        noise_px = np.sqrt(2.0 * Ed / (n_res - edof)) if n_res - edof > 0 else np.nan
    s2 = noise_px * noise_px
    return dict(status=0, sigma=S[e], jcov=jcov, pvar=pvar, edof=edof, n_res=n_res, E_data=Ed, noise_px=float(noise_px),
                joint_cov=s2 * jcov, joint_sigma=np.sqrt(s2 * np.trace(jcov, axis1=-2, axis2=-1)), param_sigma=np.sqrt(s2 * pvar), m=m)


def one_row():
    """The entry of an identity with one row (nothing was solved): status 2, NaN."""
    nan = np.nan
    return dict(status=2, jcov=np.full((18, 3, 3), nan), pvar=np.full(K, nan), edof=nan, n_res=nan, E_data=0.0, noise_px=nan,
                joint_cov=np.full((18, 3, 3), nan), joint_sigma=np.full(18, nan), param_sigma=np.full(K, nan), m=1)


class Stream(ls.Stream):
    """live_smooth_np.Stream whose tick also yields ``cov``: track_id -> window_cov of the emitted row at the end of the tick.
    ``rows``: (track_id, first frame) -> {row: (joint_sigma, param_sigma, noise_px)} as emitted, for the records."""

    def __init__(self, P, window=24, lag=8, n_iter=2, w=(1e4, 1e4, 1e4, 1e4), noise_px=None, blocks=None):
        super().__init__(P, window, lag, n_iter, w)
        self.noise_px, self.blocks = noise_px, blocks
        self.rows = {}

    def cov_at(self, tid, f, x=None):
        """The expectation for identity ``tid`` after the tick of frame f, or None when the tick emits no row of it.  x: the window's
        h + m rows to evaluate at (default: this stream's own)."""
        idn = self.ids[tid]
        r = f - self.lag - idn.f0
        if r < 0:
            return None
        n = len(idn.x)
        m = min(self.W, n)
        h = min(2, n - m)
        if n < 2:
            c = one_row()
            if self.noise_px is not None:
                c["noise_px"] = float(self.noise_px)
            return c
        rows = np.array(idn.x[n - m - h:]) if x is None else np.asarray(x, np.float64)
        assert rows.shape == (h + m, 68)
        return window_cov(rows, h, [None] * h + idn.obs[n - m:], [None] * h + idn.prs[n - m:], self.w, r - (n - m), self.noise_px,
                          self.blocks, full=self.noise_px is None)

    def tick(self, f, views_f, meta, params, joints):
        out = super().tick(f, views_f, meta, params, joints)
        out["cov"] = {}
        for tid, idn in self.ids.items():
            c = self.cov_at(tid, f)
            if c is not None:
                out["cov"][tid] = c
                self.rows.setdefault((tid, idn.f0), {})[f - self.lag - idn.f0] = (c["joint_sigma"], c["param_sigma"], c["noise_px"])
        return out

    def record_cov(self, rec):
        """A record of this stream (live_smooth_np's dict) -> joint_sigma (n,18), param_sigma (n,39), noise_px (n,): per row the values
        recorded when it was emitted, NaN on the rows that never were."""
        n = len(rec["frames"])
        js, ps, s = np.full((n, 18), np.nan), np.full((n, K), np.nan), np.full(n, np.nan)
        for r, (a, b, c) in self.rows.get((rec["track_id"], int(rec["frames"][0])), {}).items():
            if r < n:
                js[r], ps[r], s[r] = a, b, c
        return js, ps, s
