"""svt_kernel (csrc/mvmc_svt.hip) restated in NumPy float64: match_svt's ADMM in the eigen form the device uses,
Q = sum_k sign(l_k) max(|l_k| - lambda / mu, 0) v_k v_k^T from numpy.linalg.eigh of the symmetric M = Y / mu + X, in place of the
oracle's SVD (oracle_np.match_svt).  Float64 whatever the input type: a float32 S is cast to double first, as the kernel does.
The vector projection is oracle_np._proj2pav and the block projection is oracle_np._proj2dpam's loop, written out here only so that
it can report its rounds (check=True compares every block with oracle_np._proj2dpam itself, bit for bit).

match_svt() also returns what the run exercised and how far each of its decisions was from going the other way: the gates of
tests/test_gpu_svt_small.py admit a graph only when every decision is clear of its threshold (tests/svt_cases.py)."""
import numpy as np

import oracle_np as o

PROJ_TOL, PROJ_ROUNDS = 1e-2, 10


def _rel(a, b):
    """Relative distance of the comparison a < b (or a > b) from flipping; two exact zeros are no distance apart."""
    d = max(abs(a), abs(b))
    return abs(a - b) / d if d > 0 else 0.0


def _tie(T):
    """The rows of T as proj2pav sees them after clipping: does one take the simplex branch (sum >= 1) with two equal entries
    (any / positive)?"""
    y = np.where(T < 0, 0, T)
    u = np.sort(y[y.sum(axis=1) >= 1], axis=1)
    eq = u[:, 1:] == u[:, :-1]
    return bool(eq.any()), bool((eq & (u[:, 1:] > 0)).any())


def proj2dpam(Y, rec, check=False):
    """oracle_np._proj2dpam(Y, 1e-2), reporting into rec: rounds run, the margin of each stop test, ties met."""
    X0, X, I2 = Y, Y, 0
    out = None
    for r in range(PROJ_ROUNDS):
        T = X0 + I2
        a, p = _tie(T)
        rec["tie"] |= a
        rec["tie_pos"] |= p
        X1 = np.stack([o._proj2pav(T[i]) for i in range(T.shape[0])])
        I1 = X1 - T
        T = X0 + I1
        a, p = _tie(T.T)
        rec["tie"] |= a
        rec["tie_pos"] |= p
        X2 = np.stack([o._proj2pav(T[:, j]) for j in range(T.shape[1])], axis=1)
        I2 = X2 - T
        chg = np.abs(X2 - X).sum() / X.size
        X = X2
        rec["margin_blk"] = min(rec["margin_blk"], _rel(chg, PROJ_TOL))
        if r == PROJ_ROUNDS - 1:
            rec["blk_round10"] = True
        if chg < PROJ_TOL:
            if r < PROJ_ROUNDS - 1:
                rec["blk_early"] = True
            out = X
            break
    out = X if out is None else out
    if check:
        assert np.array_equal(out, o._proj2dpam(Y, PROJ_TOL))
    return out


def match_svt(S, counts, alpha=0.1, lam=50.0, mu=64.0, tol=5e-4, max_iter=20, dual_stochastic=True, check=False):
    """-> X (n,n) f64, x_bin (n,n) bool, calls (it + 1 on convergence, max_iter otherwise: the device's iters), rec."""
    S = np.asarray(S).astype(np.float64)
    n = S.shape[0]
    dim = np.concatenate([[0], np.cumsum(counts)]).astype(int)
    assert dim[-1] == n
    grp = np.repeat(np.arange(len(counts)), counts)
    same = grp[:, None] == grp[None, :]
    S = 0.5 * (S + S.T)
    S[np.arange(n), np.arange(n)] = 0.0
    X = S.copy()
    Y = np.zeros_like(S)
    mu = float(mu)
    rec = dict(margin_tol=np.inf, margin_mu=np.inf, margin_blk=np.inf, neg_eig=False, mu_up=False, mu_down=False, converged=False,
               tie=False, tie_pos=False, blk_early=False, blk_round10=False)
    calls = max_iter
    for it in range(max_iter):
        X0 = X
        inv_mu = 1.0 / mu
        M = inv_mu * Y + X
        lv, V = np.linalg.eigh(0.5 * (M + M.T))
        sh = np.abs(lv) - lam * inv_mu
        fk = np.where(sh > 0, np.sign(lv) * sh, 0.0)
        rec["neg_eig"] |= bool((fk < 0).any())
        Q = (V * fk) @ V.T
        X = Q - ((alpha - S) + Y) * inv_mu
        X[same] = 0.0
        X[np.arange(n), np.arange(n)] = 1.0
        X = np.clip(X, 0.0, 1.0)
        if dual_stochastic:
            for gi in range(len(counts)):
                r0, r1 = dim[gi], dim[gi + 1]
                for gj in range(len(counts)):
                    c0, c1 = dim[gj], dim[gj + 1]
                    if r1 > r0 and c1 > c0:
                        X[r0:r1, c0:c1] = proj2dpam(X[r0:r1, c0:c1].copy(), rec, check)
        X = 0.5 * (X + X.T)
        Y = Y + mu * (X - Q)
        p_res = float(np.linalg.norm(X - Q)) / n
        d_res = mu * float(np.linalg.norm(X - X0)) / n
        rec["margin_tol"] = min(rec["margin_tol"], _rel(p_res, tol), _rel(d_res, tol))
        if p_res < tol and d_res < tol:
            calls = it + 1
            rec["converged"] = True
            break
        rec["margin_mu"] = min(rec["margin_mu"], _rel(p_res, 10 * d_res), _rel(d_res, 10 * p_res))
        if p_res > 10 * d_res:
            mu = 2 * mu
            rec["mu_up"] = True
        elif d_res > 10 * p_res:
            mu = mu / 2
            rec["mu_down"] = True
    x_bin = X > 0.5
    rec["margin_half"] = float(np.abs(X - 0.5).min()) if n else np.inf
    rec["margin"] = min(rec["margin_tol"], rec["margin_mu"], rec["margin_blk"])
    return X, x_bin, calls, rec
