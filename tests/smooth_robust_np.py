"""NumPy restatement of the trajectory smoothers with a robust loss on the keypoint residuals (smoothing.smooth_sequences(loss=...),
live_smoothing.LiveSmoother(loss=...); csrc/mvmc_smooth_row.h: sm_row_block<LOSS>).  Everything the loss does not touch is
tests/smooth_np.py's, tests/live_smooth_np.py's and tests/smooth_cov_np.py's: the selection, the unwrapping, the prior, the banded
solve, the Levenberg-Marquardt rules, the window, the covariance's recursion.

The loss.  For one (selected view v, observed joint k) pair of a row: score s, plain pixel residual (ru, rv) = proj_v(X_k) - obs,
e^2 = ru^2 + rv^2, delta = loss_px > 0,
  huber   rho = 1/2 e^2, w = 1 for e <= delta; otherwise rho = delta (e - 1/2 delta), w = delta / e;
  cauchy  rho = 1/2 delta^2 log1p(e^2 / delta^2), w = 1 / (1 + e^2 / delta^2)
(tests/rig_robust_np.py's two functions).  The score stays outside the loss: E_data = sum s^2 rho(e^2) replaces 1/2 sum s^2 e^2
wherever the iteration reads a cost, and at every linearisation the pair's two Jacobian rows and its residual are multiplied by
sqrt(w) (iteratively reweighted least squares, no second-order correction).  A pair with s = 0 contributes nothing.  loss=None is
smooth_np.data_terms itself.

robust(loss, loss_px) binds smooth_np.data_terms to the robust one for its duration: smooth_np.smooth, live_smooth_np.Stream and
smooth_cov_np.covariance read it through the module and so run the robust model unchanged.
"""
import contextlib

import numpy as np

import oracle_np as o
import smooth_np as sm
import trf_np as t
from rig_robust_np import LOSS_PX, LOSSES, rho_w  # noqa: F401  (rho_w(e2, loss, loss_px) -> (rho, w), elementwise)

K = sm.K
_plain_data_terms = sm.data_terms


def _pairs(x_row, ob, pr):
    """One row -> (e2 (V,16) of the plain pixel residuals, r (V,16,2), s (V,16))."""
    unit = np.array(ob, np.float64)
    unit[..., 2] = 1.0
    r = o.ik_residual(x_row[:3], x_row[3:57], x_row[57:], unit, pr).reshape(-1, 16, 2)
    return r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1], r, np.asarray(ob, np.float64)[..., 2]


def data_terms(x, obs, prs, want_jac=True, loss=None, loss_px=LOSS_PX):
    """smooth_np.data_terms of the weighted model: E_data = sum s^2 rho, per-frame E, J^T W J (m,39,39), J^T W r (m,39)."""
    if loss is None:
        return _plain_data_terms(x, obs, prs, want_jac)
    m = x.shape[0]
    Et = np.zeros(m)
    H = np.zeros((m, K, K))
    g = np.zeros((m, K))
    for r in range(m):
        if obs[r] is None:
            continue
        e2, res, s = _pairs(x[r], obs[r], prs[r])
        rho, w = rho_w(e2, loss, loss_px)
        live = s != 0.0
        Et[r] = np.sum(np.where(live, s * s * rho, 0.0))
        if want_jac:
            unit = np.array(obs[r], np.float64)
            unit[..., 2] = 1.0
            J = t.ik_jacobian(x[r, :3], x[r, 3:57], x[r, 57:], unit, prs[r], False)[:, sm.COLS].reshape(-1, 16, 2, K)
            a = np.where(live, np.sqrt(w) * s, 0.0)
            J = (a[..., None, None] * J).reshape(-1, K)
            f = (a[..., None] * res).ravel()
            H[r] = J.T @ J
            g[r] = J.T @ f
    return Et.sum(), Et, H, g


def obs_weights(x, obs, prs, loss, loss_px=LOSS_PX):
    """x (m,68), obs / prs per frame -> per frame None (no data) or w (V,16) of every (selected view, observed joint) pair at x, NaN
    where the pair's score is 0.  loss=None: 1 where there is a pair."""
    out = []
    for r in range(x.shape[0]):
        if obs[r] is None:
            out.append(None)
            continue
        e2, _, s = _pairs(x[r], obs[r], prs[r])
        out.append(np.where(s != 0.0, rho_w(e2, loss, loss_px)[1], np.nan))
    return out


@contextlib.contextmanager
def robust(loss, loss_px=LOSS_PX):
    """smooth_np.data_terms is the robust one inside the block (smooth_np.lm / energy, live_smooth_np.window_*, smooth_cov_np.covariance
    call it through the module), and the plain one again after it, whatever happens inside."""
    def bound(x, obs, prs, want_jac=True):
        return data_terms(x, obs, prs, want_jac, loss, loss_px)
    before = sm.data_terms
    sm.data_terms = bound
    try:
        yield
    finally:
        sm.data_terms = before
