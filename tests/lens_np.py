"""NumPy restatement of the lens models of include/mvmc.h (mvmc_lens_undistort / mvmc_lens_distort): the forward maps, the Newton
inverses and the accept rule, vectorised over points, float64 throughout.  The tests' oracle; it shares no code with the package.

A lens row is the table's: {model, fx, fy, cx, cy, skew, k[0..7], 0, 0}; model 0 pinhole, 1 Brown (k1 k2 p1 p2 k3 k4 k5 k6), 2 fisheye
(Kannala-Brandt k1..k4)."""
import numpy as np

PINHOLE, BROWN, FISHEYE = 0, 1, 2
MAX_ITER = 12
STOP = 1e-13
FISHEYE_MAX_THETA = 1.5

# the coefficient sets of the tests, 1920 x 1080: (f, coefficients in OpenCV's order)
MILD5 = (1400.0, (-0.12, 0.03, 8e-4, -5e-4, -0.004))
WIDE5 = (1000.0, (-0.28, 0.09, 1e-3, -5e-4, -0.012))
RATIONAL8 = (1000.0, (0.9, 0.12, 1e-3, -5e-4, 0.004, 1.25, 0.35, 0.02))
FISHEYE4 = (600.0, (-0.02, 0.005, -0.001, 0.0002))
IMG_WH = (1920, 1080)


def row(model, f, coeffs=(), cx=None, cy=None, skew=0.0, fy=None):
    """A lens row; the principal point defaults to the centre of the 1920 x 1080 image."""
    r = np.zeros(16)
    r[0] = model
    r[1], r[2] = f, f if fy is None else fy
    r[3] = IMG_WH[0] / 2 if cx is None else cx
    r[4] = IMG_WH[1] / 2 if cy is None else cy
    r[5] = skew
    r[6:6 + len(coeffs)] = coeffs
    return r


def normalise(r, uv):
    y = (uv[..., 1] - r[4]) / r[2]
    x = (uv[..., 0] - r[3] - r[5] * y) / r[1]
    return x, y


def pixels(r, x, y):
    return np.stack([r[1] * x + r[5] * y + r[3], r[2] * y + r[4]], -1)


def brown_eval(k, x, y):
    """Forward map and Jacobian (j12 = j21) at normalised (x, y): X, Y, j11, j12, j22, rad."""
    k1, k2, p1, p2, k3, k4, k5, k6 = k[:8]
    r2 = x * x + y * y
    num = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
    den = 1 + r2 * (k4 + r2 * (k5 + r2 * k6))
    nump = k1 + r2 * (2 * k2 + 3 * k3 * r2)
    denp = k4 + r2 * (2 * k5 + 3 * k6 * r2)
    rad = num / den
    radp = (nump - rad * denp) / den
    X = x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    Y = y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    j11 = rad + 2 * x * x * radp + 2 * p1 * y + 6 * p2 * x
    j12 = 2 * x * y * radp + 2 * p1 * x + 2 * p2 * y
    j22 = rad + 2 * y * y * radp + 6 * p1 * y + 2 * p2 * x
    return X, Y, j11, j12, j22, rad


def fisheye_eval(k, th):
    t2 = th * th
    thd = th * (1 + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3]))))
    dthd = 1 + t2 * (3 * k[0] + t2 * (5 * k[1] + t2 * (7 * k[2] + t2 * 9 * k[3])))
    return thd, dthd


def distort_normalised(r, x, y):
    """-> xd, yd, det: the forward model and its Jacobian determinant (fisheye: d theta_d / d theta) at the ideal point."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    model = int(r[0])
    if model == BROWN:
        X, Y, j11, j12, j22, _ = brown_eval(r[6:14], x, y)
        return X, Y, j11 * j22 - j12 * j12
    if model == FISHEYE:
        rr = np.sqrt(x * x + y * y)
        thd, dthd = fisheye_eval(r[6:10], np.arctan(rr))
        with np.errstate(invalid="ignore", divide="ignore"):
            scale = np.where(rr > 0, thd / np.where(rr > 0, rr, 1.0), 1.0)
        return x * scale, y * scale, dthd
    return x.copy(), y.copy(), np.ones_like(x)


def undistort_normalised(r, xd, yd):
    """The Newton inverse with the accept rule -> x, y, ok, iterations (the steps taken until the stop rule held)."""
    xd, yd = np.asarray(xd, np.float64), np.asarray(yd, np.float64)
    model = int(r[0])
    ok = np.ones(xd.shape, bool)
    conv = np.zeros(xd.shape, bool)
    iters = np.zeros(xd.shape, int)
    with np.errstate(all="ignore"):
        if model == BROWN:
            k = r[6:14]
            x, y = xd.copy(), yd.copy()
            for _ in range(MAX_ITER):
                X, Y, j11, j12, j22, rad = brown_eval(k, x, y)
                det = j11 * j22 - j12 * j12
                run = ~conv
                ok &= ~run | ((det > 0) & (rad > 0))
                f1, f2 = X - xd, Y - yd
                dx, dy = -(j22 * f1 - j12 * f2) / det, -(j11 * f2 - j12 * f1) / det
                x = np.where(run, x + dx, x)
                y = np.where(run, y + dy, y)
                iters += run
                conv |= run & (np.abs(dx) + np.abs(dy) <= STOP * (1 + np.abs(x) + np.abs(y)))
            X, Y, j11, j12, j22, rad = brown_eval(k, x, y)
            ok &= conv & (j11 * j22 - j12 * j12 > 0) & (rad > 0) & np.isfinite(x) & np.isfinite(y)
            return x, y, ok, iters
        if model == FISHEYE:
            k = r[6:10]
            thd = np.sqrt(xd * xd + yd * yd)
            th = thd.copy()
            for _ in range(MAX_ITER):
                g, dg = fisheye_eval(k, th)
                run = ~conv
                ok &= ~run | (dg > 0)
                d = -(g - thd) / dg
                th = np.where(run, th + d, th)
                iters += run
                conv |= run & (np.abs(d) <= STOP * (1 + np.abs(th)))
            g, dg = fisheye_eval(k, th)
            scale = np.where(thd > 0, np.tan(th) / np.where(thd > 0, thd, 1.0), 1.0)
            x, y = xd * scale, yd * scale
            ok &= conv & (dg > 0) & (th >= 0) & (th < FISHEYE_MAX_THETA) & np.isfinite(x) & np.isfinite(y)
            return x, y, ok, iters
    return xd.copy(), yd.copy(), ok, iters


def distort_points(r, uv):
    """Pinhole pixels (...,2) -> raw pixels, and the Jacobian determinant at each."""
    uv = np.asarray(uv, np.float64)
    if int(r[0]) == PINHOLE:
        return uv.copy(), np.ones(uv.shape[:-1])
    x, y = normalise(r, uv)
    xd, yd, det = distort_normalised(r, x, y)
    return pixels(r, xd, yd), det


def undistort_points(r, uv):
    """Raw pixels (...,2) -> pinhole pixels, ok, iterations."""
    uv = np.asarray(uv, np.float64)
    if int(r[0]) == PINHOLE:
        return uv.copy(), np.ones(uv.shape[:-1], bool), np.zeros(uv.shape[:-1], int)
    xd, yd = normalise(r, uv)
    x, y, ok, it = undistort_normalised(r, xd, yd)
    return pixels(r, x, y), ok, it


def _apply(fn_inverse, kps, table, rig_of_frame):
    kps = np.asarray(kps)
    F, C = kps.shape[:2]
    k64 = kps.astype(np.float64).reshape(F, C, -1, 3)
    out = kps.copy().reshape(F, C, -1, 3)
    dropped = np.zeros((F, C), np.int32)
    rig = np.zeros(F, int) if rig_of_frame is None else np.asarray(rig_of_frame)
    for f in range(F):
        for c in range(C):
            r = table[rig[f], c]
            if int(r[0]) == PINHOLE:
                continue
            scored = k64[f, c, :, 2] > 0
            if fn_inverse:
                uv, ok, _ = undistort_points(r, k64[f, c, :, :2])
            else:
                uv, ok = distort_points(r, k64[f, c, :, :2])[0], np.ones(scored.shape, bool)
            good, bad = scored & ok, scored & ~ok
            out[f, c, good, :2] = uv[good].astype(kps.dtype)
            out[f, c, bad] = 0
            dropped[f, c] = bad.sum()
    return out.reshape(kps.shape), dropped


def undistort_keypoints(kps, table, rig_of_frame=None):
    """The kernel's contract on (F,C,...,3) triples of float32 or float64: -> (kps_out in the input dtype, dropped (F,C))."""
    return _apply(True, kps, table, rig_of_frame)


def distort_keypoints(kps, table, rig_of_frame=None):
    return _apply(False, kps, table, rig_of_frame)
