"""Inputs shared by the tests of the rig-refinement kernels (tests/test_rig_refine_cpu.py, tests/test_gpu_rig_kernels.py): small packed
problems made by hand -- no tracker, no scene walk -- and a table of named cases, each the smallest shape at which one path of
csrc/mvmc_rigfit.hip differs.  The CPU test proves on the restatement alone that every case takes the branch it is named for and that
every decision it makes is far from its threshold; the GPU test then asks the device for the same decisions."""
import functools

import numpy as np

import rig_refine_np as rr

MAX_ITER_CAP = 24         # include/mvmc.h: MVMC_RIG_MAX_ITER
MU_TERMS = 1e-3           # the damping the terms are compared at


def ring_rig(C):
    """K (C,3,3), Rt (C,3,4): C cameras 4 m from the origin, looking at it, spread over most of a circle at three heights (so that no
    two lines of sight coincide, also for C = 2); K = diag(1000, 1000) + (640, 360)."""
    K = np.tile(np.array([[1000.0, 0.0, 640.0], [0.0, 1000.0, 360.0], [0.0, 0.0, 1.0]]), (C, 1, 1))
    Rt = np.zeros((C, 3, 4))
    for c in range(C):
        a = 2.0 * np.pi * c / (C + 0.5)
        h = 0.5 + 0.4 * (c % 3)
        r = np.sqrt(16.0 - h * h)
        pos = np.array([r * np.cos(a), r * np.sin(a), h])
        z = -pos / np.linalg.norm(pos)
        x = np.cross(z, [0.0, 0.0, 1.0])
        x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z])
        Rt[c, :, :3] = R
        Rt[c, :, 3] = -R @ pos
    return K, Rt


def make(C, N, seed, sigma=2.0, occlusion=0.3, rot_deg=1.0, trans_m=0.03, held_extra=(), empty=None):
    """A packed problem on a perturbed ring rig -> dict(K, Rt_true, Rt (the perturbed rig: the input of the solve), prob).
    N points uniform in a 2 x 2 x 1.8 m box about the origin, projected by the true rig, N(0, sigma) px on every coordinate, every view
    hidden with probability ``occlusion``.  Cameras in ``held_extra`` are held in addition to camera 0 and their observations leave the
    problem; camera ``empty`` stays free but observes nothing.  Every point is topped up to two observations among the other cameras
    (the precondition of mvmc_rig_accumulate).  prob = dict(X, uv, held, stop=None): X by rr.dlt_points on the perturbed rig, uv NaN
    where the camera does not observe the point."""
    rng = np.random.default_rng([seed, C, N])
    K, Rt_true = ring_rig(C)
    Rt = rr.perturb_rig(Rt_true, seed, rot_deg=rot_deg, trans_m=trans_m)
    Xt = rng.uniform([-1.0, -1.0, -0.9], [1.0, 1.0, 0.9], size=(N, 3))
    uv = rr.project(K, Rt_true[:, :, :3], Rt_true[:, :, 3], Xt) + rng.normal(0.0, sigma, size=(N, C, 2))
    seen = rng.uniform(size=(N, C)) >= occlusion
    out_of_it = np.zeros(C, bool)
    out_of_it[list(held_extra)] = True
    if empty is not None:
        out_of_it[empty] = True
    seen[:, out_of_it] = False
    usable = np.flatnonzero(~out_of_it)
    for i in np.flatnonzero(seen.sum(axis=1) < 2):
        hidden = [c for c in usable if not seen[i, c]]
        seen[i, rng.choice(hidden, size=2 - int(seen[i].sum()), replace=False)] = True
    cand = np.concatenate([uv, np.ones((N, C, 1))], axis=2)
    X = rr.dlt_points(np.einsum("cij,cjk->cik", K, Rt), cand, seen)
    held = out_of_it.copy()
    held[0] = True
    if empty is not None:
        held[empty] = False
    prob = dict(X=X, uv=np.where(seen[:, :, None], uv, np.nan), held=held, stop=None)
    return dict(K=K, Rt_true=Rt_true, Rt=Rt, prob=prob)


_HARD = dict(rot_deg=8.0, trans_m=0.3)
# name -> (arguments of make, arguments of rr.solve).  The tolerances are part of the case: each is chosen so that the case's stop rule
# and every decision before it are clear of their thresholds (tests/test_rig_refine_cpu.py: test_case_margins).
CASES = {
    "c2":          (dict(C=2, N=70, seed=2), dict(max_iter=10, ftol=1e-5)),                 # nf = 1, one 16-row block, 64 + 6 points
    "c3_full":     (dict(C=3, N=64, seed=3), dict(max_iter=10, ftol=1e-8)),                 # exactly one full tile
    "c4_held_mid": (dict(C=4, N=100, seed=11, held_extra=(2,)), dict(max_iter=10, ftol=1e-8)),   # slot -1 between slots, identity rows
    "c5_65":       (dict(C=5, N=65, seed=5), dict(max_iter=10, ftol=1e-5)),                 # a tile of one point
    "c6":          (dict(C=6, N=61, seed=6), dict(max_iter=10, ftol=1e-5)),                 # one partial tile, nb = 2
    "c7":          (dict(C=7, N=199, seed=7), dict(max_iter=10, ftol=1e-5)),                # nb = 3, last tile short
    "c8":          (dict(C=8, N=130, seed=8), dict(max_iter=10, ftol=1e-5)),                # 6 blocks, 64 + 64 + 2 points
    "reject":      (dict(C=5, N=150, seed=381, **_HARD), dict(max_iter=8, mu0=1e-6)),        # rejected, then accepted trials
    "bad":         (dict(C=5, N=100, seed=22, empty=3), dict(max_iter=6)),                  # a free camera without observations
    "xtol":        (dict(C=5, N=150, seed=32), dict(max_iter=10, xtol=1e-3)),
    "ftol":        (dict(C=5, N=150, seed=32), dict(max_iter=10, ftol=1e-4)),
    "maxit":       (dict(C=5, N=150, seed=32), dict(max_iter=2)),
    "maxit0":      (dict(C=5, N=150, seed=32), dict(max_iter=0)),
    "maxit_cap":   (dict(C=5, N=150, seed=32), dict(max_iter=MAX_ITER_CAP, ftol=1e-5)),
}
SOLVE_DEFAULTS = dict(max_iter=10, mu0=rr.LM_MU0, ftol=rr.LM_FTOL, xtol=rr.LM_XTOL)


def params(name):
    """The case's arguments of the solve, defaults filled in: dict(max_iter, mu0, ftol, xtol)."""
    return {**SOLVE_DEFAULTS, **CASES[name][1]}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> make()'s dict of the case.  Shared between the tests: treat it as read-only."""
    return make(**CASES[name][0])


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (rr.solve's result on the case, its trace).  Computed once; read-only."""
    c = case(name)
    trace = []
    out = rr.solve(c["prob"], c["K"], c["Rt"], trace=trace, **params(name))
    return out, trace


def margin_violations(name, et_margin=1e-6):
    """The decisions of the case's reference solve that are NOT clear of their thresholds, as strings (none = the device, which agrees
    with the restatement to ~1e-13 on these quantities, cannot decide otherwise for rounding reasons).  At every look at the system:
    |d|_inf outside [xtol / 10, 10 xtol] and pred / E outside [ftol / 10, 10 ftol]; at every trial |Et - E| / E >= et_margin; after an
    accepted trial (E - Et) / E outside [ftol / 10, 10 ftol]."""
    p = params(name)
    out, trace = reference(name)
    band = lambda v, tol: tol / 10.0 <= v <= 10.0 * tol
    bad = []
    for k, t in enumerate(trace):
        if t["bad"]:
            continue
        if not np.isfinite([t["dmax"], t["pred"], t["Et"]]).all():
            bad.append(f"look {k}: not finite")
            continue
        if band(t["dmax"], p["xtol"]):
            bad.append(f"look {k}: |d|_inf {t['dmax']:.3e} near xtol {p['xtol']:.0e}")
        if band(t["pred"] / t["E"], p["ftol"]):
            bad.append(f"look {k}: pred / E {t['pred'] / t['E']:.3e} near ftol {p['ftol']:.0e}")
        if k < len(out["trials"]):
            rho = (t["E"] - t["Et"]) / t["E"]
            if not abs(rho) >= et_margin:
                bad.append(f"trial {k}: |Et - E| / E {abs(rho):.3e} below {et_margin:.0e}")
            if out["trials"][k] and band(rho, p["ftol"]):
                bad.append(f"trial {k}: (E - Et) / E {rho:.3e} near ftol {p['ftol']:.0e}")
    return bad
