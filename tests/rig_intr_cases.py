"""Inputs shared by the tests of the rig refinement with intrinsic unknowns (tests/test_rig_intr_cpu.py, tests/test_gpu_rig_intr.py):
tests/rig_cases.py's hand-made problems on the ring rig, given an input K whose focal lengths are off, and a table of named cases,
each the smallest shape at which one path of the _intr kernels of csrc/mvmc_rigfit.hip differs.  The CPU test proves on the
restatement alone that every case takes the branch it is named for and that every decision it makes is far from its threshold."""
import functools

import numpy as np

import rig_cases as rc
import rig_intr_np as ri
import rig_refine_np as rr


def make(focal_pct=4.0, centre_px=0.0, **kw):
    """rig_cases.make, then the input K: every camera's fx, fy times e^U(-focal_pct, +focal_pct) % and its principal point moved by
    U(-centre_px, +centre_px), seeded by the case; the start points are the DLT on the input K and rig.  -> make's dict with K the INPUT
    intrinsics and K_true."""
    c = dict(rc.make(**kw))
    rng = np.random.default_rng([kw["seed"], 77])
    C = c["K"].shape[0]
    K = c["K"].copy()
    f = np.exp(rng.uniform(-focal_pct, focal_pct, C) / 100.0)
    K[:, 0, 0] *= f
    K[:, 1, 1] *= f
    K[:, :2, 2] += rng.uniform(-centre_px, centre_px, (C, 2)) if centre_px else 0.0
    uv = c["prob"]["uv"]
    seen = ~np.isnan(uv[:, :, 0])
    cand = np.concatenate([np.nan_to_num(uv), np.ones(seen.shape + (1,))], axis=2)
    X = rr.dlt_points(np.einsum("cij,cjk->cik", K, c["Rt"]), cand, seen)
    c.update(K_true=c["K"], K=K, prob=dict(c["prob"], X=X))
    return c


_HARD = dict(rot_deg=5.0, trans_m=0.2)
F, FC = dict(intrinsics="focal"), dict(intrinsics="focal+centre", centre_sigma_px=20.0)
# name -> (arguments of make, arguments of ri.solve).  The tolerances are part of the case, as in tests/rig_cases.py.
CASES = {
    "f_c3":       (dict(C=3, N=70, seed=3), dict(F, max_iter=10, ftol=3e-6)),                   # two free cameras and camera 0's lone phi
    "f_c5_65":    (dict(C=5, N=65, seed=5), dict(F, max_iter=10, ftol=1e-5)),                   # a tile of one point
    "f_c8":       (dict(C=8, N=130, seed=8), dict(F, max_iter=10, ftol=1e-7)),                  # M = 50: a fourth 16-row block
    "fc_c8":      (dict(C=8, N=130, seed=8, centre_px=8.0), dict(FC, max_iter=10, ftol=1e-6)),  # M = 66, 64 + 64 + 2 points
    "fc_c7":      (dict(C=7, N=100, seed=7, centre_px=8.0), dict(FC, max_iter=4))            ,  # M = 57, NI = 3 at the other large C
    "fc_c2":      (dict(C=2, N=70, seed=2, centre_px=8.0), dict(FC, focal_sigma=0.05, max_iter=10, ftol=4e-6)),   # two cameras: both priors
    "k_held_mid": (dict(C=5, N=100, seed=11), dict(F, intrinsics_held=(2,), max_iter=10, ftol=1e-7)),   # a 6-column block between 7-column ones
    "k_held_0":   (dict(C=4, N=100, seed=12, centre_px=8.0), dict(FC, intrinsics_held=(0,), max_iter=10, ftol=1e-5)),   # camera 0 without a block
    "pose_held":  (dict(C=5, N=100, seed=11, held_extra=(2,)), dict(F, max_iter=10, ftol=1e-7)),     # a camera whose observations left
    "tight":      (dict(C=5, N=100, seed=13), dict(F, focal_sigma=1e-4, max_iter=10, ftol=1e-5)),    # the prior decides the result
    "sigma_inf":  (dict(C=5, N=100, seed=13), dict(F, focal_sigma=float("inf"), max_iter=10, ftol=1e-7)),
    "reject":     (dict(C=5, N=150, seed=14, **_HARD), dict(F, max_iter=6, mu0=1e-2)),               # rejected, then accepted trials
    "bad":        (dict(C=5, N=100, seed=22, empty=3), dict(F, max_iter=6)),                         # a free camera without observations
    "xtol":       (dict(C=5, N=150, seed=35), dict(F, max_iter=10, xtol=4e-3)),
    "ftol":       (dict(C=5, N=150, seed=32), dict(F, max_iter=10, ftol=1e-4)),
    "maxit":      (dict(C=5, N=150, seed=32), dict(F, max_iter=2)),
    "maxit0":     (dict(C=5, N=150, seed=32), dict(F, max_iter=0)),
    "huber":      (dict(C=5, N=150, seed=41), dict(F, loss="huber", loss_px=3.0, max_iter=6)),
    "cauchy":     (dict(C=4, N=120, seed=42, centre_px=8.0), dict(FC, loss="cauchy", loss_px=3.0, max_iter=6)),
}
SOLVE_DEFAULTS = dict(max_iter=10, mu0=rr.LM_MU0, ftol=rr.LM_FTOL, xtol=rr.LM_XTOL, loss=None, loss_px=ri.LOSS_PX, intrinsics=None,
                      focal_sigma=None, centre_sigma_px=None, intrinsics_held=())


def params(name):
    """The case's arguments of the solve, defaults filled in."""
    return {**SOLVE_DEFAULTS, **CASES[name][1]}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> make()'s dict of the case.  Shared between the tests: treat it as read-only."""
    return make(**CASES[name][0])


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (ri.solve's result on the case, its trace).  Computed once; read-only."""
    c = case(name)
    trace = []
    out = ri.solve(c["prob"], c["K"], c["Rt"], trace=trace, **params(name))
    return out, trace


def margin_violations(name, et_margin=1e-6):
    """rig_cases.margin_violations' rule on this table's reference solves: at every look at the system |d|_inf outside
    [xtol / 10, 10 xtol] and pred / E outside [ftol / 10, 10 ftol]; at every trial |Et - E| / E >= et_margin; after an accepted
    trial (E - Et) / E outside [ftol / 10, 10 ftol]."""
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
