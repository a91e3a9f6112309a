"""Inputs shared by the tests of the rig refinement's robust loss (tests/test_rig_robust_cpu.py, tests/test_gpu_rig_robust.py): the small
packed problems of tests/rig_cases.py with a seeded contamination -- no tracker, no scene walk -- and a table of named cases, each the
smallest shape at which one path of the loss in csrc/mvmc_rigfit.hip differs.  Every case runs with Huber and with Cauchy.  The CPU test
proves on the restatement (tests/rig_robust_np.py) alone that every decision a case makes is far from its threshold; the GPU test then
asks the device for the same decisions.  The reweighted iteration converges linearly, so each case carries its own ftol, xtol and
max_iter, and none rests on the noise-level tail the default ftol = 1e-12 runs into."""
import functools

import numpy as np

import rig_cases as rc
import rig_refine_np as rr
import rig_robust_np as rb

LOSSES = ("huber", "cauchy")
SHIFT_PX = 40.0           # a contaminated observation moves by U(-40, 40) px per coordinate: inside max_px = 97.88


def make(C, N, seed, share=0.15, far=0, **kw):
    """rig_cases.make's packed problem with ``share`` of its observations moved by U(-SHIFT_PX, SHIFT_PX) px per coordinate, and EVERY
    observation of its first ``far`` points with three or more views moved by 20 .. 40 px per coordinate with random signs (the DLT
    of two views absorbs any shift); the start points are the DLT of the contaminated observations on the perturbed rig
    -> rig_cases.make's dict plus hit (N,C) bool: the observations moved, and far (far,): those points."""
    c = rc.make(C=C, N=N, seed=seed, **kw)
    rng = np.random.default_rng([seed, C, N, 4])
    uv = c["prob"]["uv"].copy()
    seen = ~np.isnan(uv[:, :, 0])
    hit = seen & (rng.uniform(size=seen.shape) < share)
    uv[hit] += rng.uniform(-SHIFT_PX, SHIFT_PX, size=(int(hit.sum()), 2))
    far = np.flatnonzero(seen.sum(axis=1) >= 3)[:far]
    if far.size:
        sel = np.zeros_like(seen)
        sel[far] = seen[far] & ~hit[far]
        uv[sel] += rng.uniform(20.0, SHIFT_PX, size=(int(sel.sum()), 2)) * rng.choice([-1.0, 1.0], size=(int(sel.sum()), 2))
        hit |= sel
    cand = np.concatenate([np.nan_to_num(uv), np.ones((N, C, 1))], axis=2)
    X = rr.dlt_points(np.einsum("cij,cjk->cik", c["K"], c["Rt"]), cand, seen)
    return dict(K=c["K"], Rt_true=c["Rt_true"], Rt=c["Rt"], hit=hit, far=far, prob=dict(X=X, uv=uv, held=c["prob"]["held"], stop=None))


def violations(out, trace, ftol, xtol, et_margin=1e-6):
    """rig_cases.margin_violations on one robust solve (its result, its trace, its tolerances): the decisions that are NOT clear of
    their thresholds, as strings.  At every look |d|_inf outside [xtol / 10, 10 xtol] and pred / E outside [ftol / 10, 10 ftol]; at
    every trial |Et - E| / E >= et_margin; after an accepted trial (E - Et) / E outside [ftol / 10, 10 ftol]."""
    band = lambda v, tol: tol / 10.0 <= v <= 10.0 * tol
    bad = []
    for k, t in enumerate(trace):
        if t["bad"]:
            continue
        if not np.isfinite([t["dmax"], t["pred"], t["Et"]]).all():
            bad.append(f"look {k}: not finite")
            continue
        if band(t["dmax"], xtol):
            bad.append(f"look {k}: |d|_inf {t['dmax']:.3e} near xtol {xtol:.0e}")
        if band(t["pred"] / t["E"], ftol):
            bad.append(f"look {k}: pred / E {t['pred'] / t['E']:.3e} near ftol {ftol:.0e}")
        if k < len(out["trials"]):
            rho = (t["E"] - t["Et"]) / t["E"]
            if not abs(rho) >= et_margin:
                bad.append(f"trial {k}: |Et - E| / E {abs(rho):.3e} below {et_margin:.0e}")
            if out["trials"][k] and band(rho, ftol):
                bad.append(f"trial {k}: (E - Et) / E {rho:.3e} near ftol {ftol:.0e}")
    return bad


_HARD = dict(rot_deg=8.0, trans_m=0.3)
_MILD = dict(C=5, N=150, seed=32, share=0.02)
# name -> (arguments of make, arguments of the solve, the losses it runs with).  The shape cases stop on max_iter = 6 with the default
# tolerances far below everything they see (pred / E stays above 1e-5, |d|_inf above 1e-4 there).  The reweighted iteration gains a
# factor 2 .. 10 per trial once the weights matter, and a stop on a tolerance that is clear of its threshold by 10 x on both sides
# needs a factor 100 between two looks: the cases of the tolerance rules therefore use a mild contamination and a delta at which a
# few weights (Huber) or all of them a little (Cauchy) differ from 1 -- the rules live in the decision kernel, which the loss does
# not touch; what these cases gate is that the new entries hand ftol and xtol to it.
CASES = {
    "c2":          (dict(C=2, N=70, seed=2), dict(), LOSSES),                                  # one block, 64 + 6 points
    "c3_full":     (dict(C=3, N=64, seed=3), dict(), LOSSES),                                  # exactly one full tile
    "c4_held_mid": (dict(C=4, N=100, seed=11, held_extra=(2,)), dict(), LOSSES),               # camera 2 held between free ones
    "c5_65":       (dict(C=5, N=65, seed=5), dict(), LOSSES),                                  # a tile of one point
    "c8":          (dict(C=8, N=130, seed=8), dict(), LOSSES),                                 # six blocks, 64 + 64 + 2 points
    "far":         (dict(C=5, N=100, seed=23, far=8), dict(), LOSSES),                         # points whose every observation lies beyond delta
    "delta_inf":   (dict(C=5, N=150, seed=32), dict(loss_px=1e30, max_iter=3), LOSSES),                  # every weight 1: the plain solve
    "delta_small": (dict(C=5, N=150, seed=32), dict(loss_px=0.5), LOSSES),                     # nearly every weight < 1
    "reject":      (dict(C=5, N=150, seed=401, **_HARD), dict(max_iter=8, mu0=1e-4), ("huber",)),        # a rejected, then accepted trials
    "reject_c":    (dict(C=5, N=150, seed=418, **_HARD), dict(max_iter=8, mu0=1e-4, loss_px=300.0), ("cauchy",)),   # (Cauchy at 6 px rejects nothing here)
    "xtol":        (_MILD, dict(max_iter=10, xtol=1e-3, loss_px=20.0), ("huber",)),
    "xtol_c":      (_MILD, dict(max_iter=10, xtol=1e-3, loss_px=150.0), ("cauchy",)),
    "ftol_before": (_MILD, dict(max_iter=10, ftol=1e-4, loss_px=20.0), ("huber",)),            # the prediction falls below ftol E
    "ftol_before_c": (_MILD, dict(max_iter=10, ftol=1e-4, loss_px=60.0), ("cauchy",)),
    # ftol after a trial: an accepted trial that gains 0.07 % (0.4 %) where 97 % (62 %) were predicted, from a rig far off; a loss at 6 px
    # makes no such trial on 700 seeds, and at mu0 = 1e-6 one ulp on the input moves the restatement's own final cost by the gate's 1e-10
    "ftol_after":  (dict(C=5, N=150, seed=378, **_HARD), dict(max_iter=10, mu0=1e-4, ftol=0.026, loss_px=300.0), ("huber",)),
    "ftol_after_c": (dict(C=5, N=150, seed=401, rot_deg=14.0, trans_m=0.5), dict(max_iter=10, mu0=1e-5, ftol=0.051, loss_px=300.0), ("cauchy",)),
    "maxit0":      (dict(C=5, N=150, seed=32), dict(max_iter=0), LOSSES),
    "maxit_cap":   (_MILD, dict(max_iter=rc.MAX_ITER_CAP, ftol=1e-4, loss_px=20.0), ("huber",)),          # the largest max_iter, stopped long before it
    "maxit_cap_c": (_MILD, dict(max_iter=rc.MAX_ITER_CAP, ftol=1e-4, loss_px=60.0), ("cauchy",)),
}
SOLVE_DEFAULTS = dict(max_iter=6, mu0=rr.LM_MU0, ftol=rr.LM_FTOL, xtol=rr.LM_XTOL, loss_px=rb.LOSS_PX)
PAIRS = [(n, l) for n in CASES for l in CASES[n][2]]


def params(name):
    """The case's arguments of the solve, defaults filled in: dict(max_iter, mu0, ftol, xtol, loss_px)."""
    return {**SOLVE_DEFAULTS, **CASES[name][1]}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> make()'s dict of the case.  Shared between the tests: treat it as read-only."""
    return make(**CASES[name][0])


@functools.lru_cache(maxsize=None)
def reference(name, loss):
    """-> (rig_robust_np.solve's result on the case with the loss, its trace).  Computed once; read-only."""
    c = case(name)
    trace = []
    out = rb.solve(c["prob"], c["K"], c["Rt"], trace=trace, loss=loss, **params(name))
    return out, trace


def margin_violations(name, loss):
    p = params(name)
    out, trace = reference(name, loss)
    return violations(out, trace, p["ftol"], p["xtol"])
