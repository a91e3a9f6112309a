"""NumPy restatement of the trajectory smoother's foot contacts (smoothing.smooth_sequences(contacts=...); csrc/mvmc_smooth_row.h:
sm_row_block<LOSS, CONTACT>, csrc/mvmc_smooth_contact.hip).  Everything the contacts do not touch is tests/smooth_np.py's,
tests/smooth_robust_np.py's and tests/smooth_cov_np.py's.  The device is gated against this file.

The model.  Per identity, rows t = 0 .. m - 1 (every frame f0..f1, the filled rows too), feet f = 0 (left ankle, skeleton joint 3) and
1 (right ankle, joint 6), labels c[t, f]; a run is a maximal stretch of consecutive rows with c = 1 of one foot and has one anchor a,
  E_contact = 1/2 wc sum_{t, f: c = 1} |X_f(x_t) - a_run(t, f)|^2,        wc in px^2 / m^2 (the root prior's unit).
For fixed anchors the term belongs to one row: with D = d X_f / d x_t (3 x 39: smooth_cov_np.joint_jacobians, analytic) it adds
wc D^T D to the row's J^T J, wc D^T (X_f - a) to its J^T r and 1/2 wc |X_f - a|^2 to its cost (left, then right); it is exact (the
term is a plain square), and it stays outside the robust loss.  Over the anchors E_contact is minimised by the run's mean.

contact(cmask, anc, wc) binds smooth_np.data_terms to the version with the term of ONE identity for its duration; it stacks on
whatever is bound at the time (smooth_robust_np.robust), so smooth_np.lm / energy and smooth_cov_np.covariance run the model unchanged.
detect() and anchors() are the labels and the anchors; smooth() is the rounds driver: round 0 = smooth_np.smooth, then
``rounds`` times FK, (labels in the first round,) anchors, and smooth_np.lm from the current trajectory under the binding.
"""
import contextlib

import numpy as np

import oracle_np as o
import smooth_cov_np as sc
import smooth_np as sm

K = sm.K
FEET = (3, 6)          # include/mvmc.h: MVMC_SMOOTH_FOOT_L, MVMC_SMOOTH_FOOT_R


def _fk(p):
    return o.forward_kinematics(p[:3], p[3:57], p[57:])[0]


def runs(col):
    """col (m,) bool -> [(start, end)] of the maximal stretches of True, end exclusive."""
    out, start = [], None
    for t, c in enumerate(col):
        if c and start is None:
            start = t
        if not c and start is not None:
            out.append((start, t))
            start = None
    if start is not None:
        out.append((start, len(col)))
    return out


def detect(joints, speed, min_run, ground=None, height=0.15):
    """joints (m,18,3) -> labels (m,2) bool: the ankle's speed (central difference |p[t+1] - p[t-1]| / 2, one-sided and not halved at
    the first and the last row) strictly below ``speed``, its height over ground = (normal, offset) strictly below ``height`` when a
    ground is given; then the runs shorter than min_run are dropped.  Every product and sum is rounded on its own."""
    joints = np.asarray(joints, np.float64)
    m = joints.shape[0]
    mask = np.zeros((m, 2), bool)
    if m < 2:
        return mask
    for f, J in enumerate(FEET):
        p = joints[:, J]
        for t in range(m):
            a, b = max(t - 1, 0), min(t + 1, m - 1)
            d = p[b] - p[a]
            v = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
            if b - a == 2:
                v = 0.5 * v
            c = v < speed
            if c and ground is not None:
                n, off = np.asarray(ground[0], np.float64), float(ground[1])
                c = (((n[0] * p[t, 0] + n[1] * p[t, 1]) + n[2] * p[t, 2]) - off) < height
            mask[t, f] = c
        for a, b in runs(mask[:, f]):
            if b - a < min_run:
                mask[a:b, f] = False
    return mask


def anchors(joints, mask):
    """joints (m,18,3), labels (m,2) -> (m,2,3): on every row of a run the run's mean ankle (summed in row order), NaN elsewhere."""
    joints = np.asarray(joints, np.float64)
    out = np.full((joints.shape[0], 2, 3), np.nan)
    for f, J in enumerate(FEET):
        for a, b in runs(np.asarray(mask)[:, f]):
            s = np.zeros(3)
            for t in range(a, b):
                s = s + joints[t, J]
            out[a:b, f] = s / float(b - a)
    return out


def contact_energy(joints, mask, anc, wc):
    """E_contact of joints (m,18,3) at the anchors anc (m,2,3)."""
    E = 0.0
    for f, J in enumerate(FEET):
        for t in np.flatnonzero(np.asarray(mask)[:, f]):
            d = joints[t, J] - anc[t, f]
            E += 0.5 * wc * float(d @ d)
    return E


def contact_terms(x, mask, anc, wc, want_jac=True):
    """x (m,68) -> E_contact, per-row E (m,), wc D^T D (m,39,39), wc D^T (X - a) (m,39)."""
    m = x.shape[0]
    Et, H, g = np.zeros(m), np.zeros((m, K, K)), np.zeros((m, K))
    for r in range(m):
        if not mask[r].any():
            continue
        X = _fk(x[r])
        D = sc.joint_jacobians(x[r]) if want_jac else None
        for f, J in enumerate(FEET):     # left, then right
            if not mask[r, f]:
                continue
            d = X[J] - anc[r, f]
            Et[r] = Et[r] + 0.5 * wc * ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
            if want_jac:
                H[r] += wc * (D[J].T @ D[J])
                g[r] += wc * (D[J].T @ d)
    return Et.sum(), Et, H, g


@contextlib.contextmanager
def contact(mask, anc, wc):
    """smooth_np.data_terms carries the contact term of ONE identity (labels (m,2), anchors (m,2,3)) inside the block, on top of what
    was bound before (the plain one, or smooth_robust_np.robust's), and that one again after it, whatever happens inside."""
    mask, anc = np.asarray(mask, bool), np.asarray(anc, np.float64)
    before = sm.data_terms

    def bound(x, obs, prs, want_jac=True):
        Ed, Et, H, g = before(x, obs, prs, want_jac)
        Ec, Ect, Hc, gc = contact_terms(x, mask, anc, wc, want_jac)
        Et = Et + Ect
        return Et.sum(), Et, H + Hc, g + gc
    sm.data_terms = bound
    try:
        yield
    finally:
        sm.data_terms = before


def rounds(x, obs, prs, w, mask, wc, n_rounds=1, speed=0.01, min_run=3, ground=None, height=0.15, max_iter=10):
    """The rounds after round 0 of one identity from its trajectory x (m,68).  mask: labels (m,2) or "auto".  -> x, dict(contact (m,2),
    anchor (m,2,3) the last round's, contact_cost [E_contact at the first anchors, at the end], E (E_data without the term, E_prior)
    at the end, round_trials, trace, history: the joint energy E_data + E_contact + E_prior after the anchors of every round and after
    every trial)."""
    x = x.copy()
    trace, hist, per_round = [], [], []
    anc, first = None, 0.0
    for r in range(n_rounds):
        J = np.array([_fk(p) for p in x])
        if r == 0:
            mask = detect(J, speed, min_run, ground, height) if isinstance(mask, str) else np.array(mask, bool)
        anc = anchors(J, mask)
        if not mask.any():       # the identity stays stopped: no trial in this round
            per_round.append(0)
            continue
        if r == 0:
            first = contact_energy(J, mask, anc, wc)
        with contact(mask, anc, wc):
            x, info = sm.lm(x, obs, prs, w, max_iter)
        trace += info["trace"]
        per_round.append(len(info["trace"]))
        hist += info["history"]
    J = np.array([_fk(p) for p in x])
    if anc is None:
        anc = np.full((x.shape[0], 2, 3), np.nan)
    Ed, Ep = sm.energy(x, obs, prs, w)
    return x, dict(contact=np.asarray(mask, bool), anchor=anc, contact_cost=np.array([first, contact_energy(J, mask, anc, wc)]),
                   E=(Ed, Ep), round_trials=per_round, trace=trace, history=hist, joints=J)


def smooth(views, Ps, records, w, contacts="auto", contact_weight=1e6, contact_speed=0.01, contact_min_frames=3, contact_rounds=1,
           ground=None, contact_height=0.15, max_iter=10):
    """smooth_np.smooth with foot contacts: contacts "auto" or per sequence a list aligned with its records (None or (m,2) bool over
    f0..f1).  -> smooth_np.smooth's dicts (round 0 in "round0"), params / joints / cost / trace of the whole call, and contact,
    anchor, contact_cost, round_trials (round 0 first), history_contact."""
    base = sm.smooth(views, Ps, records, w, max_iter)
    out = []
    for s, recs in enumerate(records):
        probs = sc.problems(views[s], Ps[s], recs)
        row = []
        for r, rec in enumerate(recs):
            b = dict(base[s][r])
            b["round0"] = base[s][r]
            m = len(b["frames"])
            if probs[r] is None:
                b.update(contact=np.zeros((1, 2), bool), anchor=np.full((1, 2, 3), np.nan), contact_cost=np.zeros(2), round_trials=[],
                         history_contact=[])
                row.append(b)
                continue
            given = "auto" if isinstance(contacts, str) else contacts[s][r]
            if given is None:
                given = np.zeros((m, 2), bool)
            x, info = rounds(b["params"], probs[r][0], probs[r][1], w, given, contact_weight, contact_rounds, contact_speed,
                             contact_min_frames, ground, contact_height, max_iter)
            b.update(params=x, joints=info["joints"], cost=np.array([b["cost"][0], b["cost"][1], info["E"][0], info["E"][1]]),
                     trace=list(b["trace"]) + info["trace"], contact=info["contact"], anchor=info["anchor"],
                     contact_cost=info["contact_cost"], round_trials=[len(b["trace"])] + info["round_trials"],
                     history_contact=info["history"])
            row.append(b)
        out.append(row)
    return out
