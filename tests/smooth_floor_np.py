"""NumPy restatement of the floor under the trajectory smoother's foot contacts (smoothing.smooth_sequences(contacts=..., floor=...);
csrc/mvmc_smooth_row.h: sm_row_block<LOSS, CONTACT, FLOOR>, csrc/mvmc_smooth_contact.hip: smooth_floor_anchors_kernel) and of
smoothing.estimate_floor.  The labels, the runs and the run means are tests/smooth_contact_np.py's; the device is gated against this file.

The model.  Per sequence a unit floor normal n, T = I - n n^T; per identity ONE level h (metres along n); L the labelled (row, foot)
pairs of the contacts,
  E_contact = 1/2 wc sum_L |T (X_f(x_t) - a_run)|^2 + 1/2 wf sum_L (n . X_f(x_t) - h)^2.
h is minimised in closed form, the mean of n . X_f over L (summed left foot's rows ascending, then the right foot's); the stored anchor
of a row is the point a = T mean_run + n h on the plane, so with c = X_f - a the row's term is 1/2 wc |c|^2 + 1/2 (wf - wc)(n . c)^2:
with D = d X_f / d x_t it adds D^T (wc I + (wf - wc) n n^T) D to the row's J^T J and D^T (wc c + (wf - wc)(n . c) n) to its J^T r.

floor(mask, anc, wc, n, wf) binds smooth_np.data_terms as smooth_contact_np.contact does; level() and project() are the anchors'
second step; rounds() / smooth() are the drivers; estimate() is smoothing.estimate_floor's arithmetic on plain arrays.
"""
import contextlib

import numpy as np

import smooth_contact_np as ct
import smooth_cov_np as sc
import smooth_np as sm

K = sm.K
FEET = ct.FEET
_fk = ct._fk


def unit(n):
    n = np.asarray(n, np.float64)
    return n / np.linalg.norm(n)


def level(joints, mask, n):
    """h = the mean of n . ankle over the labelled pairs, the left foot's rows ascending, then the right foot's; NaN without one."""
    s, cnt = 0.0, 0
    for f, J in enumerate(FEET):
        for t in np.flatnonzero(np.asarray(mask)[:, f]):
            p = joints[t, J]
            s = s + ((n[0] * p[0] + n[1] * p[1]) + n[2] * p[2])
            cnt += 1
    return s / cnt if cnt else np.nan


def project(anc, mask, n, h):
    """The anchors (m,2,3) of the labelled rows moved onto the plane n . a = h along n; the others as they are (NaN)."""
    out = np.array(anc, np.float64, copy=True)
    for f in range(2):
        for t in np.flatnonzero(np.asarray(mask)[:, f]):
            a = out[t, f]
            e = ((n[0] * a[0] + n[1] * a[1]) + n[2] * a[2]) - h
            out[t, f] = a - n * e
    return out


def anchors(joints, mask, n):
    """joints (m,18,3), labels (m,2), unit normal -> (anchors (m,2,3) on the plane, level)."""
    h = level(joints, mask, n)
    a = ct.anchors(joints, mask)
    return (project(a, mask, n, h), h) if np.asarray(mask).any() else (a, np.nan)


def floor_energy(joints, mask, anc, wc, n, wf):
    """E_contact with a floor of joints (m,18,3) at the anchors anc (m,2,3) (on the plane: n . anc = h)."""
    E = 0.0
    for f, J in enumerate(FEET):
        for t in np.flatnonzero(np.asarray(mask)[:, f]):
            c = joints[t, J] - anc[t, f]
            nc = float(n @ c)
            E += 0.5 * wc * float(c @ c) + 0.5 * (wf - wc) * nc * nc
    return E


def energy_at_level(joints, mask, n, h, wc, wf):
    """E_contact written with the run means and a free level h (the model's first form): for the test that h minimises it."""
    mean = ct.anchors(joints, mask)
    T = np.eye(3) - np.outer(n, n)
    E = 0.0
    for f, J in enumerate(FEET):
        for t in np.flatnonzero(np.asarray(mask)[:, f]):
            d = T @ (joints[t, J] - mean[t, f])
            E += 0.5 * wc * float(d @ d) + 0.5 * wf * (float(n @ joints[t, J]) - h) ** 2
    return E


def floor_terms(x, mask, anc, wc, n, wf, want_jac=True):
    """x (m,68) -> E_contact, per-row E (m,), D^T (wc I + (wf - wc) n n^T) D (m,39,39), D^T (wc c + (wf - wc)(n . c) n) (m,39)."""
    m = x.shape[0]
    Et, H, g = np.zeros(m), np.zeros((m, K, K)), np.zeros((m, K))
    W = wc * np.eye(3) + (wf - wc) * np.outer(n, n)
    for r in range(m):
        if not mask[r].any():
            continue
        X = _fk(x[r])
        D = sc.joint_jacobians(x[r]) if want_jac else None
        for f, J in enumerate(FEET):     # left, then right
            if not mask[r, f]:
                continue
            c = X[J] - anc[r, f]
            nc = (n[0] * c[0] + n[1] * c[1]) + n[2] * c[2]
            Et[r] = Et[r] + 0.5 * wc * ((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]) + 0.5 * (wf - wc) * (nc * nc)
            if want_jac:
                H[r] += D[J].T @ W @ D[J]
                g[r] += D[J].T @ (W @ c)
    return Et.sum(), Et, H, g


@contextlib.contextmanager
def floor(mask, anc, wc, n, wf):
    """smooth_np.data_terms carries the contact term about the floor of ONE identity inside the block (smooth_contact_np.contact's
    way: on top of what was bound before, and that one again after it)."""
    mask, anc, n = np.asarray(mask, bool), np.asarray(anc, np.float64), np.asarray(n, np.float64)
    before = sm.data_terms

    def bound(x, obs, prs, want_jac=True):
        Ed, Et, H, g = before(x, obs, prs, want_jac)
        Ec, Ect, Hc, gc = floor_terms(x, mask, anc, wc, n, wf, want_jac)
        Et = Et + Ect
        return Et.sum(), Et, H + Hc, g + gc
    sm.data_terms = bound
    try:
        yield
    finally:
        sm.data_terms = before


def rounds(x, obs, prs, w, mask, wc, n, wf, n_rounds=1, speed=0.01, min_run=3, ground=None, height=0.15, max_iter=10):
    """smooth_contact_np.rounds with a floor: after every round's run means the level and the projection.  -> x, its dict with
    ``level`` (NaN without a contact) and ``levels`` (every round's)."""
    x = x.copy()
    trace, hist, per_round, levels = [], [], [], []
    anc, first, h = None, 0.0, np.nan
    for r in range(n_rounds):
        J = np.array([_fk(p) for p in x])
        if r == 0:
            mask = ct.detect(J, speed, min_run, ground, height) if isinstance(mask, str) else np.array(mask, bool)
        anc, h = anchors(J, mask, n)
        levels.append(h)
        if not mask.any():
            per_round.append(0)
            continue
        if r == 0:
            first = floor_energy(J, mask, anc, wc, n, wf)
        with floor(mask, anc, wc, n, wf):
            x, info = sm.lm(x, obs, prs, w, max_iter)
        trace += info["trace"]
        per_round.append(len(info["trace"]))
        hist += info["history"]
    J = np.array([_fk(p) for p in x])
    if anc is None:
        anc = np.full((x.shape[0], 2, 3), np.nan)
    Ed, Ep = sm.energy(x, obs, prs, w)
    return x, dict(contact=np.asarray(mask, bool), anchor=anc, level=h, levels=levels,
                   contact_cost=np.array([first, floor_energy(J, mask, anc, wc, n, wf) if np.asarray(mask).any() else 0.0]),
                   E=(Ed, Ep), round_trials=per_round, trace=trace, history=hist, joints=J)


def smooth(views, Ps, records, w, contacts="auto", floor_normals=None, floor_weight=None, contact_weight=1e6, contact_speed=0.01,
           contact_min_frames=3, contact_rounds=1, ground=None, contact_height=0.15, max_iter=10):
    """smooth_contact_np.smooth with floor_normals per sequence ((3,) or None: that sequence runs the contacts alone) and
    floor_weight (None: contact_weight).  Adds ``floor_level`` and ``floor_normal`` to the dicts of the sequences with a floor."""
    wf = contact_weight if floor_weight is None else floor_weight
    base = sm.smooth(views, Ps, records, w, max_iter)
    out = []
    for s, recs in enumerate(records):
        n = None if floor_normals is None or floor_normals[s] is None else unit(floor_normals[s])
        probs = sc.problems(views[s], Ps[s], recs)
        row = []
        for r, rec in enumerate(recs):
            b = dict(base[s][r])
            b["round0"] = base[s][r]
            m = len(b["frames"])
            if probs[r] is None:
                b.update(contact=np.zeros((1, 2), bool), anchor=np.full((1, 2, 3), np.nan), contact_cost=np.zeros(2), round_trials=[],
                         history_contact=[], floor_level=np.nan, floor_normal=n)
                row.append(b)
                continue
            given = "auto" if isinstance(contacts, str) else contacts[s][r]
            if given is None:
                given = np.zeros((m, 2), bool)
            if n is None:
                x, info = ct.rounds(b["params"], probs[r][0], probs[r][1], w, given, contact_weight, contact_rounds, contact_speed,
                                    contact_min_frames, ground, contact_height, max_iter)
                info["level"] = np.nan
            else:
                x, info = rounds(b["params"], probs[r][0], probs[r][1], w, given, contact_weight, n, wf, contact_rounds, contact_speed,
                                 contact_min_frames, ground, contact_height, max_iter)
            b.update(params=x, joints=info["joints"], cost=np.array([b["cost"][0], b["cost"][1], info["E"][0], info["E"][1]]),
                     trace=list(b["trace"]) + info["trace"], contact=info["contact"], anchor=info["anchor"],
                     contact_cost=info["contact_cost"], round_trials=[len(b["trace"])] + info["round_trials"],
                     history_contact=info["history"], floor_level=info["level"], floor_normal=n)
            row.append(b)
        out.append(row)
    return out


def estimate(frames, ankles, roots, labels, min_spread=0.05):
    """smoothing.estimate_floor of ONE sequence on plain arrays: per record frames (n,) int, ankles (n,2,3), roots (n,3) (joint 0),
    labels (n,2) bool.  A run is a maximal stretch of consecutive FRAMES with the label set; m_r its mean ankle, len_r its length;
    c_id the length-weighted mean of an identity's m_r over both feet; S = sum len_r (m_r - c_id)(m_r - c_id)^T over all identities;
    n = S's eigenvector of the smallest eigenvalue, oriented so that the mean of n . (root - ankle) over the labelled rows is
    positive.  -> dict(normal, status, spread (3,) = sqrt(eigenvalues / sum len) ascending, rms, levels per record, n_runs)."""
    means, lens, ids, up = [], [], [], []
    for i, (fr, A, R, lab) in enumerate(zip(frames, ankles, roots, labels)):
        fr, lab = np.asarray(fr), np.asarray(lab, bool)
        for f in range(2):
            k = 0
            while k < len(fr):
                if not lab[k, f]:
                    k += 1
                    continue
                e = k + 1
                while e < len(fr) and lab[e, f] and fr[e] == fr[e - 1] + 1:
                    e += 1
                means.append(A[k:e, f].mean(0))
                lens.append(e - k)
                ids.append(i)
                k = e
            up.append((R - A[:, f])[lab[:, f]])
    n_rec = len(frames)
    nan3 = np.full(3, np.nan)
    if not means:
        return dict(normal=nan3, status=2, spread=nan3, rms=np.nan, levels=np.full(n_rec, np.nan), n_runs=0)
    means, lens, ids = np.array(means), np.array(lens, np.float64), np.array(ids)
    S = np.zeros((3, 3))
    for i in np.unique(ids):
        k = ids == i
        c = (lens[k, None] * means[k]).sum(0) / lens[k].sum()
        d = means[k] - c
        S += (lens[k, None, None] * d[:, :, None] * d[:, None, :]).sum(0)
    lam, V = np.linalg.eigh(S)
    lam = np.maximum(lam, 0.0)
    n = V[:, 0]
    if np.concatenate(up).mean(0) @ n < 0:
        n = -n
    spread = np.sqrt(lam / lens.sum())
    status = 0 if len(means) >= 3 and spread[1] >= min_spread else 1
    levels = np.full(n_rec, np.nan)
    for i in np.unique(ids):
        k = ids == i
        levels[i] = (lens[k] * (means[k] @ n)).sum() / lens[k].sum()
    return dict(normal=n, status=status, spread=spread, rms=float(spread[0]), levels=levels, n_runs=len(means))
