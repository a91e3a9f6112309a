"""NumPy restatement of the live smoother's foot contacts (multiview_motion_capture_amd/live_smoothing.py: contacts="auto";
csrc/mvmc_smooth_window.hip: smooth_window_kernel<LOSS, true>), on top of tests/live_smooth_np.py and tests/smooth_contact_np.py.  The
device is gated against this file; this file is the definition of the model.

Per identity and foot f (0 left ankle, 1 right ankle) every row r has a label c[r, f] and an anchor a[r, f] (NaN without a label),
kept beside the row.  Rows appended by a tick have c = 0 during it.

During a tick the window's Levenberg-Marquardt trials (live_smooth_np.lm_window) run under smooth_contact_np.contact's binding of the
free rows' stored labels and anchors (it stacks on smooth_robust_np.robust); history rows carry no term.  E_data of the tick includes
the contact part, as the device's row costs do; contact_cost = [E_contact at the start, at the end] under those labels and anchors.

At the end of a tick of an identity with n >= 2 rows, on the solved values:
  frozen     rows with index <= n - 1 - lag (the emitted row and everything older, also rows a jump of the frame index carried past
             the emit position) keep their label and anchor for good;
  tentative  rows with index > n - 1 - lag are labelled again by smooth_contact_np.detect's rule on the FK joints (one-sided at the
             identity's first row and at the newest row; every neighbour is a free row because the window is longer than the lag);
  runs       over the window's rows (history included, stored labels): a run whose first visible row is frozen keeps that row's stored
             anchor on all its rows and is never dropped; a run without a frozen row is dropped when shorter than min_frames, else its
             anchor is the mean of its rows' solved ankles, summed in row order;
  write-back the tentative rows' labels and anchors are stored.
So a run's anchor moves from tick to tick until the tick that emits its first row, and is constant from then on; a committed run may
end up shorter than min_frames (its tentative tail can be un-labelled later); a row's label exists one tick after the row does (with
lag = 0 a row is emitted before it can be labelled); lag + 1 >= min_frames is required, or no run could reach its length before it
freezes.
"""
import numpy as np

import live_smooth_np as ls
import oracle_np as o
import smooth_contact_np as ct


def _fk(p):
    return o.forward_kinematics(p[:3], p[3:57], p[57:])[0]


class Stream(ls.Stream):
    """live_smooth_np.Stream with the contact state.  tick()'s dict gains ``contact``: track_id -> dict(contact (2,) bool, anchor
    (2,3)) of the emitted row; every ``solved`` entry gains contact_cost; the records gain contact (n,2) and anchor (n,2,3)."""

    def __init__(self, P, window=24, lag=8, n_iter=2, w=(1e4, 1e4, 1e4, 1e4), contact_weight=1e6, contact_speed=0.01,
                 contact_min_frames=3, ground=None, contact_height=0.15):
        super().__init__(P, window, lag, n_iter, w)
        if lag + 1 < contact_min_frames:
            raise ValueError("lag + 1 >= contact_min_frames required")
        self.wc, self.speed, self.min_run, self.ground, self.height = contact_weight, contact_speed, contact_min_frames, ground, contact_height
        self.margin = np.inf        # the smallest |speed - contact_speed| over every tentative row labelled so far (the tests' guard)
        self.seen = dict(dropped=0, kept=0, continued=0)      # tentative runs dropped / given a mean, runs continued from a frozen row

    # -- the contact state rides on the identity: c[r] (2,) bool, a[r] (2,3) --
    @staticmethod
    def _new_row(idn):
        if not hasattr(idn, "c"):
            idn.c, idn.a = [], []
        idn.c.append(np.zeros(2, bool))
        idn.a.append(np.full((2, 3), np.nan))

    def _missing(self, idn):
        super()._missing(idn)
        self._new_row(idn)

    def relabel(self, idn):
        """The end-of-tick rule on the identity's current values."""
        n = len(idn.x)
        m = min(self.W, n)
        lo = n - m - min(2, n - m)
        first = max(n - self.lag, 0)                    # the first tentative row
        a0 = max(first - 1, 0)
        J = np.array([_fk(p) for p in idn.x[a0:]])
        lab = ct.detect(J, self.speed, 1, self.ground, self.height)       # min_run 1: nothing is dropped here
        for i in range(first, n):
            idn.c[i] = lab[i - a0].copy()
            idn.a[i] = np.full((2, 3), np.nan)
            for K in ct.FEET:                           # the guard's figure: the speed detect() compared
                a, b = max(i - 1, 0), min(i + 1, n - 1)
                v = np.linalg.norm(J[b - a0, K] - J[a - a0, K]) * (0.5 if b - a == 2 else 1.0)
                self.margin = min(self.margin, abs(v - self.speed))
        for f, K in enumerate(ct.FEET):
            for s, e in ct.runs([idn.c[i][f] for i in range(lo, n)]):
                s, e = lo + s, lo + e
                if s < first:                           # the run's first visible row is frozen: its stored anchor, never dropped
                    self.seen["continued"] += e > first
                    for i in range(first, e):
                        idn.a[i][f] = idn.a[s][f]
                elif e - s < self.min_run:
                    self.seen["dropped"] += 1
                    for i in range(s, e):
                        idn.c[i][f] = False
                else:
                    self.seen["kept"] += 1
                    acc = np.zeros(3)
                    for i in range(s, e):
                        acc = acc + J[i - a0, K]
                    for i in range(s, e):
                        idn.a[i][f] = acc / float(e - s)

    def _contact_energy(self, rows, cm, an):
        return ct.contact_energy(np.array([_fk(p) for p in rows]), cm, an, self.wc)

    def tick(self, f, views_f, meta, params, joints):
        """live_smooth_np.Stream.tick with the contact binding around the solve and the end-of-tick rule after it (the append, the
        selection and the emit are that method's, line for line)."""
        if self.f_last is not None and f <= self.f_last:
            raise ValueError("frame indices must increase")
        d = 1 if self.f_last is None else f - self.f_last
        if d - 1 >= self.W:
            raise ValueError("frame index jump of a window or more")
        C = self.P.shape[0]
        tids = [int(m[0]) for m in meta]
        finished = [self._finish(self.ids.pop(t)) for t in [t for t in self.ids if t not in tids]]
        is_data = [t not in self.ids or int(meta[k][2]) > self.ids[t].hits for k, t in enumerate(tids)]
        probs = [(0, 0, k, np.asarray(joints[k], np.float64)) for k in range(len(tids)) if is_data[k]]
        sel, _, nv = ls.bf.select(probs, [[views_f]], [self.P]) if probs else (np.zeros((0, C), int), None, np.zeros(0, int))
        at = 0
        emitted, solved, contact = [], {}, {}
        for k, t in enumerate(tids):
            idn = self.ids.get(t)
            if idn is None:
                idn = self.ids[t] = ls._Identity(t, f)
            else:
                for _ in range(d - 1):
                    self._missing(idn)
            if is_data[k]:
                p = np.array(params[k], np.float64).copy()
                if idn.prev_in is not None:
                    p[3:57] = ls.unwrap_towards(idn.prev_in, p[3:57]).ravel()
                idn.prev_in = p[3:57].reshape(18, 3).copy()
                ob, pr = ls.bf.observations(sel[at], views_f, self.P)
                idn.x.append(p)
                idn.data.append(True)
                idn.obs.append(ob if len(ob) else None)
                idn.prs.append(pr if len(ob) else None)
                idn.sel.append(sel[at].copy())
                idn.views.append(int(nv[at]))
                self._new_row(idn)
                at += 1
            else:
                self._missing(idn)
            idn.hits = int(meta[k][2])
            n = len(idn.x)
            m = min(self.W, n)
            h = min(2, n - m)
            idn.n_final = n - m
            if n >= 2:
                lo = n - m - h
                obs = [None] * h + idn.obs[n - m:]
                prs = [None] * h + idn.prs[n - m:]
                cm, an = np.array(idn.c[n - m:]), np.array(idn.a[n - m:])
                e0 = self._contact_energy(idn.x[n - m:], cm, an)
                with ct.contact(cm, an, self.wc):
                    x, info = ls.lm_window(np.array(idn.x[lo:]), h, obs, prs, self.w, self.n_iter)
                for i in range(h, h + m):
                    idn.x[lo + i] = x[i]
                info["contact_cost"] = np.array([e0, self._contact_energy(idn.x[n - m:], cm, an)])
                solved[t] = info
                self.relabel(idn)
            r = f - self.lag - idn.f0
            if r >= 0:
                p = idn.x[r]
                emitted.append((t, f - self.lag, p.copy(), _fk(p), not idn.data[r], idn.views[r]))
                contact[t] = dict(contact=idn.c[r].copy(), anchor=idn.a[r].copy())
        self.f_last = f
        return dict(emitted=emitted, finished=finished, solved=solved, contact=contact)

    @staticmethod
    def _with_contact(rec, idn):
        n = len(rec["frames"])
        rec["contact"] = np.array(idn.c[:n], bool).reshape(n, 2)
        rec["anchor"] = np.array(idn.a[:n], np.float64).reshape(n, 2, 3)
        return rec

    def _finish(self, idn):
        return self._with_contact(super()._finish(idn), idn)

    def records(self):
        return [self._with_contact(idn.record(), idn) for idn in self.ids.values()]

    def window_contact(self, tid):
        """The free rows' labels (m,2) and anchors (m,2,3) of identity ``tid`` as they stand (after a tick: the re-made ones)."""
        idn = self.ids[tid]
        m = min(self.W, len(idn.x))
        return np.array(idn.c[-m:]), np.array(idn.a[-m:])
