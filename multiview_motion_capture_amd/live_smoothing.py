"""Fixed-lag smoothing of live sessions: the trajectory smoother's objective (smoothing.py) on a short sliding window per live identity,
one kernel launch per tick for every identity of every session (include/mvmc.h: mvmc_smooth_window; csrc/mvmc_smooth_window.hip).

Per identity (one tracklet of one session) the rows are the consecutive frames from its first frame f0 to the session's newest.  A row
is a DATA row when the tracker appended a pose for that frame (commit_tables' rule: the tracklet is new or its hits grew), else a
MISSING row.  A data row starts from the tracker's 68 parameters, its Euler triples unwrapped (smoothing.unwrap_euler's rule) towards
the unwrapped INPUT angles of the identity's previous data row, so that the stream of unwrapped inputs equals unwrap_euler of the
complete record; its views are sequences.select_views' selection (mvmc_body_observe on the tracker's joints, MAX_DIST, MIN_SCORE).  A missing row
starts as a copy of the previous row's current values and has no data term.  A session whose frame index jumps by d gets d - 1 missing
rows in every live identity.

Per tick, for every live identity with two rows or more whose session delivered a frame: the last m = min(window, rows) rows are free,
the up to two rows before them are frozen history, and ``n_iter`` Levenberg-Marquardt trials (smoothing.py's rules, mu from LM_MU0,
warm from the rows' current values) minimise the free rows' data terms + every velocity / acceleration term whose stencil touches a
free row.  A row that leaves the window keeps its value for good (final).  The row of frame f_new - lag is emitted.  A tracklet that
leaves the session's table is finished: rows after its last data row are dropped and its record is handed over.

The rows, their members, the row counts and the sessions' rings of the last ``window`` frames' ingested keypoints stay on the device
between ticks.  A tick costs a number of launches that does not depend on sessions or identities (ingest, selection, exactly one
mvmc_smooth_window, FK of the rows read back) and one synchronisation, the read-back.  NumPy restatement: tests/live_smooth_np.py.
INTEGRATION.md section C.5.

loss="huber" / "cauchy" at loss_px pixels puts smoothing.py's robust loss on the window's data terms: the tick's one launch is then
mvmc_smooth_window_robust (the same state, workspace and outputs; ``solved``'s cost holds the robust E_data).  loss=None is the plain
launch, bit for bit.  The live path sets no weights attribute: which keypoints were voted down is the offline smoother's
``smooth_obs_weight``.

covariance="joints" (default None: no extra launch, no new argument to any entry, the same bits) adds ONE launch per tick after the
window's, mvmc_smooth_window_cov (csrc/mvmc_smooth_window_cov.hip; restated in tests/live_smooth_cov_np.py), for every row the tick
emits; its outputs join the tick's one read-back.  At the end of a tick A_w is the matrix the window's LM step factors at the rows'
final values: the free rows' data blocks (with a loss the weighted ones) + the exact Hessian of every prior term that touches a free
row, the history held fixed.  Sigma = (A_w + smoothing.COV_MU diag A_w)^-1, and the emitted row e gets Sigma_ee: per skeleton joint
C_K = D_K Sigma_ee D_K^T and the 39 diagonal entries, scaled by noise_px^2.  This is the covariance CONDITIONAL on the frozen history
(and on the rig, the lengths, the held joints and the view selection) -- what the fixed-lag solve itself assumes.  Conditioning can
only lower a variance, so on the window's rows it is a lower bound on what the offline smoother (smoothing.py: covariance="joints")
would report; the offline smoother of the complete record also sees the frames after the window, which pushes the other way.  The gap
is measured, not promised (tools/live_smooth_cov_probe.py, INTEGRATION.md section C.5: within half a percent at unit variance for lag
8 in a window of 24, on either side).  noise_px given: the recursion stops at the emitted row (lag + 1 of
the window's rows) and edof / nres are not computed (NaN / 0).  noise_px=None: it is estimated per tick and identity over the window's
free rows, sqrt(2 E_data / (n_res - edof)), NaN when that is not positive.  Under a loss the ESTIMATED noise_px is biased low, because
rho <= 1/2 e^2 shrinks E_data while n_res still counts every residual: under a loss noise_px= is the honest choice.

contacts="auto" (default None: the launches, their arguments, the state and the bits are the ones without it) adds smoothing.py's foot
contacts with causal, committed anchors; the tick's one launch is then mvmc_smooth_window_contact (restated in
tests/live_smooth_contact_np.py, which is the definition).  Per identity and foot (0 left ankle, 1 right) every row has a label and an
anchor (3 doubles, NaN without a label), kept beside the row in two more device tensors.  During a tick every free row with a label
adds 1/2 contact_weight |ankle(x_r) - anchor|^2 under its STORED label and anchor (outside the loss); rows appended by the tick have
none yet, history rows carry no term.  At the end of the tick, on the solved values: rows with index <= n - 1 - lag -- the emitted row
and everything older, also rows a jump of the frame index carried past the emit position -- are frozen and keep label and anchor for
good; the rows after them are labelled again (smoothing.py's rule: the ankle's central-difference speed < contact_speed, one-sided at the
identity's first and newest row; with ground=(normal, offset) also its height < contact_height); a run of labelled rows whose first
row in the window is frozen keeps that row's anchor and is never dropped; a run without a frozen row is dropped when shorter than
contact_min_frames, else its anchor is the mean of its rows' solved ankles.  Consequences: a run's anchor moves from tick to tick until
the tick that emits its first row and is constant from then on, so every emitted row of one stance carries one anchor and was solved
and emitted under its final label; a committed run may end up shorter than contact_min_frames (its tentative tail can be un-labelled
later); a row's label exists one tick after the row does, so with lag = 0 a row is emitted before it can be labelled; lag + 1 >=
contact_min_frames is required, or no run could reach its length before it freezes.  ``solved``'s cost counts the contact part in
E_data, as the device's row costs do (the offline smoother subtracts it; here contact_cost gives it).  covariance="joints" with
contacts is mvmc_smooth_window_cov_contact: A_w carries the contact term of the labels and anchors as they stand after the tick, the
covariance is conditional on them as the offline one is.  Measured: tools/live_smooth_contact_probe.py, INTEGRATION.md section C.5.

lengths="auto" (default None: the launches, their arguments, the state and the bits are the ones without it) keeps ONE skeleton per
identity, estimated as frames arrive (restated in tests/live_lengths_np.py, which is the definition; csrc/mvmc_live_lengths.hip).
The tracker's IK fits the 11 side lengths again on every frame, and the window launches solve every row under its own columns 57:68;
two more launches per tick decide what those columns hold, the window launch -- plain, robust or contact -- is unchanged.  Per
identity slot one more device tensor holds A (11x11), b, the current skeleton l, l0 = the lengths of the identity's first row, and
four counters.  mvmc_live_lengths_apply, before the window launch: a new identity starts with A = b = 0 and l = l0; the data row of
every other identity gets l (a missing row copies the previous row, so it carries that row's).  mvmc_live_lengths_update, after the
window launch and before the covariance launch, on the solved values: every row that moved behind the lag (index <= n - 1 - lag;
after a jump of the frame index only the rows the jump appended, the keypoint ring may have lost the older ones), if it is a data row
with two views or more, adds the normal equations of body_fit's length residual in the 11 lengths, linearised at the row's own
lengths -- a quadratic in ABSOLUTE lengths, so rows linearised at different points add up; then (A + lengths_prior I) l = b +
lengths_prior l0 (Cholesky; a failed solve keeps l, status 1; slot 7 has no curvature, the prior holds it at l0) and l goes into
the rows n - lag .. n - 1, which the next tick solves again.  Consequences: the estimate is causal and uses rows up to f - lag; an
emitted pose was solved against the lengths it carries, and it and every older row keep them; with lengths_commit=N the identity
stops updating once N rows have contributed, and from ``committed_row`` (n - lag of that tick) on every row of the identity carries
one bit-identical vector, so bvh_export.save_bvh takes committed_part(record).  lengths_prior is in px^2 / m^2, against a diagonal of
A of about 1e7 after 20 rows; its default is tools/live_lengths_probe.py's choice (profiles/live_lengths_probe.json).
"""
from __future__ import annotations

import math
import time
from dataclasses import dataclass, field
from typing import Dict, List, NamedTuple, Optional, Sequence

import numpy as np

from . import smoothing
from ._cabi import (LIVE_LEN_INFO_DOUBLES, LIVE_LEN_STATE_DOUBLES, N_PARAM, SMOOTH_COV_INFO_DOUBLES, SMOOTH_JOINTS, SMOOTH_K,
                    SMOOTH_LIVE_CONTACT_DOUBLES, SMOOTH_MAX_VIEWS, SMOOTH_WIN_INFO_DOUBLES, SMOOTH_WIN_MAX, SMOOTH_WIN_RING)
from .body_fit import MAX_DIST, MIN_SCORE
from .sequences import frame_buckets, new_record, pose_slot, pose_tuples
from .smoothing import (ANG_ACC, ANG_VEL, CONTACT_HEIGHT, CONTACT_MIN_FRAMES, CONTACT_SPEED, CONTACT_WEIGHT, COV_E_DATA, COV_EDOF, COV_MU,
                        COV_NRES, COV_STATUS, INFO_COST, INFO_STOP, INFO_TRACE, INFO_TRIALS, LM_FTOL, LM_MU0, LM_XTOL, LOSS_PX, ROOT_ACC,
                        ROOT_VEL, check_loss, scale_covariance, unwrap_euler_many)
from .tracker import T_WIDE

ANGLES = slice(3, 3 + 3 * SMOOTH_JOINTS)     # the Euler triples in a row of N_PARAM parameters: after the root, before the lengths
LENGTHS_PRIOR = 100.0  # px^2 / m^2: the weight of the identity's first lengths in the running skeleton (tools/live_lengths_probe.py)
WINDOW_MAX = SMOOTH_WIN_MAX                  # include/mvmc.h: MVMC_SMOOTH_WIN_MAX
N_ITER_MAX = SMOOTH_WIN_INFO_DOUBLES - 8     # include/mvmc.h: "n_iter <= MVMC_SMOOTH_WIN_INFO_DOUBLES - 8"
RING = SMOOTH_WIN_RING                       # include/mvmc.h: MVMC_SMOOTH_WIN_RING
MAX_VIEWS = SMOOTH_MAX_VIEWS                 # include/mvmc.h: MVMC_SMOOTH_MAX_VIEWS
# The columns of the device's outputs and state, each with the line of include/mvmc.h it restates.
# (mvmc_smooth_window's info and mvmc_smooth_window_cov's cinfo have the offline entries' columns: smoothing.INFO_*, COV_*)
STATUS_MALFORMED = 6                         # the stop reason / status of a skipped item, in info, cinfo and linfo alike
# mvmc_smooth_window_contact, cinfo: "label L, R and anchor L (3), R (3) of the row n - 1 - lag (...), E_contact at the start and at
# the end of the tick"
CINFO_LABELS, CINFO_ANCHORS, CINFO_COST = slice(0, 2), slice(2, 8), slice(8, 10)
# mvmc_live_lengths_update, linfo: "{status (...), rows contributed this tick, contributed, committed, committed_row, l (11), 1/2 sum
# r^2 of this tick's contributing rows}"
LINFO_STATUS, LINFO_CONTRIBUTED, LINFO_COMMITTED, LINFO_COMMITTED_ROW, LINFO_LENGTHS = 0, 2, 3, 4, slice(5, 16)
# lens_state: "[77, 88) l, the current skeleton ... 99 next_row 100 contributed 101 committed (0 / 1) 102 committed_row (-1 before)"
LENS_L, LENS_CONTRIBUTED, LENS_COMMITTED_ROW = slice(77, 88), 100, 102
# the names above end where the header's widths (_cabi) end
assert INFO_TRACE + N_ITER_MAX == SMOOTH_WIN_INFO_DOUBLES and CINFO_COST.stop == SMOOTH_LIVE_CONTACT_DOUBLES
assert COV_EDOF < SMOOTH_COV_INFO_DOUBLES and LINFO_LENGTHS.stop + 1 == LIVE_LEN_INFO_DOUBLES
assert LENS_COMMITTED_ROW + 1 == LIVE_LEN_STATE_DOUBLES


def check_parameters(window, lag, n_iter, root_vel, root_acc, ang_vel, ang_acc) -> np.ndarray:
    """LiveSmoother's parameter checks (host only) -> the four prior weights."""
    if int(window) != window or not 2 <= int(window) <= WINDOW_MAX:
        raise ValueError(f"LiveSmoother: 2 <= window <= {WINDOW_MAX} required")
    if int(lag) != lag or not 0 <= int(lag) < int(window):
        raise ValueError("LiveSmoother: 0 <= lag < window required")
    if int(n_iter) != n_iter or not 1 <= int(n_iter) <= N_ITER_MAX:
        raise ValueError(f"LiveSmoother: 1 <= n_iter <= {N_ITER_MAX} required")
    return smoothing.check_prior_weights("LiveSmoother", root_vel, root_acc, ang_vel, ang_acc)


def check_covariance(covariance, noise_px) -> Optional[float]:
    """LiveSmoother's covariance arguments (host only; smooth_sequences' rules) -> noise_px as a float, or None."""
    return smoothing.check_covariance("LiveSmoother", covariance, noise_px)


def check_contacts(contacts, contact_weight, contact_speed, contact_min_frames, ground, contact_height, lag) -> Optional[dict]:
    """LiveSmoother's foot-contact arguments (host only; smooth_sequences' rules for the scalars) -> None, or the launch's dict."""
    if contacts is None:
        return None
    if not (isinstance(contacts, str) and contacts == "auto"):
        raise ValueError(f"LiveSmoother: contacts must be None or \"auto\", got {contacts if isinstance(contacts, (str, bool)) else type(contacts).__name__!r}")
    c = smoothing._check_contact_args("auto", contact_weight, contact_speed, contact_min_frames, 1, ground, contact_height,
                                      who="LiveSmoother")
    if int(lag) + 1 < c.min_frames:
        raise ValueError(f"LiveSmoother: lag + 1 >= contact_min_frames required (lag {int(lag)}, contact_min_frames {c.min_frames}): a "
                         "run could not reach its length before it freezes")
    return dict(lag=int(lag), weight=c.weight, speed=c.speed, min_frames=c.min_frames, ground=c.ground, height=c.height)


def check_lengths(lengths, lengths_prior, lengths_commit) -> Optional[dict]:
    """LiveSmoother's running-skeleton arguments (host only) -> None, or dict(prior, commit) of the update launch.  lengths_prior
    None: LENGTHS_PRIOR; a lengths_prior or a lengths_commit without lengths="auto" is an error, whatever its value."""
    if lengths is not None and not (isinstance(lengths, str) and lengths == "auto"):
        raise ValueError(f"LiveSmoother: lengths must be None or \"auto\", got {lengths if isinstance(lengths, (str, bool)) else type(lengths).__name__!r}")
    if lengths_prior is not None and (not smoothing._number(lengths_prior) or not math.isfinite(lengths_prior) or not lengths_prior > 0):
        raise ValueError(f"LiveSmoother: lengths_prior must be None or a finite number > 0, got {lengths_prior!r}")
    if lengths_commit is not None and (isinstance(lengths_commit, bool) or not isinstance(lengths_commit, (int, np.integer))
                                       or lengths_commit < 1):
        raise ValueError(f"LiveSmoother: lengths_commit must be None or an integer >= 1, got {lengths_commit!r}")
    if lengths is None:
        if lengths_commit is not None or lengths_prior is not None:
            raise ValueError("LiveSmoother: lengths_prior / lengths_commit without lengths=\"auto\" have nothing to act on")
        return None
    return dict(prior=LENGTHS_PRIOR if lengths_prior is None else float(lengths_prior),
                commit=None if lengths_commit is None else int(lengths_commit))


def committed_part(record):
    """The part of a lengths="auto" record from its ``live_lengths_committed_row`` on: a record whose rows share one bit-identical
    bone-length vector (bvh_export.save_bvh takes it), its per-row attributes (smooth_*) cut to the same rows; ``hits`` counts the
    data rows kept (the rows not in smooth_filled), as a record's hits count the poses the tracker appended.  ValueError when the
    identity never committed (no lengths_commit, too few rows, or not a record of such a smoother)."""
    c = getattr(record, "live_lengths_committed_row", None)
    n = len(getattr(record, "poses", ()))
    if c is None or c < 0 or c >= n:
        raise ValueError("committed_part: the record has no committed skeleton (LiveSmoother(lengths=\"auto\", lengths_commit=N), and N "
                         "rows must have contributed)")
    c = int(c)
    filled = getattr(record, "smooth_filled", None)
    t = new_record(record.track_id, list(record.poses[c:]), src=record, hits=n - c if filled is None else int((~filled[c:]).sum()))
    for name, v in vars(record).items():
        if name.startswith("smooth_") and isinstance(v, np.ndarray) and v.shape[:1] == (n,):
            setattr(t, name, v[c:].copy())
    t.live_lengths, t.live_lengths_rows, t.live_lengths_committed_row = record.live_lengths.copy(), record.live_lengths_rows, 0
    return t


def cov_entry(jc6, pv, ci, noise_px: Optional[float]) -> dict:
    """One emitted row's unit-variance device outputs (jcov (18,6), pvar (39,), cinfo (8,)) -> its TickOutput.cov entry."""
    status, e_data, n_res, edof = int(ci[COV_STATUS]), float(ci[COV_E_DATA]), float(ci[COV_NRES]), float(ci[COV_EDOF])
    s, joint_cov, joint_sigma, param_sigma = scale_covariance(jc6, pv, status, e_data, n_res, edof, noise_px)
    return dict(joint_cov=joint_cov, joint_sigma=joint_sigma, param_sigma=param_sigma, noise_px=s, edof=edof,
                nres=int(n_res) if status == 0 and math.isfinite(n_res) else 0, status=status)


class ReadBack:
    """One read-back of several device tensors: they are registered under a name, fetch() concatenates them as float64, copies the
    result to the host ONCE -- the caller's one synchronisation -- and hands the parts back by name in their registered shapes (views
    of the one host array; integer and bool parts come back as float64)."""

    def __init__(self):
        self._parts: Dict[str, tuple] = {}

    def add(self, name: str, tensor, shape=None) -> None:
        """Registers ``tensor`` (any dtype that float64 holds exactly) under ``name``; ``shape``: the shape to hand back, default its own."""
        if name in self._parts:
            raise ValueError(f"ReadBack: the part {name!r} is registered twice")
        self._parts[name] = (tensor, tuple(tensor.shape if shape is None else shape))

    def fetch(self) -> Dict[str, np.ndarray]:
        import torch
        if not self._parts:
            return {}
        host = torch.cat([t.to(torch.float64).reshape(-1) for t, _ in self._parts.values()]).cpu().numpy()
        out, at = {}, 0
        for name, (t, shape) in self._parts.items():
            out[name] = host[at:at + t.numel()].reshape(shape)
            at += t.numel()
        return out


class TickOutput:
    """One session's results of one tick.  ``emitted``: [(track_id, frame_idx, PoseShapeParam, Pose (FK joints), filled, views)] for
    frame idx - lag, in the table's order; ``finished``: the records of the tracklets that died this tick; ``solved``: track_id ->
    dict(cost [E_data, E_prior at the start, E_data, E_prior at the end], trials [1 accepted / 0 rejected], stop); ``cov``: empty
    unless the smoother has covariance="joints", then track_id -> dict(joint_cov (18,3,3) m^2, joint_sigma (18,) m, param_sigma (39,),
    noise_px, edof, nres, status 0 solved / 1 singular / 2 a one-row identity (NaN arrays)) of the emitted row, conditional on the
    window's frozen history (the module's docstring); ``contact``: empty unless the smoother has contacts="auto", then track_id ->
    dict(contact (2,) bool, anchor (2,3) m, NaN without a label) of the emitted row, and every ``solved`` entry has contact_cost =
    [E_contact at the start, at the end] of the tick -- its cost's E_data INCLUDES the contact part, as the device's row costs do;
    ``lengths``: empty unless the smoother has lengths="auto", then track_id -> dict(lengths (11,) the running skeleton after the tick,
    contributed (rows so far), committed, committed_row (-1 before), status 0 / 1 the tick's solve failed and the skeleton was kept)."""

    def __init__(self):
        self.emitted: list = []
        self.finished: list = []
        self.solved: Dict[int, dict] = {}
        self.cov: Dict[int, dict] = {}
        self.contact: Dict[int, dict] = {}
        self.lengths: Dict[int, dict] = {}


class _Ident:
    def __init__(self, tid: int, slot: int, f0: int):
        self.tid, self.slot, self.f0 = tid, slot, f0
        self.hits, self.state = -1, 1
        self.prev_in: Optional[np.ndarray] = None      # the unwrapped INPUT angles of the last data row (18,3)
        self.filled: List[bool] = []
        self.views: List[int] = []
        self.sel: List[Optional[np.ndarray]] = []
        self.params: List[Optional[np.ndarray]] = []   # a row's values once it is final (None before)
        self.joints: List[Optional[np.ndarray]] = []
        self.cov: Dict[int, tuple] = {}                # row -> (joint_sigma, param_sigma, noise_px) as emitted (covariance="joints")
        self.contact: Dict[int, tuple] = {}            # row -> (labels (2,) bool, anchors (2,3)) once it is final (contacts="auto")
        self.len: Optional[tuple] = None               # (skeleton (11,), rows contributed, committed_row) after its last tick (lengths="auto")
        self.n_final = 0

    @property
    def n(self) -> int:
        return len(self.filled)

    def append(self, data: bool, C: int) -> None:
        self.filled.append(not data)
        self.views.append(0)
        self.sel.append(-np.ones(C, np.int32))
        self.params.append(None)
        self.joints.append(None)

    def last_data(self) -> int:
        return max(i for i, f in enumerate(self.filled) if not f) + 1


class _Session:
    def __init__(self, key, s: int, calibs):
        self.key, self.s, self.calibs = key, s, list(calibs)
        self.f_last: Optional[int] = None
        self.ids: Dict[int, _Ident] = {}


class _Problem(NamedTuple):
    """One selection problem of a tick: a data row's joints against the frame its session delivered."""
    ring: int                 # the frame's place in the keypoint ring
    rig: int
    joints: np.ndarray        # (18,3) the tracker's
    slot: int                 # the identity's row in the session's table


class _Stepped(NamedTuple):
    """An identity a tick steps, in the order of the tick's items."""
    key: object
    idn: _Ident
    f: int
    emit_row: int             # the row of frame f - lag, negative: nothing is emitted yet
    was_final: int            # the identity's final rows before the tick


@dataclass
class _TickPlan:
    """What the host packs for one tick (LiveSmoother._pack) and hands to the launches and to the collection of the results."""
    kps: np.ndarray                                      # (sessions, C, P, 25|17, 3) the delivered frames
    counts: np.ndarray                                   # (sessions, C)
    ring_at: np.ndarray                                  # (sessions,) their places in the keypoint ring
    items: list = field(default_factory=list)            # per stepped identity the 8 ints of include/mvmc.h's window item
    new_rows: list = field(default_factory=list)         # [(identity, params (68,))] the tick's data rows, the items' src
    problems: List[_Problem] = field(default_factory=list)     # one per data row
    stepped: List[_Stepped] = field(default_factory=list)      # one per item
    finished: list = field(default_factory=list)         # [(key, identity)] the tracklets that left their session's table
    want_fin: list = field(default_factory=list)         # [(identity, row)] read back: the finished identities' rows not final yet
    want: list = field(default_factory=list)             # then per item the rows that leave the window and the emitted row
    cov_of: list = field(default_factory=list)           # the items (indices into stepped) whose emitted row gets a covariance


class LiveSmoother:
    """``capacity`` sessions of ``n_views`` cameras, up to tracker.T_WIDE live identities each."""

    def __init__(self, n_views: int, capacity: int, p_max: int = 8, window: int = 24, lag: int = 8, n_iter: int = 2,
                 root_vel: float = ROOT_VEL, root_acc: float = ROOT_ACC, ang_vel: float = ANG_VEL, ang_acc: float = ANG_ACC,
                 device=None, skeleton=None, loss: Optional[str] = None, loss_px: float = LOSS_PX, covariance: Optional[str] = None,
                 noise_px: Optional[float] = None, contacts: Optional[str] = None, contact_weight: float = CONTACT_WEIGHT,
                 contact_speed: float = CONTACT_SPEED, contact_min_frames: int = CONTACT_MIN_FRAMES, ground=None,
                 contact_height: float = CONTACT_HEIGHT, lengths: Optional[str] = None, lengths_prior: Optional[float] = None,
                 lengths_commit: Optional[int] = None):
        self.w = check_parameters(window, lag, n_iter, root_vel, root_acc, ang_vel, ang_acc)
        self._ct = check_contacts(contacts, contact_weight, contact_speed, contact_min_frames, ground, contact_height, lag)
        self._noise_px = check_covariance(covariance, noise_px)
        self._len = check_lengths(lengths, lengths_prior, lengths_commit)
        self._cov = covariance is not None
        loss_px = check_loss("LiveSmoother", loss, loss_px)
        self._rob = dict(loss=loss, loss_px=loss_px) if loss is not None else {}     # loss=None: the launch without the arguments
        if int(capacity) < 1 or not 1 <= int(n_views) <= MAX_VIEWS or int(p_max) < 1:
            raise ValueError(f"LiveSmoother: capacity >= 1, 1 <= n_views <= {MAX_VIEWS} and p_max >= 1 required")
        self.C, self.P, self.capacity = int(n_views), int(p_max), int(capacity)
        self.W, self.lag, self.n_iter = int(window), int(lag), int(n_iter)
        self.device, self.skeleton = device, skeleton
        self._sessions: Dict[object, _Session] = {}
        self._free_s = list(range(self.capacity))
        self._free_id = list(range(self.capacity * T_WIDE))
        self._next_key = 0
        self._Pm_h = np.zeros((self.capacity, self.C, 3, 4))
        self._Pm_dirty = True
        self._st = None        # the device state, allocated by the first tick
        self._pool = None
        self._stage = None
        self.timings = dict(pack=0.0, launch=0.0, records=0.0)   # seconds by part of a tick, accumulated (the probe's split)

    @classmethod
    def for_pool(cls, pool, **kw) -> "LiveSmoother":
        """A smoother that follows ``pool``'s sessions (their sids are its keys; a session is opened here on its first tick).  The
        pool itself is not changed: call update_4d / update_4d_arrays after the pool's, with the same arguments."""
        sm = cls(pool.C, pool.capacity, p_max=pool.P, device=pool.device, **kw)
        sm._pool = pool
        return sm

    # -- sessions ----------------------------------------------------------------------------------------------------------------------
    def open_session(self, calibs, key=None):
        """A new session on the rig ``calibs`` (one Calib per camera); returns its key (host only: the rig is uploaded by the next tick)."""
        if len(calibs) != self.C:
            raise ValueError(f"open_session: {len(calibs)} cameras, the smoother's sessions have {self.C}")
        from .lens import require_pinhole
        require_pinhole(calibs, "LiveSmoother.open_session")
        if not self._free_s:
            raise ValueError(f"open_session: all {self.capacity} session slots are taken")
        if key is None:
            while self._next_key in self._sessions:
                self._next_key += 1
            key = self._next_key
        if key in self._sessions:
            raise ValueError(f"open_session: session {key} is open")
        P = np.array([np.asarray(c.P, np.float64).reshape(3, 4) for c in calibs])
        s = self._free_s.pop(0)
        self._Pm_h[s] = P
        self._Pm_dirty = True
        self._sessions[key] = _Session(key, s, calibs)
        return key

    def _session(self, key, what: str) -> _Session:
        if key not in self._sessions:
            raise ValueError(f"{what}: no open session {key}")
        return self._sessions[key]

    @property
    def keys(self) -> list:
        return list(self._sessions)

    # -- device state ------------------------------------------------------------------------------------------------------------------
    def _state(self):
        import torch
        if self._st is None:
            if self.device is None:
                from .motion_capture import _d
                self.device = _d()
            d = torch.device(self.device)
            n_slots = self.capacity * T_WIDE
            self._st = dict(
                d=d, kps=torch.zeros((self.capacity * self.W, self.C, self.P, 17, 3), dtype=torch.float64, device=d),
                cnt=torch.zeros((self.capacity * self.W, self.C), dtype=torch.int32, device=d),
                rows=torch.zeros((n_slots, RING, N_PARAM), dtype=torch.float64, device=d),
                members=torch.full((n_slots, RING, self.C), -1, dtype=torch.int32, device=d),
                count=torch.zeros((n_slots, 2), dtype=torch.int32, device=d), Pm=None)
            if self._ct is not None:      # per row and foot a label and an anchor, beside the rows
                self._st["clab"] = torch.zeros((n_slots, RING, 2), dtype=torch.int32, device=d)
                self._st["canc"] = torch.full((n_slots, RING, 2, 3), math.nan, dtype=torch.float64, device=d)
            if self._len is not None:     # per slot the running skeleton's A, b, l, l0 and counters (include/mvmc.h)
                self._st["lens"] = torch.zeros((n_slots, LIVE_LEN_STATE_DOUBLES), dtype=torch.float64, device=d)
        if self._Pm_dirty:
            self._st["Pm"] = torch.from_numpy(self._Pm_h.copy()).to(self._st["d"])
            self._Pm_dirty = False
        return self._st

    def _gather(self, st, wanted, T) -> dict:
        """[(ident, row)] -> their rows (n,68) as they stand on the device, with contacts also their labels (n,2) and anchors (n,2,3):
        device tensors, nothing is read back."""
        idx = T(np.array([i.slot * RING + r % RING for i, r in wanted], np.int64))
        g = dict(rows=st["rows"].flatten(0, 1).index_select(0, idx))      # (slot, ring position) -> one axis
        if self._ct is not None:
            g["labels"] = st["clab"].flatten(0, 1).index_select(0, idx)
            g["anchors"] = st["canc"].flatten(0, 1).index_select(0, idx)
        return g

    def _read_rows(self, rb: ReadBack, gathered: list) -> None:
        """Registers the rows of _gather's results, one after the other, their FK joints and (with contacts) their labels and anchors
        as "rows" (n,68), "joints" (n,18,3), "labels" (n,2), "anchors" (n,2,3)."""
        import torch

        from . import device as dev
        cat = lambda name: torch.cat([g[name] for g in gathered]) if len(gathered) > 1 else gathered[0][name]
        rows = cat("rows")
        rb.add("rows", rows)
        rb.add("joints", dev.fk(rows, self.skeleton))
        if self._ct is not None:
            rb.add("labels", cat("labels"))
            rb.add("anchors", cat("anchors"))

    def _fetch(self, wanted):
        """[(ident, row)] -> per row (params (68,), joints (18,3)) as they stand on the device (one read-back); with contacts also the
        row's labels (2,) bool and anchors (2,3)."""
        from . import device as dev
        if not wanted:
            return []
        st = self._state()
        rb = ReadBack()
        self._read_rows(rb, [self._gather(st, wanted, dev.uploader(st["d"]))])
        h = rb.fetch()
        if self._ct is None:
            return list(zip(h["rows"], h["joints"]))
        return list(zip(h["rows"], h["joints"], h["labels"] != 0, h["anchors"]))

    # -- ticks -------------------------------------------------------------------------------------------------------------------------
    def _check_table(self, key, f, inputs, meta, params, joints):
        sess = self._sessions[key]
        if int(f) != f:
            raise ValueError(f"session {key}: the frame index must be an integer")
        if sess.f_last is not None:
            if f <= sess.f_last:
                raise ValueError(f"session {key}: frame index {f} does not increase (the last was {sess.f_last})")
            if f - sess.f_last - 1 >= self.W:
                raise ValueError(f"session {key}: frame index jumps from {sess.f_last} to {f}, a window ({self.W}) or more")
        try:
            kps, cnt = inputs
        except (TypeError, ValueError):
            raise ValueError(f"session {key}: frame_inputs must be (kps (C,P,25|17,3), counts (C,))") from None
        kps, cnt = np.asarray(kps), np.asarray(cnt)
        if kps.ndim != 4 or kps.shape[0] != self.C or kps.shape[2] not in (17, 25) or kps.shape[3] != 3 or kps.shape[1] > self.P:
            raise ValueError(f"session {key}: kps {kps.shape}, expected ({self.C}, P <= {self.P}, 25|17, 3)")
        if cnt.shape != (self.C,) or np.any(cnt < 0) or np.any(cnt > kps.shape[1]):
            raise ValueError(f"session {key}: counts must be ({self.C},) with 0 <= counts <= {kps.shape[1]}")
        meta, params, joints = np.asarray(meta), np.asarray(params, np.float64), np.asarray(joints, np.float64)
        n = meta.shape[0] if meta.ndim == 2 else -1
        if meta.ndim != 2 or meta.shape[1] != 4 or params.shape != (n, N_PARAM) or joints.shape != (n, SMOOTH_JOINTS, 3):
            raise ValueError(f"session {key}: the table must be meta (n,4), params (n,68), joints (n,18,3)")
        if n > T_WIDE:
            raise ValueError(f"session {key}: {n} live identities, at most {T_WIDE}")
        if len(set(int(t) for t in meta[:, 0])) != n:
            raise ValueError(f"session {key}: a track_id appears twice in the table")
        if not (np.all(np.isfinite(params)) and np.all(np.isfinite(joints))):
            raise ValueError(f"session {key}: parameters and joints must be finite")
        return kps, cnt.astype(np.int32), meta.astype(np.int64), params, joints

    def update_tables(self, tables: Dict[object, tuple], failed=()) -> Dict[object, TickOutput]:
        """One tick: tables[key] = (frm_idx, (kps (C,P,25|17,3), counts (C,)), meta (n,4), params (n,68), joints (n,18,3)) -- the frame's
        2-D poses and the rows commit_tables takes -- for every session that delivered a frame.  A key in ``failed`` is not stepped."""
        t_start = time.perf_counter()
        for key in tables:
            self._session(key, "update_tables")
        work = []
        for key, row in tables.items():
            if key in failed:
                continue
            try:
                f, inputs, meta, params, joints = row
            except (TypeError, ValueError):
                raise ValueError(f"session {key}: expected (frm_idx, frame_inputs, meta, params, joints)") from None
            work.append((key, int(f)) + self._check_table(key, f, inputs, meta, params, joints))
        out = {key: TickOutput() for key, *_ in work}
        if not work:
            return out
        if len({w[2].shape[2] for w in work}) != 1:
            raise ValueError("update_tables: the sessions of one tick must all deliver 25-row or all 17-row poses")
        st = self._state()
        plan = self._pack(work)
        t_pack = time.perf_counter()
        host = self._launch(plan, st).fetch()      # the tick's one synchronisation
        t_launch = time.perf_counter()
        self._collect(plan, host, out)
        t_end = time.perf_counter()
        self.timings["pack"] += t_pack - t_start
        self.timings["launch"] += t_launch - t_pack
        self.timings["records"] += t_end - t_launch
        return out

    def _pack(self, work) -> _TickPlan:
        """Stage 1, host: the checked tables [(key, f, kps, counts, meta, params, joints)] -> the tick's rows, items and selection
        problems, and which rows are wanted back.  The identities' host records grow here; the device is not touched."""
        C, W = self.C, self.W
        plan = _TickPlan(kps=np.zeros((len(work), C, self.P, work[0][2].shape[2], 3)), counts=np.zeros((len(work), C), np.int32),
                         ring_at=np.zeros(len(work), np.int64))
        items, new_rows, problems, stepped = plan.items, plan.new_rows, plan.problems, plan.stepped
        for i, (key, f, kps, cnt, meta, params, joints) in enumerate(work):
            sess = self._sessions[key]
            dd = 1 if sess.f_last is None else f - sess.f_last
            plan.kps[i, :, :kps.shape[1]] = kps
            plan.counts[i] = cnt
            plan.ring_at[i] = sess.s * W + f % W
            tids = [int(t) for t in meta[:, 0]]
            for tid in [t for t in sess.ids if t not in tids]:
                plan.finished.append((key, sess.ids.pop(tid)))
            for k, tid in enumerate(tids):
                idn = sess.ids.get(tid)
                new = idn is None
                if new:
                    idn = sess.ids[tid] = _Ident(tid, self._free_id.pop(0), f)
                data = new or int(meta[k, 2]) > idn.hits
                for _ in range(0 if new else dd - 1):
                    idn.append(False, C)
                idn.append(data, C)
                idn.hits, idn.state = int(meta[k, 2]), int(meta[k, 1])
                if data:
                    new_rows.append((idn, params[k].copy()))
                    problems.append(_Problem(int(plan.ring_at[i]), sess.s, joints[k], k))
                # include/mvmc.h, an item: {slot, rig, d, is_data, reset, src, first_frame, work_row}
                items.append([idn.slot, sess.s, dd, int(data), int(new), len(new_rows) - 1 if data else -1, f, len(items) * W])
                stepped.append(_Stepped(key, idn, f, f - self.lag - idn.f0, idn.n_final))
            sess.f_last = f
        pairs = [(idn, p) for idn, p in plan.new_rows if idn.prev_in is not None]
        un = unwrap_euler_many([np.stack([idn.prev_in, p[ANGLES].reshape(SMOOTH_JOINTS, 3)]) for idn, p in pairs])
        for (idn, p), u in zip(pairs, un):
            p[ANGLES] = u[1].ravel()
        for idn, p in plan.new_rows:
            idn.prev_in = p[ANGLES].reshape(SMOOTH_JOINTS, 3).copy()
        # rows wanted back: the finished identities' rows that are not final yet (gathered before the launch, their slots are free
        # for the tick's new identities), then per item the rows that leave the window and the emitted row
        for key, idn in plan.finished:
            plan.want_fin += [(idn, r) for r in range(idn.n_final, idn.last_data())]
            self._free_id.append(idn.slot)
        self._free_id.sort()
        for s in plan.stepped:
            nf = s.idn.n - min(W, s.idn.n)
            plan.want += [(s.idn, r) for r in range(s.idn.n_final, nf)]
            s.idn.n_final = nf
            if s.emit_row >= 0:
                plan.want.append((s.idn, s.emit_row))
        if self._cov:      # the emitted rows get a covariance; no launch when nothing is emitted (or it is not asked for)
            plan.cov_of = [a for a, s in enumerate(plan.stepped) if s.emit_row >= 0]
        return plan

    def _launch(self, plan: _TickPlan, st) -> ReadBack:
        """Stage 2, device: ingest into the sessions' rings, selection, the optional skeleton apply, ONE window launch, the optional
        skeleton update and covariance launches, and the gathers of the rows wanted back.  Nothing is synchronised: what the host
        needs is registered in the ReadBack this returns."""
        import torch

        from . import device as dev
        d, C, W = st["d"], self.C, self.W
        T = dev.uploader(d)
        rb = ReadBack()
        k17, c17 = dev.ingest(T(plan.kps), T(plan.counts))
        at_d = T(plan.ring_at)
        st["kps"].index_copy_(0, at_d, k17)
        st["cnt"].index_copy_(0, at_d, c17)
        ct = None if self._ct is None else dict(labels=st["clab"], anchors=st["canc"], **self._ct)
        ln = self._len
        # the finished identities' rows (with contacts their labels and anchors too), gathered before the launch
        gathered = [self._gather(st, plan.want_fin, T)] if plan.want_fin else []
        # the finished identities' skeletons, gathered before the apply launch as their rows are (the apply resets a reused slot): a
        # finished record reports the device's state itself.  (The host's copy from the identity's last report, idn.len, holds the
        # same values, since the state changes only in a tick that reports it; tracklets() and close_session use that copy.)
        if ln is not None and plan.finished:
            lens_fin = st["lens"].index_select(0, T(np.array([idn.slot for _, idn in plan.finished], np.int64)))
        if plan.new_rows:
            frame_of = np.array([p.ring for p in plan.problems], np.int32)
            order, lo, hi = frame_buckets(frame_of)
            mem_d, nv_d, _, _ = dev.body_observe(st["kps"], st["cnt"], st["Pm"], T(frame_of),
                                                 T(np.array([p.rig for p in plan.problems], np.int32)),
                                                 T(np.array([p.joints for p in plan.problems])), T(order), T(lo), T(hi),
                                                 T(np.array([p.slot for p in plan.problems], np.int32)), MAX_DIST, MIN_SCORE)
            newp_d = T(np.array([p for _, p in plan.new_rows]))
        else:
            mem_d = torch.zeros((0, C), dtype=torch.int32, device=d)
            nv_d = torch.zeros((0,), dtype=torch.int32, device=d)
            newp_d = torch.zeros((0, N_PARAM), dtype=torch.float64, device=d)
        if plan.items:
            items_d = T(np.array(plan.items, np.int32))
            if ln is not None:      # the running skeletons into the tick's data rows, a new identity's state from its row
                dev.live_lengths_apply(items_d, newp_d, st["lens"])
            args = (st["kps"], st["Pm"], items_d, newp_d, mem_d, st["rows"], st["members"], st["count"], W,
                    self.n_iter, self.w, LM_MU0, LM_FTOL, LM_XTOL, self.skeleton)
            if ct is None:
                rb.add("info", dev.smooth_window(*args, **self._rob))
            else:
                info, cinfo = dev.smooth_window(*args, **self._rob, contact=ct)
                rb.add("info", info)
                rb.add("cinfo", cinfo)
            if ln is not None:      # the rows that moved behind the lag into the skeletons, the skeletons into the rows after them
                rb.add("linfo", dev.live_lengths_update(st["kps"], st["Pm"], items_d, st["rows"], st["members"], st["count"], self.lag,
                                                        ln["prior"], ln["commit"], st["lens"], self.skeleton))
        if ln is not None and plan.finished:
            rb.add("lens_fin", lens_fin)
        if plan.cov_of:      # the covariance of the emitted rows: ONE launch for all of them
            # include/mvmc.h, a covariance item: {slot, rig, emit_row, work_row}
            citems = [[plan.stepped[a].idn.slot, self._sessions[plan.stepped[a].key].s, plan.stepped[a].emit_row, k * W]
                      for k, a in enumerate(plan.cov_of)]
            jcov, pvar, cinfo = dev.smooth_window_cov(st["kps"], st["Pm"], T(np.array(citems, np.int32)), st["rows"], st["members"],
                                                      st["count"], W, self.w, COV_MU, self._noise_px is None, self.skeleton,
                                                      **self._rob, **({} if ct is None else dict(contact=ct)))
            rb.add("jcov", jcov)
            rb.add("pvar", pvar)
            rb.add("cov_info", cinfo)
        if plan.want:
            gathered.append(self._gather(st, plan.want, T))
        if gathered:
            self._read_rows(rb, gathered)
        rb.add("members", mem_d)
        rb.add("n_views", nv_d)
        return rb

    def _collect(self, plan: _TickPlan, host: Dict[str, np.ndarray], out: Dict[object, TickOutput]) -> None:
        """Stage 3, host: the read-back into the identities' records, the finished records and the sessions' TickOutputs."""
        ct, ln = self._ct is not None, self._len is not None
        for (key, idn), S in zip(plan.finished, host.get("lens_fin", ())):
            idn.len = (S[LENS_L].copy(), int(S[LENS_CONTRIBUTED]), int(S[LENS_COMMITTED_ROW]))
        nv_h = host["n_views"].astype(np.int64)
        sel_h = pose_slot(host["members"].astype(np.int64), self.P)
        for b, (idn, _) in enumerate(plan.new_rows):
            idn.views[-1], idn.sel[-1] = int(nv_h[b]), sel_h[b]
        P_h, J_h = host.get("rows"), host.get("joints")
        L_h, A_h = (host["labels"] != 0, host["anchors"]) if ct and P_h is not None else (None, None)
        got = {(id(idn), r): k for k, (idn, r) in enumerate(plan.want_fin + plan.want)}

        def final(idn, lo, hi):      # rows lo .. hi - 1 keep the values read back for good
            for r in range(lo, hi):
                k = got[(id(idn), r)]
                idn.params[r], idn.joints[r] = P_h[k].copy(), J_h[k].copy()
                if ct:
                    idn.contact[r] = (L_h[k].copy(), A_h[k].copy())
        for key, idn in plan.finished:
            keep = idn.last_data()
            final(idn, idn.n_final, keep)
            idn.n_final = keep
            out[key].finished.append(self._record(idn, keep, 3))
        emit = []
        info, cinfo, linfo = host.get("info"), host.get("cinfo"), host.get("linfo")
        for a, (key, idn, f, r, was_final) in enumerate(plan.stepped):
            final(idn, was_final, idn.n_final)
            if idn.n >= 2:
                inf = info[a]
                if int(inf[INFO_STOP]) == STATUS_MALFORMED:
                    raise RuntimeError(f"session {key}, identity {idn.tid}: the device skipped a malformed item")
                out[key].solved[idn.tid] = dict(cost=inf[INFO_COST].copy(),
                                                trials=[int(v) for v in inf[INFO_TRACE:INFO_TRACE + int(inf[INFO_TRIALS])]],
                                                stop=int(inf[INFO_STOP]))
                if ct:
                    out[key].solved[idn.tid]["contact_cost"] = cinfo[a, CINFO_COST].copy()
            if ln:
                lin = linfo[a]
                if int(lin[LINFO_STATUS]) == STATUS_MALFORMED:
                    raise RuntimeError(f"session {key}, identity {idn.tid}: the device skipped a malformed skeleton item")
                q = out[key].lengths[idn.tid] = dict(lengths=lin[LINFO_LENGTHS].copy(), contributed=int(lin[LINFO_CONTRIBUTED]),
                                                     committed=bool(lin[LINFO_COMMITTED]), committed_row=int(lin[LINFO_COMMITTED_ROW]),
                                                     status=int(lin[LINFO_STATUS]))
                idn.len = (q["lengths"], q["contributed"], q["committed_row"])
            if r >= 0 and ct:
                cin = cinfo[a]
                out[key].contact[idn.tid] = dict(contact=cin[CINFO_LABELS] != 0, anchor=cin[CINFO_ANCHORS].reshape(2, 3).copy())
            if r >= 0:
                emit.append((key, idn.tid, f - self.lag, got[(id(idn), r)], bool(idn.filled[r]), int(idn.views[r])))
        for k, a in enumerate(plan.cov_of):
            key, idn, f, r, _ = plan.stepped[a]
            if int(host["cov_info"][k, COV_STATUS]) == STATUS_MALFORMED:
                raise RuntimeError(f"session {key}, identity {idn.tid}: the device skipped a malformed covariance item")
            c = out[key].cov[idn.tid] = cov_entry(host["jcov"][k], host["pvar"][k], host["cov_info"][k], self._noise_px)
            idn.cov[r] = (c["joint_sigma"], c["param_sigma"], c["noise_px"])
        if emit:      # the tick's emitted poses in one pass
            ks = [e[3] for e in emit]
            for (key, tid, _, _, filled, views), pose in zip(emit, pose_tuples([e[2] for e in emit], P_h[ks], J_h[ks])):
                out[key].emitted.append((tid,) + pose + (filled, views))

    # -- the pool route ----------------------------------------------------------------------------------------------------------------
    def _pool_table(self, sid, fi):
        """A session's table of frame fi from the pool's public records after its tick."""
        s = self._pool.session(sid)
        if sid not in self._sessions:
            self.open_session(s.calibs, key=sid)
        trs = list(s.tracklets)
        meta = np.zeros((len(trs), 4), np.int64)
        params = np.zeros((len(trs), 68))
        joints = np.zeros((len(trs), 18, 3))
        for k, t in enumerate(trs):
            meta[k] = (t.track_id, int(getattr(t.state, "value", t.state)), t.hits, len(t))
            q = t.poses[-1]
            params[k] = np.concatenate([np.ravel(q[1].root), np.ravel(q[1].euler_angles), np.ravel(q[1].bone_lens)])
            joints[k] = q[2].keypoints
            if t.frame_idxs[-1] != fi and sid in self._sessions and t.track_id not in self._sessions[sid].ids:
                raise ValueError(f"session {sid}: tracklet {t.track_id} is unknown and has no pose at frame {fi}: call update_4d after "
                                 "every tick of the pool")
        return meta, params, joints

    def update_4d(self, frames: Dict[int, tuple], failed=()) -> Dict[int, TickOutput]:
        """After pool.update_4d(frames), the same argument (failed = LiveSessionError.errors when the pool raised one)."""
        from .motion_capture import pack_frame
        if self._pool is None:
            raise ValueError("update_4d: this smoother follows no pool (LiveSmoother.for_pool)")
        tables = {}
        for sid, (fi, fr) in frames.items():
            if sid in failed:
                continue
            if len(fr) != self.C:
                raise ValueError(f"update_4d: session {sid}'s frame has {len(fr)} views, the smoother's sessions have {self.C}")
            kps = np.zeros((1, self.C, self.P, 17, 3))
            cnt = np.zeros((1, self.C), np.int32)
            pack_frame(kps, cnt, 0, fr, self.P)
            tables[sid] = (fi, (kps[0], cnt[0])) + self._pool_table(sid, fi)
        return self.update_tables(tables)

    def update_4d_arrays(self, sids: Sequence[int], frm_idxs: Sequence[int], kps25, counts, failed=()) -> Dict[int, TickOutput]:
        """After pool.update_4d_arrays(sids, frm_idxs, kps25, counts), the same arguments."""
        if self._pool is None:
            raise ValueError("update_4d_arrays: this smoother follows no pool (LiveSmoother.for_pool)")
        k = kps25.cpu().numpy() if hasattr(kps25, "cpu") else np.asarray(kps25)
        c = counts.cpu().numpy() if hasattr(counts, "cpu") else np.asarray(counts)
        if len(frm_idxs) != len(sids) or k.shape[0] != len(sids) or c.shape[0] != len(sids):
            raise ValueError(f"update_4d_arrays: {len(sids)} sessions, {len(frm_idxs)} frame indices, kps25 {k.shape}, counts {c.shape}")
        tables = {}
        for i, sid in enumerate(sids):
            if sid in failed:
                continue
            tables[int(sid)] = (int(frm_idxs[i]), (k[i], c[i])) + self._pool_table(int(sid), int(frm_idxs[i]))
        return self.update_tables(tables)

    # -- records -----------------------------------------------------------------------------------------------------------------------
    def _record(self, idn: _Ident, n: int, state: Optional[int] = None, live=None):
        """The identity's rows 0..n-1 as an MvTracklet-like record; ``live``: values of the rows not final yet.  Its rows carry the
        lengths they were solved under, which differ from row to row: bvh_export.save_bvh takes only committed_part(record) of a
        smoother with lengths="auto" and lengths_commit, or the record after body_fit.fit_sequences."""
        from .motion_capture import TrackState
        rows = [(idn.params[r], idn.joints[r]) + (idn.contact[r] if self._ct is not None else ()) if idn.params[r] is not None else live[r]
                for r in range(n)]
        poses = pose_tuples(idn.f0 + np.arange(n), np.array([q[0] for q in rows]), np.array([q[1] for q in rows], np.float64))
        t = new_record(idn.tid, poses, state=TrackState(idn.state if state is None else state), hits=idn.hits,
                       time_since_update=idn.n - idn.last_data())
        t.smooth_filled = np.array(idn.filled[:n], bool)
        t.smooth_views = np.array(idn.views[:n], np.int32)
        t.smooth_select = np.array(idn.sel[:n], np.int32).reshape(n, self.C)
        t.smooth_final = np.arange(n) < idn.n_final
        if self._ct is not None:      # the rows' stored labels and anchors as they stand
            t.smooth_contact = np.array([q[2] for q in rows], bool).reshape(n, 2)
            t.smooth_contact_anchor = np.array([q[3] for q in rows], np.float64).reshape(n, 2, 3)
        if self._len is not None:      # the running skeleton after the identity's last tick
            t.live_lengths, t.live_lengths_rows = idn.len[0].copy(), idn.len[1]
            t.live_lengths_committed_row = idn.len[2] if idn.len[2] < n else -1
        if self._cov:      # per row the values recorded when it was emitted; NaN on the rows that never were
            t.smooth_joint_sigma, t.smooth_param_sigma = np.full((n, SMOOTH_JOINTS), np.nan), np.full((n, SMOOTH_K), np.nan)
            t.smooth_noise_px = np.full(n, np.nan)
            for r, (js, ps, s) in idn.cov.items():
                if r < n:
                    t.smooth_joint_sigma[r], t.smooth_param_sigma[r], t.smooth_noise_px[r] = js, ps, s
        return t

    def tracklets(self, key) -> list:
        """The session's live identities as records f0..newest without holes: poses, smooth_filled, smooth_views, smooth_select,
        smooth_final (the row has left the window).  Reads the rows that are not final back from the device.  With contacts="auto"
        (here, in ``finished`` and from close_session) also smooth_contact (n,2) bool and smooth_contact_anchor (n,2,3), the rows'
        stored labels and anchors as they stand (those of the last <= lag rows are still tentative).  With covariance="joints"
        (here, in ``finished`` and from close_session) also smooth_joint_sigma (n,18), smooth_param_sigma (n,39), smooth_noise_px (n,): per
        row the values of TickOutput.cov when the row was emitted, NaN on the rows that never were (the last <= lag rows of a record,
        and the rows a jump of the frame index skipped).  With lengths="auto" (here, in ``finished`` and from close_session) also
        live_lengths (11,) the running skeleton after the identity's last tick, live_lengths_rows the rows that contributed to it, and
        live_lengths_committed_row (-1: not committed, or committed past the record's last row): from it on every row has live_lengths
        in its bone_lens, bit for bit (committed_part cuts the record there)."""
        sess = self._session(key, "tracklets")
        want = [(idn, r) for idn in sess.ids.values() for r in range(idn.n_final, idn.n)]
        live = {}
        for (idn, r), q in zip(want, self._fetch(want)):
            live.setdefault(id(idn), {})[r] = q
        return [self._record(idn, idn.n, live=live.get(id(idn))) for idn in sess.ids.values()]

    def close_session(self, key) -> list:
        """Ends a session: every live identity is finished (rows after its last data row dropped) and its record returned."""
        sess = self._session(key, "close_session")
        want = [(idn, r) for idn in sess.ids.values() for r in range(idn.n_final, idn.last_data())]
        for (idn, r), q in zip(want, self._fetch(want)):
            idn.params[r], idn.joints[r] = q[0].copy(), q[1].copy()
            if self._ct is not None:
                idn.contact[r] = (q[2].copy(), q[3].copy())
        done = []
        for idn in sess.ids.values():
            idn.n_final = idn.last_data()
            done.append(self._record(idn, idn.n_final, 3))
            self._free_id.append(idn.slot)
        self._free_id.sort()
        del self._sessions[key]
        self._free_s.append(sess.s)
        self._free_s.sort()
        return done
