"""Trajectory smoothing of finished tracklet records: one solve per identity over every frame from its first to its last.

The IK solves each frame on its own (the body fit's pose step too: stage 1, 5 evaluations, warm from the frame's own pose), so nothing
ties frame t to t +- 1, and a frame the tracker missed is a hole.  smooth_sequences() minimises, per identity (one record, frames f0..f1,
the missing ones included),

  E(X) = 1/2 sum_t sum_{v in V_t} |r_tv(x_t)|^2                                         (data: the IK's stage-1 residual)
       + 1/2 sum_t |Wv^1/2 (x_t - x_{t-1})|^2 + 1/2 sum_t |Wa^1/2 (x_{t+1} - 2 x_t + x_{t-1})|^2      (prior)

over x_t = the 39 stage-1 parameters of frame t (root translation, the Euler angles of the 12 joints whose rotation moves an observed
joint: the columns of the IK's stage 1).  The other 6 joints' angles and the bone lengths are held per frame.  r_tv is
solve_pose_reproj's residual (inverse_kinematics.py:219-234) at frame t's lengths; V_t is the selection (sequences.select_views: the
pose nearest to the record's joints per camera, MAX_DIST, MIN_SCORE) on the input record; a frame that is missing or has no selected
view has no data term.  Wv, Wa are diagonal: root_* on the translation (px^2 / m^2), ang_* on the angles (px^2 / rad^2).

Before the solve, every record frame's Euler triples are unwrapped towards the previous record frame's (the nearest of the 2 pi shifts
of both branches (a, b, c) and (a + pi, pi - b, c + pi) of R = Rx Ry Rz: tracker records restart the IK cold at chain heads and births),
and the missing frames start from the linear interpolation of the unwrapped record; their 6 held joints keep it, their lengths are the
nearest earlier record frame's.  The solve is Levenberg-Marquardt, (A + mu diag A) d = -grad E with A = the Gauss-Newton data blocks +
the exact prior Hessian, factored exactly by a block-banded Cholesky; mu starts at LM_MU0, / 10 after an accepted trial, x 10 after a
rejected one; stop on max_iter, LM_XTOL or LM_FTOL, as the body fit's length step.

loss="huber" / "cauchy" (default None: the quadratic data term above) puts a robust loss on every (selected view, observed joint)
pair: with the pair's score s, its plain pixel residual of length e and delta = loss_px, the data term is sum s^2 rho(e^2), Huber
rho = 1/2 e^2 for e <= delta and delta (e - 1/2 delta) beyond, Cauchy rho = 1/2 delta^2 log1p(e^2 / delta^2) (rig_refine's two
losses; the score stays outside, so loss_px is in pixels whatever the detector's confidence).  Every linearisation multiplies the
pair's Jacobian rows and residual by sqrt(w), w = 1 or delta / e (Huber), 1 / (1 + e^2 / delta^2) (Cauchy): iteratively reweighted
least squares without a second-order term; the Levenberg-Marquardt rules, the sweep and the prior are untouched, and the view gate of
the selection still comes first.  It is for the keypoint the gate cannot see: one limb exchanged, one joint put on the neighbour.

contacts="auto" or given labels (default None: nothing of it runs) adds foot contacts: per run of consecutive rows on which an ankle
is labelled as planted, 1/2 contact_weight |ankle(x_t) - a|^2 with one anchor a per run, minimised over x and the anchors in
alternation: further rounds of the same solve, the anchors (and with "auto" the labels) re-made between them by one launch.  It is
for the foot that slides under a retargeted character; smooth_sequences' docstring has the model and what it is not.  floor= (a
normal per sequence, with contacts) puts all the planted feet of one identity on one plane: the term weighs the part along the normal
with floor_weight about one level per identity, a further unknown in closed form; estimate_floor() finds the normal from the records
of a first call.

Device code: csrc/mvmc_smooth.hip (include/mvmc.h: mvmc_smooth_blocks, mvmc_smooth_step; with a loss mvmc_smooth_blocks_robust and
mvmc_smooth_obs_weights; with contacts mvmc_smooth_blocks_contact and csrc/mvmc_smooth_contact.hip: mvmc_smooth_contact_anchors; with a
floor mvmc_smooth_blocks_floor and mvmc_smooth_floor_anchors; selection: mvmc_body_observe), the optional per-frame covariance
csrc/mvmc_smooth_cov.hip (mvmc_smooth_cov);
NumPy restatement: tests/smooth_np.py, tests/smooth_cov_np.py, tests/smooth_robust_np.py, tests/smooth_contact_np.py,
tests/smooth_floor_np.py.
Sequences with the same number of cameras share every launch, each with its own rig.
"""
from __future__ import annotations

import math
import time
from typing import List, NamedTuple, Optional, Sequence

import numpy as np

from .body_fit import MAX_DIST, MIN_SCORE
from .sequences import (SequenceInput, check_records, new_record, no_sequences, plan_groups, pose_slot, pose_tuples, select_views,
                        stack_group, stopwatch)

# Default prior weights: tools/smooth_weight_sweep.py on synthetic scene walks with ground truth (profiles/smooth_weight_sweep.json)
ROOT_VEL, ROOT_ACC = 1e4, 1e4    # px^2 / m^2
ANG_VEL, ANG_ACC = 1e4, 1e4      # px^2 / rad^2
LM_MU0 = 1e-3       # Marquardt's damping: (A + mu diag(A)) d = -g, mu dimensionless
LM_FTOL = 1e-12     # stop: predicted or achieved reduction below LM_FTOL E
LM_XTOL = 1e-10     # stop: |d|_inf below LM_XTOL (m / rad)
LOSS_PX = 6.0       # the robust loss's scale in pixels, rig_refine's default: three times a 2 px detector noise
LOSSES = (None, "huber", "cauchy")
COV_MU = 1e-8       # covariance="joints" inverts A + COV_MU diag A: A alone is singular (the knees' Rz angles move no joint)
MAX_ITER_CAP = 24   # include/mvmc.h: MVMC_SMOOTH_INFO_DOUBLES - 8
MAX_VIEWS = 64      # include/mvmc.h: MVMC_SMOOTH_MAX_VIEWS
MAX_WORK_BYTES = 1 << 30
_BLOCK, _WORK = 820, 3940   # include/mvmc.h: doubles per row
_JOINTS, _K, _COV_INFO = 18, 39, 8   # include/mvmc.h: skeleton joints, MVMC_SMOOTH_K, MVMC_SMOOTH_COV_INFO_DOUBLES
_OBS = 16                            # observed joints of a view (the IK's observation rows): mvmc_smooth_obs_weights' last axis
# Foot contacts (contacts=): tools/smooth_contact_probe.py on planted walks with ground truth (profiles/smooth_contact_probe.json)
CONTACT_WEIGHT = 1e6       # px^2 / m^2, the root prior's unit
CONTACT_SPEED = 0.01       # m / frame: an ankle slower than this is planted (contacts="auto")
CONTACT_MIN_FRAMES = 3     # a detected run shorter than this is dropped
CONTACT_HEIGHT = 0.15      # m over the ground plane, when one is given
_FEET = (3, 6)             # include/mvmc.h: MVMC_SMOOTH_FOOT_L, MVMC_SMOOTH_FOOT_R (the two ankles of the 18-joint skeleton)


def stage1_columns() -> np.ndarray:
    """The 39 stage-1 columns of a 68-parameter row: translation, then the 3 angles of every joint that is a strict ancestor of an
    observed joint (Ik1Tables::act[0])."""
    from .device import SKEL_PARENTS
    obs = [1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15, 16, 17]
    moved = set()
    for k in obs:
        j = int(SKEL_PARENTS[k])
        while j >= 0:
            moved.add(j)
            j = int(SKEL_PARENTS[j])
    return np.array([0, 1, 2] + [3 + 3 * a + c for a in sorted(moved) for c in range(3)], dtype=np.int64)


def unwrap_euler(ang: np.ndarray) -> np.ndarray:
    """(n,18,3) Euler triples of consecutive record frames -> the same rotations, each triple the equivalent one nearest (Euclidean) to
    the previous frame's: per branch ((a,b,c) and (a+pi, pi-b, c+pi)) the 2 pi shift of every component nearest to it, then the nearer
    branch (a tie keeps the first).  Sequential from the first frame, which is kept."""
    return unwrap_euler_many([ang])[0]


def unwrap_euler_many(angs: Sequence[np.ndarray]) -> List[np.ndarray]:
    """unwrap_euler of several records at once: one pass over the frame index for all of them (the same operations per element)."""
    outs = [np.array(a, dtype=np.float64, copy=True).reshape(-1, 18, 3) for a in angs]
    if not outs:
        return []
    n = np.array([o.shape[0] for o in outs])
    pad = np.zeros((len(outs), int(n.max()), 18, 3))
    for r, o in enumerate(outs):
        pad[r, :o.shape[0]] = o
    tp = 2.0 * math.pi
    for k in range(1, pad.shape[1]):
        live = np.flatnonzero(n > k)
        prev, a = pad[live, k - 1], pad[live, k]
        b = np.stack([a[..., 0] + math.pi, math.pi - a[..., 1], a[..., 2] + math.pi], axis=-1)
        ca = a + tp * np.round((prev - a) / tp)
        cb = b + tp * np.round((prev - b) / tp)
        da = ((ca - prev) ** 2).sum(-1)
        db = ((cb - prev) ** 2).sum(-1)
        pad[live, k] = np.where((db < da)[..., None], cb, ca)
    return [pad[r, :n[r]].copy() for r in range(len(outs))]


def initial_trajectory(frames: np.ndarray, params: np.ndarray):
    """One record's frames (n,) (increasing) and params (n,68) -> (x (m,68) over frames[0]..frames[-1], filled (m,) bool): unwrapped
    record rows; the missing rows linearly interpolated in root and angles, lengths of the nearest earlier record frame."""
    return initial_trajectories([frames], [params])[0]


def initial_trajectories(frames_list: Sequence[np.ndarray], params_list: Sequence[np.ndarray]) -> list:
    """initial_trajectory of several records (their Euler angles unwrapped in one pass)."""
    ps = [np.array(p, np.float64, copy=True) for p in params_list]
    un = unwrap_euler_many([p[:, 3:57].reshape(-1, 18, 3) for p in ps])
    out = []
    for frames, p, u in zip(frames_list, ps, un):
        frames = np.asarray(frames, np.int64)
        p[:, 3:57] = u.reshape(-1, 54)
        full = np.arange(frames[0], frames[-1] + 1)
        m = full.size
        x = np.empty((m, 68))
        for c in range(57):
            x[:, c] = np.interp(full, frames, p[:, c])
        src = np.searchsorted(frames, full, side="right") - 1
        x[:, 57:] = p[src, 57:]
        filled = np.ones(m, dtype=bool)
        filled[frames - frames[0]] = False
        x[frames - frames[0]] = p      # the record's own rows exactly
        out.append((x, filled))
    return out


# ---- the argument checks of both smoothers (host only): ``who`` is the name in the message, "smooth_sequences" or "LiveSmoother" ----
def _number(v) -> bool:
    """A real number: int, float or a NumPy scalar of either; no bool, no string."""
    return not isinstance(v, (str, bytes, bool)) and isinstance(v, (int, float, np.integer, np.floating))


def check_prior_weights(who: str, root_vel, root_acc, ang_vel, ang_acc) -> np.ndarray:
    w = np.array([root_vel, root_acc, ang_vel, ang_acc], dtype=np.float64)
    if not np.all(np.isfinite(w)) or np.any(w < 0):
        raise ValueError(f"{who}: the prior weights must be finite and >= 0")
    if not (w[0] + w[1] > 0 and w[2] + w[3] > 0):
        raise ValueError(f"{who}: root_vel + root_acc > 0 and ang_vel + ang_acc > 0 required")
    return w


def _check_weights(root_vel, root_acc, ang_vel, ang_acc, max_iter, max_work_bytes):
    w = check_prior_weights("smooth_sequences", root_vel, root_acc, ang_vel, ang_acc)
    if int(max_iter) != max_iter or not 0 <= int(max_iter) <= MAX_ITER_CAP:
        raise ValueError(f"smooth_sequences: 0 <= max_iter <= {MAX_ITER_CAP} required")
    if not int(max_work_bytes) > 0:
        raise ValueError("smooth_sequences: max_work_bytes must be positive")
    return w


def check_covariance(who: str, covariance, noise_px) -> Optional[float]:
    """The covariance arguments of smooth_sequences and LiveSmoother -> noise_px as a float, or None."""
    if covariance is not None and not (isinstance(covariance, str) and covariance == "joints"):
        raise ValueError(f"{who}: covariance must be None or \"joints\", got {covariance!r}")
    if noise_px is None:
        return None
    if covariance is None:
        raise ValueError(f"{who}: noise_px without covariance=\"joints\" has nothing to scale")
    if not _number(noise_px) or not math.isfinite(noise_px) or not noise_px > 0:
        raise ValueError(f"{who}: noise_px must be None or a finite number > 0, got {noise_px!r}")
    return float(noise_px)


def check_loss(who: str, loss, loss_px) -> float:
    """The robust-loss arguments of smooth_sequences and LiveSmoother -> loss_px as a float."""
    if not (loss is None or isinstance(loss, str)) or loss not in LOSSES:
        raise ValueError(f"{who}: loss must be None, \"huber\" or \"cauchy\", got {loss!r}")
    if not _number(loss_px) or not math.isfinite(loss_px) or not loss_px > 0:
        raise ValueError(f"{who}: loss_px must be a finite number > 0, got {loss_px!r}")
    return float(loss_px)


class _Contacts(NamedTuple):
    """The checked scalar foot-contact arguments."""
    auto: bool
    weight: float
    speed: float
    min_frames: int
    rounds: int
    ground: Optional[tuple]      # (normal (3,), offset)
    height: float


def _check_contact_args(contacts, contact_weight, contact_speed, contact_min_frames, contact_rounds, ground, contact_height,
                        who: str = "smooth_sequences") -> _Contacts:
    """The scalar foot-contact arguments of smooth_sequences and, with contacts="auto" and one round, of LiveSmoother."""
    auto = isinstance(contacts, str)
    if auto and contacts != "auto":
        raise ValueError(f"{who}: contacts must be None, \"auto\" or per sequence a list of label arrays, got {contacts!r}")
    if not auto and not isinstance(contacts, (list, tuple)):
        raise ValueError(f"{who}: contacts must be None, \"auto\" or per sequence a list of label arrays, got {type(contacts).__name__}")
    if not _number(contact_weight) or not math.isfinite(contact_weight) or contact_weight < 0:
        raise ValueError(f"{who}: contact_weight must be a finite number >= 0, got {contact_weight!r}")
    if not _number(contact_speed) or not math.isfinite(contact_speed):
        raise ValueError(f"{who}: contact_speed must be a finite number, got {contact_speed!r}")
    if not _number(contact_height) or not math.isfinite(contact_height):
        raise ValueError(f"{who}: contact_height must be a finite number, got {contact_height!r}")
    for name, v in (("contact_min_frames", contact_min_frames), ("contact_rounds", contact_rounds)):
        if not _number(v) or int(v) != v or int(v) < 1:
            raise ValueError(f"{who}: {name} must be an integer >= 1, got {v!r}")
    g = None
    if ground is not None:
        if not auto:
            raise ValueError(f"{who}: ground gates the detection of contacts=\"auto\"; given labels are taken as they are")
        try:
            normal, off = ground
            normal = np.array(normal, np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: ground must be (normal (3,), offset)") from None
        if normal.shape != (3,) or not np.all(np.isfinite(normal)) or not _number(off) or not math.isfinite(off):
            raise ValueError(f"{who}: ground must be (normal (3,), offset) of finite numbers")
        g = (normal, float(off))
    return _Contacts(auto, float(contact_weight), float(contact_speed), int(contact_min_frames), int(contact_rounds), g,
                     float(contact_height))


def _check_floor(floor, floor_weight, contacts, contact_weight, n_seq):
    """floor= and floor_weight= (host only) -> (per sequence None or the unit normal (3,), floor weight)."""
    who = "smooth_sequences"
    if contacts is None:
        raise ValueError(f"{who}: floor needs contacts: it is the plane the planted feet stand on")
    if floor_weight is None:
        wf = float(contact_weight)
    elif not _number(floor_weight) or not math.isfinite(floor_weight) or floor_weight < 0:
        raise ValueError(f"{who}: floor_weight must be None or a finite number >= 0, got {floor_weight!r}")
    else:
        wf = float(floor_weight)

    def normal(v, what):
        try:
            n = np.array(v, np.float64)
        except (TypeError, ValueError):
            n = None
        if n is None or n.shape != (3,) or not np.all(np.isfinite(n)) or not np.linalg.norm(n) > 0:
            raise ValueError(f"{who}: {what} must be a finite non-zero normal (3,), got {v!r}")
        return n / np.linalg.norm(n)
    if isinstance(floor, np.ndarray) or (isinstance(floor, (list, tuple)) and len(floor) == 3 and all(_number(v) for v in floor)):
        n = normal(floor, "floor")
        return [n.copy() for _ in range(n_seq)], wf
    if not isinstance(floor, (list, tuple)):
        raise ValueError(f"{who}: floor must be None, a normal (3,) or per sequence a list of normals (3,) or None, got {floor!r}")
    if len(floor) != n_seq:
        raise ValueError(f"{who}: floor has {len(floor)} entries for {n_seq} sequences")
    return [None if v is None else normal(v, f"floor[{i}]") for i, v in enumerate(floor)], wf


def _check_contact_labels(contacts, recs):
    """Given labels against the checked records (host only) -> per sequence, per record None or an (m, 2) int32 array over f0..f1."""
    who = "smooth_sequences"
    if len(contacts) != len(recs):
        raise ValueError(f"{who}: contacts has {len(contacts)} entries for {len(recs)} sequences")
    out = []
    for s, (cs, rs) in enumerate(zip(contacts, recs)):
        if not isinstance(cs, (list, tuple)) or len(cs) != len(rs):
            raise ValueError(f"{who}: contacts[{s}] must be a list aligned with the sequence's {len(rs)} records")
        row = []
        for j, (c, r) in enumerate(zip(cs, rs)):
            if c is None:
                row.append(None)
                continue
            a = np.asarray(c)
            m = int(r[0][-1] - r[0][0] + 1)
            if a.dtype != np.bool_ or a.shape != (m, 2):
                raise ValueError(f"{who}: contacts[{s}][{j}] must be None or a bool array ({m}, 2) over the record's frames f0..f1 "
                                 f"(columns left, right), got {a.dtype} {a.shape}")
            row.append(a.astype(np.int32))
        out.append(row)
    return out


def _check(sequences, tracklets_per_sequence):
    return check_records(sequences, tracklets_per_sequence, "smooth_sequences", increasing=True, finite=True,
                         cameras=(1, MAX_VIEWS, f"sequence {{s}}: {{C}} cameras, at most {MAX_VIEWS}"))


class _Options(NamedTuple):
    """smooth_sequences' keyword arguments after their checks (_options)."""
    w: np.ndarray                        # the four prior weights
    max_iter: int
    fill_gaps: bool
    max_work_bytes: int
    loss: Optional[str]
    loss_px: float
    covariance: bool
    noise_px: Optional[float]
    contacts: Optional[_Contacts]
    normals: Optional[list]              # floor=: per sequence None or the unit normal (3,)
    floor_weight: Optional[float]

    @property
    def robust(self) -> dict:
        """The loss arguments of the device calls; loss=None: the calls without the arguments."""
        return dict(loss=self.loss, loss_px=self.loss_px) if self.loss is not None else {}

    def row_bytes(self, C: int) -> int:
        """Device bytes per trajectory row of a group with C cameras: what max_work_bytes caps."""
        n = 8 * (2 * _BLOCK + _WORK + 2 * 68) + 4 * 8
        if self.covariance:
            n += 8 * (_JOINTS * 6 + _K)
        if self.contacts is not None:
            n += 4 * 2 + 8 * 6 + 8 * _JOINTS * 3     # labels, anchors and the FK joints of the rounds
        if self.loss is not None:
            n += 8 * _OBS * C                        # the weights: (C, 16) per row
        return n


def _options(n_seq, root_vel, root_acc, ang_vel, ang_acc, max_iter, fill_gaps, max_work_bytes, covariance, noise_px, loss, loss_px,
             contacts, contact_weight, contact_speed, contact_min_frames, contact_rounds, ground, contact_height, floor,
             floor_weight) -> _Options:
    """smooth_sequences' keyword arguments, checked (host only): the contact arguments are read only with contacts, the floor's only
    with floor= or floor_weight=."""
    w = _check_weights(root_vel, root_acc, ang_vel, ang_acc, max_iter, max_work_bytes)
    noise_px = check_covariance("smooth_sequences", covariance, noise_px)
    loss_px = check_loss("smooth_sequences", loss, loss_px)
    ct = None
    if contacts is not None:
        ct = _check_contact_args(contacts, contact_weight, contact_speed, contact_min_frames, contact_rounds, ground, contact_height)
    normals = wf = None
    if floor is not None or floor_weight is not None:
        if floor is None:
            raise ValueError("smooth_sequences: floor_weight belongs to floor")
        normals, wf = _check_floor(floor, floor_weight, contacts, contact_weight, n_seq)
    return _Options(w, int(max_iter), bool(fill_gaps), int(max_work_bytes), loss, loss_px, covariance is not None, noise_px, ct,
                    normals, wf)


class _Identity(NamedTuple):
    """An identity with two frames or more, rows f0..f1 of its record (the missing ones included)."""
    item: int                 # its index in the group's items
    x0: np.ndarray            # (m, 68) the initial trajectory
    filled: np.ndarray        # (m,) bool: the frame is missing from the record
    members: np.ndarray       # (m, C) i32 the selected pose per camera, -1 none
    n_views: np.ndarray       # (m,) i32
    rig: int


class _Cov(NamedTuple):
    """mvmc_smooth_cov's unit-variance outputs of one identity."""
    jcov: np.ndarray          # (m, 18, 6)
    pvar: np.ndarray          # (m, 39)
    info: np.ndarray          # (8,)


class _Contact(NamedTuple):
    mask: np.ndarray          # (m, 2) bool
    anchors: np.ndarray       # (m, 2, 3)
    cost: np.ndarray          # [E_contact at the first anchors, at the end]
    round_trials: list


class _Floor(NamedTuple):
    normal: np.ndarray        # (3,) unit, NaN: the sequence has none
    level: float


class _Result(NamedTuple):
    """What the solve returns for one _Identity; the optional parts are None unless the option is on."""
    x: np.ndarray             # (m, 68)
    joints: np.ndarray        # (m, 18, 3)
    info: np.ndarray          # mvmc_smooth_step's info row (with contacts: of the whole call, _contact_result)
    cov: Optional[_Cov] = None
    weights: Optional[np.ndarray] = None
    contact: Optional[_Contact] = None
    floor: Optional[_Floor] = None


class _Group(NamedTuple):
    """What every partition of one camera group reads."""
    items: list                          # (sequence, record) per identity
    k17: object                          # the group's ingested keypoints and projections, on the device
    Pm_d: object
    normals: Optional[list]              # floor=: per rig None or the unit normal
    normals_h: Optional[np.ndarray]      # (rigs, 3), NaN: none; None: no rig of the group has a floor
    normals_d: object                    # the same on the device


# mvmc_smooth_step's and mvmc_smooth_window's info row (include/mvmc.h): "E_data, E_prior at the start; E_data, E_prior at the end;
# trials, accepted, mu, stop reason; per trial 1 / 0, -1 after the last"
INFO_COST, INFO_TRIALS, INFO_STOP, INFO_TRACE = slice(0, 4), 4, 7, 8
# mvmc_smooth_cov's and mvmc_smooth_window_cov's cinfo (include/mvmc.h): "{status, E_data at x, n_res = ..., edof, ...}"
COV_STATUS, COV_E_DATA, COV_NRES, COV_EDOF = 0, 1, 2, 3


def smooth_sequences(sequences: Sequence[SequenceInput], tracklets_per_sequence: Sequence[list], root_vel: float = ROOT_VEL,
                     root_acc: float = ROOT_ACC, ang_vel: float = ANG_VEL, ang_acc: float = ANG_ACC, max_iter: int = 10,
                     fill_gaps: bool = True, max_work_bytes: int = MAX_WORK_BYTES, device="cuda:0",
                     timings: Optional[dict] = None, covariance: Optional[str] = None, noise_px: Optional[float] = None,
                     loss: Optional[str] = None, loss_px: float = LOSS_PX, contacts=None, contact_weight: float = CONTACT_WEIGHT,
                     contact_speed: float = CONTACT_SPEED, contact_min_frames: int = CONTACT_MIN_FRAMES, contact_rounds: int = 1,
                     ground=None, contact_height: float = CONTACT_HEIGHT, floor=None, floor_weight: Optional[float] = None) -> List[list]:
    """Smooth every identity of every sequence -- (kps (F_s,C,P_s,25|17,3), counts (F_s,C), one Calib per camera), the rows
    track_sequences and fit_sequences take -- from its MvTracklet records (fit_sequences, track_sequences, run_main_batched,
    MvTracker.update_4d, LivePool).  Returns, per sequence, NEW records in the input order (the inputs are not touched): the same
    track_id, state, hits, time_since_update (and bone_lens where the input has one); frame_idxs f0..f1 without holes (fill_gaps=False:
    the input's frames, the others solved but left out); poses[k] = (frame, PoseShapeParam, FK joints); ``smooth_filled`` (n,) bool:
    the frame was missing from the input; ``smooth_views`` (n,) the views of the data term; ``smooth_select`` (n, C) the pose slot
    (ingest order) used per camera or -1; ``smooth_cost`` [E_data, E_prior] at the start and at the end; ``smooth_trials`` per trial 1
    accepted / 0 rejected.  A one-frame record is returned as a copy of the input's (cost 0).
    Sequences with the same camera count share every launch; max_work_bytes caps the device workspace (~45 KB per frame): a group
    larger than the cap runs as several launch sequences one after another (an identity larger than the cap gets one of its own).
    timings: a dict that receives the seconds spent in {"prepare" (input checks, unwrapping and interpolation, packing and uploads),
    "select", "blocks", "solve", "records"} (synchronising between the parts), and "covariance" when that is asked for.
    covariance="joints" (default None: nothing below is computed or set): how far each pose can be trusted.  After the solve, one more
    launch per partition (include/mvmc.h: mvmc_smooth_cov) takes the diagonal blocks of (A + COV_MU diag A)^-1 at the returned
    trajectory, A = the Gauss-Newton data blocks + the exact prior Hessian: the Laplace covariance of E (the damping because A alone
    is singular: the two knees' Rz angles move no joint; their smooth_param_sigma is large and says only that), conditional on the
    six held joints' angles, the per-frame bone lengths, the rig and the view selection.  Every record gets, rows as ``poses``:
    ``smooth_noise_px`` = noise_px if given, else sqrt(2 E_data / (smooth_nres - smooth_edof)) (NaN when that is not positive): the noise of a score-1 keypoint in
    pixels; ``smooth_joint_cov`` (n,18,3,3) m^2 = smooth_noise_px^2 D_K Sigma_tt D_K^T per skeleton joint; ``smooth_joint_sigma`` (n,18)
    m = sqrt(trace); ``smooth_param_sigma`` (n,39) m / rad in stage1_columns() order; ``smooth_edof`` = tr(A^-1 J^T J), ``smooth_nres``
    the residuals with a non-zero score, ``smooth_cov_status`` 0 solved, 1 A is singular (NaN arrays), 2 a record of fewer than two
    frames (NaN arrays).  The prior is a regulariser with swept weights, not a fitted motion model: the calibration of these numbers is
    measured, not promised.
    loss="huber" / "cauchy" at loss_px pixels (default None: nothing below is computed or set, the launches and the bits are those of
    a call without the argument): the robust data term of the module's docstring.  Every blocks launch of the solve and of the
    covariance is the robust one; ``smooth_cost`` holds the robust E_data = sum s^2 rho; after the solve one more launch per partition
    (mvmc_smooth_obs_weights) takes the weights at the returned trajectory, and every record gets ``smooth_obs_weight`` (n, C, 16),
    rows as ``poses``: the weight of camera c and observed joint k (the IK's observation order: COCO's 16 joints without the nose,
    then the mid spine), NaN where the camera has no selected pose in the row or the keypoint's score is 0 -- filled rows and
    one-frame records are all NaN.  It tells which keypoints of which camera were voted down.  timings gets a "weights" part.
    With covariance="joints" the launch inverts J^T W J + the prior at the final weights, and smooth_edof and smooth_nres are defined
    as above on the weighted blocks; the ESTIMATED smooth_noise_px is then biased low, because rho <= 1/2 e^2 shrinks E_data while
    smooth_nres still counts every residual: under a loss noise_px= is the honest choice.
    contacts="auto" or per sequence a list aligned with its records, each item None or a bool array (m, 2) over the record's frames
    f0..f1, columns left / right ankle (default None: nothing below is computed or set, the launches and the bits are those of a
    call without the argument): a planted foot stays where it is.  A run is a maximal stretch of consecutive rows on which one foot
    is labelled; every run has one anchor a, and E gains E_contact = 1/2 contact_weight sum |ankle(x_t) - a|^2 over the labelled
    (row, foot) pairs (contact_weight in px^2 / m^2, the root prior's unit; outside the robust loss).  The anchors are unknowns too
    and are minimised in closed form (the run's mean ankle).  Round 0 is the solve without contacts, launch for launch; then
    contact_rounds times: FK, one launch (mvmc_smooth_contact_anchors) that sets every run's anchor -- and in the first round of
    "auto" the labels: the ankle's central-difference speed on round 0's joints (one-sided at the record's ends) < contact_speed
    m / frame and, with ground=(normal (3,), offset), normal . ankle - offset < contact_height; runs shorter than
    contact_min_frames are dropped, there is no hysteresis --, and the same Levenberg-Marquardt loop on the blocks with the term
    (mvmc_smooth_blocks_contact), max_iter trials again.  The joint energy over (x, anchors) never increases from round 1 on.  An
    identity without a labelled row is not solved again: its result is that of contacts=None bit for bit.  Every record gets, rows
    as ``poses``: ``smooth_contact`` (n, 2) bool; ``smooth_contact_anchor`` (n, 2, 3) m, NaN where there is no contact;
    ``smooth_contact_cost`` [E_contact at the first anchors, at the end]; ``smooth_round_trials`` the trials of round 0 and of every
    later round, ``smooth_trials`` all of them in order; ``smooth_cost`` = E_data, E_prior at round 0's start and at the last round's
    end, E_data WITHOUT the contact part: the device sums the row costs with it, and the host subtracts E_contact computed from
    the returned joints and anchors (so the last digits of that E_data carry the rounding of a difference).  A one-frame record:
    all False / NaN / zeros.  covariance="joints" takes its blocks with the final labels and anchors: the covariance is conditional
    on them, and the E_data behind an estimated smooth_noise_px includes E_contact.  timings gets a "contacts" part (FK, the
    anchors launch and the host's share); "blocks" and "solve" hold every round's.  What this is not: the 18-joint skeleton has no
    toes, so an ankle that pivots during push-off is held too rigidly if it is labelled; without floor= every run has an anchor of
    its own and nothing ties one stance's height to the next; contact_speed is per frame, so it depends on the frame rate.
    LiveSmoother(contacts="auto") is the live twin: a fixed-lag
    window does not know a run's future, so there an anchor is re-estimated while its run is younger than the emitted row and frozen
    from the tick that emits the run's first row (live_smoothing.py).
    floor= a normal (3,) for every sequence, or per sequence a list of normals (3,) or None (default None: nothing below is
    computed or set, the launches and the bits are those of a call without the argument; needs contacts; normalised here): the
    planted feet of one identity stand on ONE plane.  With T = I - n n^T and one level h per identity (metres along n),
    E_contact = 1/2 contact_weight sum |T (ankle(x_t) - a)|^2 + 1/2 floor_weight sum (n . ankle(x_t) - h)^2 over the labelled pairs
    (floor_weight=None: contact_weight; finite >= 0): the horizontal position of a planted foot may be soft while its height is
    locked.  h is an unknown too, minimised in closed form (the mean of n . ankle over the identity's labelled pairs, both feet);
    every round's anchors launch is followed by one more (mvmc_smooth_floor_anchors) that takes h and moves the run means onto the
    plane, and every blocks launch -- the covariance's too -- is mvmc_smooth_blocks_floor.  The joint energy over (x, anchors, h)
    never increases from round 1 on.  ``smooth_contact_anchor`` is then the point T mean + n h (n . a = h to rounding),
    ``smooth_contact_cost`` the E_contact above, and every record gets ``smooth_floor_normal`` (3,) (unit; NaN for a sequence whose
    entry is None, which runs the contacts alone, bit for bit) and ``smooth_floor_level`` (NaN without a contact).  ground= keeps its
    meaning: it gates the detection only.  estimate_floor() finds the normal from the records of a first call with contacts.  What
    the floor is not: unlabelled rows carry no term (a swing foot may pass under the plane); the live twin has no floor; there are
    still no toes; neither the world nor the BVH root is moved onto the floor."""
    t_start = time.perf_counter()
    opt = _options(len(sequences), root_vel, root_acc, ang_vel, ang_acc, max_iter, fill_gaps, max_work_bytes, covariance, noise_px, loss,
                   loss_px, contacts, contact_weight, contact_speed, contact_min_frames, contact_rounds, ground, contact_height, floor,
                   floor_weight)
    if no_sequences(sequences, tracklets_per_sequence, "smooth_sequences"):
        return []
    shapes, recs = _check(sequences, tracklets_per_sequence)
    given = _check_contact_labels(contacts, recs) if opt.contacts is not None and not opt.contacts.auto else None
    import torch

    from . import device as dev
    d = torch.device(device)
    T = dev.uploader(d)
    lap, tm = stopwatch(timings, d, ("prepare", "select", "blocks", "solve", "records") + (("covariance",) if opt.covariance else ())
                        + (("weights",) if opt.loss is not None else ()) + (("contacts",) if opt.contacts is not None else ()))
    tm["prepare"] = time.perf_counter() - t_start
    out: List[list] = [[None] * len(r) for r in recs]
    for lay in plan_groups(shapes, 1):
        if not any(recs[i] for i in lay.seq_ids):
            continue
        t0 = time.perf_counter()
        stacked = stack_group(lay, sequences)
        t0 = lap("prepare", t0)
        sel = select_views(stacked, recs, d, MAX_DIST, MIN_SCORE)      # on the record frames
        mem_h, nv_h = sel.members.cpu().numpy(), sel.n_views.cpu().numpy()
        t0 = lap("select", t0)
        idents = _identities(sel, mem_h, nv_h, lay.n_views, recs)
        normals = nrm_h = nrm_d = None        # the group's floor normals: per rig, and as one array (NaN: none) when it has any
        if opt.normals is not None:
            normals = [opt.normals[i] for i in lay.seq_ids]
            if any(n is not None for n in normals):
                nrm_h = np.array([np.full(3, np.nan) if n is None else n for n in normals])
                nrm_d = T(nrm_h)
        grp = _Group(sel.items, sel.k17, sel.Pm_d, normals, nrm_h, nrm_d)
        lap("prepare", t0)
        res = {}
        for part in _partitions(idents, max(1, opt.max_work_bytes // opt.row_bytes(lay.n_views))):
            res.update(_solve_partition(part, grp, opt, given, lap, T))
        t0 = time.perf_counter()
        kept = _records(out, sel.items, recs, tracklets_per_sequence, idents, res, mem_h, nv_h, sel.rec_lo, opt.fill_gaps, sel.Pg)
        _option_fields(kept, opt, lay.n_views, [None if normals is None else normals[int(sel.rig_of[lo])] for lo in sel.rec_lo[:-1]])
        lap("records", t0)
    if timings is not None:
        timings.update(tm)
    return out


def _identities(sel, mem_h, nv_h, C: int, recs) -> List[_Identity]:
    """The group's identities with two frames or more, each with its full trajectory f0..f1: the initial values, and the selection of
    its record frames (mem_h, nv_h: select_views' members and view counts on the host) spread over the rows."""
    multi = [a for a in range(len(sel.items)) if sel.n_of[a] >= 2]
    rec_of = [recs[sel.items[a][0]][sel.items[a][1]] for a in multi]
    out = []
    for a, (frames, _, _), (x0, filled) in zip(multi, rec_of, initial_trajectories([r[0] for r in rec_of], [r[1] for r in rec_of])):
        lo, hi = sel.rec_lo[a], sel.rec_lo[a + 1]
        m = x0.shape[0]
        mem = -np.ones((m, C), np.int32)
        nvf = np.zeros(m, np.int32)
        mem[frames - frames[0]] = mem_h[lo:hi]
        nvf[frames - frames[0]] = nv_h[lo:hi]
        out.append(_Identity(a, x0, filled, mem, nvf, int(sel.rig_of[lo])))
    return out




def _partitions(idents: List[_Identity], cap: int):
    """The identities in order, cut greedily into launch sequences of at most ``cap`` rows (an identity larger than the cap alone)."""
    at = 0
    while at < len(idents):
        b, rows = at + 1, idents[at].x0.shape[0]
        while b < len(idents) and rows + idents[b].x0.shape[0] <= cap:
            rows += idents[b].x0.shape[0]
            b += 1
        yield idents[at:b]
        at = b


def _solve_partition(part: List[_Identity], grp: _Group, opt: _Options, given, lap, T) -> dict:
    """One launch sequence for the identities of ``part``: upload, round 0, the contact rounds, the optional covariance and weights
    launches, the read-back -> {item index: _Result}."""
    import torch

    from . import device as dev
    t0 = time.perf_counter()
    x_h = np.concatenate([p.x0 for p in part])
    N, n_ids = x_h.shape[0], len(part)
    m_of = np.array([p.x0.shape[0] for p in part])
    id_lo = np.concatenate([[0], np.cumsum(m_of)]).astype(np.int32)
    rows_of = [slice(id_lo[s], id_lo[s + 1]) for s in range(n_ids)]
    x = T(x_h)
    d = x.device
    xt = x.clone()
    mem_d = T(np.concatenate([p.members for p in part]))
    rig_d = T(np.repeat(np.array([p.rig for p in part], np.int32), m_of))
    ctl = torch.zeros((n_ids, 4), dtype=torch.int32, device=d)
    ctl[:, 1] = 1
    info = torch.empty((n_ids, 32), dtype=torch.float64, device=d)
    blk = torch.empty((2, N, _BLOCK), dtype=torch.float64, device=d)
    work = torch.empty((N, _WORK), dtype=torch.float64, device=d)
    id_of_d, id_lo_d = T(np.repeat(np.arange(n_ids, dtype=np.int32), m_of)), T(id_lo)
    view = (grp.k17, grp.Pm_d, rig_d, mem_d)
    t0 = lap("prepare", t0)

    def lm_loop(t0, info, **term):
        """max_iter + 1 launches of the blocks (at x, then at the trial) and of the step, under ctl; -> the clock."""
        for phase in range(opt.max_iter + 1):
            dev.smooth_blocks(*view, x if phase == 0 else xt, id_of_d, ctl, blk, **opt.robust, **term)
            t0 = lap("blocks", t0)
            dev.smooth_step(x, xt, blk, id_lo_d, opt.w, LM_MU0, LM_FTOL, LM_XTOL, opt.max_iter, phase, ctl, info, work)
            t0 = lap("solve", t0)
        return t0
    t0 = lm_loop(t0, info)
    ct, floor = opt.contacts, grp.normals_h is not None
    term = {}
    if ct is not None:
        cm_h = np.zeros((N, 2), np.int32)
        if given is not None:
            for p, sl in zip(part, rows_of):
                g = given[grp.items[p.item][0]][grp.items[p.item][1]]
                if g is not None:
                    cm_h[sl] = g
        cmask = T(cm_h)
        anch = torch.empty((N, 2, 3), dtype=torch.float64, device=d)
        term = dict(cmask=cmask, anchors=anch, contact_weight=ct.weight)
        if floor:
            term.update(normals=grp.normals_d, floor_weight=opt.floor_weight)
            lev = torch.empty((n_ids,), dtype=torch.float64, device=d)
        infos, jn1 = [info], None      # (jn1, cm1, an1: the first round's joints, labels and anchors, on the host)
        t0 = lap("prepare", t0)
        for rnd in range(ct.rounds):
            jn_d = dev.fk(x)
            dev.smooth_contact_anchors(jn_d, id_lo_d, cmask, anch, ctl, ct.auto and rnd == 0, ct.speed, ct.min_frames, ct.ground, ct.height)
            if floor:
                dev.smooth_floor_anchors(jn_d, id_lo_d, rig_d, grp.normals_d, cmask, anch, lev)
            if rnd == 0:
                jn1, cm1, an1 = jn_d.cpu().numpy(), cmask.cpu().numpy(), anch.cpu().numpy()
            infos.append(torch.zeros((n_ids, 32), dtype=torch.float64, device=d))   # (a stopped identity's row stays 0)
            t0 = lap("contacts", t0)
            t0 = lm_loop(t0, infos[-1], **term)
    cov = wts_h = None
    if opt.covariance:
        # the blocks AT x (the loop's last blocks are the last trial's, which may have been rejected) into buffer 0, steered
        # by a control word of its own: the solve's ctl and info stay as they are, and blk is not read again
        ctl_x = torch.zeros((n_ids, 4), dtype=torch.int32, device=d)
        ctl_x[:, 1] = 1
        jcov = torch.empty((N, _JOINTS, 6), dtype=torch.float64, device=d)
        pvar = torch.empty((N, _K), dtype=torch.float64, device=d)
        cinfo = torch.empty((n_ids, _COV_INFO), dtype=torch.float64, device=d)
        dev.smooth_blocks(*view, x, id_of_d, ctl_x, blk, **opt.robust, **term)
        dev.smooth_cov(x, blk[0], id_lo_d, opt.w, COV_MU, *view, work, jcov, pvar, cinfo)
        t0 = lap("covariance", t0)
        cov = _Cov(jcov.cpu().numpy(), pvar.cpu().numpy(), cinfo.cpu().numpy())
    if opt.loss is not None:
        wts = dev.smooth_obs_weights(*view, x, opt.loss, opt.loss_px)
        t0 = lap("weights", t0)
        wts_h = wts.cpu().numpy()
    jn = dev.fk(x).cpu().numpy()
    xs, inf = x.cpu().numpy(), info.cpu().numpy()
    inf_of, contact_of, floor_of = list(inf), [None] * n_ids, [None] * n_ids
    if ct is not None:
        t0 = lap("records", t0)
        infs = [inf] + [i.cpu().numpy() for i in infos[1:]]
        anc_h = anch.cpu().numpy()
        lev_h = lev.cpu().numpy() if floor else None
        for s, (p, sl) in enumerate(zip(part, rows_of)):
            n_s = grp.normals_h[p.rig] if floor and not np.isnan(grp.normals_h[p.rig, 0]) else None
            inf_of[s], contact_of[s] = _contact_result([i[s] for i in infs], jn1[sl], cm1[sl], an1[sl], jn[sl],
                                                       anc_h[sl], ct.weight, n_s, opt.floor_weight if n_s is not None else None)
            if opt.normals is not None:
                floor_of[s] = _Floor(np.full(3, np.nan), math.nan) if n_s is None else _Floor(n_s.copy(), float(lev_h[s]))
        t0 = lap("contacts", t0)
    res = {p.item: _Result(xs[sl], jn[sl], inf_of[s], None if cov is None else _Cov(cov.jcov[sl], cov.pvar[sl], cov.info[s]),
                           None if wts_h is None else wts_h[sl], contact_of[s], floor_of[s])
           for s, (p, sl) in enumerate(zip(part, rows_of))}
    lap("records", t0)
    return res


def _records(out, items, recs, tracklets_per_sequence, idents, res, mem_h, nv_h, rec_lo, fill_gaps, Pg) -> list:
    """The group's new records into ``out``, with the attributes every call sets.  idents: the _Identity of every identity that was
    solved, res: {item index: _Result} (either may be given as plain tuples in the fields' order); mem_h, nv_h, rec_lo: the selection
    of the record frames.  The identity lookup and the kept rows are made here, once: -> per item (record, _Result or None for a
    one-frame record, the kept rows of the trajectory or None) for _option_fields."""
    by_item = {p.item: p for p in (_Identity(*p) for p in idents)}
    kept = []
    for a, (i, j) in enumerate(items):
        src = tracklets_per_sequence[i][j]
        f, par, jnt = recs[i][j]
        p = by_item.get(a)
        if p is not None:
            r = _Result(*res[a])
            idx = np.arange(p.filled.size) if fill_gaps else np.flatnonzero(~p.filled)
            poses = pose_tuples(f[0] + idx, r.x[idx], r.joints[idx])
            cost = np.array(r.info[INFO_COST])
            trials = [int(v) for v in r.info[INFO_TRACE:INFO_TRACE + int(r.info[INFO_TRIALS])]]
            filled_k, views_k, mem_k = p.filled[idx], p.n_views[idx], p.members[idx]
        else:   # one frame: nothing to smooth (a copy of the input's pose)
            r = idx = None
            poses = pose_tuples(f[:1], par[:1], jnt[:1])
            cost = np.zeros(4)
            trials = []
            filled_k = np.zeros(1, bool)
            views_k = nv_h[rec_lo[a]:rec_lo[a + 1]].astype(np.int32)
            mem_k = mem_h[rec_lo[a]:rec_lo[a + 1]]
        t = out[i][j] = new_record(src.track_id, poses, src)
        if getattr(src, "bone_lens", None) is not None:
            t.bone_lens = np.array(src.bone_lens, np.float64).copy()
        t.smooth_filled = np.asarray(filled_k, bool)
        t.smooth_views = np.asarray(views_k, np.int32)
        t.smooth_select = pose_slot(mem_k, Pg)
        t.smooth_cost = cost
        t.smooth_trials = trials
        kept.append((t, r, idx))
    return kept


def _option_fields(kept: list, opt: _Options, C: int, normal_of: list) -> None:
    """The attributes of the options that are on (smooth_sequences' docstring) on _records' records; normal_of: per item the floor
    normal of its sequence or None."""
    for (t, r, idx), n in zip(kept, normal_of):
        if opt.covariance:
            _covariance_fields(t, r, idx, opt.noise_px)
        if opt.loss is not None:      # a one-frame record has nothing solved: NaN
            t.smooth_obs_weight = r.weights[idx].copy() if r is not None else np.full((1, C, _OBS), np.nan)
        if opt.contacts is not None:
            _contact_fields(t, r, idx, opt.contacts.rounds)
            if opt.normals is not None:
                t.smooth_floor_normal, t.smooth_floor_level = r.floor if r is not None else \
                    (np.full(3, np.nan) if n is None else n.copy(), math.nan)


def scale_covariance(jc6, pv, status: int, e_data: float, n_res, edof: float, noise_px: Optional[float]):
    """The covariance launches' unit-variance outputs jc6 (..., 18, 6) and pv (..., 39) -> (noise, joint_cov (..., 18, 3, 3) m^2,
    joint_sigma (..., 18) m, param_sigma (..., 39)): scaled by noise^2 with noise = noise_px if given, else the estimate
    sqrt(2 E_data / (n_res - edof)), NaN when the launch did not solve (status != 0) or that is not positive; the six stored entries
    of every symmetric 3 x 3 block expanded."""
    if noise_px is not None:
        s = noise_px
    else:
        s = math.sqrt(2.0 * e_data / (n_res - edof)) if status == 0 and n_res - edof > 0 else math.nan
    jc = jc6[..., [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(jc6.shape[:-1] + (3, 3))
    return float(s), (s * s) * jc, np.sqrt((s * s) * (jc[..., 0, 0] + jc[..., 1, 1] + jc[..., 2, 2])), np.sqrt((s * s) * pv)


def _covariance_fields(t, r: Optional[_Result], idx, noise_px) -> None:
    """The smooth_* covariance attributes of one record (smooth_sequences' docstring), from the unit-variance device outputs."""
    if r is not None:
        ci = r.cov.info
        status, e_data, n_res, edof = int(ci[COV_STATUS]), float(ci[COV_E_DATA]), ci[COV_NRES], float(ci[COV_EDOF])
        jc6, pv = r.cov.jcov[idx], r.cov.pvar[idx]
    else:   # fewer than two frames: nothing was solved
        status, e_data, n_res, edof = 2, 0.0, np.nan, np.nan
        jc6, pv = np.full((1, _JOINTS, 6), np.nan), np.full((1, _K), np.nan)
    t.smooth_noise_px, t.smooth_joint_cov, t.smooth_joint_sigma, t.smooth_param_sigma = scale_covariance(jc6, pv, status, e_data, n_res,
                                                                                                          edof, noise_px)
    t.smooth_edof = edof
    t.smooth_nres = int(n_res) if status == 0 else 0
    t.smooth_cov_status = status


def _contact_energy(joints, mask, anchors, wc, normal=None, wf=None) -> float:
    """E_contact = 1/2 wc sum over the labelled (row, foot) pairs of |ankle - anchor|^2: joints (m,18,3), mask (m,2), anchors (m,2,3).
    With a floor (normal (3,) unit, wf; the anchors on the plane): + 1/2 (wf - wc) sum (normal . (ankle - anchor))^2, which makes it
    1/2 wc sum |T (ankle - run mean)|^2 + 1/2 wf sum (normal . ankle - level)^2."""
    d = np.where(mask[..., None] != 0, joints[:, _FEET] - anchors, 0.0)
    E = 0.5 * wc * float(np.sum(d * d))
    if normal is not None:
        nd = d @ normal
        E += 0.5 * (wf - wc) * float(np.sum(nd * nd))
    return E


def _contact_result(infs, joints1, mask, anchors1, joints, anchors, wc, normal=None, wf=None):
    """One identity after its rounds: infs its info row of round 0 and of every later round, joints1 / anchors1 the first round's FK
    joints and anchors, mask (m,2) the labels, joints / anchors the returned joints and the last round's anchors -> (the info row
    _records reads, of the whole call: E_data without the contact part, every round's trials in order; (labels, anchors,
    [E_contact first, end], trials per round))."""
    live = bool(mask.any())
    n_r = [int(i[4]) for i in infs] if live else [int(infs[0][4])] + [0] * (len(infs) - 1)
    trials = np.concatenate([i[8:8 + n] for i, n in zip(infs, n_r)])
    cost = np.zeros(2)
    end = infs[0][2:4]
    if live:
        cost[:] = _contact_energy(joints1, mask, anchors1, wc, normal, wf), _contact_energy(joints, mask, anchors, wc, normal, wf)
        end = np.array([infs[-1][2] - cost[1], infs[-1][3]])
    inf = np.concatenate([infs[0][0:2], end, [float(sum(n_r)), 0.0, 0.0, 0.0], trials])
    return inf, _Contact(mask != 0, anchors, cost, n_r)


def _contact_fields(t, r: Optional[_Result], idx, rounds: int) -> None:
    """The smooth_contact* attributes and smooth_round_trials of one record (smooth_sequences' docstring)."""
    if r is not None:
        t.smooth_contact, t.smooth_contact_anchor = r.contact.mask[idx].copy(), r.contact.anchors[idx].copy()
        t.smooth_contact_cost, t.smooth_round_trials = r.contact.cost, list(r.contact.round_trials)
    else:   # one frame: nothing was solved
        t.smooth_contact, t.smooth_contact_anchor = np.zeros((1, 2), bool), np.full((1, 2, 3), np.nan)
        t.smooth_contact_cost, t.smooth_round_trials = np.zeros(2), [0] * (1 + rounds)


def smooth_tracklets(tracklets: list, kps: np.ndarray, counts: np.ndarray, calibs: list, root_vel: float = ROOT_VEL,
                     root_acc: float = ROOT_ACC, ang_vel: float = ANG_VEL, ang_acc: float = ANG_ACC, max_iter: int = 10,
                     fill_gaps: bool = True, max_work_bytes: int = MAX_WORK_BYTES, device="cuda:0", timings: Optional[dict] = None,
                     covariance: Optional[str] = None, noise_px: Optional[float] = None, loss: Optional[str] = None,
                     loss_px: float = LOSS_PX, contacts=None, contact_weight: float = CONTACT_WEIGHT,
                     contact_speed: float = CONTACT_SPEED, contact_min_frames: int = CONTACT_MIN_FRAMES, contact_rounds: int = 1,
                     ground=None, contact_height: float = CONTACT_HEIGHT, floor=None, floor_weight: Optional[float] = None) -> list:
    """smooth_sequences for one sequence: records of kps (F,C,P,25|17,3), counts (F,C) and one Calib per camera -> new records.
    contacts: None, "auto", or a list aligned with ``tracklets`` (None or a bool array (m, 2) per record); floor: None or the
    sequence's floor normal (3,)."""
    if floor is not None and isinstance(floor, (list, tuple)) and not (len(floor) == 3 and all(_number(v) for v in floor)):
        raise ValueError(f"smooth_tracklets: floor must be None or ONE normal (3,), got {floor!r}")
    # (smooth_sequences reads the contact arguments only with contacts, the floor's only with floor= or floor_weight=)
    return smooth_sequences([(kps, counts, calibs)], [tracklets], root_vel=root_vel, root_acc=root_acc, ang_vel=ang_vel, ang_acc=ang_acc,
                            max_iter=max_iter, fill_gaps=fill_gaps, max_work_bytes=max_work_bytes, device=device, timings=timings,
                            covariance=covariance, noise_px=noise_px, loss=loss, loss_px=loss_px,
                            contacts=contacts if contacts is None or isinstance(contacts, str) else [contacts],
                            contact_weight=contact_weight, contact_speed=contact_speed, contact_min_frames=contact_min_frames,
                            contact_rounds=contact_rounds, ground=ground, contact_height=contact_height, floor=floor,
                            floor_weight=floor_weight)[0]


def estimate_floor(tracklets_per_sequence: Sequence[list], min_spread: float = 0.05) -> List[dict]:
    """The floor normal of every sequence from the planted feet of its smoothed records (host only, NumPy; restated in
    tests/smooth_floor_np.py: estimate): records that carry ``smooth_contact`` -- those of smooth_sequences(contacts=...).  A run is a
    maximal stretch of consecutive frame_idxs on which one foot is labelled, m_r its mean ankle and len_r its length; c_id is the
    length-weighted mean of an identity's m_r over both feet, S = sum len_r (m_r - c_id)(m_r - c_id)^T over every identity of the
    sequence: each identity stands on a level of its own, the normal is shared.  n is S's eigenvector of the smallest eigenvalue,
    oriented so that the mean of n . (joint 0 - ankle) over the labelled rows is positive (the body is above its feet).
    Per sequence a dict: ``normal`` (3,) unit; ``status`` 0 ok, 1 fewer than three runs or sqrt(lambda_mid / sum len_r) < min_spread
    metres (the footholds do not span a plane -- somebody stepping on the spot or along one line; a condition, not a measurement: the
    normal is S's eigenvector all the same), 2 no contact at all (NaN normal); ``spread`` (3,) = sqrt(eigenvalues / sum len_r)
    ascending, metres; ``rms`` = spread[0], the run means' residual about their planes; ``levels`` per record, the length-weighted
    mean of n . m_r (NaN without a contact); ``n_runs``.  The recipe: smooth with contacts, estimate_floor, smooth again with
    floor=[f["normal"] if f["status"] == 0 else None for f in floors]."""
    if not _number(min_spread) or not math.isfinite(min_spread) or min_spread < 0:
        raise ValueError(f"estimate_floor: min_spread must be a finite number >= 0, got {min_spread!r}")
    out = []
    for s, recs in enumerate(tracklets_per_sequence):
        means, lens, ids, up = [], [], [], []
        for i, t in enumerate(recs):
            lab = getattr(t, "smooth_contact", None)
            if lab is None:
                raise ValueError(f"estimate_floor: record {i} of sequence {s} has no smooth_contact: smooth it with contacts= first")
            fr = np.asarray(t.frame_idxs)
            J = np.array([q[2].keypoints for q in t.poses], np.float64).reshape(len(fr), _JOINTS, 3)
            lab = np.asarray(lab, bool)
            for f, K in enumerate(_FEET):
                k = 0
                while k < len(fr):
                    if not lab[k, f]:
                        k += 1
                        continue
                    e = k + 1
                    while e < len(fr) and lab[e, f] and fr[e] == fr[e - 1] + 1:
                        e += 1
                    means.append(J[k:e, K].mean(0))
                    lens.append(e - k)
                    ids.append(i)
                    k = e
                up.append((J[:, 0] - J[:, K])[lab[:, f]])
        nan3 = np.full(3, np.nan)
        if not means:
            out.append(dict(normal=nan3, status=2, spread=nan3.copy(), rms=math.nan, levels=np.full(len(recs), np.nan), n_runs=0))
            continue
        means, lens, ids = np.array(means), np.array(lens, np.float64), np.array(ids)
        S = np.zeros((3, 3))
        for i in np.unique(ids):
            k = ids == i
            c = (lens[k, None] * means[k]).sum(0) / lens[k].sum()
            dm = means[k] - c
            S += (lens[k, None, None] * dm[:, :, None] * dm[:, None, :]).sum(0)
        lam, V = np.linalg.eigh(S)
        n = V[:, 0]
        if np.concatenate(up).mean(0) @ n < 0:
            n = -n
        spread = np.sqrt(np.maximum(lam, 0.0) / lens.sum())
        levels = np.full(len(recs), np.nan)
        for i in np.unique(ids):
            k = ids == i
            levels[i] = (lens[k] * (means[k] @ n)).sum() / lens[k].sum()
        out.append(dict(normal=n, status=0 if len(means) >= 3 and spread[1] >= min_spread else 1, spread=spread, rms=float(spread[0]),
                        levels=levels, n_runs=len(means)))
    return out
