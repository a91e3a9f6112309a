"""Bit-level comparison of two checkouts of the PACKAGE on the record stages, with one library (GPU):
    python tools/stage_diff.py CHECKOUT_A CHECKOUT_B LIB.so
For a host-side change: CHECKOUT_A is the parent (a ``git worktree``), CHECKOUT_B this tree, and LIB.so a build of the kernels both
share (MVMC_LIB_PATH points both at it).  Each checkout runs in a fresh child process on one small fixed scene:
track_sequences -> relink_sequences -> fit_sequences -> smooth_sequences (and once with fill_gaps=False) -> refine_rigs (plain, huber
with return_weights, cauchy), calibrate_rigs on a one-person walk (polish_loss None and "huber"), and a LiveSmoother fed the first
sequence's tables for 20 ticks, then close_session.  Every record, RigRefinement, RigCalibration and TickOutput is flattened to
arrays, and the two runs are compared with np.array_equal(..., equal_nan=True).  Exit status 1 when anything differs."""
import os, subprocess, sys, tempfile
import numpy as np


def _flat(out, name, v):
    """v -> out[name...]: arrays as they are, containers element by element, objects field by field."""
    import dataclasses, enum
    if v is None:
        out[name + ":none"] = np.zeros(0)
    elif isinstance(v, enum.Enum):
        out[name] = np.array(v.value)
    elif isinstance(v, (bool, int, float, str, np.ndarray, np.generic)):
        out[name] = np.asarray(v)
    elif isinstance(v, dict):
        for k in v:
            _flat(out, f"{name}.{k}", v[k])
    elif isinstance(v, (list, tuple)):
        out[name + ":len"] = np.array(len(v))
        for k, x in enumerate(v):
            _flat(out, f"{name}[{k}]", x)
    elif type(v).__name__ == "MvTracklet":
        _flat(out, name, _record(v))
    elif dataclasses.is_dataclass(v):
        _flat(out, name, {f.name: getattr(v, f.name) for f in dataclasses.fields(v)})
    else:
        _flat(out, name, dict(vars(v)))


def _record(t):
    """frame_idxs, the stacked pose parameters and joints, state, hits, time_since_update and every fit_* / smooth_* / relink_*."""
    d = {k: v for k, v in vars(t).items() if k.startswith(("fit_", "smooth_", "relink_")) or k in ("track_id", "hits", "time_since_update",
                                                                                                  "bone_lens")}
    d["state"] = getattr(t.state, "value", t.state)
    d["frame_idxs"] = np.asarray(t.frame_idxs)
    d["pose_frames"] = np.array([p[0] for p in t.poses])
    d["root"] = np.array([np.ravel(p[1].root) for p in t.poses])
    d["euler_angles"] = np.array([np.ravel(p[1].euler_angles) for p in t.poses])
    d["bone_lens_per_pose"] = np.array([np.ravel(p[1].bone_lens) for p in t.poses])
    d["joints"] = np.array([p[2].keypoints for p in t.poses])
    d["scores"] = np.array([p[2].keypoints_score for p in t.poses])
    return d


def child(root, path):
    sys.path[:0] = [root, os.path.join(root, "tests")]
    import rig_init_cases as rc
    from multiview_motion_capture_amd import synth
    from multiview_motion_capture_amd.body_fit import fit_sequences
    from multiview_motion_capture_amd.common import Calib
    from multiview_motion_capture_amd.live_smoothing import LiveSmoother
    from multiview_motion_capture_amd.relinking import relink_sequences
    from multiview_motion_capture_amd.rig_init import calibrate_rigs
    from multiview_motion_capture_amd.rig_refine import refine_rigs
    from multiview_motion_capture_amd.sequences import track_sequences
    from multiview_motion_capture_amd.smoothing import smooth_sequences
    seqs = []
    for F, C, P, dt, seed in ((48, 4, 2, np.float32, 31), (80, 4, 3, np.float64, 32), (64, 3, 2, np.float32, 33)):
        g = synth.generate(F, C, P, seed, dtype=dt, occlusion=0.15, walk="scene")
        seqs.append((g["kps25"], g["counts"], [Calib.from_k_rt(g["K"][c], g["Rt"][c], (1032, 776)) for c in range(C)]))
    out, tm = {}, {}
    tracked = track_sequences(seqs, timings=tm)
    _flat(out, "track", tracked)
    links = []
    linked = relink_sequences(tracked, links=links)
    _flat(out, "relink", [linked, links])
    fitted = fit_sequences(seqs, linked, timings=tm)
    _flat(out, "fit", fitted)
    _flat(out, "smooth", smooth_sequences(seqs, fitted, timings=tm))
    _flat(out, "smooth_nofill", smooth_sequences(seqs, fitted, fill_gaps=False))
    for name, kw in (("plain", {}), ("huber", dict(loss="huber", return_weights=True, ftol=1e-8)), ("cauchy", dict(loss="cauchy", ftol=1e-8))):
        problems = []
        out_refine = refine_rigs(seqs, fitted, min_cam_obs=20, problems=problems, timings=tm, **kw)
        _flat(out, "refine_" + name, [out_refine, problems])
    w = rc.walk(120, 5, 11, swaps=0.2, shifts=0.1)
    row = (w["kps25"], w["counts"], [(w["K"][c], (1032, 776)) for c in range(5)])
    for name, kw in (("plain", {}), ("huber", dict(polish_loss="huber", polish_ftol=1e-8))):
        detail = []
        out_cal = calibrate_rigs([row, row], detail=detail, timings=tm, **kw)
        _flat(out, "calibrate_" + name, [out_cal, detail])
    tables = []
    track_sequences(seqs[:1], chain_len=24, tables=tables)
    tb = tables[0]
    sm = LiveSmoother(4, 1, p_max=2)
    key = sm.open_session(seqs[0][2])
    for f in range(20):
        n = int(tb["n_tracks"][f])
        _flat(out, f"tick[{f}]", sm.update_tables({key: (f, (seqs[0][0][f], seqs[0][1][f]), tb["meta"][f, :n], tb["params"][f, :n],
                                                         tb["joints"][f, :n])})[key])
    _flat(out, "live_tracklets", sm.tracklets(key))
    _flat(out, "live_closed", sm.close_session(key))
    out["timing_keys"] = np.array(sorted(tm))
    holes = sum(len(t) < t.frame_idxs[-1] - t.frame_idxs[0] + 1 for tl in fitted for t in tl)
    print(f"{os.path.basename(root) or root}: records per sequence {[len(tl) for tl in tracked]} tracked, {[len(tl) for tl in linked]} re-linked "
          f"({holes} with holes); refine stops {[r.stop for r in out_refine]}; calibrate stops {[(r.stop, r.polish.stop) for r in out_cal]}")
    np.savez(path, **out)


def main():
    a, b, lib = (os.path.abspath(p) for p in sys.argv[1:4])
    res = []
    for root in (a, b):
        f = tempfile.mktemp(suffix=".npz")
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root, f], env=dict(os.environ, MVMC_LIB_PATH=lib), check=True,
                       timeout=600)
        res.append(dict(np.load(f)))
        os.remove(f)
    x, y = res
    bad = sorted(set(x) ^ set(y)) + [k for k in sorted(set(x) & set(y)) if not (x[k].dtype == y[k].dtype and np.array_equal(
        x[k], y[k], equal_nan=x[k].dtype.kind == "f"))]
    stages = sorted({k.split("[")[0].split(".")[0].split(":")[0] for k in x})
    for s in stages:
        ks = [k for k in x if k.split("[")[0].split(".")[0].split(":")[0] == s]
        n_bad = sum(k in bad for k in ks)
        print(f"{s:18s} {len(ks):6d} arrays  {sum(x[k].size for k in ks):9d} values  " + ("bit-identical" if not n_bad else f"{n_bad} DIFFER"))
    for k in bad[:20]:
        print("differs:", k)
    print("ALL BIT-IDENTICAL" if not bad else f"{len(bad)} arrays differ")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3])
    else:
        sys.exit(main())
