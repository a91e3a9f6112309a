"""What the live smoother's foot contacts buy and cost (live_smoothing.LiveSmoother(contacts="auto")):
    python tools/live_smooth_contact_probe.py [--sizes 1 8 64] [--frames 300] [--out profiles/live_smooth_contact_probe.json]
Quality, against ground truth: planted walks (synth.generate(walk="planted"), seeds 81 - 83, 5 views x 3 people, 300 frames) through
the real LivePool and two smoothers that follow it, contacts=None and contacts="auto", at window 24, lag 8.  Over the EMITTED poses,
every one matched to the ground-truth person whose joints are nearest: skate (the mean ankle displacement per frame over the pairs of
consecutive frames on which gt_contact has the foot down), MPJPE on frames with data and on filled frames, jitter (the mean second
difference over triples of consecutive frames), and the emitted labels' precision / recall against gt_contact.  Beside them, as the
yardstick, the offline smoother on the pool's finished records (smoothing.smooth_sequences, contacts=None and "auto") over the same
(identity, frame) pairs.
Cost: S sessions (tools/live_sessions_probe.py's), ONE pool and the two smoothers, every tick stepped through both in alternating
order, in one process; every update_4d ends in the tick's read-back, a device synchronisation.  Ticks before the window is full (the
first 2 x window) are warm-up and are not timed.  --only-none times contacts=None alone (for a run against another build of the
library through MVMC_LIB_PATH).  Prints one JSON object (the kernel-source sha of the library included)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

SEEDS = (81, 82, 83)
FEET = (3, 6)        # include/mvmc.h: MVMC_SMOOTH_FOOT_L, MVMC_SMOOTH_FOOT_R


def _figures(poses, g, labels=None):
    """poses {(tid, frame): (joints (18,3), filled)} -> skate, MPJPE (data / filled), jitter in metres, and with labels {(tid, frame):
    (2,) bool} their precision / recall."""
    gt, gc = g["gt_joints"], g["gt_contact"]
    person = {k: int(np.argmin(np.linalg.norm(J[None] - gt[k[1]], axis=-1).mean(-1))) for k, (J, _) in poses.items()}
    sk, e_data, e_fill, jit = [], [], [], []
    for (tid, f), (J, filled) in poses.items():
        p = person[(tid, f)]
        (e_fill if filled else e_data).append(float(np.linalg.norm(J - gt[f, p], axis=-1).mean()))
        nxt, prv = poses.get((tid, f + 1)), poses.get((tid, f - 1))
        if nxt is not None:
            for k, K in enumerate(FEET):
                if gc[f, p, k] and gc[f + 1, p, k]:
                    sk.append(float(np.linalg.norm(nxt[0][K] - J[K])))
            if prv is not None:
                jit.append(float(np.linalg.norm(nxt[0] - 2.0 * J + prv[0], axis=-1).mean()))
    r = {"poses": len(poses), "contact_pairs": len(sk), "skate_mm": 1e3 * float(np.mean(sk)), "mpjpe_data_mm": 1e3 * float(np.mean(e_data)),
         "mpjpe_filled_mm": 1e3 * float(np.mean(e_fill)) if e_fill else None, "filled": len(e_fill), "jitter_mm": 1e3 * float(np.mean(jit))}
    if labels is not None:
        tp = sum(int((c & gc[k[1], person[k]]).sum()) for k, c in labels.items())
        n_lab, n_true = sum(int(c.sum()) for c in labels.values()), sum(int(gc[k[1], person[k]].sum()) for k in labels)
        r.update(labels=n_lab, true_contacts=n_true, precision=tp / max(n_lab, 1), recall=tp / max(n_true, 1))
    return r


def quality(frames, window, lag):
    from test_gpu_body_fit import _calibs
    from test_gpu_live_smooth import _pool_frames

    from multiview_motion_capture_amd import synth
    from multiview_motion_capture_amd.live import LivePool
    from multiview_motion_capture_amd.live_smoothing import LiveSmoother
    from multiview_motion_capture_amd.smoothing import smooth_sequences
    per_seed = []
    for seed in SEEDS:
        g = synth.generate(frames, 5, 3, seed, walk="planted")
        cal = _calibs(g["K"], g["Rt"])
        pool = LivePool(5, 1)
        sms = {"none": LiveSmoother.for_pool(pool, window=window, lag=lag), "auto": LiveSmoother.for_pool(pool, window=window, lag=lag, contacts="auto")}
        sid = pool.open_session(cal)
        em = {k: {} for k in sms}
        lab = {}
        for f in range(frames):
            tick = {sid: (f, _pool_frames(g, cal, f))}
            pool.update_4d(tick)
            for k, sm in sms.items():
                out = sm.update_4d(tick)[sid]
                for e in out.emitted:
                    em[k][(e[0], e[1])] = (e[3].keypoints, e[4])
                    if k == "auto":
                        lab[(e[0], e[1])] = out.contact[e[0]]["contact"]
        s = pool.session(sid)
        raw = list(s.dead_tracklets) + list(s.tracklets)
        r = {"seed": seed, "live_none": _figures(em["none"], g), "live_auto": _figures(em["auto"], g, lab)}
        for name, kw in (("offline_none", {}), ("offline_auto", dict(contacts="auto"))):
            off = smooth_sequences([(g["kps25"], g["counts"], cal)], [raw], **kw)[0]
            poses, olab = {}, {}
            for t in off:
                for k, (fi, q) in enumerate(zip(t.frame_idxs, t.poses)):
                    if (t.track_id, fi) in em["auto"]:                    # the same (identity, frame) pairs as the live figures
                        poses[(t.track_id, fi)] = (q[2].keypoints, em["auto"][(t.track_id, fi)][1])
                        if kw:
                            olab[(t.track_id, fi)] = np.asarray(t.smooth_contact[k], bool)
            r[name] = _figures(poses, g, olab if kw else None)
        r["skate_auto_over_none"] = r["live_auto"]["skate_mm"] / r["live_none"]["skate_mm"]
        r["mpjpe_data_auto_over_none"] = r["live_auto"]["mpjpe_data_mm"] / r["live_none"]["mpjpe_data_mm"]
        per_seed.append(r)
        print(f"seed {seed}:", json.dumps(r), file=sys.stderr, flush=True)
    def mean(a, b):      # (None: no seed has the figure -- a planted walk without occlusion has no filled frame)
        v = [r[a][b] for r in per_seed if r[a].get(b) is not None]
        return float(np.mean(v)) if v else None
    summary = {v: {q: mean(v, q) for q in ("skate_mm", "mpjpe_data_mm", "mpjpe_filled_mm", "jitter_mm")}
               for v in ("live_none", "live_auto", "offline_none", "offline_auto")}
    for v in ("live_auto", "offline_auto"):
        summary[v].update(precision=mean(v, "precision"), recall=mean(v, "recall"))
    return {"seeds": list(SEEDS), "frames": frames, "views": 5, "people": 3, "window": window, "lag": lag, "per_seed": per_seed, "mean": summary}


def cost(sizes, frames, window, lag, only_none=False):
    import torch
    from live_sessions_probe import make
    from live_smooth_probe import _frames

    from multiview_motion_capture_amd.live import LivePool
    from multiview_motion_capture_amd.live_smoothing import LiveSmoother
    seqs_all = make(max(sizes), frames)
    variants = {"none": {}} if only_none else {"none": {}, "auto": dict(contacts="auto")}
    res = {}
    for S in sizes:
        seqs = seqs_all[:S]
        fr = _frames(seqs, frames)
        pool = LivePool(5, S)
        sms = {k: LiveSmoother.for_pool(pool, window=window, lag=lag, **kw) for k, kw in variants.items()}
        sids = [pool.open_session(q["calibs"]) for q in seqs]
        names = list(variants)
        times = {k: [] for k in names}
        items = 0
        for f in range(frames):
            tick = {sid: (f, fr[f][i]) for i, sid in enumerate(sids)}
            pool.update_4d(tick)
            torch.cuda.synchronize()
            for k in names[f % len(names):] + names[:f % len(names)]:      # alternating order, the same process
                t0 = time.perf_counter()
                out = sms[k].update_4d(tick)                               # (ends in the tick's read-back)
                dt = time.perf_counter() - t0
                if f >= 2 * window:
                    times[k].append(dt)
                    if k == "none":
                        items += sum(len(o.solved) for o in out.values())
        r = {"timed_ticks": len(times["none"]), "identities_per_tick": items / max(len(times["none"]), 1)}
        for k in names:
            a = 1e3 * np.array(times[k])
            r[k + "_tick_ms"] = {"mean": float(a.mean()), "median": float(np.median(a)), "p10": float(np.percentile(a, 10)),
                                 "p90": float(np.percentile(a, 90))}
        if not only_none:
            r["auto_over_none_median"] = r["auto_tick_ms"]["median"] / r["none_tick_ms"]["median"]
            r["auto_extra_ms_median"] = r["auto_tick_ms"]["median"] - r["none_tick_ms"]["median"]
        res[str(S)] = r
        print(f"S={S}:", json.dumps(r), file=sys.stderr, flush=True)
        del pool, sms
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--cost-frames", type=int, default=120)
    ap.add_argument("--window", type=int, default=24)
    ap.add_argument("--lag", type=int, default=8)
    ap.add_argument("--only-none", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from multiview_motion_capture_amd import _cabi, smoothing
    res = {"build": _cabi.build_info(), "library": os.environ.get("MVMC_LIB_PATH") or "the tree's", "n_iter": 2,
           "contact": dict(weight=smoothing.CONTACT_WEIGHT, speed=smoothing.CONTACT_SPEED, min_frames=smoothing.CONTACT_MIN_FRAMES),
           "weights": (smoothing.ROOT_VEL, smoothing.ROOT_ACC, smoothing.ANG_VEL, smoothing.ANG_ACC)}
    if not args.only_none:
        res["quality"] = quality(args.frames, args.window, args.lag)
    res["cost"] = cost(args.sizes, args.cost_frames, args.window, args.lag, args.only_none)
    text = json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
