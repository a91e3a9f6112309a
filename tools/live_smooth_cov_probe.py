"""Calibration and cost of the live smoother's per-joint covariance (live_smoothing.LiveSmoother(covariance="joints")):
    python tools/live_smooth_cov_probe.py [--sizes 1 8] [--frames 300] [--out profiles/live_smooth_cov_probe.json]
Calibration, against ground truth: held-out synthetic scene walks (seeds 91, 92, 93, 5 cameras x 4 people, occlusion 0.3; the live
ground-truth test scores 81, 82, tools/smooth_cov_probe.py 71 - 73) through the real LivePool and LiveSmoother.for_pool(pool,
covariance="joints") at window 24, lag 8, identities matched to the generator's people as tests/test_gpu_live_smooth.py does.  Per
emitted (identity, frame), separately for frames with data and filled frames: the rank correlation of joint_sigma with the actual
error, the share of joints whose squared Mahalanobis error e^T C^-1 e lies below the 68 % and 95 % quantiles of chi^2_3 (3.53, 7.81),
and the ratio of the live joint_sigma to the offline smoother's smooth_joint_sigma of the same frame once the record is complete
(smoothing.smooth_sequences(covariance="joints") on the pool's raw records), as emitted and at unit variance (sigma / noise_px of
each): the live number is conditional on the window's frozen history and sees lag frames of future instead of the whole record.
Cost: S sessions (tools/live_sessions_probe.py's), ONE pool and three smoothers that follow it -- covariance=None, "joints" (noise
estimated: the recursion covers the whole window) and "joints" with noise_px given (the recursion stops at the emitted row) -- every tick
stepped through all three in rotating order, in one process; every update_4d ends in the tick's read-back, a device synchronisation.
Ticks before the window is full (the first 2 x window) are warm-up and are not timed.  Per variant the mean and the median tick.
Prints one JSON object (the kernel-source sha of the library included)."""
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

CHI2_3 = (3.53, 7.81)
SEEDS = (91, 92, 93)
NOISE_PX = 1.5


def calibration(frames, window, lag):
    from scipy.stats import spearmanr
    from test_gpu_body_fit import _raw_slot_maps
    from test_gpu_live_smooth import _pool_frames, _synth_rig
    from test_gpu_smooth import _person

    from multiview_motion_capture_amd.live import LivePool
    from multiview_motion_capture_amd.live_smoothing import LiveSmoother
    from multiview_motion_capture_amd.smoothing import smooth_sequences
    acc = {k: dict(sig=[], err=[], maha=[], ratio=[], ratio_unit=[]) for k in ("data", "filled")}
    noise, status, n_ident = [], [], 0
    for seed in SEEDS:
        g, cal = _synth_rig(seed, frames)
        pool = LivePool(5, 1)
        sm = LiveSmoother.for_pool(pool, window=window, lag=lag, covariance="joints")
        sid = pool.open_session(cal)
        emitted, recs = {}, []
        for f in range(frames):
            tick = {sid: (f, _pool_frames(g, cal, f))}
            pool.update_4d(tick)
            out = sm.update_4d(tick)[sid]
            for e in out.emitted:
                emitted[(e[0], e[1])] = (e[3].keypoints, e[4], out.cov[e[0]])
            recs += out.finished
        recs += sm.close_session(sid)
        s = pool.session(sid)
        raw = list(s.dead_tracklets) + list(s.tracklets)
        off = {t.track_id: t for t in smooth_sequences([(g["kps25"], g["counts"], cal)], [raw], covariance="joints")[0]}
        maps = _raw_slot_maps(g)
        for t in recs:
            if len(t) < 60:
                continue
            person = _person(t, g, maps, t.smooth_select)
            if person < 0:
                continue
            n_ident += 1
            o = off[t.track_id]
            o_at = {f: k for k, f in enumerate(o.frame_idxs)}
            for f in t.frame_idxs:
                if (t.track_id, f) not in emitted:
                    continue
                J, filled, c = emitted[(t.track_id, f)]
                status.append(c["status"])
                if c["status"] != 0 or not np.isfinite(c["noise_px"]):
                    continue
                noise.append(c["noise_px"])
                e = J - g["gt_joints"][f, person]
                a = acc["filled" if filled else "data"]
                a["sig"].append(c["joint_sigma"])
                a["err"].append(np.linalg.norm(e, axis=-1))
                a["maha"].append(np.einsum("ka,ka->k", e, np.linalg.solve(c["joint_cov"], e[..., None])[..., 0]))
                if f in o_at and getattr(o, "smooth_cov_status", 1) == 0:
                    k = o_at[f]
                    a["ratio"].append(c["joint_sigma"] / o.smooth_joint_sigma[k])
                    a["ratio_unit"].append((c["joint_sigma"] / c["noise_px"]) / (o.smooth_joint_sigma[k] / o.smooth_noise_px))
    res = {"seeds": list(SEEDS), "frames": frames, "window": window, "lag": lag, "identities": n_ident, "emitted_rows": len(status),
           "status_0": int(np.sum(np.array(status) == 0)), "median_noise_px": float(np.median(noise)),
           "noise_px_min_max": [float(np.min(noise)), float(np.max(noise))],
           "noise_px_of_a_perfect_model": float(2.0 * np.sqrt((1.0 ** 3 - 0.5 ** 3) / (3 * 0.5)))}
    pool_s, pool_e = [], []
    for key, a in acc.items():
        if not a["sig"]:
            res[key] = {"joints": 0}
            continue
        sg, er, m2 = (np.concatenate(a[k]) for k in ("sig", "err", "maha"))
        pool_s.append(sg)
        pool_e.append(er)
        r = {"joints": int(sg.size), "rank_correlation_sigma_error": float(spearmanr(sg, er)[0]),
             "share_below_chi2_68": float(np.mean(m2 < CHI2_3[0])), "share_below_chi2_95": float(np.mean(m2 < CHI2_3[1])),
             "median_mahalanobis2": float(np.median(m2)), "median_sigma_mm": float(1e3 * np.median(sg)),
             "median_error_mm": float(1e3 * np.median(er))}
        if a["ratio"]:
            q, u = np.concatenate(a["ratio"]), np.concatenate(a["ratio_unit"])
            r.update(live_over_offline_sigma={"median": float(np.median(q)), "p10": float(np.percentile(q, 10)), "p90": float(np.percentile(q, 90))},
                     live_over_offline_sigma_unit_variance={"median": float(np.median(u)), "p10": float(np.percentile(u, 10)),
                                                            "p90": float(np.percentile(u, 90)), "share_at_most_1": float(np.mean(u <= 1.0 + 1e-9))})
        res[key] = r
    res["rank_correlation_pooled"] = float(spearmanr(np.concatenate(pool_s), np.concatenate(pool_e))[0])
    return res


def cost(sizes, frames, window, lag):
    import torch
    from live_sessions_probe import make
    from live_smooth_probe import _frames

    from multiview_motion_capture_amd.live import LivePool
    from multiview_motion_capture_amd.live_smoothing import LiveSmoother
    seqs_all = make(max(sizes), frames)
    variants = {"none": {}, "joints": dict(covariance="joints"), "joints_noise_px": dict(covariance="joints", noise_px=NOISE_PX)}
    res = {}
    for S in sizes:
        seqs = seqs_all[:S]
        fr = _frames(seqs, frames)
        pool = LivePool(5, S)
        sms = {k: LiveSmoother.for_pool(pool, window=window, lag=lag, **kw) for k, kw in variants.items()}
        sids = [pool.open_session(q["calibs"]) for q in seqs]
        names = list(variants)
        times = {k: [] for k in names}
        emitted = 0
        for f in range(frames):
            tick = {sid: (f, fr[f][i]) for i, sid in enumerate(sids)}
            pool.update_4d(tick)
            torch.cuda.synchronize()
            for k in names[f % 3:] + names[:f % 3]:            # rotating order, the same process
                t0 = time.perf_counter()
                out = sms[k].update_4d(tick)                   # (ends in the tick's read-back)
                dt = time.perf_counter() - t0
                if f >= 2 * window:
                    times[k].append(dt)
                    if k == "joints":
                        emitted += sum(len(o.emitted) for o in out.values())
        r = {"timed_ticks": len(times["none"]), "emitted_rows_per_tick": emitted / max(len(times["joints"]), 1)}
        for k in names:
            a = 1e3 * np.array(times[k])
            r[k + "_tick_ms"] = {"mean": float(a.mean()), "median": float(np.median(a)), "p10": float(np.percentile(a, 10)),
                                 "p90": float(np.percentile(a, 90))}
        for k in names[1:]:
            r[k + "_over_none_median"] = r[k + "_tick_ms"]["median"] / r["none_tick_ms"]["median"]
            r[k + "_extra_ms_median"] = r[k + "_tick_ms"]["median"] - r["none_tick_ms"]["median"]
        res[str(S)] = r
        print(f"S={S}:", json.dumps(r), file=sys.stderr, flush=True)
        del pool, sms
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--window", type=int, default=24)
    ap.add_argument("--lag", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from multiview_motion_capture_amd import _cabi, smoothing
    res = {"build": _cabi.build_info(), "cov_mu": smoothing.COV_MU, "n_iter": 2, "noise_px_given": NOISE_PX,
           "weights": (smoothing.ROOT_VEL, smoothing.ROOT_ACC, smoothing.ANG_VEL, smoothing.ANG_ACC)}
    res["calibration"] = calibration(args.frames, args.window, args.lag)
    print("calibration:", json.dumps(res["calibration"]), file=sys.stderr, flush=True)
    res["cost"] = cost(args.sizes, args.frames, args.window, args.lag)
    text = json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
