"""Calibration and cost of the smoother's per-frame covariance (smoothing.smooth_sequences(covariance="joints")):
    python tools/smooth_cov_probe.py [--sizes 1 8 64] [--frames 300] [--repeats 5] [--out profiles/smooth_cov_probe.json]
Calibration, against ground truth: held-out synthetic scene walks (seeds 71, 72, 73, rigs (5,4), (4,3), (5,2), 300 frames, occlusion
0.3, 10-20-frame holes from hole stream 9: the weight sweep tunes on seeds 51, 52 and stream 7, the ground-truth test scores 61, 62 and
stream 8), identities matched to the generator's people as tests/test_gpu_smooth.py::test_ground_truth_of_synthetic_scene_walks does.
Separately for frames with data and filled frames: the share of joints whose squared Mahalanobis error e^T C^-1 e lies below the 68 %
and 95 % quantiles of chi^2_3 (3.53, 7.81), the rank correlation of smooth_joint_sigma with the actual error, and the median
smooth_noise_px beside the 2 sqrt(E[s^2]) = 1.53 px that synth.py's N(0, 2 px) noise and U(0.5, 1) scores would give a perfectly
specified model.
Cost: S synthetic sequences of 300 frames (tools/smooth_probe.py's), smooth_sequences with covariance=None and "joints" alternating in
one session, --repeats timed calls each after one untimed call of each: the best and the median call, and the "covariance" share of one
more call with timings.  profiles/smooth_probe.json's tracklet-frames/s of the parent commit are shown beside covariance=None's.
Prints one JSON object (the kernel-source sha of the library included)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

CHI2_3 = (3.53, 7.81)


def calibration(frames):
    from scipy.stats import spearmanr
    from test_gpu_body_fit import _raw_slot_maps
    from test_gpu_smooth import _cut, _person, _synth

    from multiview_motion_capture_amd.body_fit import fit_sequences
    from multiview_motion_capture_amd.sequences import track_sequences
    from multiview_motion_capture_amd.smoothing import smooth_sequences
    seqs, gts = _synth(seeds=(71, 72, 73), n_frames=frames)
    fitted = fit_sequences(seqs, track_sequences(seqs, chain_len=16))
    rng = np.random.default_rng(9)
    cut = [_cut(r, rng) for r in fitted]
    out = smooth_sequences(seqs, cut, covariance="joints")
    maha = {"data": [], "filled": []}
    sig = {"data": [], "filled": []}
    err = {"data": [], "filled": []}
    noise, status = [], []
    for s, g in enumerate(gts):
        maps = _raw_slot_maps(g)
        for t_fit, t in zip(fitted[s], out[s]):
            if len(t_fit) < 60 or len(t) < 2:
                continue
            person = _person(t_fit, g, maps, t_fit.fit_select)
            if person < 0:
                continue
            status.append(t.smooth_cov_status)
            noise.append(t.smooth_noise_px)
            J = np.array([q[2].keypoints for q in t.poses])
            e = J - g["gt_joints"][np.array(t.frame_idxs), person]                      # (n,18,3)
            m2 = np.einsum("nka,nka->nk", e, np.linalg.solve(t.smooth_joint_cov, e[..., None])[..., 0])
            for key, rows in (("data", ~t.smooth_filled & (t.smooth_views > 0)), ("filled", t.smooth_filled)):
                maha[key].append(m2[rows].ravel())
                sig[key].append(t.smooth_joint_sigma[rows].ravel())
                err[key].append(np.linalg.norm(e[rows], axis=-1).ravel())
    res = {"seeds": [71, 72, 73], "hole_stream": 9, "frames": frames, "identities": len(noise), "status_0": int(np.sum(np.array(status) == 0)),
           "median_noise_px": float(np.median(noise)), "noise_px_min_max": [float(np.min(noise)), float(np.max(noise))],
           "noise_px_of_a_perfect_model": float(2.0 * np.sqrt((1.0 ** 3 - 0.5 ** 3) / (3 * 0.5)))}
    pool_s, pool_e = [], []
    for key in ("data", "filled"):
        m2, sg, er = (np.concatenate(v[key]) for v in (maha, sig, err))
        pool_s.append(sg)
        pool_e.append(er)
        res[key] = {"joints": int(m2.size), "share_below_chi2_68": float(np.mean(m2 < CHI2_3[0])), "share_below_chi2_95": float(np.mean(m2 < CHI2_3[1])),
                    "median_mahalanobis2": float(np.median(m2)), "rank_correlation_sigma_error": float(spearmanr(sg, er)[0]),
                    "median_sigma_mm": float(1e3 * np.median(sg)), "median_error_mm": float(1e3 * np.median(er))}
    res["rank_correlation_pooled"] = float(spearmanr(np.concatenate(pool_s), np.concatenate(pool_e))[0])
    return res


def cost(sizes, frames, repeats):
    import torch
    from body_fit_probe import make

    from multiview_motion_capture_amd import smoothing
    from multiview_motion_capture_amd.body_fit import fit_sequences
    from multiview_motion_capture_amd.sequences import track_sequences
    seqs_all = make(max(sizes), frames)
    recs_all = fit_sequences(seqs_all, track_sequences(seqs_all))
    try:
        with open(os.path.join(ROOT, "profiles", "smooth_probe.json")) as f:
            parent = json.load(f)["sizes"]
    except (OSError, ValueError, KeyError):
        parent = {}
    res = {}
    for S in sizes:
        seqs, recs = seqs_all[:S], recs_all[:S]
        n_tf = sum(t.frame_idxs[-1] - t.frame_idxs[0] + 1 for r in recs for t in r)
        times = {None: [], "joints": []}
        for cov in (None, "joints"):
            smoothing.smooth_sequences(seqs, recs, covariance=cov)
        torch.cuda.synchronize()
        for _ in range(repeats):
            for cov in (None, "joints"):          # alternating, the same session
                t0 = time.perf_counter()
                smoothing.smooth_sequences(seqs, recs, covariance=cov)
                torch.cuda.synchronize()
                times[cov].append(time.perf_counter() - t0)
        split = {}
        smoothing.smooth_sequences(seqs, recs, covariance="joints", timings=split)
        a, b = np.array(times[None]), np.array(times["joints"])
        res[str(S)] = {"tracklet_frames": n_tf, "identities": sum(len(r) for r in recs),
                       "none_s": {"best": float(a.min()), "median": float(np.median(a)), "max": float(a.max())},
                       "joints_s": {"best": float(b.min()), "median": float(np.median(b)), "max": float(b.max())},
                       "none_tracklet_frames_per_s": n_tf / float(a.min()),
                       "parent_tracklet_frames_per_s": parent.get(str(S), {}).get("tracklet_frames_per_s"),
                       "joints_over_none_best": float(b.min() / a.min()), "joints_over_none_median": float(np.median(b) / np.median(a)),
                       "split_ms": {k: 1e3 * v for k, v in split.items()},
                       "covariance_share_of_split": split["covariance"] / sum(split.values()),
                       "covariance_over_one_lm_iteration": split["covariance"] / ((split["blocks"] + split["solve"]) / 11.0)}
        print(f"S={S}: {n_tf} tracklet-frames, None {a.min():.3f} s (median {np.median(a):.3f}), joints {b.min():.3f} s (median "
              f"{np.median(b):.3f}), split ms {json.dumps({k: round(1e3 * v, 2) for k, v in split.items()})}", file=sys.stderr, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from multiview_motion_capture_amd import _cabi, smoothing
    res = {"build": _cabi.build_info(), "cov_mu": smoothing.COV_MU,
           "weights": (smoothing.ROOT_VEL, smoothing.ROOT_ACC, smoothing.ANG_VEL, smoothing.ANG_ACC)}
    res["calibration"] = calibration(args.frames)
    print("calibration:", json.dumps(res["calibration"]), file=sys.stderr, flush=True)
    res["cost"] = cost(args.sizes, args.frames, args.repeats)
    text = json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    main()
