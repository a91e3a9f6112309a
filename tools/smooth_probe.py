"""Throughput of the trajectory smoother (smoothing.smooth_sequences) on S synthetic sequences, each with its own rig:
    python tools/smooth_probe.py [--sizes 1 8 64] [--frames 300] [--repeats 3] [--numpy] [--out FILE]
Every sequence is synth.generate(frames, 5, 4, seed_s, walk="scene") with its own seed, so its own cameras; its records come from
sequences.track_sequences -> body_fit.fit_sequences (untimed).  Per S it reports tracklet-frames/s of the whole smooth_sequences call
(default weights, max_iter 10, best of --repeats timed calls after one untimed call) and, from one more call with timings, the seconds in
each part: host preparation (input checks, unwrapping and interpolation, packing and uploads), selection (ingest + observe, one host
read), block launches, step launches, host records; and the number of launch sequences the default workspace cap splits the call into.
The largest S is timed again with --big-cap bytes of workspace (one launch sequence).  --numpy also times the NumPy restatement
(tests/smooth_np.py) at S = 1.  Prints one JSON object (the kernel-source sha of the library included)."""
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


def main():
    from body_fit_probe import make
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--numpy", action="store_true")
    ap.add_argument("--big-cap", type=int, default=1 << 33)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from multiview_motion_capture_amd import _cabi, smoothing
    from multiview_motion_capture_amd.body_fit import fit_sequences
    from multiview_motion_capture_amd.sequences import track_sequences
    seqs_all = make(max(args.sizes), args.frames)
    recs_all = fit_sequences(seqs_all, track_sequences(seqs_all))
    w = (smoothing.ROOT_VEL, smoothing.ROOT_ACC, smoothing.ANG_VEL, smoothing.ANG_ACC)
    res = {"frames_per_sequence": args.frames, "views": 5, "people": 4, "max_iter": 10, "weights": w, "build": _cabi.build_info(),
           "sizes": {}}
    def launches(recs, cap_bytes):
        """launch sequences of smooth_sequences' greedy packing (one camera group here)"""
        per_row = 8 * (2 * smoothing._BLOCK + smoothing._WORK + 2 * 68) + 4 * 8
        cap = max(1, cap_bytes // per_row)
        spans = [t.frame_idxs[-1] - t.frame_idxs[0] + 1 for r in recs for t in r if len(t) >= 2]
        n, rows = 0, None
        for m in spans:
            if rows is None or rows + m > cap:
                n, rows = n + 1, m
            else:
                rows += m
        return n

    def run(S, cap, key):
        seqs, recs = seqs_all[:S], recs_all[:S]
        n_tf = sum(t.frame_idxs[-1] - t.frame_idxs[0] + 1 for r in recs for t in r)
        smoothing.smooth_sequences(seqs, recs, max_work_bytes=cap)
        torch.cuda.synchronize()
        best = np.inf
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            smoothing.smooth_sequences(seqs, recs, max_work_bytes=cap)
            torch.cuda.synchronize()
            best = min(best, time.perf_counter() - t0)
        split = {}
        smoothing.smooth_sequences(seqs, recs, max_work_bytes=cap, timings=split)
        res["sizes"][key] = {"tracklet_frames": n_tf, "identities": sum(len(r) for r in recs), "max_work_bytes": cap,
                             "launch_sequences": launches(recs, cap), "smooth_s": best, "tracklet_frames_per_s": n_tf / best,
                             "split_ms": {k: 1e3 * v for k, v in split.items()}, "split_sum_over_call": sum(split.values()) / best}
        print(f"S={key}: {n_tf} tracklet-frames, {n_tf / best:10.0f} tracklet-frames/s ({best:.3f} s), {launches(recs, cap)} launch "
              f"sequence(s), split ms {json.dumps({k: round(1e3 * v, 2) for k, v in split.items()})}", file=sys.stderr, flush=True)

    for S in args.sizes:
        run(S, smoothing.MAX_WORK_BYTES, str(S))
    run(max(args.sizes), args.big_cap, f"{max(args.sizes)}_big_cap")
    if args.numpy:
        import body_fit_np as bf
        import smooth_np as sm
        from test_gpu_body_fit import _np_records
        g = seqs_all[0]
        Ps = np.array([np.asarray(c.P, np.float64).reshape(3, 4) for c in g[2]])
        t0 = time.perf_counter()
        sm.smooth([bf.ingest_np(g[0], g[1])], [Ps], [_np_records(recs_all[0])], w)
        dt = time.perf_counter() - t0
        n_tf = res["sizes"][str(args.sizes[0])]["tracklet_frames"] if args.sizes[0] == 1 else None
        res["numpy_S1_s"] = dt
        if n_tf:
            res["numpy_S1_tracklet_frames_per_s"] = n_tf / dt
        print(f"NumPy restatement, S=1: {dt:.1f} s", file=sys.stderr, flush=True)
    text = json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    main()
