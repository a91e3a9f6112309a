"""Cost of the re-linking step (relinking.relink_sequences) on S synthetic sequences, each with its own rig:
    python tools/relink_probe.py [--sizes 1 8 64] [--frames 300] [--repeats 5] [--long] [--out FILE]
Every sequence is synth.generate(frames, 5, 4, seed_s, walk="scene", occlusion=0.3) with its own seed, so its own cameras; its records
come from sequences.track_sequences, timed beside (best of two calls).  Per S: the whole relink_sequences call (best of --repeats after
one untimed call) and its parts from the same calls -- pack (input checks and host arrays), launch (one upload, the kernel, one
read-back), records (the merged MvTracklet records) -- the NumPy restatement (tests/relink_np.py) on the same records, and the records
before -> after.  --long adds one call on a single sequence of more than 256 records (8 people over 3,000 frames of ground truth, 40
cuts each: tests/test_gpu_relink.py's case, the cost matrix outside LDS), so that a rocprofv3 --kernel-trace --stats run of this tool
shows relink_kernel alone for it.  Prints one JSON object (the kernel-source sha of the library included)."""
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


def make(S, F, seed0=20271101):
    from multiview_motion_capture_amd import synth
    from multiview_motion_capture_amd.common import Calib
    out = []
    for s in range(S):
        d = synth.generate(F, 5, 4, seed0 + 17 * s, walk="scene", occlusion=0.3)
        out.append((d["kps25"], d["counts"], [Calib.from_k_rt(d["K"][c], d["Rt"][c]) for c in range(5)]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--long", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import relink_np as rn
    import torch
    from multiview_motion_capture_amd import _cabi, relinking
    from multiview_motion_capture_amd.sequences import track_sequences
    seqs_all = make(max(args.sizes), args.frames)
    par = dict(max_gap=relinking.MAX_GAP, max_dist=relinking.MAX_DIST, near_dist=relinking.NEAR_DIST, speed=relinking.SPEED)
    res = {"frames_per_sequence": args.frames, "views": 5, "people": 4, "occlusion": 0.3, "parameters": par,
           "build": _cabi.build_info(), "sizes": {}}
    for S in args.sizes:
        seqs = seqs_all[:S]
        t_track = []
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            recs = track_sequences(seqs)
            t_track.append(time.perf_counter() - t0)
        relinking.relink_sequences(recs)
        best = None
        for _ in range(args.repeats):
            tm = {}
            t0 = time.perf_counter()
            out = relinking.relink_sequences(recs, timings=tm)
            tm["call"] = time.perf_counter() - t0
            if best is None or tm["call"] < best["call"]:
                best = tm
        t0 = time.perf_counter()
        for r in recs:
            rn.relink(rn.records_of(r), **par)
        t_np = time.perf_counter() - t0
        row = dict(track_sequences_ms=1e3 * min(t_track), relink_ms=1e3 * best["call"], pack_ms=1e3 * best["pack"],
                   launch_readback_ms=1e3 * best["launch"], records_ms=1e3 * best["records"], numpy_restatement_ms=1e3 * t_np,
                   share_of_track_sequences=best["call"] / min(t_track), records_before=sum(len(r) for r in recs),
                   records_after=sum(len(r) for r in out), links=sum(len(r) for r in recs) - sum(len(r) for r in out),
                   records_of_10_poses_before=sum(len(t) >= 10 for r in recs for t in r),
                   records_of_10_poses_after=sum(len(t) >= 10 for r in out for t in r))
        res["sizes"][str(S)] = row
        print(S, json.dumps(row), file=sys.stderr, flush=True)
    if args.long:
        from multiview_motion_capture_amd import synth
        from relink_cases import fragments, make_tracklets
        gt = synth.generate(3000, 8, 8, 20270505, walk="scene")["gt_joints"]
        tl = make_tracklets([(i, f, j) for i, (_, f, j) in enumerate(fragments(gt, 20270505, 40, 16, 0.01))])
        relinking.relink_tracklets(tl, **par)
        tm = {}
        out = relinking.relink_tracklets(tl, timings=tm, **par)
        res["long"] = dict(records_before=len(tl), records_after=len(out), pack_ms=1e3 * tm["pack"],
                           launch_readback_ms=1e3 * tm["launch"], records_ms=1e3 * tm["records"])
        print("long", json.dumps(res["long"]), file=sys.stderr, flush=True)
    text = json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
