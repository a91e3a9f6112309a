"""Cost of the rig calibration (rig_init.calibrate_rigs) on S synthetic one-person walks, each with its own cameras, beside a
track_sequences call on S four-person sequences of the same length and cameras:
    python tools/rig_init_probe.py [--sizes 1 8 64] [--frames 300] [--repeats 3] [--out profiles/rig_init_probe.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/rig_init_probe.py --sizes 64 --trace-run
    python tools/rig_init_probe.py --merge FILE --stats DIR/.../*_kernel_stats.csv
Walk s is the four people of synth.generate(frames / 4, 5, 4, seed_s, walk="scene") concatenated into one person who visits four
places (tests/rig_init_cases.py: walk); the tracked sequence is generate(frames, 5, 4, seed_s, walk="scene") on the true rig.  Per S:
milliseconds of calibrate_rigs and of track_sequences (best of --repeats after one untimed call), the parts of one more call with
timings (observations, the three pair launches, the pose graph, the polish), and the worst camera's error against ground truth.
--trace-run makes one calibrate_rigs call for a kernel trace; --merge adds that trace's pair_* and rig_* kernels to the JSON."""
import argparse
import csv
import json
import os
import re
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))


def make(S, F, seed0=20281101):
    import rig_init_cases as rc
    from multiview_motion_capture_amd import synth
    from multiview_motion_capture_amd.common import Calib
    walks, scenes, truth = [], [], []
    for s in range(S):
        w = rc.walk(F, 5, seed0 + 17 * s)
        walks.append((w["kps25"], w["counts"], [(w["K"][c], (1032, 776)) for c in range(5)]))
        d = synth.generate(F, 5, 4, seed0 + 17 * s, walk="scene")
        scenes.append((d["kps25"], d["counts"], [Calib.from_k_rt(d["K"][c], d["Rt"][c]) for c in range(5)]))
        truth.append(w["Rt"])
    return walks, scenes, truth


def best_of(fn, repeats):
    import torch
    fn()
    torch.cuda.synchronize()
    best = np.inf
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best


def merge(path, stats):
    with open(path) as f:
        res = json.load(f)
    rows = []
    with open(stats) as f:
        for r in csv.DictReader(f):
            r = {k.lower(): v for k, v in r.items()}
            m = re.search(r"(pair|rig)_\w+(<[\w, ]+>)?", r.get("name", ""))
            if m:
                rows.append({"kernel": m.group(0), "calls": int(r["calls"]), "total_us": float(r["totaldurationns"]) / 1e3,
                             "mean_us": float(r["averagens"]) / 1e3, "max_us": float(r["maxns"]) / 1e3})
    res["trace_run_S64_kernels"] = rows
    text = json.dumps(res)
    with open(path, "w") as f:
        f.write(text + "\n")
    print(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--merge", default=None)
    ap.add_argument("--stats", default=None)
    args = ap.parse_args()
    if args.merge:
        return merge(args.merge, args.stats)
    import rig_refine_np as rr
    import torch
    from multiview_motion_capture_amd import _cabi
    from multiview_motion_capture_amd.rig_init import calibrate_rigs
    from multiview_motion_capture_amd.sequences import track_sequences
    walks_all, scenes_all, truth = make(max(args.sizes), args.frames)
    if args.trace_run:
        calibrate_rigs(walks_all[:max(args.sizes)])
        torch.cuda.synchronize()
        return
    res = {"frames_per_sequence": args.frames, "views": 5, "hypotheses": 128, "sample_frames": 8, "polish_iter": 10,
           "build": _cabi.build_info(), "sizes": {}}
    for S in args.sizes:
        walks, scenes = walks_all[:S], scenes_all[:S]
        t_cal = best_of(lambda: calibrate_rigs(walks), args.repeats)
        t_track = best_of(lambda: track_sequences(scenes), args.repeats)
        split = {}
        out = calibrate_rigs(walks, timings=split)
        errs = [rr.rig_errors(np.array([c.Rt for c in o.calibs]), truth[s]) for s, o in enumerate(out) if o.calibs is not None]
        res["sizes"][str(S)] = {"calibrated": len(errs), "calibrate_ms": 1e3 * t_cal, "track_ms": 1e3 * t_track,
                                "split_ms": {k: 1e3 * v for k, v in split.items()},
                                "worst_centre_mm": 1e3 * float(max(e[0].max() for e in errs)) if errs else None,
                                "worst_rotation_deg": float(np.degrees(max(e[1].max() for e in errs))) if errs else None,
                                "rms_px": float(np.mean([o.rms_px for o in out if o.calibs is not None])) if errs else None}
        print(f"S={S:3d}: {json.dumps(res['sizes'][str(S)])}", file=sys.stderr, flush=True)
    text = json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
