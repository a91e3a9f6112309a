"""Cost of the rig refinement (rig_refine.refine_rigs) on S synthetic sequences, each with its own rig, beside the track_sequences call
that produced its records:
    python tools/rig_refine_probe.py [--sizes 1 8 64] [--frames 300] [--repeats 3] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/rig_refine_probe.py --sizes 64 --trace-run
    python tools/rig_refine_probe.py --merge FILE --stats DIR/.../*_kernel_stats.csv
Every sequence is synth.generate(frames, 5, 4, seed_s, walk="scene") with its own seed, so its own cameras, perturbed by 1 degree / 3 cm
(cameras 1-4); its records come from sequences.track_sequences on the perturbed rig.  Per S: milliseconds of track_sequences and of
refine_rigs (best of --repeats after one untimed call) with the tile products on the matrix cores (variant 1) and as FMAs (variant 0),
and from one more call with timings the parts: selection, start values, trials, host records.  --trace-run makes one refine_rigs call
per variant for a kernel trace; --merge adds the rig kernels of that trace's statistics to the JSON."""
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


def make(S, F, seed0=20271101):
    import rig_refine_np as rr
    from multiview_motion_capture_amd import synth
    from multiview_motion_capture_amd.common import Calib
    out = []
    for s in range(S):
        d = synth.generate(F, 5, 4, seed0 + 17 * s, walk="scene")
        Rt = rr.perturb_rig(d["Rt"], seed0 + 17 * s + 1)
        out.append((d["kps25"], d["counts"], [Calib.from_k_rt(d["K"][c], Rt[c]) for c in range(5)]))
    return out


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
            if "rig_" in r.get("name", ""):
                rows.append({"kernel": re.search(r"rig_\w+(<[\w, ]+>)?", r["name"]).group(0), "calls": int(r["calls"]), "total_us": float(r["totaldurationns"]) / 1e3,
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
    import torch
    from multiview_motion_capture_amd import _cabi
    from multiview_motion_capture_amd.rig_refine import refine_rigs
    from multiview_motion_capture_amd.sequences import track_sequences
    seqs_all = make(max(args.sizes), args.frames)
    recs_all = track_sequences(seqs_all)
    if args.trace_run:
        S = max(args.sizes)
        for variant in (1, 0):
            refine_rigs(seqs_all[:S], recs_all[:S], variant=variant)
        torch.cuda.synchronize()
        return
    res = {"frames_per_sequence": args.frames, "views": 5, "people": 4, "max_iter": 10, "build": _cabi.build_info(), "sizes": {}}
    for S in args.sizes:
        seqs, recs = seqs_all[:S], recs_all[:S]
        t_track = best_of(lambda: track_sequences(seqs), args.repeats)
        t_ref = {v: best_of(lambda: refine_rigs(seqs, recs, variant=v), args.repeats) for v in (1, 0)}
        split = {}
        out = refine_rigs(seqs, recs, timings=split)
        res["sizes"][str(S)] = {"points": int(sum(o.n_points for o in out)), "observations": int(sum(o.n_obs for o in out)),
                                "trials": int(sum(len(o.trials) for o in out)), "track_ms": 1e3 * t_track,
                                "refine_ms_mfma": 1e3 * t_ref[1], "refine_ms_fma": 1e3 * t_ref[0],
                                "split_ms": {k: 1e3 * v for k, v in split.items()},
                                "rms_px": [float(np.mean([o.rms_before for o in out])), float(np.mean([o.rms_after for o in out]))]}
        print(f"S={S:3d}: {json.dumps(res['sizes'][str(S)])}", file=sys.stderr, flush=True)
    text = json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
