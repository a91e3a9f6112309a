"""Throughput of the body fit (body_fit.fit_sequences) on S synthetic sequences, each with its own rig:
    python tools/body_fit_probe.py [--sizes 1 8 64] [--frames 300] [--repeats 3] [--out FILE]
Every sequence is synth.generate(frames, 5, 4, seed_s, walk="scene") with its own seed, so its own cameras; its records come from
sequences.track_sequences (untimed).  Per S it reports tracklet-frames/s of the whole fit_sequences call (3 rounds, best of --repeats
timed calls after one untimed call) and, from one more call with timings, the seconds in each part: selection (ingest + observe, one
host read), length steps, pose steps, host records.  Prints one JSON object (the kernel-source sha of the library included)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def make(S, F, seed0=20271001):
    from multiview_motion_capture_amd import synth
    from multiview_motion_capture_amd.common import Calib
    out = []
    for s in range(S):
        d = synth.generate(F, 5, 4, seed0 + 17 * s, walk="scene")
        out.append((d["kps25"], d["counts"], [Calib.from_k_rt(d["K"][c], d["Rt"][c]) for c in range(5)]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from multiview_motion_capture_amd import _cabi
    from multiview_motion_capture_amd.body_fit import fit_sequences
    from multiview_motion_capture_amd.sequences import track_sequences
    seqs_all = make(max(args.sizes), args.frames)
    recs_all = track_sequences(seqs_all)
    res = {"frames_per_sequence": args.frames, "views": 5, "people": 4, "rounds": 3, "build": _cabi.build_info(), "sizes": {}}
    for S in args.sizes:
        seqs, recs = seqs_all[:S], recs_all[:S]
        n_tf = sum(len(t) for r in recs for t in r)
        fit_sequences(seqs, recs)
        torch.cuda.synchronize()
        best = np.inf
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            fit_sequences(seqs, recs)
            torch.cuda.synchronize()
            best = min(best, time.perf_counter() - t0)
        split = {}
        fit_sequences(seqs, recs, timings=split)
        res["sizes"][str(S)] = {"tracklet_frames": n_tf, "identities": sum(len(r) for r in recs), "fit_s": best,
                                "tracklet_frames_per_s": n_tf / best, "split_ms": {k: 1e3 * v for k, v in split.items()}}
        print(f"S={S:3d}: {n_tf} tracklet-frames, {n_tf / best:10.0f} tracklet-frames/s ({best:.3f} s)   split ms "
              f"{json.dumps({k: round(1e3 * v, 2) for k, v in split.items()})}", file=sys.stderr, flush=True)
    text = json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
