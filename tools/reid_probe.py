"""Cost of the re-identification step (relinking.reidentify_sequences) on S synthetic sequences, each with its own rig:
    python tools/reid_probe.py [--sizes 1 8 64] [--frames 300] [--repeats 5] [--out FILE]
Every sequence is synth.generate(frames, 5, 4, seed_s, walk="scene", occlusion=0.3) with its own seed, as in tools/relink_probe.py; its
records come from sequences.track_sequences(relink=True), timed beside in the same session (best of two calls).  Per S: the whole
reidentify_sequences call (best of --repeats after one untimed call) and its parts -- pack (input checks, every pose read once),
launch (upload, two launches, read-back), records -- and, from one more call that synchronises between them, upload, the two launches
by device events, and read-back; the NumPy restatement (tests/reid_np.py) on the same records; records and poses before -> after.
Prints one JSON object (the kernel-source sha of the library included)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import reid_np as rp
    import torch
    from multiview_motion_capture_amd import _cabi, relinking
    from multiview_motion_capture_amd.sequences import track_sequences
    from relink_probe import make
    seqs_all = make(max(args.sizes), args.frames)
    par = dict(max_z=relinking.MAX_Z, ratio=relinking.RATIO, floor=relinking.FLOOR, min_poses=relinking.MIN_POSES, reach=relinking.REACH,
               speed=relinking.REID_SPEED)
    res = {"frames_per_sequence": args.frames, "views": 5, "people": 4, "occlusion": 0.3, "parameters": par,
           "build": _cabi.build_info(), "sizes": {}}
    for S in args.sizes:
        seqs = seqs_all[:S]
        t_track = []
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            recs = track_sequences(seqs, relink=True)
            t_track.append(time.perf_counter() - t0)
        relinking.reidentify_sequences(recs)
        best = None
        for _ in range(args.repeats):
            tm = {}
            t0 = time.perf_counter()
            out = relinking.reidentify_sequences(recs, timings=tm)
            tm["call"] = time.perf_counter() - t0
            if best is None or tm["call"] < best["call"]:
                best = tm
        ev = {}
        relinking.solve_reid(relinking.pack_reid(recs), events=ev, **par)
        t0 = time.perf_counter()
        for r in recs:
            rp.reidentify(rp.records_of(r), **par)
        t_np = time.perf_counter() - t0
        row = dict(track_sequences_ms=1e3 * min(t_track), reidentify_ms=1e3 * best["call"], pack_ms=1e3 * best["pack"],
                   launch_readback_ms=1e3 * best["launch"], records_ms=1e3 * best["records"], upload_ms=ev["upload_ms"],
                   signature_launch_ms=ev["signature_ms"], link_launch_ms=ev["link_ms"], readback_ms=ev["readback_ms"],
                   numpy_restatement_ms=1e3 * t_np, share_of_track_sequences=best["call"] / min(t_track),
                   poses=sum(len(t) for r in recs for t in r), records_before=sum(len(r) for r in recs),
                   records_after=sum(len(r) for r in out), records_of_10_poses_before=sum(len(t) >= 10 for r in recs for t in r),
                   records_of_10_poses_after=sum(len(t) >= 10 for r in out for t in r))
        res["sizes"][str(S)] = row
        print(S, json.dumps(row), file=sys.stderr, flush=True)
    text = json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
