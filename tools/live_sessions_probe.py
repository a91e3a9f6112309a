"""Throughput of the live session pool (live.LivePool) against solo trackers, on S synthetic sessions with their own rigs:
    python tools/live_sessions_probe.py [--sizes 1 8 64 256] [--frames 300] [--solo-frames 60] [--out FILE]
Every session is synth.generate(frames, 5, 4, seed_s, walk="scene") with the seeds of tools/multi_rig_probe.py, so its own cameras; its
frames are FrameData of the device-ingested poses (made before the clock starts).  Per S it reports
  * pool:        LivePool(5, S) (p_max 8, t_max 8), one update_4d tick per frame for all S sessions, frames/s over S x frames;
  * pool_arrays: the same through update_4d_arrays (OpenPose rows, device ingest inside the tick);
  * solo:        S MvTrackers stepped round-robin on the same frames (the first --solo-frames frames), frames/s;
  * split:       the pool's tick time by part {pack (host packing + upload), launch (launch + read-back), records (MvTracklet
                 records), solo (detached sessions)}, in ms per tick.
Prints one JSON object."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def make(S, F, seed0=20271001):
    import torch
    from multiview_motion_capture_amd import device as dev, synth
    from multiview_motion_capture_amd.common import Calib
    out = []
    for s in range(S):
        d = synth.generate(F, 5, 4, seed0 + 17 * s, walk="scene")
        k17, c17 = dev.ingest(torch.from_numpy(d["kps25"]).cuda(), torch.from_numpy(d["counts"]).cuda())
        out.append(dict(kps25=d["kps25"], counts=d["counts"], k17=k17.cpu().numpy(), c17=c17.cpu().numpy(),
                        calibs=[Calib.from_k_rt(d["K"][c], d["Rt"][c]) for c in range(5)]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1, 8, 64, 256])
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--solo-frames", type=int, default=60, help="frames per session timed through the solo trackers")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from multiview_motion_capture_amd import motion_capture as mc
    from multiview_motion_capture_amd.live import LivePool, _frame_data
    F = args.frames
    seqs_all = make(max(args.sizes), F)
    res = {"frames_per_session": F, "views": 5, "people": 4, "p_max": 8, "t_max": 8, "sizes": {}}
    for S in args.sizes:
        seqs = seqs_all[:S]
        frames = [[_frame_data(f, q["k17"][f], q["c17"][f], q["calibs"]) for q in seqs] for f in range(F)]
        # pool, FrameData route
        pool = LivePool(5, S)
        sids = [pool.open_session(q["calibs"]) for q in seqs]
        pool.update_4d({sid: (0, frames[0][i]) for i, sid in enumerate(sids)})      # (first tick: allocations, untimed)
        for k in pool.timings:
            pool.timings[k] = 0.0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for f in range(1, F):
            pool.update_4d({sid: (f, frames[f][i]) for i, sid in enumerate(sids)})
        torch.cuda.synchronize()
        t_pool = time.perf_counter() - t0
        split = {k: 1e3 * v / (F - 1) for k, v in pool.timings.items()}
        detached = sum(pool.session(s).detached for s in sids)
        # pool, array route
        pa = LivePool(5, S)
        sa = [pa.open_session(q["calibs"]) for q in seqs]
        k25 = np.stack([q["kps25"] for q in seqs], 1).astype(np.float64)   # (F,S,C,P,25,3)
        cn = np.stack([q["counts"] for q in seqs], 1)
        pa.update_4d_arrays(sa, [0] * S, k25[0], cn[0])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for f in range(1, F):
            pa.update_4d_arrays(sa, [f] * S, k25[f], cn[f])
        torch.cuda.synchronize()
        t_arr = time.perf_counter() - t0
        # solo trackers, round-robin
        Fs = min(args.solo_frames, F)
        solos = [mc.MvTracker() for _ in range(S)]
        for i in range(S):
            solos[i].update_4d(0, frames[0][i])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for f in range(1, Fs):
            for i in range(S):
                solos[i].update_4d(f, frames[f][i])
        torch.cuda.synchronize()
        t_solo = time.perf_counter() - t0
        same = all(len(solos[i].tracklets) == len(pool.session(sids[i]).tracklets) for i in range(S)) if Fs == F else None
        r = dict(pool_fps=S * (F - 1) / t_pool, pool_arrays_fps=S * (F - 1) / t_arr, solo_fps=S * (Fs - 1) / t_solo,
                 tick_ms=1e3 * t_pool / (F - 1), tick_split_ms=split, detached_at_end=int(detached), same_tracklet_counts=same)
        r["speedup"] = r["pool_fps"] / r["solo_fps"]
        res["sizes"][S] = r
        print(S, json.dumps(r), flush=True)
        del pool, pa, solos
    txt = json.dumps(res)
    print(txt)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
