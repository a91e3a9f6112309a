"""Cost of the fixed-lag live smoother (live_smoothing.LiveSmoother) beside the live session pool it follows:
    python tools/live_smooth_probe.py [--sizes 1 8 64 256] [--frames 300] [--no-trace] [--out FILE]
Every session is synth.generate(frames, 5, 4, seed_s, walk="scene") with the seeds of tools/live_sessions_probe.py, so its own cameras;
its frames are FrameData of the device-ingested poses (made before the clock starts).  Per S, in the same run:
  * pool_tick_ms:       LivePool(5, S).update_4d alone, per tick (the first tick, with its allocations, is not timed);
  * both_tick_ms:       a second pool on the same frames, pool.update_4d + LiveSmoother.update_4d (default window, lag, trials);
  * smoother_tick_ms:   the smoother's share of it, and its split {pack (host: tables, rows, items), launch (uploads, launches and the
                        read-back), records}, in ms per tick; items and free rows per tick.
Unless --no-trace, two rocprofv3 --kernel-trace runs of fresh child processes follow (the program itself after "--"):
  * this file with --child: one session, every tick's mvmc_smooth_window launch matched with the tick's free rows and sweeps ->
    window_us_per_block_row: kernel time per (free row x sweep) of the launch's largest identity over the steady ticks (full window),
    the row blocks of the trials included;
  * tools/smooth_probe.py --sizes 1: mvmc_smooth_step's kernel time per (row x sweep), the offline block row (its row blocks are a
    kernel of their own and are NOT included) -> step_us_per_block_row.
Prints one JSON object (the kernel-source sha of the library included)."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _frames(seqs, F):
    from multiview_motion_capture_amd.live import _frame_data
    return [[_frame_data(f, q["k17"][f], q["c17"][f], q["calibs"]) for q in seqs] for f in range(F)]


def _sweeps(s):
    """Sweeps of one solve: one per trial, and one more when the solve stopped on a step that was not tried."""
    return len(s["trials"]) + (1 if s["stop"] in (2, 3, 5) else 0)


def child(F):
    """One session through pool + smoother; prints per tick the free rows and sweeps of the identity with the most (rows x sweeps)."""
    from live_sessions_probe import make
    from multiview_motion_capture_amd.live import LivePool
    from multiview_motion_capture_amd.live_smoothing import LiveSmoother
    seqs = make(1, F)
    frames = _frames(seqs, F)
    pool = LivePool(5, 1)
    sm = LiveSmoother.for_pool(pool)
    sid = pool.open_session(seqs[0]["calibs"])
    ticks = []
    for f in range(F):
        pool.update_4d({sid: (f, frames[f][0])})
        out = sm.update_4d({sid: (f, frames[f][0])})[sid]
        rows = {i.tid: min(sm.W, i.n) for i in sm._sessions[sid].ids.values()}
        work = [(rows[t] * _sweeps(s), rows[t], _sweeps(s)) for t, s in out.solved.items()]
        ticks.append(dict(launched=bool(rows), work=max(work)[0] if work else 0, rows=max(work)[1] if work else 0,
                          sweeps=max(work)[2] if work else 0))
    print("CHILD " + json.dumps(dict(window=sm.W, n_iter=sm.n_iter, ticks=ticks)))


def _trace(cmd, kernel):
    """Runs cmd under rocprofv3 --kernel-trace in a fresh process -> (stdout, [duration in us of every launch of ``kernel``, in order])."""
    with tempfile.TemporaryDirectory() as d:
        p = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"] + cmd, capture_output=True,
                           text=True, cwd=ROOT)
        if p.returncode != 0:
            raise RuntimeError(f"rocprofv3 {' '.join(cmd)}: exit {p.returncode}: {p.stderr[-2000:]}")
        files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        rows = sorted((r for f in files for r in csv.DictReader(open(f))), key=lambda r: int(r["Start_Timestamp"]))
        dur = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if kernel in r["Kernel_Name"]]
    return p.stdout, dur


def trace(F):
    py = sys.executable
    out, dur = _trace([py, os.path.abspath(__file__), "--child", "--frames", str(F)], "smooth_window_kernel")
    info = json.loads([ln for ln in out.splitlines() if ln.startswith("CHILD ")][-1][6:])
    ticks = [t for t in info["ticks"] if t["launched"]]
    if len(ticks) != len(dur):
        raise RuntimeError(f"{len(dur)} traced launches of mvmc_smooth_window for {len(ticks)} ticks with identities")
    steady = [(t, u) for t, u in zip(ticks, dur) if t["rows"] == info["window"] and t["sweeps"] == info["n_iter"]]
    res = dict(window_launches=len(dur), window_steady_launches=len(steady), window_kernel_us_mean=float(np.mean(dur)),
               window_steady_kernel_us_mean=float(np.mean([u for _, u in steady])),
               window_us_per_block_row=float(np.sum([u for _, u in steady]) / np.sum([t["work"] for t, _ in steady])))
    out, dur = _trace([py, os.path.join(ROOT, "tools", "smooth_probe.py"), "--sizes", "1", "--repeats", "1", "--frames", str(F)],
                      "smooth_step_kernel")
    sp = json.loads(out.strip().splitlines()[-1])
    it = int(sp["max_iter"])
    calls = len(dur) // (it + 1)             # smooth_sequences calls: max_iter + 1 step launches each, the last without a sweep
    res.update(step_launches=len(dur), step_kernel_us_total=float(np.sum(dur)), step_rows=F,
               step_us_per_block_row=float(np.sum(dur) / (calls * it * F)))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1, 8, 64, 256])
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    F = args.frames
    if args.child:
        return child(F)
    import torch
    from live_sessions_probe import make
    from multiview_motion_capture_amd import _cabi
    from multiview_motion_capture_amd.live import LivePool
    from multiview_motion_capture_amd.live_smoothing import LiveSmoother
    seqs_all = make(max(args.sizes), F)
    res = {"frames_per_session": F, "views": 5, "people": 4, "build": _cabi.build_info(), "sizes": {}}
    for S in args.sizes:
        seqs = seqs_all[:S]
        frames = _frames(seqs, F)
        pool = LivePool(5, S)
        sids = [pool.open_session(q["calibs"]) for q in seqs]
        pool.update_4d({sid: (0, frames[0][i]) for i, sid in enumerate(sids)})
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for f in range(1, F):
            pool.update_4d({sid: (f, frames[f][i]) for i, sid in enumerate(sids)})
        torch.cuda.synchronize()
        t_pool = time.perf_counter() - t0
        del pool
        pool = LivePool(5, S)
        sm = LiveSmoother.for_pool(pool)
        res.update(window=sm.W, lag=sm.lag, n_iter=sm.n_iter)
        sids = [pool.open_session(q["calibs"]) for q in seqs]
        tick = {sid: (0, frames[0][i]) for i, sid in enumerate(sids)}
        pool.update_4d(tick)
        sm.update_4d(tick)
        for k in sm.timings:
            sm.timings[k] = 0.0
        torch.cuda.synchronize()
        t_sm, items, rows = 0.0, 0, 0
        t0 = time.perf_counter()
        for f in range(1, F):
            tick = {sid: (f, frames[f][i]) for i, sid in enumerate(sids)}
            pool.update_4d(tick)
            t1 = time.perf_counter()
            out = sm.update_4d(tick)
            t_sm += time.perf_counter() - t1
            items += sum(len(o.solved) for o in out.values())
            rows += sum(min(sm.W, i.n) for s in sm._sessions.values() for i in s.ids.values() if i.n >= 2)
        torch.cuda.synchronize()
        t_both = time.perf_counter() - t0
        n = F - 1
        r = dict(pool_tick_ms=1e3 * t_pool / n, both_tick_ms=1e3 * t_both / n, smoother_tick_ms=1e3 * t_sm / n,
                 smoother_split_ms={k: 1e3 * v / n for k, v in sm.timings.items()}, solved_per_tick=items / n, free_rows_per_tick=rows / n,
                 smoother_over_pool=t_sm / t_pool)
        res["sizes"][S] = r
        print(S, json.dumps(r), file=sys.stderr, flush=True)
        del pool, sm
    if not args.no_trace:
        res["kernel"] = trace(F)
        k = res["kernel"]
        k["window_faster_than_step"] = bool(k["window_us_per_block_row"] < k["step_us_per_block_row"])
    txt = json.dumps(res)
    print(txt)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
