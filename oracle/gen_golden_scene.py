"""Golden vectors of the REFERENCE tracker on the frames the benchmark times (bench.py --walk continuous, its default).

TEST INFRASTRUCTURE (build container only).  Runs the reference's own MvTracker.update_4d (motion_capture.py:873-963) from
/root/reference/src through ``oracle/ref_shim.py`` over selected 16-frame chains of whole benchmark steps, one fresh tracker per chain
(the benchmark's protocol); only checksums of the inputs and the outputs are written:

  synth_c4_scene_tracker.npz  config 4 (C5 P4, seed 20260103), the 10,000-frame step of segment 0: chain 0, the last chain and the two
                              chains whose heads have the smallest closest-pair root distance
  synth_c5_scene_tracker.npz  config 5 (C8 P8, seed 20260104), the 25,008-frame steps of segments 0 and 7 (segment 7: the last rank
                              of --frames-total 200064): chain 0 and the closest-pair chain of each

Each fixture holds the same per-frame tables as synth_c4_tracker.npz (oracle/gen_golden_ikconv.py) plus every frame's match_als
iteration count, the selected chains (``chains``, with ``segments`` giving each one's segment), and checksums of the whole step and of
the selected frames.  The steps are generated whole (tests/helpers.bench_step_data): a segment is not a prefix of a longer one.

    PYTHONDONTWRITEBYTECODE=1 python oracle/gen_golden_scene.py [--procs 8] [--only c4|c5]

Chains run in parallel worker processes (each chain has its own tracker, so the results do not depend on the split); BLAS is
single-threaded, as in oracle/gen_golden_ikconv.py (LAPACK's rounding depends on the thread count)."""
import argparse
import multiprocessing as mp
import os
import sys
import time

os.environ["OPENBLAS_NUM_THREADS"] = "1"
os.environ["OMP_NUM_THREADS"] = "1"

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_shim  # noqa: E402
import gen_golden_ikconv as gk  # noqa: E402
from helpers import bench_step_data, closest_pair_root  # noqa: E402

L = 16
SCENES = {
    "c4": dict(name="synth_c4_scene_tracker.npz", n_frames=10000, n_views=5, n_people=4, seed=20260103, segments=(0,), T=8,
               n_close=2, last=True),
    "c5": dict(name="synth_c5_scene_tracker.npz", n_frames=25008, n_views=8, n_people=8, seed=20260104, segments=(0, 7), T=16,
               n_close=1, last=False),
}

_M = None
_DATA = {}


def select_chains(gt_joints, n_close, last):
    """Chain 0, [the last chain,] and the n_close chains whose heads have the smallest closest-pair root distance (ties: lower index)."""
    n = gt_joints.shape[0] // L
    head = closest_pair_root(gt_joints[0::L])
    sel = [0] + ([n - 1] if last else [])
    for b in np.argsort(head, kind="stable"):
        if len(sel) == 1 + int(last) + n_close:
            break
        if int(b) not in sel:
            sel.append(int(b))
    return sel, head


def _run_chain(job):
    key, seg, b = job
    cfg = SCENES[key]
    syn = dict(n_frames=cfg["n_frames"], n_views=cfg["n_views"], n_people=cfg["n_people"], seed=cfg["seed"], chain_len=L)
    t0 = time.time()
    fix, cases = gk.run_synth_tracker(_M, syn, T=cfg["T"], data=_DATA[(key, seg)], chains=[b], with_als_iters=True)
    fix["solve_views"] = np.array([len(c["poses"]) for c in cases])
    print(f"{key} segment {seg} chain {b}: {len(cases)} solves in {time.time() - t0:.0f}s", flush=True)
    return fix


def main():
    global _M
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=8)
    ap.add_argument("--only", choices=sorted(SCENES), default=None)
    args = ap.parse_args()
    _M = ref_shim.load_modules()
    keys = [args.only] if args.only else sorted(SCENES)
    jobs, meta = [], {}
    for key in keys:
        cfg = SCENES[key]
        for seg in cfg["segments"]:
            data = bench_step_data(cfg["n_frames"], cfg["n_views"], cfg["n_people"], cfg["seed"], seg, L)
            _DATA[(key, seg)] = data
            sel, head = select_chains(data["gt_joints"], cfg["n_close"], cfg["last"])
            meta[(key, seg)] = (sel, head)
            jobs += [(key, seg, b) for b in sel]
            print(f"{key} segment {seg}: chains {sel}, closest-pair root distance at their heads "
                  f"{np.round(head[sel], 4).tolist()} m (all heads: median {np.median(head):.3f})", flush=True)
    t0 = time.time()
    with mp.get_context("fork").Pool(min(args.procs, len(jobs))) as pool:       # forked after the data exist: workers share them
        res = pool.map(_run_chain, jobs, chunksize=1)
    print(f"reference runs done in {time.time() - t0:.0f}s", flush=True)
    res = dict(zip(jobs, res))
    for key in keys:
        cfg = SCENES[key]
        parts, chains, segs, heads, sel_sum, step_sum = [], [], [], [], [], []
        for seg in cfg["segments"]:
            data = _DATA[(key, seg)]
            sel, head = meta[(key, seg)]
            parts += [res[(key, seg, b)] for b in sel]
            chains += sel
            segs += [seg] * len(sel)
            heads += [float(head[b]) for b in sel]
            step_sum.append(float(np.abs(data["kps25"].astype(np.float64)).sum()))
            sel_sum += [float(np.abs(data["kps25"][b * L:(b + 1) * L].astype(np.float64)).sum()) for b in sel]
        fix = {k: np.concatenate([p[k] for p in parts]) for k in ("meta", "params", "joints", "n_tracks", "n_dead", "n_solves",
                                                                    "solve_joints", "solve_cost", "solve_views", "als_iters")}
        fix["solve_info"] = np.concatenate([p["solve_info"] for p in parts])
        # where each chain's solves start in the solve tables
        fix["solve_start"] = np.cumsum([0] + [len(p["solve_cost"]) for p in parts])
        fix.update(seed=np.array(cfg["seed"]), n_frames=np.array(cfg["n_frames"]), chain_len=np.array(L), n_views=np.array(cfg["n_views"]),
                   n_people=np.array(cfg["n_people"]), segments=np.array(segs), chains=np.array(chains), head_closest_pair=np.array(heads),
                   step_checksum=np.array(step_sum), chain_checksum=np.array(sel_sum))
        np.savez_compressed(os.path.join(gk.OUT, cfg["name"]), **fix)
        it = fix["als_iters"]
        print(f"saved {cfg['name']}: chains {chains} (segments {segs}), {int(fix['n_solves'].sum())} solves, ALS iterations per frame "
              f"median {int(np.median(it))} max {int(it.max())} ({int((it >= 1000).sum())} at the cap)", flush=True)


if __name__ == "__main__":
    main()
