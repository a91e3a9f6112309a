"""Cost of the rig refinement's intrinsic unknowns (rig_refine.refine_rigs(intrinsics=...)) beside the refinement without them, in one run:
    python tools/rig_intr_probe.py [--sizes 1 8 64] [--frames 300] [--repeats 3] [--out profiles/rig_intr_probe.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/rig_intr_probe.py --sizes 64 --trace-run
(--trace-run: three trials per way at the largest size, for a kernel trace.)
The sequences are tools/rig_refine_probe.py's (synth.generate(frames, 5, 4, seed_s, walk="scene"), each rig perturbed by 1 degree /
3 cm) with every camera's focal length off by a seeded U(-3 %, +3 %); the records come from track_sequences on that rig.  Per S:
  trial_ms    device-event milliseconds of ONE trial's two entries at the packed start state of the S problems -- accumulate (tile
              parts, sum, solve) and step (back-substitution, trial cost, decision) -- through the entries without intrinsics (the
              code every earlier revision runs) and through the _intr entries with "focal" and with "focal+centre" (centre_sigma_px
              20), the three ways alternating in every repeat; the median; and the ratios to the trial without intrinsics;
  refine_ms   whole refine_rigs calls (best of --repeats after one untimed call) with intrinsics None, "focal" and "focal+centre",
              the trials they made, the plain rms and the worst focal error they end with; and track_ms, the track_sequences call
              that produced the records."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

CENTRE_SIGMA_PX = 20.0
WAYS = (("none", 0), ("focal", 1), ("focal+centre", 3))


def off_focal(seqs, seed=20271103, pct=3.0):
    """The sequences with every camera's fx, fy times e^U(-pct, +pct) % -> (sequences, the true K per sequence)."""
    from multiview_motion_capture_amd.common import Calib
    rng = np.random.default_rng(seed)
    out, true = [], []
    for kps, cnt, cal in seqs:
        K = np.array([np.asarray(c.K, np.float64) for c in cal])
        true.append(K.copy())
        f = np.exp(rng.uniform(-pct, pct, len(cal)) / 100.0)
        K[:, 0, 0] *= f
        K[:, 1, 1] *= f
        out.append((kps, cnt, [Calib.from_k_rt(K[c], np.asarray(cal[c].Rt, np.float64)) for c in range(len(cal))]))
    return out, true


def pack(seqs, problems):
    """The packed start state of refine_rigs for the given sequences -> dict of device tensors, with the work buffers of each way."""
    import torch
    from multiview_motion_capture_amd import _cabi
    from multiview_motion_capture_amd import device as dev
    from multiview_motion_capture_amd import rig_refine as rg
    d = torch.device("cuda:0")
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(d)
    S, C = len(seqs), len(seqs[0][2])
    tile, seq = rg.tile_tables([p["X0"].shape[0] for p in problems])
    slot = np.tile(np.arange(-1, C - 1, dtype=np.int32), (S, 1))
    K = np.array([[np.asarray(c.K, np.float64) for c in s[2]] for s in seqs])
    Rt = np.array([[np.asarray(c.Rt, np.float64) for c in s[2]] for s in seqs])
    cams = np.concatenate([K.reshape(S, C, 9), Rt[:, :, :, :3].reshape(S, C, 9), Rt[:, :, :, 3]], axis=2)
    work = {0: dev.rig_work(tile.shape[0], S, C, d), 1: dev.rig_work_intr(tile.shape[0], S, C, 1, d), 3: dev.rig_work_intr(tile.shape[0], S, C, 3, d)}
    return dict(X=T(np.concatenate([p["X0"] for p in problems])), uv=T(np.concatenate([p["uv"] for p in problems])), tile=T(tile), seq=T(seq),
                slot=T(slot), islot=T(np.tile(np.arange(C, dtype=np.int32), (S, 1))), K0=T(K[:, :, [0, 0, 1], [0, 2, 2]]), cams=T(cams),
                info=T(np.zeros((S, _cabi.RIG_INFO_DOUBLES))), ctl=torch.zeros((S, 4), dtype=torch.int32, device=d), work=work,
                tiles=int(tile.shape[0]))


def one_trial(st, n_intr, events=None):
    """One trial from the packed start state (on copies) without intrinsics (n_intr 0) or through the _intr entries."""
    from multiview_motion_capture_amd import device as dev
    from multiview_motion_capture_amd.body_fit import LM_FTOL, LM_MU0, LM_XTOL
    X, Xt, cams, camt, info, ctl = st["X"].clone(), st["X"].clone(), st["cams"].clone(), st["cams"].clone(), st["info"].clone(), st["ctl"].clone()
    part, part2, red = st["work"][n_intr]
    a = (X, st["uv"], st["tile"], st["seq"], st["slot"], cams, camt, ctl, info, 10, LM_MU0, part, red)
    b = (X, Xt, st["uv"], st["tile"], st["seq"], st["slot"], cams, camt, ctl, info, red, 10, LM_FTOL, LM_XTOL, part2)
    k = (n_intr, st["islot"], st["K0"], float("inf"), CENTRE_SIGMA_PX)
    if events:
        events[0].record()
    if n_intr:
        dev.rig_accumulate_intr(*a, *k)
    else:
        dev.rig_accumulate(*a, 1)
    if events:
        events[1].record()
    if n_intr:
        dev.rig_step_intr(*b, *k)
    else:
        dev.rig_step(*b)
    if events:
        events[2].record()


def trial_times(st, repeats):
    import torch
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    for _, n in WAYS:
        one_trial(st, n)
    torch.cuda.synchronize()
    t = {name: [] for name, _ in WAYS}
    for _ in range(repeats):
        for name, n in WAYS:
            one_trial(st, n, ev)
            torch.cuda.synchronize()
            t[name].append((ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2])))
    return {name: {"accumulate": float(np.median([x[0] for x in v])), "step": float(np.median([x[1] for x in v]))} for name, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-run", action="store_true")
    args = ap.parse_args()
    from multiview_motion_capture_amd import _cabi
    from multiview_motion_capture_amd.rig_refine import refine_rigs
    from multiview_motion_capture_amd.sequences import track_sequences
    from rig_refine_probe import best_of, make
    seqs_all, K_true = off_focal(make(max(args.sizes), args.frames))
    print(f"{len(seqs_all)} sequences made", file=sys.stderr, flush=True)
    recs_all = track_sequences(seqs_all)
    probs_all = []
    refine_rigs(seqs_all, recs_all, max_iter=0, problems=probs_all)
    if args.trace_run:
        import torch
        st = pack(seqs_all, probs_all)
        for _ in range(3):
            for _, n in WAYS:
                one_trial(st, n)
        torch.cuda.synchronize()
        return
    modes ={"None": {}, "focal": dict(intrinsics="focal"), "focal+centre": dict(intrinsics="focal+centre", centre_sigma_px=CENTRE_SIGMA_PX)}
    res = {"frames_per_sequence": args.frames, "views": 5, "people": 4, "max_iter": 10, "focal_off_pct": 3.0, "centre_sigma_px": CENTRE_SIGMA_PX,
           "build": _cabi.build_info(), "sizes": {}}
    for S in args.sizes:
        seqs, recs = seqs_all[:S], recs_all[:S]
        st = pack(seqs, probs_all[:S])
        tt = trial_times(st, args.repeats)
        total = {k: v["accumulate"] + v["step"] for k, v in tt.items()}
        row = {"points": int(st["X"].shape[0]), "tiles": st["tiles"], "trial_ms": tt, "trial_ratio_to_none": {k: v / total["none"] for k, v in total.items()},
               "track_ms": 1e3 * best_of(lambda: track_sequences(seqs), args.repeats), "refine": {}}
        for name, kw in modes.items():
            ms = 1e3 * best_of(lambda: refine_rigs(seqs, recs, **kw), args.repeats)
            out = refine_rigs(seqs, recs, **kw)
            fe = [np.abs(np.log(np.array([c.K[0, 0] for c in o.calibs]) / K_true[i][:, 0, 0])).max() for i, o in enumerate(out)]
            row["refine"][name] = {"ms": ms, "trials": int(sum(len(o.trials) for o in out)), "stops": sorted({o.stop for o in out}),
                                   "rms_px": [float(np.mean([o.rms_before for o in out])), float(np.mean([o.rms_after for o in out]))],
                                   "worst_focal_error_pct": [100.0 * float(np.mean(fe)), 100.0 * float(np.max(fe))]}
        res["sizes"][str(S)] = row
        print(f"S={S:3d}: {json.dumps(row)}", file=sys.stderr, flush=True)
    text = json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
