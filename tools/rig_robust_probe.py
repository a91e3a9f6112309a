"""Cost of the rig refinement's robust loss (rig_refine.refine_rigs(loss=...)) beside the plain least squares, in one run:
    python tools/rig_robust_probe.py [--sizes 1 8 64] [--frames 300] [--repeats 5] [--out profiles/rig_robust_probe.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/rig_robust_probe.py --sizes 64 --trace-run
    python tools/rig_robust_probe.py --merge FILE --stats DIR/.../*_kernel_stats.csv
The sequences are tools/rig_refine_probe.py's (synth.generate(frames, 5, 4, seed_s, walk="scene"), each rig perturbed by 1 degree /
3 cm, records from track_sequences on the perturbed rig).  Per S:
  trial_ms    device-event milliseconds of ONE trial's two entries at the packed start state of the S problems -- accumulate (tile
              parts, sum, solve) and step (back-substitution, trial cost, decision) -- through the entries without a loss and through
              the _robust entries with loss none, huber and cauchy at 6 px, alternating the four in every repeat; the median;
  refine_ms   whole refine_rigs calls (best of --repeats after one untimed call) with loss None, "huber" and "cauchy", with the trials
              they made: the reweighted iteration converges linearly, so the robust calls make more trials.
--trace-run makes one trial per loss for a kernel trace; --merge adds the rig kernels of that trace's statistics to the JSON, and the
ratios of the robust instantiations' mean times to the plain ones'."""
import argparse
import csv
import json
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

LOSS_PX = 6.0
WAYS = (("plain", None), ("none", 0), ("huber", 1), ("cauchy", 2))      # the entries without a loss, then the _robust entries


def pack(seqs, problems):
    """The packed start state of refine_rigs for the given sequences -> dict of device tensors."""
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
    info = np.zeros((S, _cabi.RIG_INFO_DOUBLES))
    part, part2, red = dev.rig_work(tile.shape[0], S, C, d)
    return dict(X=T(np.concatenate([p["X0"] for p in problems])), uv=T(np.concatenate([p["uv"] for p in problems])), tile=T(tile), seq=T(seq),
                slot=T(slot), cams=T(cams), info=T(info), ctl=torch.zeros((S, 4), dtype=torch.int32, device=d), part=part, part2=part2, red=red,
                tiles=int(tile.shape[0]))


def one_trial(st, code, events=None):
    """One trial from the packed start state (on copies) through the entries of ``code`` (None: those without a loss)."""
    from multiview_motion_capture_amd import device as dev
    from multiview_motion_capture_amd.body_fit import LM_FTOL, LM_MU0, LM_XTOL
    X, Xt, cams, camt, info, ctl = st["X"].clone(), st["X"].clone(), st["cams"].clone(), st["cams"].clone(), st["info"].clone(), st["ctl"].clone()
    a = (X, st["uv"], st["tile"], st["seq"], st["slot"], cams, camt, ctl, info, 10, LM_MU0, st["part"], st["red"], 1)
    b = (X, Xt, st["uv"], st["tile"], st["seq"], st["slot"], cams, camt, ctl, info, st["red"], 10, LM_FTOL, LM_XTOL, st["part2"])
    if events:
        events[0].record()
    if code is None:
        dev.rig_accumulate(*a)
    else:
        dev.rig_accumulate_robust(*a, code, LOSS_PX)
    if events:
        events[1].record()
    if code is None:
        dev.rig_step(*b)
    else:
        dev.rig_step_robust(*b, code, LOSS_PX)
    if events:
        events[2].record()


def trial_times(st, repeats):
    import torch
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    for _, code in WAYS:
        one_trial(st, code)
    torch.cuda.synchronize()
    t = {name: [] for name, _ in WAYS}
    for _ in range(repeats):
        for name, code in WAYS:
            one_trial(st, code, ev)
            torch.cuda.synchronize()
            t[name].append((ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2])))
    return {name: {"accumulate": float(np.median([x[0] for x in v])), "step": float(np.median([x[1] for x in v]))} for name, v in t.items()}


def merge(path, stats):
    with open(path) as f:
        res = json.load(f)
    rows = {}
    with open(stats) as f:
        for r in csv.DictReader(f):
            r = {k.lower(): v for k, v in r.items()}
            m = re.search(r"rig_\w+_kernel(<[\w, ]+>)?", r.get("name", ""))
            if m:
                rows[m.group(0)] = {"calls": int(r["calls"]), "mean_us": float(r["averagens"]) / 1e3, "max_us": float(r["maxns"]) / 1e3}
    res["trace_run_kernels"] = rows
    ratio = {}
    for k, v in rows.items():   # rig_accum_kernel<MFMA, LOSS, NI>, rig_backsub_kernel<LOSS, NI>
        m = re.fullmatch(r"(rig_(?:accum|backsub)_kernel)<(.*?)([12]), (\d)>", k)
        base = rows.get(f"{m.group(1)}<{m.group(2)}0, {m.group(4)}>") if m else None
        if base:
            ratio[k] = v["mean_us"] / base["mean_us"]
    res["trace_run_ratio_to_loss_none"] = ratio
    text = json.dumps(res)
    with open(path, "w") as f:
        f.write(text + "\n")
    print(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=5)
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
    from rig_refine_probe import best_of, make
    seqs_all = make(max(args.sizes), args.frames)
    recs_all = track_sequences(seqs_all)
    probs_all = []
    refine_rigs(seqs_all, recs_all, max_iter=0, problems=probs_all)
    if args.trace_run:
        S = max(args.sizes)
        st = pack(seqs_all[:S], probs_all[:S])
        for _ in range(3):
            for _, code in WAYS:
                one_trial(st, code)
        torch.cuda.synchronize()
        return
    res = {"frames_per_sequence": args.frames, "views": 5, "people": 4, "max_iter": 10, "loss_px": LOSS_PX, "build": _cabi.build_info(), "sizes": {}}
    for S in args.sizes:
        seqs, recs = seqs_all[:S], recs_all[:S]
        st = pack(seqs, probs_all[:S])
        tt = trial_times(st, args.repeats)
        row = {"points": int(st["X"].shape[0]), "tiles": st["tiles"], "trial_ms": tt,
               "trial_ratio_to_plain": {k: (v["accumulate"] + v["step"]) / (tt["plain"]["accumulate"] + tt["plain"]["step"]) for k, v in tt.items()},
               "refine": {}}
        for loss in (None, "huber", "cauchy"):
            ms = 1e3 * best_of(lambda: refine_rigs(seqs, recs, loss=loss), args.repeats)
            out = refine_rigs(seqs, recs, loss=loss)
            row["refine"][str(loss)] = {"ms": ms, "trials": int(sum(len(o.trials) for o in out)), "stops": sorted({o.stop for o in out}),
                                        "rms_px": [float(np.mean([o.rms_before for o in out])), float(np.mean([o.rms_after for o in out]))]}
        res["sizes"][str(S)] = row
        print(f"S={S:3d}: {json.dumps(row)}", file=sys.stderr, flush=True)
    text = json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
