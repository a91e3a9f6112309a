"""What the exchange repair (exchanges.repair_sequences) finds, buys and costs on the device:
    python tools/exchange_probe.py [--sizes 1 8 64] [--frames 300] [--cost-frames 150] [--repeats 5] [--out profiles/exchange_probe.json]
Accuracy: tools/smooth_robust_probe.py's held-out synthetic scene walks (seeds 71, 72, 73, rigs (5,4), (4,3), (5,2), 300 frames,
occlusion 0.3), contaminated at the door and through the real tracker (at the longest chain length of 16, 8, 4 its stitch takes), twice:
with the exchanges alone (20 % of the detections with the arms OR the legs exchanged: what the repair is for), and with the probe's whole
contamination (then 10 % of the keypoints moved by 30 - 150 px, which the repair does not address).
  sources     precision and recall of the flags per group against the drawn exchanges (a slot that holds a detection of a real person),
              with the records taken from (a) the tracker, (b) the body fit, (c) the Cauchy smoother;
  downstream  on the clean, the contaminated and the repaired keypoints (repaired against (c); "repaired_twice": the contaminated
              keypoints repaired against the Cauchy smoother's records of the repaired ones): the tracker's MPJPE, fit_sequences'
              length error (the slots the fit measures: all but the three the mid-spine guess biases), smooth_sequences' MPJPE on the
              frames with data and on the filled frames (10-20-frame holes, hole stream 9) and its jitter, with loss=None and "cauchy";
  sweep       margin_px x ratio against (c): precision and recall over all groups.
A record follows the generator's person its joints are nearest to; records shorter than 10 frames are left out of the errors.
Cost: S synthetic sequences of --cost-frames frames (tools/body_fit_probe.py's) with the tracker's records: the best and the median of
--repeats calls, the parts of one more call with timings, and the observe launch sequence beside mvmc_body_observe's on the same
problems (device events around 20 launches each).
Prints one JSON object (the kernel-source sha of the library included)."""
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

GROUPS = ("arms", "legs", "face")
GUESSED = (7, 8, 9)


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def track(seqs):
    from multiview_motion_capture_amd.sequences import track_sequences
    refused = []
    for chain_len in (16, 8, 4):           # (the stitch may refuse contaminated chains: too many identities in one of them)
        try:
            return track_sequences(seqs, chain_len=chain_len), chain_len
        except RuntimeError as e:
            refused.append(f"chain_len {chain_len}: {e}")
            log(f"tracker refused {refused[-1]}")
    raise RuntimeError("; ".join(refused))


def person_of(t, g):
    J = np.array([q[2].keypoints for q in t.poses])
    e = np.linalg.norm(J[:, None] - g["gt_joints"][np.array(t.frame_idxs)], axis=-1).mean(-1)
    p = int(e.mean(0).argmin())
    return p, J, e[:, p]


def mpjpe(recs, gts, min_len=10):
    err = [person_of(t, g)[2] for r, g in zip(recs, gts) for t in r if len(t) >= min_len]
    return float(1e3 * np.mean(np.concatenate(err))), int(sum(len(e) for e in err))


def length_error(fitted, gts, seeds, min_len=60):
    from multiview_motion_capture_amd.device import skeleton_arrays
    side = skeleton_arrays()[1]
    keep = [s for s in range(11) if s not in GUESSED]
    err = []
    for r, g, seed in zip(fitted, gts, seeds):
        true = side * np.random.default_rng([seed, 4]).uniform(0.9, 1.1, size=(g["gt_joints"].shape[1], 1)) * np.ones((1, 11))
        err += [np.abs(t.bone_lens - true[person_of(t, g)[0]])[keep] for t in r if len(t) >= min_len]
    return {"fit_length_error_mm": float(1e3 * np.mean(err)) if err else None, "fit_records_of_60_frames": len(err)}


def smoother_numbers(seqs, fitted, gts, loss):
    from test_gpu_smooth import _cut

    from multiview_motion_capture_amd.smoothing import smooth_sequences
    rng = np.random.default_rng(9)
    out = smooth_sequences(seqs, [_cut(r, rng) for r in fitted], loss=loss)
    e_data, e_fill, jit = [], [], []
    for r, g in zip(out, gts):
        for t in r:
            if len(t) < 10:
                continue
            _, J, err = person_of(t, g)
            fl = t.smooth_filled
            e_data.append(err[~fl & (t.smooth_views > 0)])
            e_fill.append(err[fl])
            ok = ~fl
            jit.append(np.linalg.norm(J[2:] - 2 * J[1:-1] + J[:-2], axis=-1).mean(-1)[ok[2:] & ok[1:-1] & ok[:-2]])
    mm = lambda x: float(1e3 * np.concatenate(x).mean()) if x and np.concatenate(x).size else None
    return {"data_mpjpe_mm": mm(e_data), "filled_mpjpe_mm": mm(e_fill), "filled_frames": int(sum(e.size for e in e_fill)),
            "jitter_mm": mm(jit)}


def score(reports, truths):
    res = {}
    tp_all = fl_all = tr_all = 0
    for b, name in enumerate(GROUPS):
        tp = sum(int(np.count_nonzero(r["flags"] & t & (1 << b))) for r, t in zip(reports, truths))
        fl = sum(int(np.count_nonzero(r["flags"] & (1 << b))) for r in reports)
        tr = sum(int(np.count_nonzero(t & (1 << b))) for t in truths)
        res[name] = {"exchanged": tr, "flagged": fl, "correct": tp, "precision": tp / fl if fl else None, "recall": tp / tr if tr else None}
        tp_all, fl_all, tr_all = tp_all + tp, fl_all + fl, tr_all + tr
    res["all"] = {"exchanged": tr_all, "flagged": fl_all, "correct": tp_all, "precision": tp_all / max(fl_all, 1), "recall": tp_all / max(tr_all, 1)}
    res["selected_detections"] = sum(int((r["record"] >= 0).sum()) for r in reports)
    return res


def accuracy(frames, moved):
    """moved False: the scenes carry the exchanges alone (what the repair is for); True: the robust probe's whole contamination."""
    import exchange_cases as ec
    from smooth_robust_probe import contaminate
    from test_gpu_smooth import _synth

    from multiview_motion_capture_amd import exchanges
    from multiview_motion_capture_amd.body_fit import fit_sequences
    from multiview_motion_capture_amd.smoothing import smooth_sequences
    seeds = (71, 72, 73)
    clean, gts = _synth(seeds=seeds, n_frames=frames)
    dirty = [((contaminate(s[0], 900 + i) if moved else ec.draw_exchanges(s[0], 900 + i)[0]), s[1], s[2]) for i, s in enumerate(clean)]
    truths = []
    for i, g in enumerate(gts):
        drawn = ec.draw_exchanges(g["kps25"], 900 + i)[1]              # contaminate()'s first draws
        P = g["kps25"].shape[2]
        present = (np.arange(P)[None, None, :] < g["counts"][:, :, None]) & (g["gt_order"] >= 0)
        truths.append(np.where(present, drawn, 0).astype(np.uint8))
    res = {"seeds": list(seeds), "frames": frames, "detections": int(sum(int(g["counts"].sum()) for g in gts)),
           "contamination": "exchanges and moved keypoints" if moved else "exchanges only"}
    first, chain_len = track(dirty)        # the door: the real tracker, at the longest chain its stitch takes
    res["door_chain_len"] = chain_len
    fitted = fit_sequences(dirty, first)
    smoothed = smooth_sequences(dirty, fitted, loss="cauchy")
    res["sources"] = {}
    repaired = None
    for name, recs in (("tracker", first), ("fit", fitted), ("cauchy_smoother", smoothed)):
        repaired, reports = exchanges.repair_sequences(dirty, recs)
        res["sources"][name] = score(reports, truths)
        log(f"records of the {name}: {json.dumps(res['sources'][name]['all'])}")
    res["sweep"] = []
    for margin in (2.0, 4.0, 8.0):
        for ratio in (0.5, 0.7, 0.9):
            sc = score(exchanges.repair_sequences(dirty, smoothed, margin_px=margin, ratio=ratio)[1], truths)["all"]
            res["sweep"].append({"margin_px": margin, "ratio": ratio, "precision": sc["precision"], "recall": sc["recall"],
                                 "flagged": sc["flagged"]})
            log(f"margin_px {margin}, ratio {ratio}: precision {sc['precision']:.4f}, recall {sc['recall']:.4f}")
    res["downstream"] = {}
    second = None
    for name, seqs in (("clean", clean), ("contaminated", dirty), ("repaired", repaired), ("repaired_twice", None)):
        if name == "repaired_twice":       # the loop once more: the CONTAMINATED keypoints repaired against the records of the repaired ones
            if second is None:
                continue
            seqs, reports = exchanges.repair_sequences(dirty, second)
            res["sources"]["cauchy_smoother_second_round"] = score(reports, truths)
            log(f"second round: {json.dumps(res['sources']['cauchy_smoother_second_round']['all'])}")
        try:
            recs, cl = (first, chain_len) if name == "contaminated" else track(seqs)
        except RuntimeError as e:
            res["downstream"][name] = {"tracker_refused": str(e)}
            continue
        fit = fitted if name == "contaminated" else fit_sequences(seqs, recs)
        if name == "repaired":
            second = smooth_sequences(seqs, fit, loss="cauchy")
        err, n = mpjpe(recs, gts)
        row = {"chain_len": cl, "tracker_mpjpe_mm": err, "tracker_poses": n, "records": sum(len(r) for r in recs)}
        row.update(length_error(fit, gts, seeds))
        for loss in (None, "cauchy"):
            row[f"smooth_{loss}"] = smoother_numbers(seqs, fit, gts, loss)
        res["downstream"][name] = row
        log(f"{name}: {json.dumps(row)}")
    return res


def cost(sizes, frames, repeats):
    import torch
    from body_fit_probe import make

    from multiview_motion_capture_amd import device as dev, exchanges
    from multiview_motion_capture_amd.sequences import check_records, plan_groups, select_views, stack_group, track_sequences
    seqs_all = make(max(sizes), frames)
    recs_all = track_sequences(seqs_all)
    d = torch.device("cuda:0")
    T = dev.uploader(d)
    res = {}
    for S in sizes:
        seqs, recs = seqs_all[:S], recs_all[:S]
        exchanges.repair_sequences(seqs, recs)
        torch.cuda.synchronize()
        times = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            exchanges.repair_sequences(seqs, recs)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        split = {}
        exchanges.repair_sequences(seqs, recs, timings=split)
        # the observe launches beside mvmc_body_observe's on the same problems
        shapes, arrs = check_records(seqs, recs, "probe")
        lay, = plan_groups(shapes, 1)
        sel = select_views(stack_group(lay, seqs), arrs, d, exchanges.MAX_DIST, exchanges.MIN_SCORE)
        args = (sel.k17, sel.c17, sel.Pm_d, T(sel.frame_of), sel.rig_d, T(sel.joints), T(sel.order), T(sel.lo), T(sel.hi), T(sel.rank))
        launch = {}
        for name, fn in (("body_observe", lambda: dev.body_observe(*args, exchanges.MAX_DIST, exchanges.MIN_SCORE)),
                         ("exchange_observe", lambda: dev.exchange_observe(*args, exchanges.MAX_DIST, exchanges.MIN_SCORE))):
            fn()
            torch.cuda.synchronize()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            for _ in range(20):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            launch[name + "_us"] = 1e3 * ev[0].elapsed_time(ev[1]) / 20
        launch["ratio"] = launch["exchange_observe_us"] / launch["body_observe_us"]
        a = np.array(times)
        res[str(S)] = {"problems": int(sel.frame_of.shape[0]), "keypoint_bytes": int(sum(np.asarray(s[0]).nbytes for s in seqs)),
                       "best_s": float(a.min()), "median_s": float(np.median(a)), "split_ms": {k: 1e3 * v for k, v in split.items()},
                       "observe_launch": launch}
        log(f"S={S}: {json.dumps(res[str(S)])}")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--cost-frames", type=int, default=150)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from multiview_motion_capture_amd import _cabi, exchanges
    res = {"build": _cabi.build_info(), "margin_px": exchanges.MARGIN_PX, "ratio": exchanges.RATIO}
    for part, run in (("accuracy_exchanges", lambda: accuracy(args.frames, False)),
                      ("accuracy_exchanges_and_moved", lambda: accuracy(args.frames, True)), ("cost", lambda: cost(args.sizes, args.cost_frames, args.repeats))):
        res[part] = run()
        if args.out:                      # (after every part: a run cut short leaves what it measured)
            with open(args.out, "w") as f:
                f.write(json.dumps(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    main()
