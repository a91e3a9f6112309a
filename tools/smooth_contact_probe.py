"""What the smoother's foot contacts (smoothing.smooth_sequences(contacts=...)) buy and cost on the device:
    python tools/smooth_contact_probe.py [--sizes 1 8] [--frames 300] [--repeats 3] [--out profiles/smooth_contact_probe.json]
Scenes: synth.generate(walk="planted"), 5 views x 3 people, seeds 81, 82, ... (one foot of every person planted on every frame, the
stance foot changing every 8 frames), through track_sequences -> fit_sequences -> smooth_sequences; a 10-20-frame hole is cut out of
every other long record (hole stream 11).  Where the tracker refuses a scene, "door" says so and the records are built from the ground
truth plus noise (0.01 m / rad on root and angles).  Every identity is matched to the generator's person nearest to it.
Accuracy (the first three scenes), with contacts None, "auto" and the generator's labels: skate (the mean ankle displacement per frame
over the ground-truth contact pairs, mm), MPJPE on the frames with data and on the filled frames, jitter (mean second difference of
the joints), and for "auto" the detection's precision and recall; then contact_weight over {1e5, 1e6, 1e7} and contact_speed over
{0.005, 0.01, 0.02}.
Cost: S scenes, the three kinds of call alternating in one session, --repeats timed calls each after one untimed call of each: the
best and the median call, and the parts of one more call with timings.
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

FEET = [3, 6]
WEIGHTS, SPEEDS = (1e5, 1e6, 1e7), (0.005, 0.01, 0.02)


def _records_from_truth(g, seed):
    """Records of the generator's people with 0.01 noise on root and angles (the tracker refused the scene)."""
    from test_body_fit_cpu import _Rec

    from multiview_motion_capture_amd import synth

    class Rec(_Rec):
        def __len__(self):
            return len(self.frame_idxs)
    rng = np.random.default_rng([seed, 12])
    F, P = g["gt_joints"].shape[:2]
    root, ang, _ = synth.planted_walk(F, P, seed)
    lens = synth.skeleton_arrays()[1] * np.random.default_rng([seed, 4]).uniform(0.9, 1.1, size=(P, 1)) * np.ones((P, 11))
    out = []
    for p in range(P):
        par = np.concatenate([root[:, p], ang[:, p].reshape(F, 54), np.tile(lens[p], (F, 1))], axis=1)
        par[:, :57] += rng.normal(0, 0.01, (F, 57))
        J = synth.batched_fk(par[:, :3], par[:, 3:57].reshape(F, 18, 3), par[:, 57:])
        out.append(Rec(list(range(F)), par, J, tid=p))
    return out


def scenes(n, frames):
    """-> seqs, gts, records (holes cut), door per scene."""
    from test_gpu_smooth import _calibs, _cut

    from multiview_motion_capture_amd import synth
    from multiview_motion_capture_amd.body_fit import fit_sequences
    from multiview_motion_capture_amd.sequences import track_sequences
    seqs, gts, recs, doors = [], [], [], []
    rng = np.random.default_rng(11)
    for s in range(n):
        g = synth.generate(frames, 5, 3, 81 + s, walk="planted")
        seq = (g["kps25"], g["counts"], _calibs(g["K"], g["Rt"]))
        try:
            r = fit_sequences([seq], track_sequences([seq], chain_len=16))[0]
            door = "tracker, chain_len 16"
        except RuntimeError as e:
            r = _records_from_truth(g, 81 + s)
            door = f"ground truth + noise (the tracker refused: {e})"
        seqs.append(seq)
        gts.append(g)
        recs.append(_cut(r, rng))
        doors.append(door)
    return seqs, gts, recs, doors


def _match(t, g):
    J = np.array([q[2].keypoints for q in t.poses])
    d = np.linalg.norm(J[:, None] - g["gt_joints"][np.array(t.frame_idxs)], axis=-1).mean((0, 2))
    return int(d.argmin()), float(d.min())


def true_labels(recs, gts):
    out = []
    for r, g in zip(recs, gts):
        row = []
        for t in r:
            if len(t) < 2:
                row.append(None)
                continue
            p, _ = _match(t, g)
            row.append(np.ascontiguousarray(g["gt_contact"][t.frame_idxs[0]:t.frame_idxs[-1] + 1, p]))
        out.append(row)
    return out


def measure(out, recs, gts):
    sk, e_data, e_fill, jit, tp, n_det, n_true, trials = [], [], [], [], 0, 0, 0, []
    for r_out, r_in, g in zip(out, recs, gts):
        for t, t_in in zip(r_out, r_in):
            if len(t_in) < 60 or len(t) < 2:
                continue
            p, dist = _match(t_in, g)
            if dist > 0.3:
                continue
            fr = np.array(t.frame_idxs)
            J = np.array([q[2].keypoints for q in t.poses])
            lab = g["gt_contact"][fr, p]
            d = np.linalg.norm(np.diff(J[:, FEET], axis=0), axis=-1)
            sk.append(d[lab[1:] & lab[:-1]])
            err = np.linalg.norm(J - g["gt_joints"][fr, p], axis=-1).mean(-1)
            fl = t.smooth_filled
            e_data.append(err[~fl & (t.smooth_views > 0)])
            e_fill.append(err[fl])
            jit.append(np.linalg.norm(J[2:] - 2 * J[1:-1] + J[:-2], axis=-1).mean(-1))
            trials.append(len(t.smooth_trials))
            if hasattr(t, "smooth_contact"):
                c = t.smooth_contact
                tp += int((c & lab).sum())
                n_det += int(c.sum())
                n_true += int(lab.sum())
    res = {"identities": len(trials), "skate_mm": float(1e3 * np.mean(np.concatenate(sk))),
           "data_mpjpe_mm": float(1e3 * np.mean(np.concatenate(e_data))), "filled_mpjpe_mm": float(1e3 * np.mean(np.concatenate(e_fill))),
           "filled_frames": int(np.concatenate(e_fill).size), "jitter_mm": float(1e3 * np.mean(np.concatenate(jit))),
           "trials_mean": float(np.mean(trials))}
    if n_true:
        res["label_precision"], res["label_recall"] = tp / max(n_det, 1), tp / n_true
    return res


def accuracy(seqs, gts, recs):
    from multiview_motion_capture_amd.smoothing import smooth_sequences
    truth = true_labels(recs, gts)
    res = {}

    def run(name, **kw):
        res[name] = measure(smooth_sequences(seqs, recs, **kw), recs, gts)
        print(f"{name}: {json.dumps(res[name])}", file=sys.stderr, flush=True)
    run("None")
    run("auto", contacts="auto")
    run("true", contacts=truth)
    for w in WEIGHTS:
        run(f"true, weight {w:g}", contacts=truth, contact_weight=w)
        for v in SPEEDS:
            run(f"auto, weight {w:g}, speed {v:g}", contacts="auto", contact_weight=w, contact_speed=v)
    run("true, 2 rounds", contacts=truth, contact_rounds=2)
    return res


def cost(seqs_all, gts_all, recs_all, sizes, repeats):
    import torch

    from multiview_motion_capture_amd import smoothing
    res = {}
    for S in sizes:
        seqs, recs = seqs_all[:S], recs_all[:S]
        kinds = {"None": {}, "auto": {"contacts": "auto"}, "true": {"contacts": true_labels(recs, gts_all[:S])}}
        n_tf = sum(t.frame_idxs[-1] - t.frame_idxs[0] + 1 for r in recs for t in r)
        times = {k: [] for k in kinds}
        for kw in kinds.values():
            smoothing.smooth_sequences(seqs, recs, **kw)
        torch.cuda.synchronize()
        for _ in range(repeats):
            for k, kw in kinds.items():                    # alternating, the same session
                t0 = time.perf_counter()
                smoothing.smooth_sequences(seqs, recs, **kw)
                torch.cuda.synchronize()
                times[k].append(time.perf_counter() - t0)
        row = {"tracklet_frames": n_tf, "identities": sum(len(r) for r in recs)}
        for k, kw in kinds.items():
            split = {}
            smoothing.smooth_sequences(seqs, recs, timings=split, **kw)
            a = np.array(times[k])
            row[k] = {"best_s": float(a.min()), "median_s": float(np.median(a)), "over_none_best": float(a.min() / np.min(times["None"])),
                      "split_ms": {n: 1e3 * v for n, v in split.items()}}
            print(f"S={S}, contacts {k}: best {a.min():.3f} s, median {np.median(a):.3f} s, split ms "
                  f"{json.dumps({n: round(1e3 * v, 2) for n, v in split.items()})}", file=sys.stderr, flush=True)
        res[str(S)] = row
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from multiview_motion_capture_amd import _cabi, smoothing
    res = {"build": _cabi.build_info(), "defaults": {"contact_weight": smoothing.CONTACT_WEIGHT, "contact_speed": smoothing.CONTACT_SPEED,
                                                     "contact_min_frames": smoothing.CONTACT_MIN_FRAMES},
           "weights": (smoothing.ROOT_VEL, smoothing.ROOT_ACC, smoothing.ANG_VEL, smoothing.ANG_ACC), "frames": args.frames}
    seqs, gts, recs, doors = scenes(max(max(args.sizes), 3), args.frames)
    res["door"] = doors
    print(f"doors: {doors}", file=sys.stderr, flush=True)
    res["accuracy"] = accuracy(seqs[:3], gts[:3], recs[:3])
    res["cost"] = cost(seqs, gts, recs, args.sizes, args.repeats)
    text = json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
