"""What the floor under the smoother's foot contacts (smoothing.smooth_sequences(contacts=..., floor=...)) buys and costs on the device:
    python tools/smooth_floor_probe.py [--scenes 3] [--frames 300] [--repeats 3] [--out profiles/smooth_floor_probe.json]
Scenes: tools/smooth_contact_probe.py's -- synth.generate(walk="planted"), 5 views x 3 people, seeds 81, 82, ..., through
track_sequences -> fit_sequences -> smooth_sequences, a 10-20-frame hole cut out of every other long record -- on the floor-bound walk
(floor_normal ~ (0.1, -0.05, 1)): every person's footholds lie on one plane with that normal.  "walk" reports, per scene, the largest
tilt of the construction and the ratio of the tilted root's largest second difference to the plain walk's (a ratio near 2 or above is
a person the tilt has made jerky: say so when quoting the figures).
Accuracy, with the generator's labels and with "auto": the planted ankles' height along the TRUE normal -- its std per identity and
its rms about the identity's true level, mm, averaged over the identities --, skate, MPJPE on the frames with data and jitter
(smooth_contact_probe.measure), for contacts only, for floor = the true normal at floor_weight in {1, 10, 100} x contact_weight, and
for floor = estimate_floor's normal (from the contacts-only records; its angle to the truth, status, spread and rms are reported).
Cost: the contacts-only call and the floor call (true labels, floor_weight = contact_weight) alternating in one session, --repeats timed
calls each after one untimed call of each: the best and the median call, and the parts of one more call with timings.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import smooth_contact_probe as cp  # noqa: E402

FEET = cp.FEET
NORMAL = np.array([0.1, -0.05, 1.0]) / np.linalg.norm([0.1, -0.05, 1.0])
FLOOR_WEIGHTS = (1.0, 10.0, 100.0)        # x contact_weight


def _records_from_truth(g, seed):
    """smooth_contact_probe._records_from_truth on the floor-bound walk (the tracker refused the scene)."""
    from test_body_fit_cpu import _Rec

    from multiview_motion_capture_amd import synth

    class Rec(_Rec):
        def __len__(self):
            return len(self.frame_idxs)
    rng = np.random.default_rng([seed, 12])
    F, P = g["gt_joints"].shape[:2]
    lens = synth.skeleton_arrays()[1] * np.random.default_rng([seed, 4]).uniform(0.9, 1.1, size=(P, 1)) * np.ones((P, 11))
    root, ang, _ = synth.planted_walk(F, P, seed, side_lens=lens, floor_normal=NORMAL)
    out = []
    for p in range(P):
        par = np.concatenate([root[:, p], ang[:, p].reshape(F, 54), np.tile(lens[p], (F, 1))], axis=1)
        par[:, :57] += rng.normal(0, 0.01, (F, 57))
        J = synth.batched_fk(par[:, :3], par[:, 3:57].reshape(F, 18, 3), par[:, 57:])
        out.append(Rec(list(range(F)), par, J, tid=p))
    return out


def walk_report(seed, frames):
    """The construction's largest tilt (degrees) and second-difference ratios against the plain walk, per person."""
    from multiview_motion_capture_amd import synth
    lens = synth.skeleton_arrays()[1] * np.random.default_rng([seed, 4]).uniform(0.9, 1.1, size=(3, 1)) * np.ones((3, 11))
    r1, a1, _ = synth.planted_walk(frames, 3, seed, side_lens=lens, floor_normal=NORMAL)
    r0, a0, _ = synth.planted_walk(frames, 3, seed, side_lens=lens)
    R = lambda a: synth._rot(0, a[..., 0]) @ synth._rot(1, a[..., 1]) @ synth._rot(2, a[..., 2])
    Q = R(a1[:, :, 0]) @ np.swapaxes(R(a0[:, :, 0]), -1, -2)
    tilt = np.degrees(np.arccos(np.clip((np.trace(Q, axis1=-2, axis2=-1) - 1.0) / 2.0, -1.0, 1.0))).max(0)
    dd = lambda v: np.abs(np.diff(v, 2, axis=0)).reshape(frames - 2, 3, -1).max((0, 2))
    return {"tilt_deg_max": tilt.tolist(), "angle_dd_ratio": (dd(a1[:, :, 0]) / dd(a0[:, :, 0])).tolist(),
            "root_dd_ratio": (dd(r1) / dd(r0)).tolist()}


def scenes(n, frames):
    """smooth_contact_probe.scenes with floor_normal: -> seqs, gts, records (holes cut), door and walk report per scene."""
    from test_gpu_smooth import _calibs, _cut

    from multiview_motion_capture_amd import synth
    from multiview_motion_capture_amd.body_fit import fit_sequences
    from multiview_motion_capture_amd.sequences import track_sequences
    seqs, gts, recs, doors, walks = [], [], [], [], []
    rng = np.random.default_rng(11)
    for s in range(n):
        g = synth.generate(frames, 5, 3, 81 + s, walk="planted", floor_normal=NORMAL)
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
        walks.append(walk_report(81 + s, frames))
    return seqs, gts, recs, doors, walks


def heights(out, recs, gts):
    """Per identity (smooth_contact_probe.measure's filter) the planted ankles' height along the true normal: std and rms about the
    true level (the generator's planted ankles of the matched person), mm, averaged over the identities."""
    std, rms = [], []
    for r_out, r_in, g in zip(out, recs, gts):
        for t, t_in in zip(r_out, r_in):
            if len(t_in) < 60 or len(t) < 2:
                continue
            p, dist = cp._match(t_in, g)
            if dist > 0.3:
                continue
            fr = np.array(t.frame_idxs)
            J = np.array([q[2].keypoints for q in t.poses])
            lab = g["gt_contact"][fr, p]
            h = (J[:, FEET] @ NORMAL)[lab]
            level = float((g["gt_joints"][:, p][:, FEET] @ NORMAL)[g["gt_contact"][:, p]].mean())
            std.append(h.std())
            rms.append(np.sqrt(np.mean((h - level) ** 2)))
    return {"height_std_mm": float(1e3 * np.mean(std)), "height_rms_mm": float(1e3 * np.mean(rms))}


def accuracy(seqs, gts, recs):
    from multiview_motion_capture_amd.smoothing import CONTACT_WEIGHT, estimate_floor, smooth_sequences
    truth = cp.true_labels(recs, gts)
    res, outs = {}, {}

    def run(name, **kw):
        outs[name] = smooth_sequences(seqs, recs, **kw)
        res[name] = dict(cp.measure(outs[name], recs, gts), **heights(outs[name], recs, gts))
        print(f"{name}: {json.dumps(res[name])}", file=sys.stderr, flush=True)
    for lab_name, lab in (("true", truth), ("auto", "auto")):
        run(f"{lab_name}, contacts only", contacts=lab)
        for m in FLOOR_WEIGHTS:
            run(f"{lab_name}, floor true normal, floor_weight {m:g} x", contacts=lab, floor=NORMAL, floor_weight=m * CONTACT_WEIGHT)
        est = estimate_floor(outs[f"{lab_name}, contacts only"])
        res[f"{lab_name}, estimate_floor"] = [
            {"angle_deg": float(np.degrees(np.arctan2(np.linalg.norm(np.cross(e["normal"], NORMAL)), e["normal"] @ NORMAL))),
             "status": int(e["status"]), "spread_m": np.asarray(e["spread"]).tolist(), "rms_mm": 1e3 * float(e["rms"]),
             "n_runs": int(e["n_runs"])} for e in est]
        print(f"{lab_name}, estimate_floor: {json.dumps(res[f'{lab_name}, estimate_floor'])}", file=sys.stderr, flush=True)
        run(f"{lab_name}, floor estimated normal", contacts=lab, floor=[e["normal"] if e["status"] == 0 else None for e in est])
    return res


def cost(seqs, gts, recs, repeats):
    import torch

    from multiview_motion_capture_amd import smoothing
    truth = cp.true_labels(recs, gts)
    kinds = {"contacts": {"contacts": truth}, "floor": {"contacts": truth, "floor": NORMAL}}
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
    row = {"tracklet_frames": int(sum(t.frame_idxs[-1] - t.frame_idxs[0] + 1 for r in recs for t in r)),
           "identities": sum(len(r) for r in recs)}
    for k, kw in kinds.items():
        split = {}
        smoothing.smooth_sequences(seqs, recs, timings=split, **kw)
        a = np.array(times[k])
        row[k] = {"best_s": float(a.min()), "median_s": float(np.median(a)), "over_contacts_best": float(a.min() / np.min(times["contacts"])),
                  "split_ms": {n: 1e3 * v for n, v in split.items()}}
        print(f"{k}: best {a.min():.3f} s, median {np.median(a):.3f} s", file=sys.stderr, flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=3)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from multiview_motion_capture_amd import _cabi, smoothing
    res = {"build": _cabi.build_info(), "normal": NORMAL.tolist(), "frames": args.frames, "seeds": [81 + s for s in range(args.scenes)],
           "defaults": {"contact_weight": smoothing.CONTACT_WEIGHT, "floor_weight": "contact_weight"}}
    seqs, gts, recs, doors, walks = scenes(args.scenes, args.frames)
    res["door"], res["walk"] = doors, walks
    print(f"doors: {doors}\nwalks: {json.dumps(walks)}", file=sys.stderr, flush=True)
    res["accuracy"] = accuracy(seqs, gts, recs)
    res["cost"] = cost(seqs, gts, recs, args.repeats)
    text = json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
