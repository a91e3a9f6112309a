"""The sweep behind relinking.py's defaults:
    python tools/relink_sweep.py [--out FILE]
Synthetic scene walks with ground truth (300 frames, 5 cameras, 4 people, occlusion 0.3; seeds other than the tests'), records from
track_sequences, every pose labelled with the ground-truth person nearest to it (within 0.2 m).  A TRUE link joins a record to the next
record (by first frame) of the person at its end, when that record starts 1 .. 16 frames after it ends.  Per (near_dist, speed,
max_gap) on the device (relink_sequences): links taken, WRONG links (both ends labelled, two different people), MISSED links (true, not
taken), links with an unlabelled end, and records of >= 10 poses per person after re-linking (1.0 = one identity per person).  The
same counts on ground-truth tracks cut into pieces (tests/relink_cases.py: fragments, 8 cameras x 8 people, other seeds than the
tests').  Prints one JSON object."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

SEEDS = (20270801, 20270802, 20270803, 20270804, 20270805, 20270806)
CUT_SEEDS = (20270811, 20270812, 20270813, 20270814)


def true_links(ends, max_gap=16):
    """ends: per record (first frame, last frame, person at the start, person at the end) -> {(a, b)}."""
    out = set()
    for a, (_, la, _, pa) in enumerate(ends):
        if pa < 0:
            continue
        nxt = [(fb, b) for b, (fb, _, pb, _) in enumerate(ends) if pb == pa and fb > la]
        if nxt:
            fb, b = min(nxt)
            if fb - la <= max_gap:
                out.add((a, b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--near", type=float, nargs="+", default=[0.05, 0.10, 0.15, 0.25, 0.50])
    ap.add_argument("--speed", type=float, nargs="+", default=[0.0, 0.015, 0.03, 0.06])
    ap.add_argument("--gap", type=int, nargs="+", default=[8, 16, 32])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from multiview_motion_capture_amd import _cabi, parallel, synth
    from multiview_motion_capture_amd.common import Calib
    from multiview_motion_capture_amd.relinking import relink_sequences
    from multiview_motion_capture_amd.sequences import track_sequences
    from relink_cases import fragments, label_poses, make_tracklets
    gts = [synth.generate(300, 5, 4, s, walk="scene", occlusion=0.3) for s in SEEDS]
    seqs = [(g["kps25"], g["counts"], [Calib.from_k_rt(g["K"][c], g["Rt"][c]) for c in range(5)]) for g in gts]
    sets = {"tracked": ([], [], []), "cut": ([], [], [])}
    for g, tl in zip(gts, track_sequences(seqs)):
        ends = []
        for t in tl:
            lab = label_poses(t.frame_idxs, np.array([p[2].keypoints for p in t.poses]), g["gt_joints"])
            ends.append((t.frame_idxs[0], t.frame_idxs[-1], int(lab[0]), int(lab[-1])))
        sets["tracked"][0].append(tl); sets["tracked"][1].append(ends); sets["tracked"][2].append(4)
    for s in CUT_SEEDS:
        pieces = fragments(synth.generate(300, 8, 8, s, walk="scene")["gt_joints"], s, 3, 16, 0.01)
        sets["cut"][0].append(make_tracklets([(i, f, j) for i, (_, f, j) in enumerate(pieces)]))
        sets["cut"][1].append([(int(f[0]), int(f[-1]), p, p) for p, f, _ in pieces]); sets["cut"][2].append(8)
    rows = []
    for near in args.near:
        for speed in args.speed:
            for gap in args.gap:
                row = dict(near_dist=near, speed=speed, max_gap=gap)
                for name, (tls, ends_all, people) in sets.items():
                    links = []
                    out = relink_sequences(tls, max_gap=gap, max_dist=parallel.MAX_DIST, near_dist=near, speed=speed, links=links)
                    taken = wrong = missed = unl = 0
                    for ends, ln in zip(ends_all, links):
                        o = ln["order"]
                        got = {(int(o[a]), int(o[b])) for a, b in enumerate(ln["succ"]) if b >= 0}
                        taken += len(got)
                        unl += sum(ends[a][3] < 0 or ends[b][2] < 0 for a, b in got)
                        wrong += sum(ends[a][3] >= 0 and ends[b][2] >= 0 and ends[a][3] != ends[b][2] for a, b in got)
                        missed += len(true_links(ends) - got)
                    row[name] = dict(links=taken, wrong=wrong, missed=missed, unlabelled=unl,
                                     records_of_10_poses_per_person=sum(len(t) >= 10 for r in out for t in r) / sum(people))
                rows.append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
    text = json.dumps({"build": _cabi.build_info(), "seeds": SEEDS, "cut_seeds": CUT_SEEDS,
                       "records_of_10_poses_per_person_before": {k: sum(len(t) >= 10 for r in v[0] for t in r) / sum(v[2])
                                                                 for k, v in sets.items()}, "rows": rows})
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
