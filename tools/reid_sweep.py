"""The sweep behind the defaults of relinking.reidentify_sequences:
    python tools/reid_sweep.py [--out FILE]
Three kinds of input, all held out from the tests:
  tracked  scene walks with ground truth (300 frames, 5 cameras x 4 people, seeds 202806xx; half with occlusion 0.3) in which two people
           are hidden in every view for 30 - 80 frames (tests/reid_cases.py: hide_people), through track_sequences(relink=True); every
           record end labelled with the ground-truth person nearest to its pose (within 0.2 m);
  cut      ground-truth scene walks of 400 frames at (5, 4) and (8, 8), seeds 20280601 .. 20280604, every person cut twice with holes
           of 20 - 80 frames, N(0, sigma) on every joint, sigma = 1 cm and 2 cm (tests/reid_cases.py: long_hole_fragments);
  shelf    the noise-free oracle tracker's Shelf records (tests/relink_cases.py: shelf_oracle_records); they have no labels, so only
           the links taken are reported.
A TRUE link joins a record to the next record (by first frame) of the person at its end.  Per (max_z, ratio, floor, min_poses) on the
device: links taken, WRONG links (both ends labelled, two different people), true links found, links with an unlabelled end.  The
records are packed once and uploaded per setting.
SELECTED: the setting with no wrong link on any input that finds the most true links; ties go to the smaller max_z, then the larger
floor, then the ratio and min_poses nearest to 0.7 and 10.  Prints one JSON object."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

TRACKED_SEEDS = (20280611, 20280612, 20280613, 20280614, 20280615, 20280616, 20280617, 20280618)
CUT_SEEDS = (20280601, 20280602, 20280603, 20280604)


def true_links(ends):
    """ends: per record (first frame, last frame, person at the start, person at the end) -> {(a, b)}."""
    out = set()
    for a, (_, la, _, pa) in enumerate(ends):
        if pa < 0:
            continue
        nxt = [(fb, b) for b, (fb, _, pb, _) in enumerate(ends) if pb == pa and fb > la]
        if nxt:
            out.add((a, min(nxt)[1]))
    return out


def inputs():
    """name -> (tracklets per sequence, ends per sequence)."""
    from multiview_motion_capture_amd import synth
    from multiview_motion_capture_amd.common import Calib
    from multiview_motion_capture_amd.sequences import track_sequences
    from reid_cases import hide_people, long_hole_fragments, scene_gt
    from relink_cases import label_poses, make_tracklets, shelf_oracle_records
    sets = {}
    gts = []
    for k, s in enumerate(TRACKED_SEEDS):
        rng = np.random.default_rng([s, 80])
        g = synth.generate(300, 5, 4, s, walk="scene", occlusion=0.3 if k % 2 else 0.0)
        who = rng.choice(4, size=2, replace=False)
        hidden = [(int(who[0]), int(rng.integers(40, 110)), int(rng.integers(30, 81))),
                  (int(who[1]), int(rng.integers(150, 210)), int(rng.integers(30, 81)))]
        gts.append(dict(hide_people(g, hidden), hidden=hidden))
    seqs = [(g["kps25"], g["counts"], [Calib.from_k_rt(g["K"][c], g["Rt"][c]) for c in range(5)]) for g in gts]
    tls, ends_all = track_sequences(seqs, relink=True), []
    for g, tl in zip(gts, tls):
        ends = []
        for t in tl:
            lab = label_poses(t.frame_idxs, np.array([p[2].keypoints for p in t.poses]), g["gt_joints"])
            ends.append((t.frame_idxs[0], t.frame_idxs[-1], int(lab[0]), int(lab[-1])))
        ends_all.append(ends)
    sets["tracked"] = (tls, ends_all)
    for sigma in (0.01, 0.02):
        for C, P in ((5, 4), (8, 8)):
            tls, ends_all = [], []
            for s in CUT_SEEDS:
                pieces = long_hole_fragments(scene_gt(C, P, s), s, sigma)
                tls.append(make_tracklets([(i, f, j) for i, (_, f, j) in enumerate(pieces)]))
                ends_all.append([(int(f[0]), int(f[-1]), p, p) for p, f, _ in pieces])
            sets[f"cut_{C}x{P}_{sigma}"] = (tls, ends_all)
    shelf = shelf_oracle_records()
    sets["shelf"] = ([make_tracklets(shelf)], [[(int(f[0]), int(f[-1]), -1, -1) for _, f, _ in shelf]])
    return sets, [g["hidden"] for g in gts]


def count(ends_all, links):
    taken = wrong = found = unl = true = 0
    for ends, ln in zip(ends_all, links):
        o = ln["order"]
        got = {(int(o[a]), int(o[b])) for a, b in enumerate(ln["succ"]) if b >= 0}
        tr = true_links(ends)
        taken += len(got)
        unl += sum(ends[a][3] < 0 or ends[b][2] < 0 for a, b in got)
        wrong += sum(ends[a][3] >= 0 and ends[b][2] >= 0 and ends[a][3] != ends[b][2] for a, b in got)
        found += len(tr & got)
        true += len(tr)
    return dict(links=taken, wrong=wrong, found=found, true=true, unlabelled=unl)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-z", type=float, nargs="+", default=[1.5, 2.0, 3.0, 4.0])
    ap.add_argument("--ratio", type=float, nargs="+", default=[0.5, 0.7, 0.9])
    ap.add_argument("--floor", type=float, nargs="+", default=[0.001, 0.002, 0.004, 0.008])
    ap.add_argument("--min-poses", type=int, nargs="+", default=[5, 10, 20])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from multiview_motion_capture_amd import _cabi, relinking
    sets, hidden = inputs()
    names = list(sets)
    flat = [tl for n in names for tl in sets[n][0]]
    packed = relinking.pack_reid(flat)
    rows = []
    for mp in args.min_poses:
        for mz in args.max_z:
            for ratio in args.ratio:
                for floor in args.floor:
                    solved = relinking.solve_reid(packed, mz, ratio, floor, mp, relinking.REACH, relinking.REID_SPEED)
                    links = [dict(r, order=o) for o, r in zip(packed["order"], solved)]
                    row, k = dict(max_z=mz, ratio=ratio, floor=floor, min_poses=mp), 0
                    for n in names:
                        row[n] = count(sets[n][1], links[k:k + len(sets[n][0])])
                        k += len(sets[n][0])
                    row["wrong"] = sum(row[n]["wrong"] for n in names)
                    row["found"] = sum(row[n]["found"] for n in names)
                    rows.append(row)
                    print(json.dumps(row), file=sys.stderr, flush=True)
    clean = [r for r in rows if r["wrong"] == 0]
    best = min(clean, key=lambda r: (-r["found"], r["max_z"], -r["floor"], abs(r["ratio"] - 0.7), abs(r["min_poses"] - 10))) if clean else None
    par = dict(max_z=relinking.MAX_Z, ratio=relinking.RATIO, floor=relinking.FLOOR, min_poses=relinking.MIN_POSES)
    at = [r for r in rows if all(r[k] == v for k, v in par.items())]
    defaults = dict(par, reach=relinking.REACH, speed=relinking.REID_SPEED)
    if at:
        d = at[0]
        defaults.update(row=d, cut_recall_5x4={str(s): d[f"cut_5x4_{s}"]["found"] / d[f"cut_5x4_{s}"]["true"] for s in (0.01, 0.02)})
        # the links the defaults take on Shelf: (track id, last frame) -> (track id, first frame), z
        solved = relinking.solve_reid(packed, *[par[k] for k in ("max_z", "ratio", "floor", "min_poses")], relinking.REACH,
                                      relinking.REID_SPEED)
        tl, o, r = flat[-1], packed["order"][-1], solved[-1]
        defaults["shelf_links"] = [dict(a=int(tl[o[a]].track_id), a_last=int(tl[o[a]].frame_idxs[-1]), b=int(tl[o[b]].track_id),
                                        b_first=int(tl[o[b]].frame_idxs[0]), z=float(r["cost"][a])) for a, b in enumerate(r["succ"]) if b >= 0]
    text = json.dumps({"build": _cabi.build_info(), "tracked_seeds": TRACKED_SEEDS, "cut_seeds": CUT_SEEDS, "hidden": hidden,
                       "records": {n: sum(len(t) for t in sets[n][0]) for n in names}, "selected": best, "defaults": defaults,
                       "rows": rows})
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
