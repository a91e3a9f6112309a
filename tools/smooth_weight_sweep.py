"""The sweep that chose smoothing.py's default prior weights:
    python tools/smooth_weight_sweep.py [--out FILE]
Two synthetic scene walks (300 frames, 5 cameras, 4 people, occlusion 0.3), records from track_sequences -> fit_sequences with one
10-20-frame hole cut out of every other long record (tests/test_gpu_smooth.py's setup); per (velocity, acceleration) weight pair -- the
same on root (px^2/m^2) and angles (px^2/rad^2) -- the ground-truth MPJPE of the smoothed joints on the filled frames and on the frames
with data, and the joints' mean second difference.  Prints one JSON object."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vel", type=float, nargs="+", default=[0.0, 1e3, 1e4, 1e5])
    ap.add_argument("--acc", type=float, nargs="+", default=[0.0, 1e3, 1e4, 1e5])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from multiview_motion_capture_amd import _cabi
    from multiview_motion_capture_amd.body_fit import fit_sequences
    from multiview_motion_capture_amd.sequences import track_sequences
    from multiview_motion_capture_amd.smoothing import smooth_sequences
    from test_gpu_body_fit import _raw_slot_maps
    from test_gpu_smooth import _cut, _person, _synth
    seqs, gts = _synth(seeds=(51, 52), rigs=((5, 4), (5, 4)), n_frames=300)
    fitted = fit_sequences(seqs, track_sequences(seqs, chain_len=16))
    rng = np.random.default_rng(7)
    cut = [_cut(r, rng) for r in fitted]
    maps = [_raw_slot_maps(g) for g in gts]
    people = [[_person(t, g, mp, t.fit_select) if len(t) >= 60 else -1 for t in r] for r, g, mp in zip(fitted, gts, maps)]
    rows = []
    for v in args.vel:
        for a in args.acc:
            if v + a <= 0:
                continue
            out = smooth_sequences(seqs, cut, root_vel=v, root_acc=a, ang_vel=v, ang_acc=a)
            ef, ed, jt = [], [], []
            for s, g in enumerate(gts):
                for t, p in zip(out[s], people[s]):
                    if p < 0:
                        continue
                    fr = np.array(t.frame_idxs)
                    J = np.array([q[2].keypoints for q in t.poses])
                    err = np.linalg.norm(J - g["gt_joints"][fr, p], axis=-1).mean(-1)
                    ef.append(err[t.smooth_filled])
                    ed.append(err[~t.smooth_filled & (t.smooth_views > 0)])
                    jt.append(np.linalg.norm(J[2:] - 2 * J[1:-1] + J[:-2], axis=-1).mean(-1))
            row = dict(vel=v, acc=a, mpjpe_filled=float(np.mean(np.concatenate(ef))), mpjpe_data=float(np.mean(np.concatenate(ed))),
                       jitter=float(np.mean(np.concatenate(jt))))
            rows.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    text = json.dumps({"build": _cabi.build_info(), "rows": rows})
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
