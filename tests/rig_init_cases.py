"""Inputs shared by the tests of the rig calibration (tests/test_rig_init_cpu.py, tests/test_gpu_rig_init.py): the walk of one person
through the volume, its contaminations, and the small cases of the kernel tests.

A person who only wanders 0.2 m around one spot is near-degenerate for the 8-point fit, so the walk is assembled from a scene of four
people: generate(F / 4, C, 4, seed, walk="scene"), its people concatenated through gt_order into ONE one-person sequence of F frames
whose "walker" visits four places of the 4 x 4 m area."""
import functools

import numpy as np

OP25_OF_COCO = [0, 16, 15, 18, 17, 5, 2, 6, 3, 7, 4, 12, 9, 13, 10, 14, 11]      # pose_def.py: OpenPose-25 row of each COCO-17 joint
COCO_LR = [(1, 2), (3, 4), (5, 6), (7, 8), (9, 10), (11, 12), (13, 14), (15, 16)]


def walk(F, C, seed, swaps=0.0, shifts=0.0, doubles=0.0, drop_views=(), cut=None):
    """-> dict(kps25 (F,C,2,25,3) f32, counts (F,C) i32, k17 (F,C,2,17,3) f64 the COCO-17 rows of kps25, K, Rt, gt (F,18,3)).
    swaps: share of (frame, view) detections with left and right joints exchanged; shifts: share moved as a whole by up to 150 px in
    each coordinate; doubles: share of (frame, view) with a second detection (counts == 2: the frame drops out for that view);
    drop_views: views that detect nothing at all (counts == 0); cut: keep only the first ``cut`` frames of the F."""
    from multiview_motion_capture_amd import synth
    n = F // 4
    g = synth.generate(n, C, 4, seed, walk="scene")
    kps = np.zeros((4 * n, C, 2, 25, 3), np.float32)
    order = g["gt_order"]
    for p in range(4):
        slot = np.argmax(order == p, axis=2)                                           # (n, C): where person p sits in each view
        kps[p * n:(p + 1) * n, :, 0] = np.take_along_axis(g["kps25"], slot[:, :, None, None, None], axis=2)[:, :, 0]
    gt = np.concatenate([g["gt_joints"][:, p] for p in range(4)], axis=0)
    counts = np.ones((4 * n, C), np.int32)
    rng = np.random.default_rng([seed, 77])
    r = rng.uniform(size=(3, 4 * n, C))
    for f, c in zip(*np.nonzero(r[0] < swaps)):
        for a, b in COCO_LR:
            ia, ib = OP25_OF_COCO[a], OP25_OF_COCO[b]
            kps[f, c, 0, [ia, ib]] = kps[f, c, 0, [ib, ia]]
    for f, c in zip(*np.nonzero(r[1] < shifts)):
        seen = kps[f, c, 0, :, 2] > 0
        kps[f, c, 0, seen, :2] += rng.uniform(-150.0, 150.0, size=2).astype(np.float32)
    for f, c in zip(*np.nonzero(r[2] < doubles)):
        kps[f, c, 1] = kps[f, c, 0]
        kps[f, c, 1, :, :2] += np.float32(40.0)
        counts[f, c] = 2
    for c in drop_views:
        kps[:, c] = 0.0
        counts[:, c] = 0
    if cut is not None:
        kps, counts, gt = kps[:cut], counts[:cut], gt[:cut]
    k17 = kps[:, :, :, OP25_OF_COCO, :].astype(np.float64)
    return dict(kps25=kps, counts=counts, k17=k17, K=np.asarray(g["K"], np.float64), Rt=np.asarray(g["Rt"], np.float64), gt=gt)


CONTAMINATED = dict(swaps=0.2, shifts=0.1)
# the whole-rig cases: 5 views x 120 frames, clean and contaminated
# (seed 57: the walker of the floor test -- generate()'s people lean by N(0, 0.3 rad); its four stand within 2 degrees of upright on average)
RIGS = {"upright_57": (dict(F=120, C=5, seed=57), {}), "clean_11": (dict(F=120, C=5, seed=11), {}), "clean_12": (dict(F=120, C=5, seed=12), {}),
        "dirty_11": (dict(F=120, C=5, seed=11, **CONTAMINATED), {}), "dirty_12": (dict(F=120, C=5, seed=12, **CONTAMINATED), {})}
# the kernel cases: (walk arguments, calibrate arguments); H = 32, m = 6
_K = dict(hypotheses=32, sample_frames=6, min_pair_inliers=30)
SMALL = {
    "c2_f24": (dict(F=24, C=2, seed=21), _K),                                      # one pair
    "c3_f65": (dict(F=68, C=3, seed=22, doubles=0.1, cut=65), _K),                 # three pairs, a second chunk of one frame, counts == 2
    "c4_f24": (dict(F=24, C=4, seed=24, swaps=0.2, shifts=0.1), _K),               # six pairs, contaminated; tree through (3, 1)
    "c3_f40_drop": (dict(F=40, C=3, seed=24, drop_views=(2,)), _K),                # a view with counts 0: two pairs without a frame
    "c2_f1": (dict(F=4, C=2, seed=25, cut=1), _K),                                 # one frame: few_frames
}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (walk dict, calibrate arguments); shared between the tests: read-only."""
    args, kw = {**RIGS, **SMALL}[name]
    return walk(**args), kw


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (rig_init_np.calibrate's result on the case, its detail dict).  Computed once; read-only."""
    import rig_init_np as ri
    w, kw = case(name)
    detail = {}
    out = ri.calibrate(w["k17"], w["counts"], w["K"], detail=detail, **kw)
    return out, detail
