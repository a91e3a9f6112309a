"""ctypes binding of the C ABI in include/mvmc.h (libmvmc_hip.so, gfx950).

The product path has no CPU fallback: if the HIP library is missing or a call
fails, this module raises.  Build the library with ``python -c "import
__graft_entry__ as g; g.build()"`` or ``make -C multiview_motion_capture_amd/csrc``.
"""
from __future__ import annotations

import ctypes as C
import os

_LIB_PATH = os.environ.get("MVMC_LIB_PATH") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib",
                                                           "libmvmc_hip.so")
_lib = None

MVMC_OK = 0
MVMC_ABI = 6    # MVMC_ABI_VERSION of include/mvmc.h that the argument types in load() describe
MVMC_F32, MVMC_F64 = 0, 1
N_PARAM = 68
MAX_NODES = 80
IK_SCRATCH_DOUBLES = 7680
IK_FD_WORK_DOUBLES = 40960
IK_STEP_OUT_DOUBLES = 240
BOUND_WORDS, ROW_WORDS = 56, 128
BODY_INFO_DOUBLES, BODY_WORK_DOUBLES = 16, 270
SMOOTH_K, SMOOTH_BLOCK_DOUBLES, SMOOTH_WORK_DOUBLES, SMOOTH_INFO_DOUBLES, SMOOTH_MAX_VIEWS = 39, 820, 3940, 32, 64
SMOOTH_COV_INFO_DOUBLES, SMOOTH_JOINTS = 8, 18
SMOOTH_WIN_MAX, SMOOTH_WIN_RING, SMOOTH_WIN_ITEM_INTS, SMOOTH_WIN_INFO_DOUBLES = 32, 66, 8, 16
SMOOTH_COV_ITEM_INTS = 4                                                                          # MVMC_SMOOTH_COV_ITEM_INTS
SMOOTH_LIVE_CONTACT_DOUBLES = 10                                                                  # MVMC_SMOOTH_LIVE_CONTACT_DOUBLES
LIVE_LEN_STATE_DOUBLES, LIVE_LEN_INFO_DOUBLES = 103, 17                                            # MVMC_LIVE_LEN_*
SMOOTH_LOSS_NONE, SMOOTH_LOSS_HUBER, SMOOTH_LOSS_CAUCHY = 0, 1, 2                                     # MVMC_SMOOTH_LOSS_*
SMOOTH_FOOT_L, SMOOTH_FOOT_R = 3, 6                                                                   # MVMC_SMOOTH_FOOT_*: the ankles
RELINK_MAX_RECORDS, RELINK_REC_DOUBLES = 512, 120
REID_MAX_POSES, REID_LDS_POSES = 65536, 512                                                            # MVMC_REID_*
RIG_TILE, RIG_MAX_CAMS, RIG_MAX_ITER, RIG_CAM_DOUBLES, RIG_INFO_DOUBLES = 64, 8, 24, 21, 64
LENS_DOUBLES, LENS_PINHOLE, LENS_BROWN, LENS_FISHEYE, LENS_MAX_ITER, LENS_FISHEYE_MAX_THETA = 16, 0, 1, 2, 12, 1.5
RIGINIT_NORM_DOUBLES, RIGINIT_POSE_DOUBLES, RIGINIT_MAX_ROUNDS, RIGINIT_MAX_SAMPLE = 8, 32, 8, 32
RIG_LOSS_NONE, RIG_LOSS_HUBER, RIG_LOSS_CAUCHY = 0, 1, 2                                              # MVMC_RIG_LOSS_*
RIG_STOP = {0: "running", 1: "xtol", 2: "ftol", 3: "few_cameras", 4: "few_points", 5: "max_iter"}    # MVMC_RIG_STOP_*

# every symbol declared in include/mvmc.h
SYMBOLS = (
    "mvmc_abi_version", "mvmc_status_string", "mvmc_als_seed_table", "mvmc_ingest", "mvmc_fmats",
    "mvmc_affinity", "mvmc_als_associate", "mvmc_closure_labels", "mvmc_cluster_members", "mvmc_dlt", "mvmc_triangulate_postopt", "mvmc_fk", "mvmc_ik_solve",
    "mvmc_fmats_from_projections", "mvmc_st_affinity", "mvmc_track_assign", "mvmc_track_commit", "mvmc_debug_eigh",
    "mvmc_debug_trstep", "mvmc_ik_solve_stages", "mvmc_chain_run", "mvmc_svt_associate", "mvmc_debug_ik_solve_fd", "mvmc_debug_ik_model_step", "mvmc_ingest_dlt", "mvmc_ingest_dlt_f32", "mvmc_pack_message_words", "mvmc_pack_work_words", "mvmc_stitch_work_words", "mvmc_pack_tracks", "mvmc_stitch_chains",
    "mvmc_chain_run_rigs", "mvmc_chain_run_sessions", "mvmc_body_observe", "mvmc_body_lengths", "mvmc_ik_solve_stages_rigs",
    "mvmc_smooth_blocks", "mvmc_smooth_step", "mvmc_smooth_cov", "mvmc_smooth_window_work_doubles", "mvmc_smooth_window", "mvmc_relink_work_words", "mvmc_relink",
    "mvmc_reid_work_words", "mvmc_reid_signature", "mvmc_reid_link",
    "mvmc_smooth_blocks_robust", "mvmc_smooth_obs_weights", "mvmc_smooth_window_robust",
    "mvmc_smooth_blocks_contact", "mvmc_smooth_contact_anchors",
    "mvmc_smooth_blocks_floor", "mvmc_smooth_floor_anchors",
    "mvmc_smooth_window_cov_work_doubles", "mvmc_smooth_window_cov",
    "mvmc_smooth_window_contact", "mvmc_smooth_window_cov_contact",
    "mvmc_live_lengths_apply", "mvmc_live_lengths_update",
    "mvmc_rig_part_doubles", "mvmc_rig_red_doubles", "mvmc_rig_start", "mvmc_rig_accumulate", "mvmc_rig_step",
    "mvmc_rig_accumulate_robust", "mvmc_rig_step_robust", "mvmc_rig_weights",
    "mvmc_rig_part_doubles_intr", "mvmc_rig_red_doubles_intr", "mvmc_rig_accumulate_intr", "mvmc_rig_step_intr",
    "mvmc_lens_undistort", "mvmc_lens_distort",
    "mvmc_pair_moments", "mvmc_pair_consensus", "mvmc_pair_refit",
    "mvmc_exchange_observe", "mvmc_exchange_apply",
    "mvmc_debug_st_affinity_wg", "mvmc_debug_track_wave",
)


class MvmcSkeleton(C.Structure):
    """mvmcSkeleton of include/mvmc.h."""
    _fields_ = [("bone_dirs", (C.c_double * 3) * 18), ("parents", C.c_int32 * 18),
                ("side_map", C.c_int32 * 18), ("n_side", C.c_int32), ("ref_side_lens", C.c_double * 18)]


class MvmcChainBuffers(C.Structure):
    """mvmcChainBuffers of include/mvmc.h (field order matters)."""
    _INTS = ("n_chains", "chain_len", "n_views", "p_max", "t_max", "k_max", "v_max", "max_nfev_cold", "max_nfev_warm",
             "n_inits", "seed_len", "n_parts", "force_big", "hand_over")
    _PTRS = ("kps17", "counts", "Pmats", "Fmats", "F2", "seed_table", "params", "joints", "meta", "n_tracks", "next_id",
             "n_dead", "slot_src", "S_sp", "W_st", "group_counts", "labels_sp", "labels_st", "n_clusters_sp", "n_clusters_st",
             "iters_sp", "iters_st", "members", "n_members", "cold", "init", "status", "n_new", "ik_params", "ik_joints", "ik_info",
             "ik_scratch", "out_params", "out_joints", "out_meta", "out_n_tracks", "out_info", "out_als_iters", "flags", "out_phase_cycles")
    _fields_ = [(n, C.c_int32) for n in _INTS] + [(n, C.c_void_p) for n in _PTRS]


class MvmcError(RuntimeError):
    pass


def lib_path() -> str:
    return _LIB_PATH


def build_info():
    """lib/BUILD_INFO.json of the shipped library (kernel-source hash, compiler, host, time), or None for an MVMC_LIB_PATH library."""
    if os.environ.get("MVMC_LIB_PATH"):
        return None
    from . import _buildinfo
    return _buildinfo.read()


def load():
    """Load libmvmc_hip.so (once) and declare the argument types."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise MvmcError(
            f"HIP extension not built: {_LIB_PATH} is missing. There is no CPU fallback; "
            "run __graft_entry__.build() (or make -C multiview_motion_capture_amd/csrc).")
    if not os.environ.get("MVMC_LIB_PATH"):
        # the shipped library must be a build of THIS tree's kernel sources (lib/BUILD_INFO.json, written by csrc/Makefile): a stale
        # .so -- built before an edit, or carried to the GPU box from another checkout -- would be measured and tested in place of the
        # code under review.  (A library named through MVMC_LIB_PATH is a deliberate A/B partner and is not checked.)
        from . import _buildinfo
        # (a deployment without the kernel sources beside the library has nothing to compare with: the check is for source trees)
        info, want = _buildinfo.read(), (_buildinfo.sources_sha() if os.path.isdir(_buildinfo.CSRC) else None)
        if want is not None and (info is None or info.get("kernel_sources_sha") != want):
            have = "no BUILD_INFO.json beside it" if info is None else f"built from kernel sources {info.get('kernel_sources_sha')}"
            raise MvmcError(f"{_LIB_PATH} is stale: {have}, the tree's are {want}.  Rebuild it: python -c \"import __graft_entry__ as g; "
                            "g.build()\" (or make -C multiview_motion_capture_amd/csrc)")
    lib = C.CDLL(_LIB_PATH)
    # The argument types declared below are those of ABI version MVMC_ABI: a library of another version (an old build loaded through
    # MVMC_LIB_PATH for an A/B run, a stale .so) would receive shifted pointers and ints -- device faults or silent garbage.  Refuse it.
    try:
        lib.mvmc_abi_version.restype = C.c_int
        have = int(lib.mvmc_abi_version())
    except AttributeError:
        have = -1
    if have != MVMC_ABI:
        raise MvmcError(f"{_LIB_PATH} has ABI version {have}, this package binds version {MVMC_ABI} (include/mvmc.h): rebuild it "
                        "(make -C multiview_motion_capture_amd/csrc) or load a build of the same ABI version")
    vp, i32, f64 = C.c_void_p, C.c_int, C.c_double
    SK = C.POINTER(MvmcSkeleton)
    argtypes = {
        "mvmc_status_string": [C.c_int],
        "mvmc_als_seed_table": [vp, i32],
        "mvmc_ingest": [vp, i32, i32, i32, i32, i32, vp, f64, i32, f64, vp, vp, vp],
        "mvmc_fmats": [vp, vp, i32, vp, vp],
        "mvmc_affinity": [vp, vp, vp, i32, i32, i32, vp, vp, vp],
        "mvmc_als_associate": [vp, i32, vp, i32, i32, i32, i32, vp, i32, vp, vp, vp, vp, vp, vp],
        "mvmc_closure_labels": [vp, vp, i32, i32, vp, vp, vp, vp],
        "mvmc_cluster_members": [vp, vp, i32, i32, i32, i32, i32, vp, vp, vp],
        "mvmc_dlt": [vp, vp, vp, i32, i32, i32, i32, i32, f64, vp, vp],
        "mvmc_ingest_dlt": [vp, i32, i32, i32, i32, i32, vp, f64, i32, f64, vp, vp, i32, i32, f64, vp, vp, vp],
        "mvmc_ingest_dlt_f32": [vp, i32, i32, i32, i32, vp, f64, i32, f64, vp, vp, i32, i32, f64, vp, vp, vp],
        "mvmc_triangulate_postopt": [vp, vp, vp, i32, i32, i32, i32, i32, vp, vp],
        "mvmc_fk": [SK, vp, i32, vp, vp, vp],
        "mvmc_ik_solve": [SK, vp, vp, vp, i32, i32, i32, i32, vp, vp, i32, i32, vp, vp, vp, vp, vp],
        "mvmc_fmats_from_projections": [vp, i32, vp, vp],
        "mvmc_st_affinity": [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, f64, vp, vp, vp, vp],
        "mvmc_track_assign": [vp] * 8 + [i32] * 6 + [vp] * 7,
        "mvmc_track_commit": [vp] * 4 + [i32] * 4 + [vp] * 9,
        "mvmc_debug_eigh": [vp, vp, i32, i32, vp, vp, vp, vp, vp],
        "mvmc_debug_st_affinity_wg": [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, f64, i32, i32, vp, vp, vp, vp],
        "mvmc_debug_track_wave": [i32] + [vp] * 8 + [i32] * 6 + [vp] * 8 + [i32] + [vp] * 7,
        "mvmc_debug_trstep": [vp, vp, i32, i32, i32, f64, f64, vp, vp, vp, vp],
        "mvmc_chain_run": [SK, C.POINTER(MvmcChainBuffers), vp],
        "mvmc_chain_run_rigs": [SK, C.POINTER(MvmcChainBuffers), vp, i32, vp],
        "mvmc_chain_run_sessions": [SK, C.POINTER(MvmcChainBuffers), vp, i32, vp, vp],
        "mvmc_ik_solve_stages": [SK, vp, vp, vp, vp, i32, i32, i32, i32, vp, i32, i32, vp, vp, vp, vp, vp],
        "mvmc_debug_ik_solve_fd": [SK, vp, vp, vp, i32, i32, i32, i32, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp],
        "mvmc_debug_ik_model_step": [SK, vp, vp, vp, i32, i32, i32, i32, vp, i32, vp, vp, vp, vp, vp],
        "mvmc_pack_message_words": [i32, i32, i32, i32],
        "mvmc_pack_work_words": [i32, i32, i32],
        "mvmc_stitch_work_words": [i32, i32, i32],
        "mvmc_pack_tracks": [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, f64, vp, i32, vp, vp, vp],
        "mvmc_stitch_chains": [vp, C.c_longlong, i32, i32, i32, i32, i32, f64, i32, vp, vp, vp, vp, vp],
        "mvmc_body_observe": [vp, vp, i32, i32, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp, i32, f64, f64, vp, vp, vp, vp, vp],
        "mvmc_body_lengths": [SK, vp, i32, i32, vp, vp, vp, vp, vp, i32, vp, vp, i32, i32, f64, f64, f64, vp, vp, vp],
        "mvmc_ik_solve_stages_rigs": [SK, vp, vp, i32, vp, vp, i32, i32, i32, i32, vp, i32, i32, vp, vp, vp, vp, vp],
        "mvmc_smooth_blocks": [SK, vp, i32, i32, vp, vp, vp, vp, vp, vp, i32, vp, vp],
        "mvmc_smooth_step": [SK, vp, vp, vp, vp, i32, i32, f64, f64, f64, f64, f64, f64, f64, i32, i32, vp, vp, vp, vp],
        "mvmc_smooth_cov": [SK, vp, vp, vp, i32, i32, f64, f64, f64, f64, f64, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp],
        "mvmc_smooth_window_work_doubles": [i32, i32],
        "mvmc_smooth_window": [SK, vp, i32, i32, vp, i32, vp, i32, vp, vp, i32, vp, vp, vp, i32, i32, i32, f64, f64, f64, f64, f64, f64,
                               f64, vp, vp, C.c_longlong, vp],
        "mvmc_smooth_blocks_robust": [SK, vp, i32, i32, vp, vp, vp, vp, vp, vp, i32, vp, i32, f64, vp],
        "mvmc_smooth_obs_weights": [SK, vp, i32, i32, vp, vp, vp, vp, i32, i32, f64, vp, vp],
        "mvmc_smooth_window_robust": [SK, vp, i32, i32, vp, i32, vp, i32, vp, vp, i32, vp, vp, vp, i32, i32, i32, f64, f64, f64, f64, f64,
                                      f64, f64, vp, vp, C.c_longlong, i32, f64, vp],
        "mvmc_smooth_blocks_contact": [SK, vp, i32, i32, vp, vp, vp, vp, vp, vp, i32, vp, i32, f64, vp, vp, f64, vp],
        "mvmc_smooth_contact_anchors": [vp, vp, i32, i32, i32, f64, i32, i32, C.POINTER(C.c_double), f64, vp, vp, vp, vp],
        "mvmc_smooth_blocks_floor": [SK, vp, i32, i32, vp, vp, vp, vp, vp, vp, i32, vp, i32, f64, vp, vp, f64, vp, f64, vp],
        "mvmc_smooth_floor_anchors": [vp, vp, i32, i32, vp, vp, vp, vp, vp, vp],
        "mvmc_smooth_window_cov_work_doubles": [i32, i32],
        "mvmc_smooth_window_cov": [SK, vp, i32, i32, vp, i32, vp, i32, vp, vp, vp, i32, i32, f64, f64, f64, f64, f64, i32, i32, f64, vp,
                                   C.c_longlong, vp, vp, vp, vp],
        "mvmc_smooth_window_contact": [SK, vp, i32, i32, vp, i32, vp, i32, vp, vp, i32, vp, vp, vp, i32, i32, i32, f64, f64, f64, f64, f64,
                                       f64, f64, vp, vp, C.c_longlong, i32, f64, vp, vp, i32, f64, f64, i32, i32, C.POINTER(C.c_double),
                                       f64, vp, vp],
        "mvmc_smooth_window_cov_contact": [SK, vp, i32, i32, vp, i32, vp, i32, vp, vp, vp, i32, i32, f64, f64, f64, f64, f64, i32, i32, f64,
                                           vp, C.c_longlong, vp, vp, vp, vp, vp, f64, vp],
        "mvmc_live_lengths_apply": [vp, i32, vp, i32, vp, i32, vp],
        "mvmc_live_lengths_update": [SK, vp, i32, i32, vp, i32, vp, i32, vp, vp, vp, i32, i32, f64, i32, vp, vp, vp],
        "mvmc_relink_work_words": [i32],
        "mvmc_relink": [vp, vp, vp, i32, i32, i32, f64, f64, f64, vp, vp, vp, vp, vp, vp, C.c_longlong, vp],
        "mvmc_reid_work_words": [i32],
        "mvmc_reid_signature": [vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, C.c_longlong, vp],
        "mvmc_reid_link": [vp, vp, vp, vp, i32, i32, i32, f64, f64, f64, f64, f64, vp, vp, vp, vp, vp, vp, C.c_longlong, vp],
        "mvmc_rig_part_doubles": [i32],
        "mvmc_rig_red_doubles": [i32],
        "mvmc_rig_start": [vp, vp, vp, i32, i32, i32, f64, vp, vp, vp],
        "mvmc_rig_accumulate": [vp] * 9 + [i32] * 5 + [f64, i32, vp, vp, vp],
        "mvmc_rig_step": [vp] * 11 + [i32] * 5 + [f64, f64, vp, vp],
        "mvmc_rig_accumulate_robust": [vp] * 9 + [i32] * 5 + [f64, i32, vp, vp, i32, f64, vp],
        "mvmc_rig_step_robust": [vp] * 11 + [i32] * 5 + [f64, f64, vp, i32, f64, vp],
        "mvmc_rig_weights": [vp] * 4 + [i32] * 5 + [f64, vp, vp],
        "mvmc_rig_part_doubles_intr": [i32, i32],
        "mvmc_rig_red_doubles_intr": [i32, i32],
        "mvmc_rig_accumulate_intr": [vp] * 9 + [i32] * 5 + [f64, i32, vp, vp, i32, f64, i32, vp, vp, f64, f64, vp],
        "mvmc_rig_step_intr": [vp] * 11 + [i32] * 5 + [f64, f64, vp, i32, f64, i32, vp, vp, f64, f64, vp],
        "mvmc_lens_undistort": [vp, i32, i32, i32, i32, vp, vp, i32, vp, vp, vp],
        "mvmc_lens_distort": [vp, i32, i32, i32, i32, vp, vp, i32, vp, vp, vp],
        "mvmc_pair_moments": [vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp],
        "mvmc_pair_consensus": [vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp],
        "mvmc_pair_refit": [vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp],
        "mvmc_exchange_observe": [vp, vp, i32, i32, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp, i32, f64, f64, f64, f64, vp, vp, vp, vp, vp],
        "mvmc_exchange_apply": [vp, i32, C.c_longlong, i32, vp, vp, vp],
    }
    restypes = {"mvmc_status_string": C.c_char_p, "mvmc_pack_message_words": C.c_longlong, "mvmc_pack_work_words": C.c_longlong,
                "mvmc_stitch_work_words": C.c_longlong, "mvmc_smooth_window_work_doubles": C.c_longlong,
                "mvmc_smooth_window_cov_work_doubles": C.c_longlong, "mvmc_relink_work_words": C.c_longlong,
                "mvmc_reid_work_words": C.c_longlong,
                "mvmc_rig_part_doubles": C.c_longlong, "mvmc_rig_red_doubles": C.c_longlong,
                "mvmc_rig_part_doubles_intr": C.c_longlong, "mvmc_rig_red_doubles_intr": C.c_longlong}
    # A build of another revision loaded through MVMC_LIB_PATH for a same-box A/B comparison (tools/lib_diff.py, tools/*_ab.sh) may
    # lack entry points that were added since WITHIN the same ABI version (checked above); only then is a missing symbol skipped -- the
    # shipped library must export every one.
    ab = bool(os.environ.get("MVMC_LIB_PATH"))
    for name in SYMBOLS:
        if ab and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)  # AttributeError if the library does not export it
        if name in argtypes:
            fn.argtypes = argtypes[name]
        fn.restype = restypes.get(name, C.c_int)
    _lib = lib
    return lib


def check(status: int, what: str):
    """Status -> exception (the reference raises Python exceptions, motion_capture.py:112)."""
    if status == MVMC_OK:
        return
    msg = load().mvmc_status_string(status).decode()
    if status == 1:
        raise ValueError(f"{what}: {msg}")
    raise MvmcError(f"{what}: {msg} (status {status})")
