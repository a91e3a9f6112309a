"""Batched device entry points: torch CUDA tensors in, torch CUDA tensors out.

Thin, allocation-only wrappers over the C ABI (include/mvmc.h).  PyTorch is the
device-memory container and the stream provider; all arithmetic happens in the
hand-written gfx950 kernels.  Every function launches on the current torch
stream and does not synchronise.

Shapes use F frames, C views, P max people per view, N = C*P graph nodes.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _cabi
from ._cabi import MvmcSkeleton, check

_SEED_CACHE = {}


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def uploader(device):
    """-> T(a): the host array ``a`` (made contiguous) as a tensor on ``device``; the one upload helper of the record stages."""
    return lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _req(t: torch.Tensor, dtype, name: str, shape=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{name}: expected a CUDA tensor")
    if t.dtype != dtype:
        raise ValueError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous tensor")
    if shape is not None:
        if t.dim() != len(shape) or any(s is not None and int(d) != int(s) for d, s in zip(t.shape, shape)):
            raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    return t


def _call(name: str, *args) -> None:
    """The library's entry ``name`` on the current stream (its last argument); a status other than MVMC_OK raises."""
    check(getattr(_cabi.load(), name)(*args, _stream()), name)


def _ground4(ground):
    """(normal (3,), offset) or None -> the 4 host doubles {normal, offset} the contact entries take, or None."""
    return None if ground is None else (C.c_double * 4)(*[float(v) for v in ground[0]], float(ground[1]))


# ----------------------------------------------------------------------------
# skeleton constants (inverse_kinematics.py:120-173) -- data, restated
# ----------------------------------------------------------------------------
SKEL_OFFSETS = np.array([
    [0, 0, 0], [0.15, 0, 0], [0, 0, -0.5], [0, 0, -0.5], [-0.15, 0, 0], [0, 0, -0.5],
    [0, 0, -0.5], [0, 0, 0.3], [0, 0, 0.3], [0.2, 0, 0], [0.3, 0, 0], [0.3, 0, 0],
    [-0.2, 0, 0], [-0.3, 0, 0], [-0.3, 0, 0], [0, -0.02, 0.15], [0.07, 0.02, 0.1],
    [-0.07, 0.02, 0.1]], dtype=np.float64)
SKEL_PARENTS = np.array([-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 9, 10, 8, 12, 13, 8, 15, 15], dtype=np.int32)
SKEL_SIDE_MAP = np.array([7, 0, 1, 2, 0, 1, 2, 8, 9, 3, 4, 5, 3, 4, 5, 10, 6, 6], dtype=np.int32)
SKEL_SIDE_JOINTS = np.array([1, 2, 3, 9, 10, 11, 16, 0, 7, 8, 15])


def skeleton_arrays():
    """(ref_bone_dirs[18,3], ref_side_bone_lens[11])."""
    lens = np.linalg.norm(SKEL_OFFSETS, axis=-1)
    dirs = SKEL_OFFSETS.copy()
    dirs[1:] = dirs[1:] / lens[1:, None]
    return dirs, lens[SKEL_SIDE_JOINTS].copy()


def make_skeleton(bone_dirs=None, parents=None, side_map=None, n_side=11, ref_side_lens=None) -> MvmcSkeleton:
    sk = MvmcSkeleton()
    rl = skeleton_arrays()[1] if ref_side_lens is None else np.asarray(ref_side_lens, np.float64)
    for k in range(18):
        sk.ref_side_lens[k] = float(rl[k]) if k < len(rl) else 0.0
    bd = skeleton_arrays()[0] if bone_dirs is None else np.asarray(bone_dirs, np.float64)
    pa = SKEL_PARENTS if parents is None else np.asarray(parents, np.int32)
    sm = SKEL_SIDE_MAP if side_map is None else np.asarray(side_map, np.int32)
    for j in range(18):
        for k in range(3):
            sk.bone_dirs[j][k] = float(bd[j, k])
        sk.parents[j] = int(pa[j])
        sk.side_map[j] = int(sm[j])
    sk.n_side = int(n_side)
    return sk


# ----------------------------------------------------------------------------
def als_seed_table(count: int, device) -> torch.Tensor:
    """First ``count`` doubles of RandomState(0).rand() (host MT19937 in the library), on ``device``."""
    key = (str(device), int(count))
    hit = _SEED_CACHE.get(key)
    if hit is not None:
        return hit
    buf = (C.c_double * count)()
    check(_cabi.load().mvmc_als_seed_table(C.cast(buf, C.c_void_p), count), "mvmc_als_seed_table")
    t = torch.from_numpy(np.frombuffer(buf, dtype=np.float64).copy()).to(device)
    _SEED_CACHE[key] = t
    return t


def ingest(kps: torch.Tensor, counts: Optional[torch.Tensor] = None, min_score=0.01, min_valid=4, min_bb=5.0):
    """IN-1/IN-2.  kps (F,C,P,25|17,3) f32|f64 -> (kps17 (F,C,P,17,3) f64, counts (F,C) i32)."""
    if kps.dtype not in (torch.float32, torch.float64):
        raise ValueError("ingest: kps must be float32 or float64")
    _req(kps, kps.dtype, "kps")
    if kps.dim() != 5 or kps.shape[3] not in (17, 25) or kps.shape[4] != 3:
        raise ValueError(f"ingest: expected (F,C,P,25|17,3), got {tuple(kps.shape)}")
    F, Cn, P, J, _ = kps.shape
    if counts is not None:
        _req(counts, torch.int32, "counts", (F, Cn))
    out = torch.empty((F, Cn, P, 17, 3), dtype=torch.float64, device=kps.device)
    cnt = torch.empty((F, Cn), dtype=torch.int32, device=kps.device)
    dt = _cabi.MVMC_F32 if kps.dtype == torch.float32 else _cabi.MVMC_F64
    check(_cabi.load().mvmc_ingest(_p(kps), dt, F, Cn, P, J, _p(counts), float(min_score), int(min_valid),
                                   float(min_bb), _p(out), _p(cnt), _stream()), "mvmc_ingest")
    return out, cnt


def fmats(K: torch.Tensor, Rt: torch.Tensor) -> torch.Tensor:
    """AS-1.  K (C,3,3), Rt (C,3,4) f64 -> F (C,C,3,3) f32."""
    Cn = K.shape[0]
    _req(K, torch.float64, "K", (Cn, 3, 3))
    _req(Rt, torch.float64, "Rt", (Cn, 3, 4))
    F = torch.empty((Cn, Cn, 3, 3), dtype=torch.float32, device=K.device)
    check(_cabi.load().mvmc_fmats(_p(K), _p(Rt), Cn, _p(F), _stream()), "mvmc_fmats")
    return F


def affinity(kps17: torch.Tensor, counts: torch.Tensor, Fm: torch.Tensor, want_D=True):
    """AS-2/AS-3.  -> (D, S) each (F,N,N) f32 in compact node order."""
    F, Cn, P = kps17.shape[:3]
    _req(kps17, torch.float64, "kps17", (F, Cn, P, 17, 3))
    _req(counts, torch.int32, "counts", (F, Cn))
    _req(Fm, torch.float32, "Fm", (Cn, Cn, 3, 3))
    N = Cn * P
    D = torch.empty((F, N, N), dtype=torch.float32, device=kps17.device) if want_D else None
    S = torch.empty((F, N, N), dtype=torch.float32, device=kps17.device)
    check(_cabi.load().mvmc_affinity(_p(kps17), _p(counts), _p(Fm), F, Cn, P, _p(D), _p(S), _stream()),
          "mvmc_affinity")
    return D, S


def als_associate(W: torch.Tensor, group_counts: torch.Tensor, g_max: int, want_mats=False):
    """AS-4/5/6.  W (F,N,N) f32|f64, group_counts (F,G) i32 -> dict(labels (F,N), n_clusters, iters[, x_bin, match_mat])."""
    if W.dtype not in (torch.float32, torch.float64):
        raise ValueError("als_associate: W must be float32 or float64")
    F, N, N2 = W.shape
    _req(W, W.dtype, "W", (F, N, N))
    G = group_counts.shape[1]
    _req(group_counts, torch.int32, "group_counts", (F, G))
    dev = W.device
    seed = als_seed_table(_cabi.MAX_NODES * _cabi.MAX_NODES, dev)
    labels = torch.empty((F, N), dtype=torch.int32, device=dev)
    ncl = torch.empty((F,), dtype=torch.int32, device=dev)
    iters = torch.empty((F,), dtype=torch.int32, device=dev)
    xb = torch.empty((F, N, N), dtype=torch.uint8, device=dev) if want_mats else None
    mm = torch.empty((F, N, N), dtype=torch.uint8, device=dev) if want_mats else None
    dt = _cabi.MVMC_F32 if W.dtype == torch.float32 else _cabi.MVMC_F64
    check(_cabi.load().mvmc_als_associate(_p(W), dt, _p(group_counts), F, G, N, int(g_max), _p(seed),
                                          seed.numel(), _p(xb), _p(mm), _p(labels), _p(ncl), _p(iters), _stream()),
          "mvmc_als_associate")
    return dict(labels=labels, n_clusters=ncl, iters=iters, x_bin=xb, match_mat=mm)


def svt_associate(S: torch.Tensor, group_counts: torch.Tensor, g_max: int, alpha=0.1, lam=50.0, mu=64.0, tol=5e-4, max_iter=20,
                  dual_stochastic=True, want_x=False):
    """match_svt (mv_association.py:321-411) + transform_closure + the cluster rule.  S (F,N,N) f32|f64, group_counts (F,G) i32 ->
    dict(x_bin, match_mat (F,N,N) u8, labels (F,N), n_clusters (F), iters (F)[, X (F,N,N) f64])."""
    if S.dtype not in (torch.float32, torch.float64):
        raise ValueError("svt_associate: S must be float32 or float64")
    F, N, _ = S.shape
    _req(S, S.dtype, "S", (F, N, N))
    G = group_counts.shape[1]
    _req(group_counts, torch.int32, "group_counts", (F, G))
    dev = S.device
    work = torch.empty((F, 3, N, N), dtype=torch.float64, device=dev)
    xb = torch.empty((F, N, N), dtype=torch.uint8, device=dev)
    xo = torch.empty((F, N, N), dtype=torch.float64, device=dev) if want_x else None
    iters = torch.empty((F,), dtype=torch.int32, device=dev)
    dt = _cabi.MVMC_F32 if S.dtype == torch.float32 else _cabi.MVMC_F64
    check(_cabi.load().mvmc_svt_associate(_p(S), dt, _p(group_counts), F, G, N, int(g_max), C.c_double(alpha), C.c_double(lam),
                                          C.c_double(mu), C.c_double(tol), int(max_iter), int(bool(dual_stochastic)), _p(work),
                                          _p(xb), _p(xo), _p(iters), _stream()), "mvmc_svt_associate")
    # a row the kernel refused (iters = -1: a count below 0 or above the launch's g_max, or more than N nodes) gets labels -1 and no cluster
    n_nodes = torch.where(iters < 0, 0, group_counts.sum(dim=1)).to(torch.int32)
    mm, labels, ncl = closure_labels(xb, n_nodes)
    return dict(x_bin=xb, match_mat=mm, labels=labels, n_clusters=ncl, iters=iters, X=xo)


def closure_labels(x_bin: torch.Tensor, n_nodes: torch.Tensor, want_mat=True):
    """AS-5/AS-6 alone.  x_bin (F,N,N) u8, n_nodes (F) i32 -> (match_mat (F,N,N) u8 | None, labels (F,N), n_clusters (F))."""
    F, N, _ = x_bin.shape
    _req(x_bin, torch.uint8, "x_bin", (F, N, N))
    _req(n_nodes, torch.int32, "n_nodes", (F,))
    mm = torch.empty((F, N, N), dtype=torch.uint8, device=x_bin.device) if want_mat else None
    labels = torch.empty((F, N), dtype=torch.int32, device=x_bin.device)
    ncl = torch.empty((F,), dtype=torch.int32, device=x_bin.device)
    check(_cabi.load().mvmc_closure_labels(_p(x_bin), _p(n_nodes), F, N, _p(mm), _p(labels), _p(ncl), _stream()),
          "mvmc_closure_labels")
    return mm, labels, ncl


def cluster_members(labels: torch.Tensor, counts: torch.Tensor, p_max: int, k_max: int, v_max: int):
    """labels (F,N), counts (F,C) -> members (F,K,V) pose indices (-1 padded), n_members (F,K)."""
    F, Cn = counts.shape
    _req(counts, torch.int32, "counts")
    _req(labels, torch.int32, "labels", (F, Cn * p_max))
    mem = torch.empty((F, k_max, v_max), dtype=torch.int32, device=labels.device)
    nm = torch.empty((F, k_max), dtype=torch.int32, device=labels.device)
    check(_cabi.load().mvmc_cluster_members(_p(labels), _p(counts), F, Cn, p_max, k_max, v_max, _p(mem), _p(nm),
                                            _stream()), "mvmc_cluster_members")
    return mem, nm


def dlt(kps: torch.Tensor, Pmats: torch.Tensor, members: torch.Tensor, min_score=0.01, post_optimize=False) -> torch.Tensor:
    """TR-1/TR-2.  kps (F,C,P,J,3); Pmats (C,3,4); members (...,V) pose indices -> (...,J,4)."""
    F, Cn, P, J = kps.shape[:4]
    _req(kps, torch.float64, "kps", (F, Cn, P, J, 3))
    _req(Pmats, torch.float64, "Pmats", (Cn, 3, 4))
    _req(members, torch.int32, "members")
    mem = members.reshape(-1, members.shape[-1])
    B, V = mem.shape
    out = torch.empty((B, J, 4), dtype=torch.float64, device=kps.device)
    check(_cabi.load().mvmc_dlt(_p(kps), _p(Pmats), _p(mem), B, V, Cn, P, J, float(min_score), _p(out), _stream()),
          "mvmc_dlt")
    if post_optimize:
        check(_cabi.load().mvmc_triangulate_postopt(_p(kps), _p(Pmats), _p(mem), B, V, Cn, P, J, _p(out), _stream()),
              "mvmc_triangulate_postopt")
    return out.reshape(members.shape[:-1] + (J, 4))


def ingest_dlt(kps: torch.Tensor, counts: Optional[torch.Tensor], Pmats: torch.Tensor, members: torch.Tensor, min_score=0.01,
               ingest_min_score=0.01, min_valid=4, min_bb=5.0, want_counts=False, out_dtype=torch.float64):
    """ingest() + dlt() in one pass (include/mvmc.h: mvmc_ingest_dlt).  kps (F,C,P,25|17,3) f32|f64; members (F,K,V) i32 in ingest()'s
    output numbering, every cluster inside its own frame -> pts3d (F,K,17,4) f64 [, counts (F,C)].  out_dtype=torch.float32
    (float32 keypoints only; mvmc_ingest_dlt_f32): the same float64 arithmetic, the points rounded once at a 16-byte store."""
    if kps.dtype not in (torch.float32, torch.float64):
        raise ValueError("ingest_dlt: kps must be float32 or float64")
    _req(kps, kps.dtype, "kps")
    if kps.dim() != 5 or kps.shape[3] not in (17, 25) or kps.shape[4] != 3:
        raise ValueError(f"ingest_dlt: expected (F,C,P,25|17,3), got {tuple(kps.shape)}")
    F, Cn, P, J, _ = kps.shape
    if counts is not None:
        _req(counts, torch.int32, "counts", (F, Cn))
    _req(Pmats, torch.float64, "Pmats", (Cn, 3, 4))
    if members.dim() != 3 or members.shape[0] != F:
        raise ValueError("ingest_dlt: members must be (F,K,V)")
    _req(members, torch.int32, "members")
    K, V = members.shape[1:]
    if out_dtype not in (torch.float32, torch.float64) or (out_dtype == torch.float32 and kps.dtype != torch.float32):
        raise ValueError("ingest_dlt: out_dtype float32 needs float32 keypoints")
    out = torch.empty((F, K, 17, 4), dtype=out_dtype, device=kps.device)
    cnt = torch.empty((F, Cn), dtype=torch.int32, device=kps.device) if want_counts else None
    if out_dtype == torch.float32:
        check(_cabi.load().mvmc_ingest_dlt_f32(_p(kps), F, Cn, P, J, _p(counts), float(ingest_min_score), int(min_valid), float(min_bb),
                                               _p(Pmats), _p(members), K, V, float(min_score), _p(out), _p(cnt), _stream()),
              "mvmc_ingest_dlt_f32")
        return (out, cnt) if want_counts else out
    dt = _cabi.MVMC_F32 if kps.dtype == torch.float32 else _cabi.MVMC_F64
    check(_cabi.load().mvmc_ingest_dlt(_p(kps), dt, F, Cn, P, J, _p(counts), float(ingest_min_score), int(min_valid), float(min_bb),
                                       _p(Pmats), _p(members), K, V, float(min_score), _p(out), _p(cnt), _stream()), "mvmc_ingest_dlt")
    return (out, cnt) if want_counts else out


def fk(params: torch.Tensor, skeleton: Optional[MvmcSkeleton] = None, want_G=False):
    """FK-1/FK-2.  params (B, 57+n_side) f64 -> joints (B,18,3)[, G (B,18,4,4)]."""
    sk = skeleton if skeleton is not None else make_skeleton()
    B = params.shape[0]
    _req(params, torch.float64, "params", (B, 57 + sk.n_side))
    joints = torch.empty((B, 18, 3), dtype=torch.float64, device=params.device)
    G = torch.empty((B, 18, 4, 4), dtype=torch.float64, device=params.device) if want_G else None
    check(_cabi.load().mvmc_fk(C.byref(sk), _p(params), B, _p(joints), _p(G), _stream()), "mvmc_fk")
    return (joints, G) if want_G else joints


_STREAM_BUFFERS = {}


def stream_buffer(name: str, n: int, tail: tuple, dev) -> torch.Tensor:
    """The f64 device workspace ``name`` of (device, current stream): at least n rows of shape ``tail``, grown on demand and never read
    by the host."""
    key = (name, str(dev), torch.cuda.current_stream(dev).cuda_stream)
    buf = _STREAM_BUFFERS.get(key)
    if buf is None or buf.shape[0] < n:
        buf = torch.empty((n,) + tuple(tail), dtype=torch.float64, device=dev)
        _STREAM_BUFFERS[key] = buf
    return buf


def _ik_scratch(n_problems: int, dev) -> torch.Tensor:
    """Workspace of the IK kernel's eigensolver fallback (include/mvmc.h: MVMC_IK_SCRATCH_DOUBLES per problem)."""
    return stream_buffer("ik", n_problems, (_cabi.IK_SCRATCH_DOUBLES,), dev)


def ik_solve(kps17: torch.Tensor, Pmats: torch.Tensor, members: torch.Tensor,
             init_params: Optional[torch.Tensor] = None, cold: Optional[torch.Tensor] = None,
             max_nfev_cold=50, max_nfev_warm=5, skeleton: Optional[MvmcSkeleton] = None, want_info=True):
    """IK-1..IK-4.  members (B,V) -> params (B,68), joints (B,18,3), info (B,8)."""
    sk = skeleton if skeleton is not None else make_skeleton()
    F, Cn, P = kps17.shape[:3]
    _req(kps17, torch.float64, "kps17", (F, Cn, P, 17, 3))
    _req(Pmats, torch.float64, "Pmats", (Cn, 3, 4))
    _req(members, torch.int32, "members")
    B, V = members.shape
    dev = kps17.device
    if init_params is not None:
        _req(init_params, torch.float64, "init_params", (B, 68))
    if cold is not None:
        _req(cold, torch.uint8, "cold", (B,))
    if init_params is None and cold is not None:
        raise ValueError("ik_solve: warm problems need init_params")
    params = torch.empty((B, 68), dtype=torch.float64, device=dev)
    joints = torch.empty((B, 18, 3), dtype=torch.float64, device=dev)
    info = torch.empty((B, 8), dtype=torch.float64, device=dev) if want_info else None
    check(_cabi.load().mvmc_ik_solve(C.byref(sk), _p(kps17), _p(Pmats), _p(members), B, V, Cn, P, _p(init_params),
                                     _p(cold if init_params is not None else None), int(max_nfev_cold),
                                     int(max_nfev_warm), _p(params), _p(joints), _p(info), _p(_ik_scratch(B, dev)),
                                     _stream()),
          "mvmc_ik_solve")
    return params, joints, info


def ik_solve_stages(init_params: torch.Tensor, stage_mask: int, max_nfev: int, kps17: Optional[torch.Tensor] = None,
                    Pmats: Optional[torch.Tensor] = None, members: Optional[torch.Tensor] = None,
                    targets3d: Optional[torch.Tensor] = None, skeleton: Optional[MvmcSkeleton] = None):
    """Single stages of PoseSolver.solve (stage_mask 1 / 2 / 3) from init_params (B,68), either on the reprojection
    residual (kps17, Pmats, members as in ik_solve) or on 3-D targets (B,18,4) = x, y, z, weight per observation row."""
    sk = skeleton if skeleton is not None else make_skeleton()
    B = init_params.shape[0]
    _req(init_params, torch.float64, "init_params", (B, 68))
    dev = init_params.device
    if targets3d is not None:
        _req(targets3d, torch.float64, "targets3d", (B, 18, 4))
        V = Cn = P = 1
    else:
        if kps17 is None or Pmats is None or members is None:
            raise ValueError("ik_solve_stages: reprojection mode needs kps17, Pmats and members")
        F, Cn, P = kps17.shape[:3]
        _req(kps17, torch.float64, "kps17", (F, Cn, P, 17, 3))
        _req(Pmats, torch.float64, "Pmats", (Cn, 3, 4))
        _req(members, torch.int32, "members", (B, None))
        V = members.shape[1]
    params = torch.empty((B, 68), dtype=torch.float64, device=dev)
    joints = torch.empty((B, 18, 3), dtype=torch.float64, device=dev)
    info = torch.empty((B, 8), dtype=torch.float64, device=dev)
    check(_cabi.load().mvmc_ik_solve_stages(C.byref(sk), _p(kps17), _p(Pmats), _p(members), _p(targets3d), B, V, Cn, P,
                                            _p(init_params), int(stage_mask), int(max_nfev), _p(params), _p(joints),
                                            _p(info), _p(_ik_scratch(B, dev)), _stream()), "mvmc_ik_solve_stages")
    return params, joints, info



def ik_solve_stages_rigs(init_params: torch.Tensor, stage_mask: int, max_nfev: int, kps17: torch.Tensor, Pmats: torch.Tensor,
                         rig_of_problem: torch.Tensor, members: torch.Tensor, skeleton: Optional[MvmcSkeleton] = None):
    """ik_solve_stages in reprojection mode with a calibration per problem: Pmats (R,C,3,4), rig_of_problem (B,) i32
    (include/mvmc.h: mvmc_ik_solve_stages_rigs)."""
    sk = skeleton if skeleton is not None else make_skeleton()
    B = init_params.shape[0]
    _req(init_params, torch.float64, "init_params", (B, 68))
    F, Cn, P = kps17.shape[:3]
    _req(kps17, torch.float64, "kps17", (F, Cn, P, 17, 3))
    _req(Pmats, torch.float64, "Pmats", (None, Cn, 3, 4))
    _req(rig_of_problem, torch.int32, "rig_of_problem", (B,))
    _req(members, torch.int32, "members", (B, None))
    dev = init_params.device
    params = torch.empty((B, 68), dtype=torch.float64, device=dev)
    joints = torch.empty((B, 18, 3), dtype=torch.float64, device=dev)
    info = torch.empty((B, 8), dtype=torch.float64, device=dev)
    check(_cabi.load().mvmc_ik_solve_stages_rigs(C.byref(sk), _p(kps17), _p(Pmats), int(Pmats.shape[0]), _p(rig_of_problem), _p(members),
                                                 B, members.shape[1], Cn, P, _p(init_params), int(stage_mask), int(max_nfev), _p(params),
                                                 _p(joints), _p(info), _p(_ik_scratch(B, dev)), _stream()), "mvmc_ik_solve_stages_rigs")
    return params, joints, info


def body_observe(kps17: torch.Tensor, counts: torch.Tensor, Pmats: torch.Tensor, frame_of: torch.Tensor, rig_of: torch.Tensor,
                 joints: torch.Tensor, order: torch.Tensor, grp_lo: torch.Tensor, grp_hi: torch.Tensor, rank: torch.Tensor,
                 max_dist: float, min_score=0.1):
    """Observation selection of the body fit (include/mvmc.h: mvmc_body_observe).  kps17 (F,C,P,17,3) and counts (F,C) from ingest();
    Pmats (R,C,3,4); per problem (B,): frame_of, rig_of, order, grp_lo, grp_hi, rank i32 and joints (B,18,3) f64
    -> members (B,C) i32 (pose index into kps17 or -1), n_views (B,) i32, choice (B,C) i32, dist (B,C) f64."""
    F, Cn, P = kps17.shape[:3]
    _req(kps17, torch.float64, "kps17", (F, Cn, P, 17, 3))
    _req(counts, torch.int32, "counts", (F, Cn))
    _req(Pmats, torch.float64, "Pmats", (None, Cn, 3, 4))
    B = joints.shape[0]
    _req(joints, torch.float64, "joints", (B, 18, 3))
    for name, t in (("frame_of", frame_of), ("rig_of", rig_of), ("order", order), ("grp_lo", grp_lo), ("grp_hi", grp_hi),
                    ("rank", rank)):
        _req(t, torch.int32, name, (B,))
    d = joints.device
    choice = torch.empty((B, Cn), dtype=torch.int32, device=d)
    dist = torch.empty((B, Cn), dtype=torch.float64, device=d)
    members = torch.empty((B, Cn), dtype=torch.int32, device=d)
    n_views = torch.empty((B,), dtype=torch.int32, device=d)
    check(_cabi.load().mvmc_body_observe(_p(kps17), _p(counts), F, Cn, P, _p(Pmats), int(Pmats.shape[0]), _p(frame_of), _p(rig_of),
                                         _p(joints), _p(order), _p(grp_lo), _p(grp_hi), _p(rank), B, float(min_score), float(max_dist),
                                         _p(choice), _p(dist), _p(members), _p(n_views), _stream()), "mvmc_body_observe")
    return members, n_views, choice, dist


def exchange_observe(kps17: torch.Tensor, counts: torch.Tensor, Pmats: torch.Tensor, frame_of: torch.Tensor, rig_of: torch.Tensor,
                     joints: torch.Tensor, order: torch.Tensor, grp_lo: torch.Tensor, grp_hi: torch.Tensor, rank: torch.Tensor,
                     max_dist: float, min_score=0.1, margin_px=4.0, ratio=0.7):
    """Exchange-aware observation selection (include/mvmc.h: mvmc_exchange_observe); the arguments of body_observe plus the decision's
    margin_px and ratio -> members (B,C) i32 (kept pose index into kps17 or -1), dist (B,C) f64 (d* of the nearest pose before the
    conflicts, +inf: none), flags (B,C) u8 (bit 0 arms, 1 legs, 2 face exchanged), cost (B,C,3,2) f64 (e0, e1 per group, NaN:
    undecided)."""
    F, Cn, P = kps17.shape[:3]
    _req(kps17, torch.float64, "kps17", (F, Cn, P, 17, 3))
    _req(counts, torch.int32, "counts", (F, Cn))
    _req(Pmats, torch.float64, "Pmats", (None, Cn, 3, 4))
    B = joints.shape[0]
    _req(joints, torch.float64, "joints", (B, 18, 3))
    for name, t in (("frame_of", frame_of), ("rig_of", rig_of), ("order", order), ("grp_lo", grp_lo), ("grp_hi", grp_hi),
                    ("rank", rank)):
        _req(t, torch.int32, name, (B,))
    d = joints.device
    members = torch.empty((B, Cn), dtype=torch.int32, device=d)
    dist = torch.empty((B, Cn), dtype=torch.float64, device=d)
    flags = torch.empty((B, Cn), dtype=torch.uint8, device=d)
    cost = torch.empty((B, Cn, 3, 2), dtype=torch.float64, device=d)
    check(_cabi.load().mvmc_exchange_observe(_p(kps17), _p(counts), F, Cn, P, _p(Pmats), int(Pmats.shape[0]), _p(frame_of), _p(rig_of),
                                             _p(joints), _p(order), _p(grp_lo), _p(grp_hi), _p(rank), B, float(min_score),
                                             float(max_dist), float(margin_px), float(ratio), _p(members), _p(dist), _p(flags), _p(cost),
                                             _stream()), "mvmc_exchange_observe")
    return members, dist, flags, cost


def exchange_apply(kps: torch.Tensor, slot_flags: torch.Tensor) -> torch.Tensor:
    """The repaired copy of kps (F,C,P,25|17,3) f32|f64 (include/mvmc.h: mvmc_exchange_apply): slot_flags (F,C,P) u8, bit 0 arms, 1
    legs, 2 face of the slot exchanged.  Same shape and dtype; every triple of the result is a triple of the input."""
    if not isinstance(kps, torch.Tensor) or kps.dtype not in (torch.float32, torch.float64):
        raise ValueError("exchange_apply: kps must be float32 or float64")
    _req(kps, kps.dtype, "kps")
    if kps.dim() != 5 or kps.shape[3] not in (17, 25) or kps.shape[4] != 3:
        raise ValueError(f"exchange_apply: expected (F,C,P,25|17,3), got {tuple(kps.shape)}")
    F, Cn, P, J, _ = kps.shape
    _req(slot_flags, torch.uint8, "slot_flags", (F, Cn, P))
    out = torch.empty_like(kps)
    dt = _cabi.MVMC_F32 if kps.dtype == torch.float32 else _cabi.MVMC_F64
    check(_cabi.load().mvmc_exchange_apply(_p(kps), dt, F * Cn * P, J, _p(slot_flags), _p(out), _stream()), "mvmc_exchange_apply")
    return out


def body_lengths(kps17: torch.Tensor, Pmats: torch.Tensor, rig_of: torch.Tensor, members: torch.Tensor, params: torch.Tensor,
                 id_lo: torch.Tensor, lens: torch.Tensor, free_mask: torch.Tensor, fix_free: bool, max_iter: int, mu0: float,
                 ftol: float, xtol: float, skeleton: Optional[MvmcSkeleton] = None):
    """Length step of the body fit (include/mvmc.h: mvmc_body_lengths), one workgroup per identity.  lens (n_ids,11) f64 and free_mask
    (n_ids,) i32 are updated in place; -> info (n_ids, 16) f64."""
    sk = skeleton if skeleton is not None else make_skeleton()
    F, Cn, P = kps17.shape[:3]
    _req(kps17, torch.float64, "kps17", (F, Cn, P, 17, 3))
    _req(Pmats, torch.float64, "Pmats", (None, Cn, 3, 4))
    B = params.shape[0]
    _req(params, torch.float64, "params", (B, 68))
    _req(rig_of, torch.int32, "rig_of", (B,))
    _req(members, torch.int32, "members", (B, Cn))
    n_ids = id_lo.shape[0] - 1
    _req(id_lo, torch.int32, "id_lo", (n_ids + 1,))
    _req(lens, torch.float64, "lens", (n_ids, 11))
    _req(free_mask, torch.int32, "free_mask", (n_ids,))
    info = torch.empty((n_ids, _cabi.BODY_INFO_DOUBLES), dtype=torch.float64, device=params.device)
    work = torch.empty((max(B, 1), _cabi.BODY_WORK_DOUBLES), dtype=torch.float64, device=params.device)
    check(_cabi.load().mvmc_body_lengths(C.byref(sk), _p(kps17), Cn, P, _p(Pmats), _p(rig_of), _p(members), _p(params), _p(id_lo),
                                         n_ids, _p(lens), _p(free_mask), int(bool(fix_free)), int(max_iter), float(mu0), float(ftol),
                                         float(xtol), _p(info), _p(work), _stream()), "mvmc_body_lengths")
    return info

def smooth_loss_args(loss, loss_px, what: str):
    """loss (None, "huber", "cauchy") and loss_px -> the (int, double) pair of the *_robust entries (include/mvmc.h: MVMC_SMOOTH_LOSS_*)."""
    codes = {None: _cabi.SMOOTH_LOSS_NONE, "huber": _cabi.SMOOTH_LOSS_HUBER, "cauchy": _cabi.SMOOTH_LOSS_CAUCHY}
    if not (loss is None or isinstance(loss, str)) or loss not in codes:
        raise ValueError(f"{what}: loss must be None, \"huber\" or \"cauchy\", got {loss!r}")
    if loss is None:
        return codes[loss], 0.0      # (not read)
    if loss_px is None:
        raise ValueError(f"{what}: loss {loss!r} needs a loss_px")
    return codes[loss], float(loss_px)


def smooth_blocks(kps17: torch.Tensor, Pmats: torch.Tensor, rig_of: torch.Tensor, members: torch.Tensor, x: torch.Tensor,
                  id_of: torch.Tensor, ctl: torch.Tensor, blk: torch.Tensor, skeleton: Optional[MvmcSkeleton] = None, *,
                  loss: Optional[str] = None, loss_px: Optional[float] = None, cmask: Optional[torch.Tensor] = None,
                  anchors: Optional[torch.Tensor] = None, contact_weight: Optional[float] = None,
                  normals: Optional[torch.Tensor] = None, floor_weight: Optional[float] = None) -> None:
    """The data blocks of the trajectory smoother at x (include/mvmc.h: mvmc_smooth_blocks), one wave per row, into blk (2,N,820).
    loss "huber" / "cauchy" with loss_px > 0 (pixels): the blocks of the reweighted model, J^T W J, J^T W r and sum s^2 rho
    (mvmc_smooth_blocks_robust); loss=None is the plain entry.  cmask (N,2) i32 with anchors (N,2,3) f64 and contact_weight >= 0:
    the blocks with the foot-contact term of the labelled rows (mvmc_smooth_blocks_contact), with or without a loss.  With them,
    normals (R,3) f64 (a unit floor normal per rig, NaN: none) and floor_weight >= 0: the term about the floor
    (mvmc_smooth_blocks_floor)."""
    sk = skeleton if skeleton is not None else make_skeleton()
    F, Cn, P = kps17.shape[:3]
    _req(kps17, torch.float64, "kps17", (F, Cn, P, 17, 3))
    _req(Pmats, torch.float64, "Pmats", (None, Cn, 3, 4))
    N = x.shape[0]
    _req(x, torch.float64, "x", (N, 68))
    _req(rig_of, torch.int32, "rig_of", (N,))
    _req(id_of, torch.int32, "id_of", (N,))
    _req(members, torch.int32, "members", (N, Cn))
    _req(ctl, torch.int32, "ctl", (None, 4))
    _req(blk, torch.float64, "blk", (2, N, _cabi.SMOOTH_BLOCK_DOUBLES))
    if (normals is None) != (floor_weight is None) or (normals is not None and cmask is None):
        raise ValueError("smooth_blocks: normals and floor_weight go together, with cmask, anchors and contact_weight")
    name = "mvmc_smooth_blocks"
    args = [C.byref(sk), _p(kps17), Cn, P, _p(Pmats), _p(rig_of), _p(members), _p(x), _p(id_of), _p(ctl), N, _p(blk)]
    if cmask is not None or anchors is not None or contact_weight is not None:
        if cmask is None or anchors is None or contact_weight is None:
            raise ValueError("smooth_blocks: cmask, anchors and contact_weight go together")
        _req(cmask, torch.int32, "cmask", (N, 2))
        _req(anchors, torch.float64, "anchors", (N, 2, 3))
        name += "_contact"
        args += [*smooth_loss_args(loss, loss_px, "smooth_blocks"), _p(cmask), _p(anchors), float(contact_weight)]
        if normals is not None:
            _req(normals, torch.float64, "normals", (Pmats.shape[0], 3))
            name = "mvmc_smooth_blocks_floor"
            args += [_p(normals), float(floor_weight)]
    elif loss is not None:
        name += "_robust"
        args += smooth_loss_args(loss, loss_px, "smooth_blocks")
    _call(name, *args)


def smooth_contact_anchors(joints: torch.Tensor, id_lo: torch.Tensor, cmask: torch.Tensor, anchors: torch.Tensor, ctl: torch.Tensor,
                           detect: bool, speed: float, min_run: int, ground=None, height: float = 0.0) -> None:
    """The foot-contact labels and anchors of every identity from its FK joints (include/mvmc.h: mvmc_smooth_contact_anchors), one
    launch.  joints (N,18,3), id_lo (n_ids + 1,) i32; cmask (N,2) i32 is written when ``detect`` (speed in m / frame, runs of at
    least min_run rows, ground = (normal (3,), offset) with ``height`` or None) and read as given otherwise; anchors (N,2,3) f64 out,
    NaN off the runs; ctl (n_ids,4) i32: the stop word of an identity with a run is cleared."""
    N = joints.shape[0]
    n_ids = id_lo.shape[0] - 1
    _req(joints, torch.float64, "joints", (N, 18, 3))
    _req(id_lo, torch.int32, "id_lo", (n_ids + 1,))
    _req(cmask, torch.int32, "cmask", (N, 2))
    _req(anchors, torch.float64, "anchors", (N, 2, 3))
    _req(ctl, torch.int32, "ctl", (n_ids, 4))
    g = _ground4(ground)
    check(_cabi.load().mvmc_smooth_contact_anchors(_p(joints), _p(id_lo), n_ids, N, int(bool(detect)), float(speed), int(min_run),
                                                   int(g is not None), g, float(height), _p(cmask), _p(anchors), _p(ctl), _stream()),
          "mvmc_smooth_contact_anchors")


def smooth_floor_anchors(joints: torch.Tensor, id_lo: torch.Tensor, rig_of: torch.Tensor, normals: torch.Tensor, cmask: torch.Tensor,
                         anchors: torch.Tensor, levels: torch.Tensor) -> None:
    """The floor level of every identity and its anchors moved onto the floor (include/mvmc.h: mvmc_smooth_floor_anchors), one launch
    after smooth_contact_anchors.  joints (N,18,3), id_lo (n_ids + 1,) i32, rig_of (N,) i32, normals (R,3) f64 unit or NaN, cmask
    (N,2) i32 read; anchors (N,2,3) f64 in place, levels (n_ids,) f64 out: NaN (and the anchors untouched) for an identity without
    a labelled row or with a NaN normal."""
    N = joints.shape[0]
    n_ids = id_lo.shape[0] - 1
    _req(joints, torch.float64, "joints", (N, 18, 3))
    _req(id_lo, torch.int32, "id_lo", (n_ids + 1,))
    _req(rig_of, torch.int32, "rig_of", (N,))
    _req(normals, torch.float64, "normals", (None, 3))
    _req(cmask, torch.int32, "cmask", (N, 2))
    _req(anchors, torch.float64, "anchors", (N, 2, 3))
    _req(levels, torch.float64, "levels", (n_ids,))
    check(_cabi.load().mvmc_smooth_floor_anchors(_p(joints), _p(id_lo), n_ids, N, _p(rig_of), _p(normals), _p(cmask), _p(anchors),
                                                 _p(levels), _stream()), "mvmc_smooth_floor_anchors")


def smooth_obs_weights(kps17: torch.Tensor, Pmats: torch.Tensor, rig_of: torch.Tensor, members: torch.Tensor, x: torch.Tensor,
                       loss: Optional[str], loss_px: Optional[float], skeleton: Optional[MvmcSkeleton] = None) -> torch.Tensor:
    """The loss's weight of every (camera, observed joint) pair of every row at x (include/mvmc.h: mvmc_smooth_obs_weights), one wave
    per row -> w (N,C,16) f64: NaN where the camera has no member in the row or the pair's score is 0; loss=None gives 1 elsewhere."""
    sk = skeleton if skeleton is not None else make_skeleton()
    F, Cn, P = kps17.shape[:3]
    _req(kps17, torch.float64, "kps17", (F, Cn, P, 17, 3))
    _req(Pmats, torch.float64, "Pmats", (None, Cn, 3, 4))
    N = x.shape[0]
    _req(x, torch.float64, "x", (N, 68))
    _req(rig_of, torch.int32, "rig_of", (N,))
    _req(members, torch.int32, "members", (N, Cn))
    code, px = smooth_loss_args(loss, loss_px, "smooth_obs_weights")
    w = torch.empty((N, Cn, 16), dtype=torch.float64, device=x.device)
    check(_cabi.load().mvmc_smooth_obs_weights(C.byref(sk), _p(kps17), Cn, P, _p(Pmats), _p(rig_of), _p(members), _p(x), N, code, px,
                                               _p(w), _stream()), "mvmc_smooth_obs_weights")
    return w


def smooth_step(x: torch.Tensor, x_trial: torch.Tensor, blk: torch.Tensor, id_lo: torch.Tensor, weights, mu0: float, ftol: float,
                xtol: float, max_iter: int, phase: int, ctl: torch.Tensor, info: torch.Tensor, work: torch.Tensor,
                skeleton: Optional[MvmcSkeleton] = None) -> None:
    """One Levenberg-Marquardt step of every identity (include/mvmc.h: mvmc_smooth_step); weights = (root_vel, root_acc, ang_vel,
    ang_acc).  x, x_trial (N,68), ctl (n_ids,4) i32, info (n_ids,32) and work (N,3940) are updated in place."""
    sk = skeleton if skeleton is not None else make_skeleton()
    N = x.shape[0]
    n_ids = id_lo.shape[0] - 1
    _req(x, torch.float64, "x", (N, 68))
    _req(x_trial, torch.float64, "x_trial", (N, 68))
    _req(blk, torch.float64, "blk", (2, N, _cabi.SMOOTH_BLOCK_DOUBLES))
    _req(id_lo, torch.int32, "id_lo", (n_ids + 1,))
    _req(ctl, torch.int32, "ctl", (n_ids, 4))
    _req(info, torch.float64, "info", (n_ids, _cabi.SMOOTH_INFO_DOUBLES))
    _req(work, torch.float64, "work", (N, _cabi.SMOOTH_WORK_DOUBLES))
    rv, ra, av, aa = (float(w) for w in weights)
    check(_cabi.load().mvmc_smooth_step(C.byref(sk), _p(x), _p(x_trial), _p(blk), _p(id_lo), n_ids, N, rv, ra, av, aa, float(mu0),
                                        float(ftol), float(xtol), int(max_iter), int(phase), _p(ctl), _p(info), _p(work), _stream()),
          "mvmc_smooth_step")


def smooth_cov(x: torch.Tensor, blk: torch.Tensor, id_lo: torch.Tensor, weights, mu: float, kps17: torch.Tensor, Pmats: torch.Tensor,
               rig_of: torch.Tensor, members: torch.Tensor, work: torch.Tensor, jcov: torch.Tensor, pvar: torch.Tensor,
               cinfo: torch.Tensor, skeleton: Optional[MvmcSkeleton] = None) -> None:
    """The per-frame covariance of the smoothed trajectory at x (include/mvmc.h: mvmc_smooth_cov), one workgroup per identity; blk
    (N,820) the data blocks AT x, weights = (root_vel, root_acc, ang_vel, ang_acc), mu the damping of the inverted A + mu diag A.
    work (N,3940) is overwritten; jcov (N,18,6), pvar (N,39) and cinfo (n_ids,8) are filled (unit variance)."""
    sk = skeleton if skeleton is not None else make_skeleton()
    F, Cn, P = kps17.shape[:3]
    _req(kps17, torch.float64, "kps17", (F, Cn, P, 17, 3))
    _req(Pmats, torch.float64, "Pmats", (None, Cn, 3, 4))
    N = x.shape[0]
    n_ids = id_lo.shape[0] - 1
    _req(x, torch.float64, "x", (N, 68))
    _req(blk, torch.float64, "blk", (N, _cabi.SMOOTH_BLOCK_DOUBLES))
    _req(id_lo, torch.int32, "id_lo", (n_ids + 1,))
    _req(rig_of, torch.int32, "rig_of", (N,))
    _req(members, torch.int32, "members", (N, Cn))
    _req(work, torch.float64, "work", (N, _cabi.SMOOTH_WORK_DOUBLES))
    _req(jcov, torch.float64, "jcov", (N, _cabi.SMOOTH_JOINTS, 6))
    _req(pvar, torch.float64, "pvar", (N, _cabi.SMOOTH_K))
    _req(cinfo, torch.float64, "cinfo", (n_ids, _cabi.SMOOTH_COV_INFO_DOUBLES))
    rv, ra, av, aa = (float(w) for w in weights)
    check(_cabi.load().mvmc_smooth_cov(C.byref(sk), _p(x), _p(blk), _p(id_lo), n_ids, N, rv, ra, av, aa, float(mu), _p(kps17), Cn, P,
                                       _p(Pmats), _p(rig_of), _p(members), _p(work), _p(jcov), _p(pvar), _p(cinfo), _stream()),
          "mvmc_smooth_cov")


def smooth_window_work(n_items: int, window: int, dev) -> torch.Tensor:
    """Workspace of mvmc_smooth_window for ``n_items`` identities of one tick, sized by the identities active in the tick
    (include/mvmc.h: mvmc_smooth_window_work_doubles)."""
    need = int(_cabi.load().mvmc_smooth_window_work_doubles(int(n_items), int(window)))
    if need < 0:
        raise ValueError(f"smooth_window: no workspace for {n_items} items of window {window}")
    return stream_buffer("smooth_window", max(need, 1), (), dev)


def smooth_window(kps17: torch.Tensor, Pmats: torch.Tensor, items: torch.Tensor, new_params: torch.Tensor, new_members: torch.Tensor,
                  rows: torch.Tensor, members: torch.Tensor, count: torch.Tensor, window: int, n_iter: int, weights, mu0: float,
                  ftol: float, xtol: float, skeleton: Optional[MvmcSkeleton] = None, *, loss: Optional[str] = None,
                  loss_px: Optional[float] = None, contact: Optional[dict] = None):
    """One tick of the live smoother for every item (include/mvmc.h: mvmc_smooth_window), one launch.  kps17 (F,C,P,17,3) the
    sessions' keypoint ring; Pmats (R,C,3,4); items (n,8) i32; new_params (B,68), new_members (B,C) the tick's data rows; rows
    (n_slots,66,68), members (n_slots,66,C), count (n_slots,2) the identities' device state, updated in place.  -> info (n,16).
    loss "huber" / "cauchy" with loss_px > 0: the same launch on the robust data term (mvmc_smooth_window_robust).
    contact = dict(labels (n_slots,66,2) i32, anchors (n_slots,66,2,3) f64 -- state, updated in place --, lag, weight, speed,
    min_frames, ground (normal (3,), offset) or None, height): the launch with foot contacts (mvmc_smooth_window_contact), with or
    without a loss -> (info (n,16), cinfo (n,10))."""
    sk = skeleton if skeleton is not None else make_skeleton()
    F, Cn, P = kps17.shape[:3]
    _req(kps17, torch.float64, "kps17", (F, Cn, P, 17, 3))
    _req(Pmats, torch.float64, "Pmats", (None, Cn, 3, 4))
    n = items.shape[0]
    _req(items, torch.int32, "items", (n, _cabi.SMOOTH_WIN_ITEM_INTS))
    B = new_params.shape[0]
    _req(new_params, torch.float64, "new_params", (B, 68))
    _req(new_members, torch.int32, "new_members", (B, Cn))
    n_slots = rows.shape[0]
    _req(rows, torch.float64, "rows", (n_slots, _cabi.SMOOTH_WIN_RING, 68))
    _req(members, torch.int32, "members", (n_slots, _cabi.SMOOTH_WIN_RING, Cn))
    _req(count, torch.int32, "count", (n_slots, 2))
    rv, ra, av, aa = (float(w) for w in weights)
    info = torch.empty((n, _cabi.SMOOTH_WIN_INFO_DOUBLES), dtype=torch.float64, device=rows.device)
    work = smooth_window_work(n, window, rows.device)
    name = "mvmc_smooth_window"
    args = [C.byref(sk), _p(kps17), Cn, P, _p(Pmats), int(Pmats.shape[0]), _p(items), n, _p(new_params), _p(new_members), B, _p(rows),
            _p(members), _p(count), n_slots, int(window), int(n_iter), rv, ra, av, aa, float(mu0), float(ftol), float(xtol), _p(info),
            _p(work), int(work.numel())]
    if contact is not None:
        _req(contact["labels"], torch.int32, "contact labels", (n_slots, _cabi.SMOOTH_WIN_RING, 2))
        _req(contact["anchors"], torch.float64, "contact anchors", (n_slots, _cabi.SMOOTH_WIN_RING, 2, 3))
        code, px = smooth_loss_args(loss, loss_px, "smooth_window")
        g = _ground4(contact["ground"])
        cinfo = torch.empty((n, _cabi.SMOOTH_LIVE_CONTACT_DOUBLES), dtype=torch.float64, device=rows.device)
        _call(name + "_contact", *args, code, px, _p(contact["labels"]), _p(contact["anchors"]), int(contact["lag"]),
              float(contact["weight"]), float(contact["speed"]), int(contact["min_frames"]), int(g is not None), g,
              float(contact["height"]), _p(cinfo))
        return info, cinfo
    if loss is None:
        _call(name, *args)
    else:
        _call(name + "_robust", *args, *smooth_loss_args(loss, loss_px, "smooth_window"))
    return info


def smooth_window_cov_work(n_items: int, window: int, dev) -> torch.Tensor:
    """Workspace of mvmc_smooth_window_cov for ``n_items`` emitted rows of one tick (include/mvmc.h:
    mvmc_smooth_window_cov_work_doubles)."""
    need = int(_cabi.load().mvmc_smooth_window_cov_work_doubles(int(n_items), int(window)))
    if need < 0:
        raise ValueError(f"smooth_window_cov: no workspace for {n_items} items of window {window}")
    return stream_buffer("smooth_window_cov", max(need, 1), (), dev)


def smooth_window_cov(kps17: torch.Tensor, Pmats: torch.Tensor, items: torch.Tensor, rows: torch.Tensor, members: torch.Tensor,
                      count: torch.Tensor, window: int, weights, mu: float, full: bool, skeleton: Optional[MvmcSkeleton] = None, *,
                      loss: Optional[str] = None, loss_px: Optional[float] = None, contact: Optional[dict] = None):
    """The covariance of the rows a tick emits, conditional on the frozen history (include/mvmc.h: mvmc_smooth_window_cov), one launch
    after smooth_window that only reads the state.  items (n,4) i32 {slot, rig, emit_row, work_row}; kps17, Pmats, rows, members,
    count, window, weights and the loss as smooth_window takes them; mu the damping of the inverted A_w + mu diag A_w; full: the
    recursion covers every free row and cinfo carries n_res and edof (else NaN).  -> jcov (n,18,6), pvar (n,39), cinfo (n,8), unit
    variance.  contact = smooth_window's dict (labels, anchors, weight are read): the free rows' blocks carry the foot-contact term of
    the labels and anchors as they stand (mvmc_smooth_window_cov_contact)."""
    sk = skeleton if skeleton is not None else make_skeleton()
    F, Cn, P = kps17.shape[:3]
    _req(kps17, torch.float64, "kps17", (F, Cn, P, 17, 3))
    _req(Pmats, torch.float64, "Pmats", (None, Cn, 3, 4))
    n = items.shape[0]
    _req(items, torch.int32, "items", (n, _cabi.SMOOTH_COV_ITEM_INTS))
    n_slots = rows.shape[0]
    _req(rows, torch.float64, "rows", (n_slots, _cabi.SMOOTH_WIN_RING, 68))
    _req(members, torch.int32, "members", (n_slots, _cabi.SMOOTH_WIN_RING, Cn))
    _req(count, torch.int32, "count", (n_slots, 2))
    rv, ra, av, aa = (float(w) for w in weights)
    code, px = smooth_loss_args(loss, loss_px, "smooth_window_cov")
    jcov = torch.empty((n, _cabi.SMOOTH_JOINTS, 6), dtype=torch.float64, device=rows.device)
    pvar = torch.empty((n, _cabi.SMOOTH_K), dtype=torch.float64, device=rows.device)
    cinfo = torch.empty((n, _cabi.SMOOTH_COV_INFO_DOUBLES), dtype=torch.float64, device=rows.device)
    work = smooth_window_cov_work(n, window, rows.device)
    name = "mvmc_smooth_window_cov"
    args = [C.byref(sk), _p(kps17), Cn, P, _p(Pmats), int(Pmats.shape[0]), _p(items), n, _p(rows), _p(members), _p(count), n_slots,
            int(window), rv, ra, av, aa, float(mu), int(bool(full)), code, px, _p(work), int(work.numel()), _p(jcov), _p(pvar), _p(cinfo)]
    if contact is not None:
        _req(contact["labels"], torch.int32, "contact labels", (n_slots, _cabi.SMOOTH_WIN_RING, 2))
        _req(contact["anchors"], torch.float64, "contact anchors", (n_slots, _cabi.SMOOTH_WIN_RING, 2, 3))
        name += "_contact"
        args += [_p(contact["labels"]), _p(contact["anchors"]), float(contact["weight"])]
    _call(name, *args)
    return jcov, pvar, cinfo


def live_lengths_apply(items: torch.Tensor, new_params: torch.Tensor, lens_state: torch.Tensor) -> None:
    """Before the tick's smooth_window (include/mvmc.h: mvmc_live_lengths_apply), one launch: a reset item's slot of lens_state
    (n_slots,103) starts from its row of new_params (B,68); the data row of every other item gets the slot's skeleton in columns
    57:68.  Both tensors are updated in place."""
    n = items.shape[0]
    _req(items, torch.int32, "items", (n, _cabi.SMOOTH_WIN_ITEM_INTS))
    B = new_params.shape[0]
    _req(new_params, torch.float64, "new_params", (B, 68))
    n_slots = lens_state.shape[0]
    _req(lens_state, torch.float64, "lens_state", (n_slots, _cabi.LIVE_LEN_STATE_DOUBLES))
    check(_cabi.load().mvmc_live_lengths_apply(_p(items), n, _p(new_params), B, _p(lens_state), n_slots, _stream()),
          "mvmc_live_lengths_apply")


def live_lengths_update(kps17: torch.Tensor, Pmats: torch.Tensor, items: torch.Tensor, rows: torch.Tensor, members: torch.Tensor,
                        count: torch.Tensor, lag: int, prior: float, commit: Optional[int], lens_state: torch.Tensor,
                        skeleton: Optional[MvmcSkeleton] = None) -> torch.Tensor:
    """After the tick's smooth_window (include/mvmc.h: mvmc_live_lengths_update), one launch: the rows that moved behind ``lag`` add
    their normal equations in the 11 lengths to lens_state (n_slots,103), the skeleton is solved again under ``prior`` and written
    into the rows the next tick solves again (rows and lens_state are updated in place).  items, kps17, Pmats, rows, members, count
    as smooth_window takes them; commit None: never.  -> linfo (n,17)."""
    sk = skeleton if skeleton is not None else make_skeleton()
    F, Cn, P = kps17.shape[:3]
    _req(kps17, torch.float64, "kps17", (F, Cn, P, 17, 3))
    _req(Pmats, torch.float64, "Pmats", (None, Cn, 3, 4))
    n = items.shape[0]
    _req(items, torch.int32, "items", (n, _cabi.SMOOTH_WIN_ITEM_INTS))
    n_slots = rows.shape[0]
    _req(rows, torch.float64, "rows", (n_slots, _cabi.SMOOTH_WIN_RING, 68))
    _req(members, torch.int32, "members", (n_slots, _cabi.SMOOTH_WIN_RING, Cn))
    _req(count, torch.int32, "count", (n_slots, 2))
    _req(lens_state, torch.float64, "lens_state", (n_slots, _cabi.LIVE_LEN_STATE_DOUBLES))
    linfo = torch.empty((n, _cabi.LIVE_LEN_INFO_DOUBLES), dtype=torch.float64, device=rows.device)
    check(_cabi.load().mvmc_live_lengths_update(C.byref(sk), _p(kps17), Cn, P, _p(Pmats), int(Pmats.shape[0]), _p(items), n, _p(rows),
                                                _p(members), _p(count), n_slots, int(lag), float(prior),
                                                0 if commit is None else int(commit), _p(lens_state), _p(linfo), _stream()),
          "mvmc_live_lengths_update")
    return linfo


def ik_solve_fd(kps17: torch.Tensor, Pmats: torch.Tensor, members: torch.Tensor, init_params: Optional[torch.Tensor] = None,
                cold: Optional[torch.Tensor] = None, max_nfev_cold=50, max_nfev_warm=5, stage_mask=3,
                skeleton: Optional[MvmcSkeleton] = None):
    """Diagnostic: the same problems as ik_solve through the TRF-faithful solver (finite-difference Jacobian, SVD step;
    mvmc_debug_ik_solve_fd).  -> params (B,68), joints (B,18,3), info (B,8)."""
    sk = skeleton if skeleton is not None else make_skeleton()
    F, Cn, P = kps17.shape[:3]
    _req(kps17, torch.float64, "kps17", (F, Cn, P, 17, 3))
    _req(Pmats, torch.float64, "Pmats", (Cn, 3, 4))
    _req(members, torch.int32, "members")
    B, V = members.shape
    dev = kps17.device
    if init_params is not None:
        _req(init_params, torch.float64, "init_params", (B, 68))
    if cold is not None:
        _req(cold, torch.uint8, "cold", (B,))
    if init_params is None and cold is not None:
        raise ValueError("ik_solve_fd: warm problems need init_params")
    params = torch.empty((B, 68), dtype=torch.float64, device=dev)
    joints = torch.empty((B, 18, 3), dtype=torch.float64, device=dev)
    info = torch.empty((B, 8), dtype=torch.float64, device=dev)
    work = torch.empty((B, _cabi.IK_FD_WORK_DOUBLES), dtype=torch.float64, device=dev)
    check(_cabi.load().mvmc_debug_ik_solve_fd(C.byref(sk), _p(kps17), _p(Pmats), _p(members), B, V, Cn, P, _p(init_params),
                                              _p(cold if init_params is not None else None), int(max_nfev_cold),
                                              int(max_nfev_warm), int(stage_mask), _p(params), _p(joints), _p(info), _p(work),
                                              _stream()), "mvmc_debug_ik_solve_fd")
    return params, joints, info


def ik_model_step(kps17: torch.Tensor, Pmats: torch.Tensor, members: torch.Tensor, params: torch.Tensor, stage: int,
                  Delta: torch.Tensor, alpha0: torch.Tensor, skeleton: Optional[MvmcSkeleton] = None) -> torch.Tensor:
    """Diagnostic: one trust-region model + one trial step of the production IK from (params, Delta, alpha0) per problem
    (mvmc_debug_ik_model_step; layout of the (B, 240) result in include/mvmc.h)."""
    sk = skeleton if skeleton is not None else make_skeleton()
    F, Cn, P = kps17.shape[:3]
    _req(kps17, torch.float64, "kps17", (F, Cn, P, 17, 3))
    _req(Pmats, torch.float64, "Pmats", (Cn, 3, 4))
    _req(members, torch.int32, "members")
    B, V = members.shape
    _req(params, torch.float64, "params", (B, 68))
    _req(Delta, torch.float64, "Delta", (B,))
    _req(alpha0, torch.float64, "alpha0", (B,))
    dev = kps17.device
    out = torch.empty((B, _cabi.IK_STEP_OUT_DOUBLES), dtype=torch.float64, device=dev)
    check(_cabi.load().mvmc_debug_ik_model_step(C.byref(sk), _p(kps17), _p(Pmats), _p(members), B, V, Cn, P, _p(params), int(stage),
                                                _p(Delta), _p(alpha0), _p(out), _p(_ik_scratch(B, dev)), _stream()),
          "mvmc_debug_ik_model_step")
    return out


# ----------------------------------------------------------------------------
# temporal layer (match_spatial_time + tracker), batched over chains
# ----------------------------------------------------------------------------
def fmats_from_projections(Pmats: torch.Tensor) -> torch.Tensor:
    """AS-8 helper.  Pmats (C,3,4) f64 -> F2 (C,C,3,3) f64."""
    Cn = Pmats.shape[0]
    _req(Pmats, torch.float64, "Pmats", (Cn, 3, 4))
    F2 = torch.empty((Cn, Cn, 3, 3), dtype=torch.float64, device=Pmats.device)
    check(_cabi.load().mvmc_fmats_from_projections(_p(Pmats), Cn, _p(F2), _stream()), "mvmc_fmats_from_projections")
    return F2


def _st_affinity(name, kps17, counts, frame_idx, track_joints, n_tracks, Pmats, F2, want_D, min_score, form=()):
    F, Cn, P = kps17.shape[:3]
    B, T = track_joints.shape[:2]
    _req(kps17, torch.float64, "kps17", (F, Cn, P, 17, 3))
    _req(counts, torch.int32, "counts", (F, Cn))
    _req(frame_idx, torch.int32, "frame_idx", (B,))
    _req(track_joints, torch.float64, "track_joints", (B, T, 18, 3))
    _req(n_tracks, torch.int32, "n_tracks", (B,))
    _req(Pmats, torch.float64, "Pmats", (Cn, 3, 4))
    _req(F2, torch.float64, "F2", (Cn, Cn, 3, 3))
    NS = T + Cn * P
    W = torch.empty((B, NS, NS), dtype=torch.float64, device=kps17.device)
    D = torch.empty((B, NS, NS), dtype=torch.float64, device=kps17.device) if want_D else None
    gc = torch.empty((B, Cn + 1), dtype=torch.int32, device=kps17.device)
    check(getattr(_cabi.load(), name)(_p(kps17), _p(counts), _p(frame_idx), _p(track_joints), _p(n_tracks), _p(Pmats), _p(F2), B, Cn, P,
                                      T, float(min_score), *form, _p(W), _p(D), _p(gc), _stream()), name)
    return W, D, gc


def st_affinity(kps17, counts, frame_idx, track_joints, n_tracks, Pmats, F2, want_D=False, min_score=0.1):
    """AS-7/8/9.  -> (W (B,NS,NS) f64, D | None, group_counts (B,C+1) i32)."""
    return _st_affinity("mvmc_st_affinity", kps17, counts, frame_idx, track_joints, n_tracks, Pmats, F2, want_D, min_score)


def debug_st_affinity_wg(kps17, counts, frame_idx, track_joints, n_tracks, Pmats, F2, nt_threads, pair_form, want_D=False, min_score=0.1):
    """Diagnostic: st_affinity's arguments and results from the form the chain kernels run -- one workgroup of nt_threads (256 | 512)
    per chain, the 2-D / 2-D block computed in place (pair_form 0), made ahead per pose pair (1) or by line tables (2)."""
    return _st_affinity("mvmc_debug_st_affinity_wg", kps17, counts, frame_idx, track_joints, n_tracks, Pmats, F2, want_D, min_score,
                        form=(int(nt_threads), int(pair_form)))


def _track_assign_outputs(labels_sp, labels_st, counts, track_params, p_max, k_max, v_max):
    B, T = track_params.shape[:2]
    Cn = counts.shape[1]
    dev_ = track_params.device
    _req(labels_sp, torch.int32, "labels_sp", (B, Cn * p_max))
    _req(labels_st, torch.int32, "labels_st", (B, T + Cn * p_max))
    _req(track_params, torch.float64, "track_params", (B, T, 68))
    NP = T + k_max
    mem = torch.empty((B, NP, v_max), dtype=torch.int32, device=dev_)
    cold = torch.empty((B, NP), dtype=torch.uint8, device=dev_)
    init = torch.empty((B, NP, 68), dtype=torch.float64, device=dev_)
    status = torch.empty((B, T), dtype=torch.int32, device=dev_)
    n_new = torch.empty((B,), dtype=torch.int32, device=dev_)
    return B, T, Cn, mem, cold, init, status, n_new


def track_assign(labels_sp, ncl_sp, labels_st, ncl_st, counts, frame_idx, n_tracks, track_params, p_max, k_max, v_max, overflow=None):
    """TK-1 first half -> members (B,T+K,V), cold (B,T+K), init (B,T+K,68), status (B,T), n_new (B).
    overflow (B) i32 in/out: bit 0 set where a cluster or member did not fit (k_max new clusters, v_max views)."""
    B, T, Cn, mem, cold, init, status, n_new = _track_assign_outputs(labels_sp, labels_st, counts, track_params, p_max, k_max, v_max)
    check(_cabi.load().mvmc_track_assign(_p(labels_sp), _p(ncl_sp), _p(labels_st), _p(ncl_st), _p(counts), _p(frame_idx),
                                         _p(n_tracks), _p(track_params), B, Cn, p_max, T, k_max, v_max, _p(mem), _p(cold),
                                         _p(init), _p(status), _p(n_new), _p(overflow), _stream()), "mvmc_track_assign")
    return mem, cold, init, status, n_new


def debug_track_assign_wave(labels_sp, ncl_sp, labels_st, ncl_st, counts, frame_idx, n_tracks, track_params, p_max, k_max, v_max,
                            overflow=None, want_counts=False):
    """Diagnostic: track_assign's arguments and results from the 64-lane ballot form the chain kernels run (one wave per chain).
    want_counts: -> also n_members (B,T+K) i32, and rows of members are then valid in [0, count) only (no -1 padding)."""
    B, T, Cn, mem, cold, init, status, n_new = _track_assign_outputs(labels_sp, labels_st, counts, track_params, p_max, k_max, v_max)
    n_mem = torch.empty((B, T + k_max), dtype=torch.int32, device=mem.device) if want_counts else None
    check(_cabi.load().mvmc_debug_track_wave(0, _p(labels_sp), _p(ncl_sp), _p(labels_st), _p(ncl_st), _p(counts), _p(frame_idx),
                                             _p(n_tracks), _p(track_params), B, Cn, p_max, T, k_max, v_max, _p(mem), _p(n_mem),
                                             _p(cold), _p(init), _p(status), _p(n_new), None, None, 0, None, None, None, None, None,
                                             _p(overflow), _stream()), "mvmc_debug_track_wave")
    return (mem, cold, init, status, n_new, n_mem) if want_counts else (mem, cold, init, status, n_new)


def _track_commit_req(ik_params, ik_joints, track_params, meta, k_max):
    B, T = track_params.shape[:2]
    _req(ik_params, torch.float64, "ik_params", (B, T + k_max, 68))
    _req(ik_joints, torch.float64, "ik_joints", (B, T + k_max, 18, 3))
    _req(meta, torch.int32, "meta", (B, T, 4))
    return B, T


def track_commit(status, n_new, ik_params, ik_joints, track_params, track_joints, meta, n_tracks, next_id, n_dead,
                 k_max, n_inits=3, slot_src=None, overflow=None):
    """TK-1 second half: updates the tracklet table tensors in place (overflow bit 1: a new tracklet did not fit t_max slots)."""
    B, T = _track_commit_req(ik_params, ik_joints, track_params, meta, k_max)
    check(_cabi.load().mvmc_track_commit(_p(status), _p(n_new), _p(ik_params), _p(ik_joints), B, T, k_max, n_inits,
                                         _p(track_params), _p(track_joints), _p(meta), _p(n_tracks), _p(next_id),
                                         _p(n_dead), _p(slot_src), _p(overflow), _stream()), "mvmc_track_commit")


def debug_track_commit_wave(status, n_new, ik_params, ik_joints, track_params, track_joints, meta, n_tracks, next_id, n_dead,
                            k_max, n_inits=3, slot_src=None, overflow=None):
    """Diagnostic: track_commit from the multi-lane form the chain kernels run (one 64-lane wave per chain)."""
    B, T = _track_commit_req(ik_params, ik_joints, track_params, meta, k_max)
    check(_cabi.load().mvmc_debug_track_wave(1, None, None, None, None, None, None, _p(n_tracks), _p(track_params), B, 0, 0, T, k_max,
                                             0, None, None, None, None, _p(status), _p(n_new), _p(ik_params), _p(ik_joints), n_inits,
                                             _p(track_joints), _p(meta), _p(next_id), _p(n_dead), _p(slot_src), _p(overflow),
                                             _stream()), "mvmc_debug_track_wave")


def rig_start(obs: torch.Tensor, rig_of: torch.Tensor, Pmats: torch.Tensor, min_score=0.1):
    """Start values of the rig refinement (include/mvmc.h: mvmc_rig_start).  obs (N,C,3) f64 u, v, score per candidate point and
    camera; rig_of (N,) i32; Pmats (R,C,3,4) -> X0 (N,4) the DLT of the views with score > min_score, dist (N,C) px (NaN: not used)."""
    N, Cn = obs.shape[:2]
    _req(obs, torch.float64, "obs", (N, Cn, 3))
    _req(rig_of, torch.int32, "rig_of", (N,))
    _req(Pmats, torch.float64, "Pmats", (None, Cn, 3, 4))
    X0 = torch.empty((N, 4), dtype=torch.float64, device=obs.device)
    dist = torch.empty((N, Cn), dtype=torch.float64, device=obs.device)
    check(_cabi.load().mvmc_rig_start(_p(obs), _p(rig_of), _p(Pmats), N, Cn, int(Pmats.shape[0]), float(min_score), _p(X0), _p(dist),
                                      _stream()), "mvmc_rig_start")
    return X0, dist


def _rig_doubles(n_views: int, n_intr=None):
    """(doubles of part per tile, doubles of red per sequence) of the trial entries -- n_intr None: those without intrinsic unknowns;
    -1 where the library refuses the sizes."""
    lib = _cabi.load()
    if n_intr is None:
        return int(lib.mvmc_rig_part_doubles(int(n_views))), int(lib.mvmc_rig_red_doubles(int(n_views)))
    return int(lib.mvmc_rig_part_doubles_intr(int(n_views), int(n_intr))), int(lib.mvmc_rig_red_doubles_intr(int(n_views), int(n_intr)))


def _rig_work(pd: int, rd: int, n_tiles: int, n_seqs: int, dev):
    return (torch.empty((max(n_tiles, 1), pd), dtype=torch.float64, device=dev),
            torch.empty((max(n_tiles, 1), 4), dtype=torch.float64, device=dev), torch.zeros((n_seqs, rd), dtype=torch.float64, device=dev))


def rig_work(n_tiles: int, n_seqs: int, n_views: int, dev):
    """(part (T, mvmc_rig_part_doubles), part2 (T,4), red (S, mvmc_rig_red_doubles)) of mvmc_rig_accumulate / mvmc_rig_step."""
    pd, rd = _rig_doubles(n_views)
    if pd < 0 or rd < 0:
        raise ValueError(f"rig_work: {n_views} cameras outside 2 .. {_cabi.RIG_MAX_CAMS}")
    return _rig_work(pd, rd, n_tiles, n_seqs, dev)


def rig_work_intr(n_tiles: int, n_seqs: int, n_views: int, n_intr: int, dev):
    """rig_work for the entries with intrinsic unknowns (mvmc_rig_part_doubles_intr, mvmc_rig_red_doubles_intr)."""
    pd, rd = _rig_doubles(n_views, n_intr)
    if pd < 0 or rd < 0:
        raise ValueError(f"rig_work_intr: {n_views} cameras outside 2 .. {_cabi.RIG_MAX_CAMS} or n_intr {n_intr} not 1 or 3")
    return _rig_work(pd, rd, n_tiles, n_seqs, dev)


def _rig_trial(name, X, X_trial, uv, tile, seq, slot, cams, cams_trial, ctl, info, red, scalars, work, loss=None, intr=None):
    """What the six wrappers of the trial entries share: the buffers' checks and the call of the entry ``name``.  X_trial None: an
    accumulate entry (scalars max_iter, mu0, variant; work is part), else a step entry (scalars max_iter, ftol, xtol; work is part2).
    loss: None or (loss, loss_px); intr: None or (n_intr, islot, K0, focal_sigma, centre_sigma) -- n_intr is checked by the entry
    itself (the widths of red and part only where it is valid)."""
    N, T, S, Cn = X.shape[0], int(tile.shape[0]), seq.shape[0], slot.shape[1]
    _req(X, torch.float64, "X", (N, 3))
    _req(uv, torch.float64, "uv", (N, Cn, 2))
    _req(tile, torch.int32, "tile", (None, 4))
    _req(seq, torch.int32, "seq", (S, 4))
    _req(slot, torch.int32, "slot", (S, Cn))
    if intr is not None:
        _req(intr[1], torch.int32, "islot", (S, Cn))
        _req(intr[2], torch.float64, "K0", (S, Cn, 3))
    _req(cams, torch.float64, "cams", (S, Cn, _cabi.RIG_CAM_DOUBLES))
    _req(cams_trial, torch.float64, "cams_trial", (S, Cn, _cabi.RIG_CAM_DOUBLES))
    _req(ctl, torch.int32, "ctl", (S, 4))
    _req(info, torch.float64, "info", (S, _cabi.RIG_INFO_DOUBLES))
    pd, rd = _rig_doubles(Cn, None if intr is None else intr[0])
    _req(red, torch.float64, "red", (S, rd if rd >= 0 else None))
    if X_trial is None:
        what = "part"
        _req(work, torch.float64, what, (None, pd if pd >= 0 else None))
        args = [_p(X), _p(uv), _p(tile), _p(seq), _p(slot), _p(cams), _p(cams_trial), _p(ctl), _p(info), N, T, S, Cn, int(scalars[0]),
                float(scalars[1]), int(scalars[2]), _p(work), _p(red)]
    else:
        what = "part2"
        _req(X_trial, torch.float64, "X_trial", (N, 3))
        _req(work, torch.float64, what, (None, 4))
        args = [_p(X), _p(X_trial), _p(uv), _p(tile), _p(seq), _p(slot), _p(cams), _p(cams_trial), _p(ctl), _p(info), _p(red), N, T, S, Cn,
                int(scalars[0]), float(scalars[1]), float(scalars[2]), _p(work)]
    if work.shape[0] < T:
        raise ValueError(f"{what}: {work.shape[0]} rows for {T} tiles")
    if loss is not None:
        args += [int(loss[0]), float(loss[1])]
    if intr is not None:
        args += [int(intr[0]), _p(intr[1]), _p(intr[2]), float(intr[3]), float(intr[4])]
    check(getattr(_cabi.load(), name)(*args, _stream()), name)


def rig_accumulate(X: torch.Tensor, uv: torch.Tensor, tile: torch.Tensor, seq: torch.Tensor, slot: torch.Tensor, cams: torch.Tensor,
                   cams_trial: torch.Tensor, ctl: torch.Tensor, info: torch.Tensor, max_iter: int, mu0: float, part: torch.Tensor,
                   red: torch.Tensor, variant: int = 1) -> None:
    """First half of a trial of the rig refinement (include/mvmc.h: mvmc_rig_accumulate): the reduced camera system of every running
    sequence at (X, cams) and its mu into red, its solution and the trial cameras.  variant 1: matrix cores, 0: FMAs."""
    _rig_trial("mvmc_rig_accumulate", X, None, uv, tile, seq, slot, cams, cams_trial, ctl, info, red, (max_iter, mu0, variant), part)


def rig_step(X: torch.Tensor, X_trial: torch.Tensor, uv: torch.Tensor, tile: torch.Tensor, seq: torch.Tensor, slot: torch.Tensor,
             cams: torch.Tensor, cams_trial: torch.Tensor, ctl: torch.Tensor, info: torch.Tensor, red: torch.Tensor, max_iter: int,
             ftol: float, xtol: float, part2: torch.Tensor) -> None:
    """Second half of a trial (include/mvmc.h: mvmc_rig_step): the points' steps, the trial cost, accept / reject with the gauge
    rescale, the stop rules.  X, cams, ctl and info are updated in place."""
    _rig_trial("mvmc_rig_step", X, X_trial, uv, tile, seq, slot, cams, cams_trial, ctl, info, red, (max_iter, ftol, xtol), part2)


def rig_accumulate_robust(X: torch.Tensor, uv: torch.Tensor, tile: torch.Tensor, seq: torch.Tensor, slot: torch.Tensor,
                          cams: torch.Tensor, cams_trial: torch.Tensor, ctl: torch.Tensor, info: torch.Tensor, max_iter: int, mu0: float,
                          part: torch.Tensor, red: torch.Tensor, variant: int = 1, loss: int = 0, loss_px: float = 0.0) -> None:
    """rig_accumulate with a robust loss (include/mvmc.h: mvmc_rig_accumulate_robust): loss 0 none, 1 Huber, 2 Cauchy at loss_px."""
    _rig_trial("mvmc_rig_accumulate_robust", X, None, uv, tile, seq, slot, cams, cams_trial, ctl, info, red, (max_iter, mu0, variant), part,
               loss=(loss, loss_px))


def rig_step_robust(X: torch.Tensor, X_trial: torch.Tensor, uv: torch.Tensor, tile: torch.Tensor, seq: torch.Tensor, slot: torch.Tensor,
                    cams: torch.Tensor, cams_trial: torch.Tensor, ctl: torch.Tensor, info: torch.Tensor, red: torch.Tensor, max_iter: int,
                    ftol: float, xtol: float, part2: torch.Tensor, loss: int = 0, loss_px: float = 0.0) -> None:
    """rig_step with a robust loss (include/mvmc.h: mvmc_rig_step_robust): the trial cost and every cost in info are sum rho."""
    _rig_trial("mvmc_rig_step_robust", X, X_trial, uv, tile, seq, slot, cams, cams_trial, ctl, info, red, (max_iter, ftol, xtol), part2,
               loss=(loss, loss_px))


def rig_accumulate_intr(X: torch.Tensor, uv: torch.Tensor, tile: torch.Tensor, seq: torch.Tensor, slot: torch.Tensor, cams: torch.Tensor,
                        cams_trial: torch.Tensor, ctl: torch.Tensor, info: torch.Tensor, max_iter: int, mu0: float, part: torch.Tensor,
                        red: torch.Tensor, n_intr: int, islot: torch.Tensor, K0: torch.Tensor, focal_sigma: float, centre_sigma: float,
                        variant: int = 1, loss: int = 0, loss_px: float = 0.0) -> None:
    """rig_accumulate_robust with n_intr (1: phi, 3: phi, dcx, dcy) intrinsic unknowns per camera with islot >= 0 and a Gaussian
    prior about K0 (S,C,3: fx, cx, cy) of focal_sigma (relative) and centre_sigma (px), +inf = none
    (include/mvmc.h: mvmc_rig_accumulate_intr)."""
    _rig_trial("mvmc_rig_accumulate_intr", X, None, uv, tile, seq, slot, cams, cams_trial, ctl, info, red, (max_iter, mu0, variant), part,
               loss=(loss, loss_px), intr=(n_intr, islot, K0, focal_sigma, centre_sigma))


def rig_step_intr(X: torch.Tensor, X_trial: torch.Tensor, uv: torch.Tensor, tile: torch.Tensor, seq: torch.Tensor, slot: torch.Tensor,
                  cams: torch.Tensor, cams_trial: torch.Tensor, ctl: torch.Tensor, info: torch.Tensor, red: torch.Tensor, max_iter: int,
                  ftol: float, xtol: float, part2: torch.Tensor, n_intr: int, islot: torch.Tensor, K0: torch.Tensor, focal_sigma: float,
                  centre_sigma: float, loss: int = 0, loss_px: float = 0.0) -> None:
    """rig_step_robust with intrinsic unknowns (include/mvmc.h: mvmc_rig_step_intr): every cost includes the prior, and cams takes the
    trial K of an accepted trial."""
    _rig_trial("mvmc_rig_step_intr", X, X_trial, uv, tile, seq, slot, cams, cams_trial, ctl, info, red, (max_iter, ftol, xtol), part2,
               loss=(loss, loss_px), intr=(n_intr, islot, K0, focal_sigma, centre_sigma))


def rig_weights(X: torch.Tensor, uv: torch.Tensor, tile: torch.Tensor, cams: torch.Tensor, loss: int, loss_px: float) -> torch.Tensor:
    """The loss's weight of every observation at (X, cams) (include/mvmc.h: mvmc_rig_weights) -> w (N,C) f64, NaN where the camera
    does not observe the point (and on points outside every tile)."""
    N, Cn = uv.shape[:2]
    S = cams.shape[0]
    _req(X, torch.float64, "X", (N, 3))
    _req(uv, torch.float64, "uv", (N, Cn, 2))
    _req(tile, torch.int32, "tile", (None, 4))
    _req(cams, torch.float64, "cams", (S, Cn, _cabi.RIG_CAM_DOUBLES))
    w = torch.full((N, Cn), float("nan"), dtype=torch.float64, device=X.device)
    check(_cabi.load().mvmc_rig_weights(_p(X), _p(uv), _p(tile), _p(cams), N, int(tile.shape[0]), S, Cn, int(loss), float(loss_px), _p(w),
                                        _stream()), "mvmc_rig_weights")
    return w


def _pair_req(xn, seq, pair):
    _req(xn, torch.float64, "xn", (None, 17, 2))
    _req(seq, torch.int32, "seq", (None, 4))
    _req(pair, torch.int32, "pair", (None, 4))
    return int(seq.shape[0]), int(pair.shape[0]), int(xn.shape[0])


def pair_moments(xn: torch.Tensor, seq: torch.Tensor, pair: torch.Tensor, n_slots: int):
    """Rig calibration, per camera pair (include/mvmc.h: mvmc_pair_moments).  xn (rows,17,2) normalised coordinates, NaN = not usable;
    seq (S,4) i32 first row, frames, cameras, 0; pair (Q,4) i32 sequence, a, b, first frame slot; n_slots: frame slots of all pairs
    -> norm (Q,8), mom (n_slots,45), cnt (n_slots,) i32, usable (n_slots,) i32, n_usable (Q,) i32."""
    S, Q, R = _pair_req(xn, seq, pair)
    n_slots = int(n_slots)
    d = xn.device
    norm = torch.zeros((Q, _cabi.RIGINIT_NORM_DOUBLES), dtype=torch.float64, device=d)
    mom = torch.zeros((n_slots, 45), dtype=torch.float64, device=d)
    cnt = torch.zeros((n_slots,), dtype=torch.int32, device=d)
    usable = torch.full((n_slots,), -1, dtype=torch.int32, device=d)
    n_usable = torch.zeros((Q,), dtype=torch.int32, device=d)
    check(_cabi.load().mvmc_pair_moments(_p(xn), _p(seq), _p(pair), S, Q, R, n_slots, _p(norm), _p(mom), _p(cnt), _p(usable),
                                         _p(n_usable), _stream()), "mvmc_pair_moments")
    return norm, mom, cnt, usable, n_usable


def pair_consensus(xn: torch.Tensor, seq: torch.Tensor, pair: torch.Tensor, norm: torch.Tensor, mom: torch.Tensor, usable: torch.Tensor,
                   n_usable: torch.Tensor, u: torch.Tensor, thr: torch.Tensor):
    """The hypotheses of every pair (include/mvmc.h: mvmc_pair_consensus).  u (H,m) f64 in [0, 1): the frame samples; thr (Q,) f64 the
    Sampson thresholds -> E (Q,H,9) f64, count (Q,H) i32."""
    S, Q, R = _pair_req(xn, seq, pair)
    n_slots = int(mom.shape[0])
    _req(norm, torch.float64, "norm", (Q, _cabi.RIGINIT_NORM_DOUBLES))
    _req(mom, torch.float64, "mom", (n_slots, 45))
    _req(usable, torch.int32, "usable", (n_slots,))
    _req(n_usable, torch.int32, "n_usable", (Q,))
    _req(u, torch.float64, "u", (None, None))
    _req(thr, torch.float64, "thr", (Q,))
    H, m = int(u.shape[0]), int(u.shape[1])
    E = torch.zeros((Q, H, 9), dtype=torch.float64, device=xn.device)
    count = torch.zeros((Q, H), dtype=torch.int32, device=xn.device)
    check(_cabi.load().mvmc_pair_consensus(_p(xn), _p(seq), _p(pair), S, Q, R, n_slots, _p(norm), _p(mom), _p(usable), _p(n_usable),
                                           _p(u), _p(thr), H, m, _p(E), _p(count), _stream()), "mvmc_pair_consensus")
    return E, count


def pair_refit(xn: torch.Tensor, seq: torch.Tensor, pair: torch.Tensor, n_slots: int, norm: torch.Tensor, E: torch.Tensor,
               count: torch.Tensor, thr: torch.Tensor, refit_rounds: int):
    """The pose of every pair from its best hypothesis (include/mvmc.h: mvmc_pair_refit) -> pose (Q,32) f64, round_count (Q,9) i32,
    mask (n_slots 17,) i32, points (n_slots 17, 3) f64 in the frame of the pair's first camera (NaN: not an inlier)."""
    S, Q, R = _pair_req(xn, seq, pair)
    n_slots = int(n_slots)
    _req(norm, torch.float64, "norm", (Q, _cabi.RIGINIT_NORM_DOUBLES))
    _req(E, torch.float64, "E", (Q, None, 9))
    H = int(E.shape[1])
    _req(count, torch.int32, "count", (Q, H))
    _req(thr, torch.float64, "thr", (Q,))
    d = xn.device
    pose = torch.zeros((Q, _cabi.RIGINIT_POSE_DOUBLES), dtype=torch.float64, device=d)
    rounds = torch.zeros((Q, _cabi.RIGINIT_MAX_ROUNDS + 1), dtype=torch.int32, device=d)
    mask = torch.zeros((n_slots * 17,), dtype=torch.int32, device=d)
    pts = torch.full((n_slots * 17, 3), float("nan"), dtype=torch.float64, device=d)
    check(_cabi.load().mvmc_pair_refit(_p(xn), _p(seq), _p(pair), S, Q, R, n_slots, _p(norm), _p(E), _p(count), _p(thr), H,
                                       int(refit_rounds), _p(pose), _p(rounds), _p(mask), _p(pts), _stream()), "mvmc_pair_refit")
    return pose, rounds, mask, pts


def _lens_call(name: str, kps: torch.Tensor, lens: torch.Tensor, rig_of_frame, out: Optional[torch.Tensor]):
    if not isinstance(kps, torch.Tensor) or kps.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{name}: kps must be a float32 or float64 tensor")
    _req(kps, kps.dtype, "kps")
    if kps.dim() < 3 or kps.shape[-1] != 3:
        raise ValueError(f"{name}: expected (F,C,...,3) triples, got {tuple(kps.shape)}")
    F, Cn = int(kps.shape[0]), int(kps.shape[1])
    n_points = int(np.prod(kps.shape[2:-1], dtype=np.int64))
    if Cn < 1 or n_points < 1:
        raise ValueError(f"{name}: no cameras or no points in {tuple(kps.shape)}")
    _req(lens, torch.float64, "lens", (None, Cn, _cabi.LENS_DOUBLES))
    R = int(lens.shape[0])
    if R < 1:
        raise ValueError(f"{name}: the lens table holds no rig")
    rig = None
    if rig_of_frame is not None:
        # the rig indices are checked on the host, before anything is launched: a host array as it comes (and uploaded), a device tensor
        # by reading its extremes back (one small transfer; callers on a hot path pass the host array they built the indices in)
        if isinstance(rig_of_frame, torch.Tensor) and rig_of_frame.is_cuda:
            rig = _req(rig_of_frame, torch.int32, "rig_of_frame", (F,))
            lo, hi = (int(v) for v in torch.aminmax(rig)) if F else (0, 0)
        else:
            host = np.ascontiguousarray(np.asarray(rig_of_frame.cpu() if isinstance(rig_of_frame, torch.Tensor) else rig_of_frame))
            if host.shape != (F,) or host.dtype.kind not in "iu":
                raise ValueError(f"rig_of_frame: expected ({F},) integers, got {host.dtype} {host.shape}")
            lo, hi = (int(host.min()), int(host.max())) if F else (0, 0)
            rig = torch.from_numpy(host.astype(np.int32)).to(kps.device) if lo >= 0 and hi < R else None
        if lo < 0 or hi >= R:
            raise ValueError(f"{name}: rig_of_frame holds indices in [{lo}, {hi}], the lens table has rigs 0 .. {R - 1}")
    if out is None:
        out = torch.empty_like(kps)
    else:
        _req(out, kps.dtype, "out", tuple(kps.shape))
        if out.device != kps.device:
            raise ValueError("out: expected a tensor on the device of kps")
    dropped = torch.empty((F, Cn), dtype=torch.int32, device=kps.device)
    dt = _cabi.MVMC_F32 if kps.dtype == torch.float32 else _cabi.MVMC_F64
    if F:
        check(getattr(_cabi.load(), name)(_p(kps), dt, F, Cn, n_points, _p(lens), _p(rig), R, _p(out), _p(dropped), _stream()), name)
    return out, dropped


def lens_undistort(kps: torch.Tensor, lens: torch.Tensor, rig_of_frame=None, out: Optional[torch.Tensor] = None):
    """Raw detector pixels -> pinhole pixels (include/mvmc.h: mvmc_lens_undistort).  kps (F,C,...,3) f32|f64 triples (x, y, score), any
    dimensions between the cameras and the triple (P, J); lens (R,C,16) f64 (lens.lens_table); rig_of_frame (F,) rig of every frame -- a
    host integer array (checked, uploaded) or an int32 device tensor -- or None: rig 0; out: a tensor like kps, which may be kps itself.
    -> (kps_out, dropped (F,C) i32: scored keypoints without a valid pre-image, written (0,0,0)).  An index outside the table raises
    ValueError before anything is launched."""
    return _lens_call("mvmc_lens_undistort", kps, lens, rig_of_frame, out)


def lens_distort(kps: torch.Tensor, lens: torch.Tensor, rig_of_frame=None, out: Optional[torch.Tensor] = None):
    """Pinhole pixels -> raw pixels, the forward lens model (include/mvmc.h: mvmc_lens_distort); arguments and results as
    lens_undistort; nothing is dropped."""
    return _lens_call("mvmc_lens_distort", kps, lens, rig_of_frame, out)
