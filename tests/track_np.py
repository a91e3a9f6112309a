"""The temporal-layer kernels (csrc/mvmc_track.hip: mvmc_st_affinity, mvmc_track_assign, mvmc_track_commit) restated in plain NumPy on
the batched, padded tensors the device entry points take.  Written from the reference's semantics as oracle/oracle_np.py and
oracle/tracker_np.py restate them (match_spatial_time motion_capture.py:634-826, match_spatial :618-626, MvTracker.update_4d :873-963,
MvTracklet :312-400) plus the DEVICE CONTRACT of include/mvmc.h where the batched form needs one: n_tracks is clamped to [0, T] and
counts to [0, P] before anything is indexed, a chain without tracklets takes the match_spatial path (an empty spatial-time graph),
K new tracklets and V members per problem are all there is room for, and overflow bits say where that changed the result.
tests/test_track_np_cpu.py pins these functions to oracle/tracker_np.OracleTracker on the Shelf sequence."""
import numpy as np

import oracle_np as o

SP_MEMBER_CAP = 64        # the device keeps at most 64 poses of one match_spatial cluster (and reports the cut in overflow bit 0)
TENTATIVE, CONFIRMED = 1, 2


def clamp(v, lo, hi):
    return int(min(max(int(v), lo), hi))


def st_affinity_np(kps17, counts, frame_idx, track_joints, n_tracks, P, F2=None, min_score=0.1):
    """kps17 (F,C,Pmax,17,3), counts (F,C), frame_idx (B,), track_joints (B,T,18,3), n_tracks (B,), P (C,3,4) projection matrices,
    F2 (C,C,3,3) fundamental matrices or None (made from P as the reference makes them).
    -> W (B,NS,NS), D (B,NS,NS) (NaN where the reference's matrix holds NaN before its nanmax fill), group_counts (B,C+1) int32, all
    padded with 0; NS = T + C * Pmax.  Node order: the chain's live tracklets, then the frame's 2-D poses by view."""
    kps17 = np.asarray(kps17, np.float64)
    _, C, Pmax = kps17.shape[:3]
    B, T = np.asarray(track_joints).shape[:2]
    NS = T + C * Pmax
    W, D, gc = np.zeros((B, NS, NS)), np.zeros((B, NS, NS)), np.zeros((B, C + 1), np.int32)
    for b in range(B):
        nt, f = clamp(n_tracks[b], 0, T), int(frame_idx[b])
        if nt == 0:
            continue        # (the chain takes the match_spatial path: no spatial-time graph)
        cnt = [clamp(counts[f, c], 0, Pmax) for c in range(C)]
        views = [[kps17[f, c, p] for p in range(cnt[c])] for c in range(C)]
        Db, dim = o.spatial_time_distance([np.asarray(track_joints[b][t], np.float64) for t in range(nt)], views, P, min_score, F2)
        _, Sb = o.spatial_time_affinity(Db)
        n = dim[-1]
        D[b, :n, :n], W[b, :n, :n], gc[b] = Db, Sb, np.diff(dim)
    return W, D, gc


def uncut_affinity(D_b, n):
    """The sigmoid of spatial_time_affinity BEFORE its cut at 1e-3, on the leading n x n block of one chain's D (for the tests' margins)."""
    d = np.array(D_b[:n, :n], np.float64)
    d[np.isnan(d)] = np.nanmax(d) + 1.0
    return 1 / (1 + np.exp(5 * ((d - 15) / 30)))


def chain_clusters(labels, n_clusters, nt, cnt):
    """One chain's clusters as parse_match_result gives them: a list, in cluster order, of node lists [(group, local, node)] in node
    order; group 0 = tracklets (only where nt > 0), group 1 + c = view c.  labels: per node of the COMPACT graph (tracklets, then the
    poses by view); nodes labelled -1 (or beyond n_clusters) are in no cluster."""
    nodes = [(0, t) for t in range(nt)] + [(1 + c, p) for c in range(len(cnt)) for p in range(cnt[c])]
    out = [[] for _ in range(max(int(n_clusters), 0))]
    for i, (g, l) in enumerate(nodes):
        k = int(labels[i])
        if 0 <= k < len(out):
            out[k].append((g, l, i))
    return out


def assign_np(labels_sp, ncl_sp, labels_st, ncl_st, counts, frame_idx, n_tracks, track_params, P, K, V):
    """labels_sp (B,C*P) / labels_st (B,T+C*P): cluster label per node of the chain's compact graph; counts (F,C); P = people per view.
    -> members (B,T+K,V) int32 padded with -1, cold (B,T+K) uint8, init (B,T,68) (the warm starts: rows of live tracklets, else 0),
    status (B,T) int32, n_new (B,) int32, overflow (B,) int32 (bit 0).  Member value: (f * C + view) * P + pose."""
    track_params = np.asarray(track_params, np.float64)
    B, T = track_params.shape[:2]
    C = np.asarray(counts).shape[1]
    members = -np.ones((B, T + K, V), np.int32)
    cold = np.zeros((B, T + K), np.uint8)
    cold[:, T:] = 1
    init = np.zeros((B, T, 68))
    status, n_new, ovf = np.zeros((B, T), np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)
    for b in range(B):
        nt, f = clamp(n_tracks[b], 0, T), int(frame_idx[b])
        cnt = [clamp(counts[f, c], 0, P) for c in range(C)]
        init[b, :nt] = track_params[b, :nt]
        val = lambda grp, loc: (f * C + (grp - 1)) * P + loc
        tm, nm = {}, []
        if nt == 0:
            # match_spatial: every pose of a cluster, no per-view dedupe (tracker_np.associate, motion_capture.py:621-626)
            for cl in chain_clusters(labels_sp[b], ncl_sp[b], 0, cnt):
                nm.append([val(g, l) for g, l, _ in cl])
        else:
            for cl in chain_clusters(labels_st[b], ncl_st[b], nt, cnt):
                tidx = next((l for g, l, _ in cl if g == 0), -1)       # the first tracklet of the cluster owns it
                match, seen = [], set()
                for g, l, _ in cl:
                    if g > 0 and g not in seen:                          # the first pose of each view
                        seen.add(g)
                        match.append(val(g, l))
                if tidx >= 0:
                    if match:
                        tm[tidx] = match
                elif match:
                    nm.append(match)
        cap = min(V, SP_MEMBER_CAP) if nt == 0 else V
        for t, m in tm.items():
            status[b, t] = 2 if len(m) >= 2 else 1
            if len(m) >= 2:
                members[b, t, :min(len(m), V)] = m[:V]
        for m in [x for x in tm.values()] + nm:
            if len(m) >= 2 and len(m) > cap:
                ovf[b] |= 1
        k = 0
        for m in nm:
            if len(m) < 2:
                continue
            if k >= K:
                ovf[b] |= 1
                continue
            members[b, T + k, :min(len(m), cap)] = m[:cap]
            k += 1
        n_new[b] = k
    return members, cold, init, status, n_new, ovf


def commit_np(status, n_new, ik_params, ik_joints, track_params, track_joints, meta, n_tracks, next_id, n_dead, K, n_inits):
    """MvTracklet.update / mark_missed (max_age = 0) / births on the padded tables.  status (B,T), n_new (B,), ik_params (B,T+K,68),
    ik_joints (B,T+K,18,3), tables track_params (B,T,68), track_joints (B,T,18,3), meta (B,T,4) = (id, state, hits, length).
    -> dict(params, joints, meta, n_tracks, next_id, n_dead, slot_src (B,T) with -1 where the row was not solved this frame and in the
    tail, overflow (B,) (bit 1)).  Rows at and beyond n_tracks of the returned tables are not specified (the inputs' are kept)."""
    tp, tj, mt = np.array(track_params, np.float64), np.array(track_joints, np.float64), np.array(meta, np.int32)
    B, T = tp.shape[:2]
    nt_out, id_out, dead_out = np.zeros(B, np.int32), np.array(next_id, np.int32), np.array(n_dead, np.int32)
    slot_src, ovf = -np.ones((B, T), np.int32), np.zeros(B, np.int32)
    for b in range(B):
        nt = clamp(n_tracks[b], 0, T)
        rows = []                                   # (params, joints, meta row, IK slot or -1), survivors in order, then births
        for s in range(nt):
            st = int(status[b, s])
            if st == 0:
                dead_out[b] += 1
                continue
            tid, state, hits, length = (int(x) for x in meta[b][s])
            if st == 2:
                hits, length = hits + 1, length + 1
                if state == TENTATIVE and hits >= n_inits:
                    state = CONFIRMED
                rows.append((ik_params[b][s], ik_joints[b][s], (tid, state, hits, length), s))
            else:
                rows.append((track_params[b][s], track_joints[b][s], (tid, state, hits, length), -1))
        for k in range(int(n_new[b])):
            if len(rows) >= T:
                ovf[b] |= 2                         # dropped: no row, no id
                break
            rows.append((ik_params[b][T + k], ik_joints[b][T + k], (int(id_out[b]), TENTATIVE, 1, 1), T + k))
            id_out[b] += 1
        for w, (p, j, m, src) in enumerate(rows):
            tp[b, w], tj[b, w], mt[b, w], slot_src[b, w] = np.array(p), np.array(j), m, src
        nt_out[b] = len(rows)
    return dict(params=tp, joints=tj, meta=mt, n_tracks=nt_out, next_id=id_out, n_dead=dead_out, slot_src=slot_src, overflow=ovf)
