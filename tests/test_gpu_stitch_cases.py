"""GPU: the pack and stitch kernels (csrc/mvmc_stitch.hip through parallel.pack_tracks / parallel.stitch_chains) against their host
restatement (oracle/stitch_np.py) on the hand-built cases of tests/stitch_cases.py, under every split of every case.  All outputs are
integers or copied bit patterns: every comparison is np.array_equal.  The one exception is the case with two identical tracklets,
where WHICH of them is matched is open: there the match table must be an injection of the right size and cost.
(tests/test_stitch_cases_cpu.py shows on the CPU that the cases reach the branches they are made for, and checks the restatement.)"""
import numpy as np
import pytest
import torch

import stitch_cases as sc
import stitch_np as sn

pytestmark = pytest.mark.gpu


def _sections(msg, n, b_cap, T, row_cap, IC):
    """the parts of one message that are defined when the shard has n chains"""
    o_b = 8 + b_cap
    o_r = o_b + b_cap * 2 * T * 56
    o_l = o_r + row_cap * 128
    n_written = min(int(msg[4]), row_cap) if n else 0
    return dict(header=msg[:8], ids=msg[8:8 + n], bounds=msg[o_b:o_r].reshape(b_cap, 2, T, 56)[:n, :, :, :55],
                rows=msg[o_r:o_r + n_written * 128], local_header=msg[o_l:o_l + 8],
                lmatch=msg[o_l + 8:o_l + 8 + b_cap * T].reshape(b_cap, T)[:n],
                lgid=msg[o_l + 8 + b_cap * T:o_l + 8 + b_cap * (T + IC)].reshape(b_cap, IC)[:n])


def _check_tie(c, match, info, exp_info):
    """two identical tracklets: the pairs are an injection between live slots, as many and as cheap as the enumeration's"""
    assert np.array_equal(info, exp_info)
    n_pairs = 0
    for g, ip, pj, inn, nj in sc.boundaries(c):
        pairs = [(int(match[g, s]), s) for s in range(c["t_msg"]) if match[g, s] >= 0]
        assert all(a in ip and b in inn for a, b in pairs) and len({a for a, _ in pairs}) == len(pairs)
        total, best = sn.match_boundary_brute(pj, nj, c["max_dist"])
        cost = sn.boundary_costs(pj, nj)
        assert len(pairs) == len(best) == min(len(ip), len(inn))
        assert sum(sorted(cost[list(ip).index(a), list(inn).index(b)] for a, b in pairs)) == sum(sorted(cost[i, j] for i, j in best)) == total
        n_pairs += len(pairs)
    assert info[3] == n_pairs
    assert (match[0] == -1).all()


@pytest.mark.parametrize("name,split", sc.PARAMS, ids=[f"{n}-{s}" for n, s in sc.PARAMS])
def test_pack_and_stitch_equal_the_restatement(name, split):
    from multiview_motion_capture_amd import parallel as par
    c, ref = sc.case(name), sc.reference(name, split)
    T, IC, b_cap, row_cap = c["t_msg"], c["id_cap"], ref["b_cap"], ref["row_cap"]
    d = torch.device("cuda:0")
    # every input on the device first; then the launches; then ONE copy back (which is the one synchronisation)
    shards = [{k: torch.from_numpy(v).to(d) for k, v in sc.shard_tables(c, lo, hi).items()} for lo, hi in ref["ranges"]]
    vw = None if c["void_words"] is None else torch.from_numpy(np.ascontiguousarray(c["void_words"], dtype=np.int32)).to(d)
    msgs = torch.stack([par.pack_tracks(t, t["next_id"], c["chain_len"], b_cap, row_cap, t_msg=T, void_words=vw, max_dist=c["max_dist"],
                                        id_cap=IC) for t in shards])
    for r, w, v in ref["patches"]:
        msgs[r, w] = v
    parts = [msgs.view(-1)]
    if c["stitch"]:
        st = par.stitch_chains(msgs, b_cap, T, row_cap, c["max_dist"], IC)
        parts += [st["info"], st["match"].view(-1), st["gid"].view(-1)]
    blob = torch.cat(parts).cpu().numpy()
    world, words = msgs.shape
    got_msgs = blob[:world * words].reshape(world, words)
    # ---- pack, shard by shard ----
    assert got_msgs.shape == ref["messages"].shape
    for r, (lo, hi) in enumerate(ref["ranges"]):
        got, exp = _sections(got_msgs[r], hi - lo, b_cap, T, row_cap, IC), _sections(ref["messages"][r], hi - lo, b_cap, T, row_cap, IC)
        for k in got:
            if ref["compare"] == "tie" and k in ("lmatch", "lgid"):
                continue
            assert np.array_equal(got[k], exp[k]), (name, split, r, k)
    if not c["stitch"]:
        return
    # ---- stitch ----
    cap = world * b_cap
    info = blob[world * words:world * words + 4]
    match = blob[world * words + 4:world * words + 4 + cap * T].reshape(cap, T)
    gid = blob[world * words + 4 + cap * T:].reshape(cap, IC)
    exp = ref["stitched"]
    print(f"{name} / {split}: info {info.tolist()} expected {exp['info'].tolist()}")
    if ref["compare"] == "flags":
        assert info[2] == exp["info"][2] and info[2] & 1
        return
    if ref["compare"] == "tie":
        _check_tie(c, match, info, exp["info"])
        n_tot = int(info[0])
    else:
        assert np.array_equal(info, exp["info"])
        n_tot = int(info[0])
        assert np.array_equal(match[:n_tot], exp["match"][:n_tot])
        assert np.array_equal(gid[:n_tot], exp["gid"][:n_tot])
        # sharding does not change the identities
        assert np.array_equal(gid[:n_tot], sc.reference(name, 1)["stitched"]["gid"][:n_tot])
    assert n_tot == c["n_chains"]
    assert (match[n_tot:] == -1).all() and (gid[n_tot:] == -1).all()
