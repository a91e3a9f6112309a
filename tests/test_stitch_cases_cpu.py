"""The hand-built cases of the pack and stitch kernels (tests/stitch_cases.py) on the CPU, without the library: the restatement
(oracle/stitch_np.py) against an assignment by enumeration on every boundary small enough, against itself under re-sharding and
between its two levels, and the cases against the branch labels they claim.  The kernels meet the same cases in
tests/test_gpu_stitch_cases.py."""
import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

import stitch_cases as sc
import stitch_np as sn
from multiview_motion_capture_amd.parallel import unpack_message


@pytest.mark.parametrize("name", sc.NAMES)
def test_assignment_equals_enumeration_on_every_small_boundary(name):
    c = sc.case(name)
    truth = sc.expected_pairs(c) if c["truth"] else None
    for g, ip, pj, inn, nj in sc.boundaries(c):
        got = sorted(sn.match_boundary(pj, nj, c["max_dist"]))
        if truth is not None:
            # the same person, live and finite on both sides, is matched -- whoever else is broken -- and nobody else is
            assert [(int(ip[i]), int(inn[j])) for i, j in got] == truth[g], (name, g)
        for i, j in got:
            assert np.isfinite(pj[i]).all() and np.isfinite(nj[j]).all()
        if max(len(sn.finite_tracklets(pj)), len(sn.finite_tracklets(nj))) > 7:
            continue
        total, pairs = sn.match_boundary_brute(pj, nj, c["max_dist"])
        cost = sn.boundary_costs(pj, nj)
        if c["compare"] == "tie":
            # which of two identical tracklets is taken is open; what the pairs cost is not (every assigned pair is accepted here)
            assert len(got) == len(pairs) == min(len(ip), len(inn))
            assert sum(sorted(cost[i, j] for i, j in got)) == sum(sorted(cost[i, j] for i, j in pairs)) == total
            assert len({i for i, _ in got}) == len(got) == len({j for _, j in got})
        else:
            assert got == pairs, (name, g)


def test_greedy_wrong_case_has_its_margin():
    """the 3 x 3 boundary: the optimum beats every other injection by at least 0.05 m, and nearest-first is one of the others"""
    import itertools
    c = sc.case("greedy-wrong")
    (g, ip, pj, inn, nj), = sc.boundaries(c)
    cost = sn.boundary_costs(pj, nj)
    totals = sorted(sum(cost[i, j] for i, j in enumerate(p)) for p in itertools.permutations(range(3)))
    assert totals[0] == sn.match_boundary_brute(pj, nj, c["max_dist"])[0] and totals[1] - totals[0] >= 0.05
    assert sc.greedy_pairs(cost, c["max_dist"]) != sorted(sn.match_boundary(pj, nj, c["max_dist"]))
    assert len(sn.match_boundary(pj, nj, c["max_dist"])) == 3 and len(sc.greedy_pairs(cost, c["max_dist"])) == 2


def test_threshold_case_is_exact():
    c = sc.case("threshold")
    (g, ip, pj, inn, nj), = sc.boundaries(c)
    for j in (c["joints"][0, 0], c["joints"][1, 1]):                  # the pair at the threshold: nothing is lost in the cast
        assert np.array_equal(j, j.astype(np.float32).astype(np.float64))
    cost = sn.boundary_costs(pj, nj)
    assert cost[0, 1] == 0.5 == c["max_dist"] and 0.5 + 5e-5 < cost[1, 0] < 0.5 + 6e-5
    assert sn.match_boundary(pj, nj, c["max_dist"]) == [(0, 1)]


def test_a_sentinel_cost_loses_the_healthy_pair():
    """Why a tracklet with a non-finite joint is left out of the assignment instead of being given a cost beyond any max_dist: 1e30
    swallows the metre-sized costs, both assignments of the 2 x 2 example cost 1e30 exactly, and the solver returns the one that
    loses the healthy pair."""
    c = sc.case("nan-2x2")
    (g, ip, pj, inn, nj), = sc.boundaries(c)

    def old_rule(a, b, max_dist):
        cost = sn.boundary_costs(a, b)
        cost = np.where(np.isfinite(cost), cost, 1e30)
        r, k = linear_sum_assignment(cost)
        return [(int(i), int(j)) for i, j in zip(r, k) if cost[i, j] <= max_dist]

    cost = sn.boundary_costs(pj, nj)
    assert abs(cost[0, 0] - 1.43) < 1e-6 and abs(cost[1, 0] - 0.11) < 1e-6 and np.isnan(cost[:, 1]).all()
    assert 1.43 + 1e30 == 0.11 + 1e30
    assert old_rule(pj, nj, 0.5) == []
    assert sn.match_boundary(pj, nj, 0.5) == [(1, 0)] == sn.match_boundary_brute(pj, nj, 0.5)[1]


@pytest.mark.parametrize("name", sc.NAMES)
def test_restatement_is_the_same_under_every_split_and_between_its_levels(name):
    c = sc.case(name)
    B, T, IC = c["n_chains"], c["t_msg"], c["id_cap"]
    one = sc.reference(name, 1)
    for s in sc.splits(c):
        ref = sc.reference(name, s)
        # pack_np's local section = stitch_np on that shard alone
        for m, (lo, hi) in zip(ref["messages"], ref["ranges"]):
            if ref["b_cap"] == 0 or any(w in (0, 2) for _, w, _ in ref["patches"]):
                continue
            u = unpack_message(m, ref["b_cap"], T, ref["row_cap"], IC)
            alone = sn.stitch_np(m[None], ref["b_cap"], T, ref["row_cap"], c["max_dist"], IC)
            n = hi - lo
            assert u["n_chains"] == n == alone["info"][0]
            assert np.array_equal(u["lgid"], alone["gid"][:n]) and np.array_equal(u["lmatch"], alone["match"][:n])
            if n:
                assert (u["local_roots"], u["local_pairs"]) == (alone["info"][1], alone["info"][3])
        if ref["compare"] == "flags":
            assert ref["stitched"]["info"][2] & 1
            continue
        if ref["stitched"] is None:
            continue
        st = ref["stitched"]
        assert st["info"][0] == B
        for k in ("gid", "match"):
            assert np.array_equal(st[k][:B], one["stitched"][k][:B]), (name, s, k)
            assert (st[k][B:] == -1).all()
        assert np.array_equal(st["info"], one["stitched"]["info"])


@pytest.mark.parametrize("name", sc.NAMES)
def test_case_carries_exactly_the_labels_it_claims(name):
    c = sc.case(name)
    assert sc.measured_labels(c) == c["labels"], (name, sorted(sc.measured_labels(c) ^ c["labels"]))
    assert c["labels"] <= set(sc.LABELS)


def test_every_label_is_carried_by_one_case_and_absent_from_another():
    carried = {n: sc.measured_labels(sc.case(n)) for n in sc.NAMES}
    for lab in sc.LABELS:
        have = [n for n in sc.NAMES if lab in carried[n]]
        assert have and len(have) < len(sc.NAMES), (lab, have)


def test_expected_outcomes_of_the_capacity_and_non_finite_cases():
    # ids-over-cap: error bit 0 set (value 1); the tracklet of local id 16 is matched on both sides, linked on neither
    c, st = sc.case("ids-over-cap"), sc.reference("ids-over-cap", 1)["stitched"]
    assert st["info"][2] == 1 and st["info"][3] == 6
    assert st["match"][1, 0] == 1 and st["match"][2, 1] == 0            # person 1: slots 1 -> 0 -> 1
    assert (st["gid"][1] >= 0).all() and st["gid"][2, 1] not in st["gid"][1] and st["gid"][2, 1] not in st["gid"][0]
    # the broken tracklets: live, matched to nobody, a new identity each; the healthy ones keep theirs
    for name in ("nan-2x2", "inf-3x3-prev", "nan-inf-both"):
        c, st = sc.case(name), sc.reference(name, 1)["stitched"]
        ids, jo = sc.bound_tables(c)
        truth = sc.expected_pairs(c)
        assert st["info"][2] == 0 and st["info"][3] == sum(len(v) for v in truth.values()) > 0
        for g in range(1, c["n_chains"]):
            for s in range(c["t_msg"]):
                if ids[g, 0, s] < 0:
                    continue
                partner = [a for a, b in truth[g] if b == s]
                assert st["match"][g, s] == (partner[0] if partner else -1)
                if partner:
                    assert st["gid"][g, ids[g, 0, s]] == st["gid"][g - 1, ids[g - 1, 1, partner[0]]]
                else:
                    assert st["gid"][g, ids[g, 0, s]] not in st["gid"][:g]
