"""CPU: the statement of the re-identification step (tests/reid_np.py) on hand-built records against values worked by hand, and on
ground-truth scene walks cut into pieces with long holes; the host side of relinking.reidentify_sequences without a GPU."""
import json
import os

import numpy as np
import pytest

import reid_cases as rc
import reid_np as rp
from conftest import ROOT


def _poses(side, values, nan_at=()):
    """One pose per value: the skeleton of rc.BASE with side ``side`` (index into SIDES order) at that length."""
    out = []
    for v in values:
        L = rc.BASE.copy()
        L[side] = v
        out.append(rc.skeleton(L))
    J = np.array(out)
    for pose, joint in nan_at:
        J[pose, joint] = np.nan
    return J


def test_lower_median_at_an_even_and_an_odd_count_with_duplicates():
    # side index 7 is side 8: the single bone of joint 7
    med, se, cnt = rp.signature(_poses(7, [0.5, 0.25, 0.25, 0.75]), 1)
    assert cnt[7] == 4 and med[7] == 0.25 and se[7] == 0.0                    # sorted .25 .25 .5 .75: rank 1; |x - med| 0 0 .25 .5: rank 1
    med, se, cnt = rp.signature(_poses(7, [0.5, 0.25, 0.25, 0.75, 1.0]), 1)
    assert cnt[7] == 5 and med[7] == 0.5                                      # rank 2 of .25 .25 .5 .75 1
    assert se[7] == 1.4826 * 0.25 * 1.2533 / np.sqrt(5.0)                     # |x - med| 0 .25 .25 .25 .5: rank 2
    others = [q for q in range(10) if q != 7]
    assert np.array_equal(med[others], rc.BASE[others]) and np.all(se[others] == 0.0)


def test_a_side_is_the_mean_of_its_left_and_right_bone():
    right = rc.BASE.copy()
    right[0] = 0.5                                                             # joints 1 and 4: 0.25 and 0.5
    med, se, cnt = rp.signature(np.repeat(rc.skeleton(rc.BASE, right=right)[None], 3, axis=0), 1)
    assert rc.BASE[0] == 0.25 and med[0] == 0.375 and np.array_equal(med[1:], rc.BASE[1:]) and np.all(cnt == 3)


def test_a_nan_joint_removes_only_the_sides_of_its_bones():
    J = np.repeat(rc.skeleton(rc.BASE)[None], 4, axis=0)
    J[0, 3] = np.nan                        # a leaf: bone 3, side 2
    J[1, 8] = np.nan                        # bones 8, 9, 12, 15: sides 9, 3, 10 (index 8, 3, 9)
    med, se, cnt = rp.signature(J, 1)
    assert cnt.tolist() == [4, 4, 3, 3, 4, 4, 4, 4, 3, 3]
    assert np.array_equal(med, rc.BASE)


def test_min_poses_and_common_sides():
    J = np.repeat(rc.skeleton(rc.BASE)[None], 10, axis=0)
    assert np.all(np.isnan(rp.signature(J[:9], 10)[0])) and np.array_equal(rp.signature(J, 10)[0], rc.BASE)
    a = (rc.BASE.copy(), np.zeros(10))
    b5 = (np.where(np.arange(10) < 5, rc.BASE + rc.DB, np.nan), np.where(np.arange(10) < 5, 0.0, np.nan))
    b4 = (np.where(np.arange(10) < 4, rc.BASE + rc.DB, np.nan), np.where(np.arange(10) < 4, 0.0, np.nan))
    assert np.isnan(rp.distance(a, b4, 0.002)) and np.isnan(rp.distance(b4, a, 0.002))
    assert rp.distance(a, b5, 0.002) == rp.distance(b5, a, 0.002)
    assert abs(rp.distance(a, b5, 0.002) - rc.z_of(rc.DB)) < 1e-12           # every common side differs by DB, se = 0
    c = (rc.BASE + 0.01, np.full(10, 0.003))                                  # z = 0.01 / sqrt(0.003^2 + 2 x 0.002^2)
    assert abs(rp.distance(a, c, 0.002) - 0.01 / np.sqrt(0.003 ** 2 + 2 * 0.002 ** 2)) < 1e-12


@pytest.mark.parametrize("name", sorted(rc.link_cases()))
def test_hand_built_links(name):
    recs, want, par = rc.link_cases()[name]
    res = rp.reidentify(recs, **par)
    assert rc.taken(recs, res) == want, (name, res["matrix"])
    for i, j in enumerate(res["succ"]):
        if j >= 0:
            assert res["cost"][i] == res["z"][i, j]
    # independence of the order of the caller's list
    back = rp.reidentify(recs[::-1], **par)
    assert rc.taken(recs[::-1], back) == want
    assert np.array_equal(np.sort(back["cost"]), np.sort(res["cost"]))


def test_hand_built_z_values_and_what_the_veto_does():
    cases = rc.link_cases()
    recs, _, par = cases["no veto by a record that overlaps both ends"]
    res = rp.reidentify(recs, **par)
    assert abs(res["cost"][0] - rc.z_of(rc.DB)) < 1e-12 and abs(rc.z_of(rc.DB) - 0.1726) < 1e-4
    for name in ("veto by a record that overlaps B", "veto by a record that overlaps A"):
        recs, want, par = cases[name]
        assert want == set() and rc.taken(recs, rp.reidentify(recs, veto=False, **par)) == {(0, 1)}, name
        z = rp.reidentify(recs, **par)["z"]
        assert abs(z[0, 2] - rc.z_of(rc.DB)) < 1e-12                          # nodes: A, Q, B
        assert min(abs(z[0, 1] - rc.z_of(rc.DQ)), abs(z[1, 2] - rc.z_of(rc.DQ))) < 1e-12
        assert rc.z_of(rc.DB) > 10 * par["ratio"] * rc.z_of(rc.DQ)


def _ground_truth(C, P, seed, sigma, veto=True, same_lengths=None):
    people, recs = rc.cut_case(C, P, seed, sigma, same_lengths=same_lengths)
    links = rp.record_links(recs, rp.reidentify(recs, veto=veto, **rc.defaults()))
    true = rc.true_links(people, recs)
    wrong = {l for l in links if people[l[0]] != people[l[1]]}
    return people, links, true, wrong


def test_cut_ground_truth_takes_no_link_between_two_people_and_finds_most():
    """Scene walks of 400 frames, every person cut twice with holes of 20 - 80 frames, N(0, sigma) on every joint, at the defaults.
    Hard: NO link between two people.  The share of the true links found on the 5 x 4 scenes must reach 0.8 x what
    profiles/reid_sweep.json records for the defaults on its own (other) scenes.  Without the veto at least one scene takes a wrong
    link."""
    sweep = json.load(open(os.path.join(ROOT, "profiles", "reid_sweep.json")))
    wrong_without = 0
    for sigma in rc.SIGMAS:
        found = total = 0
        for C, P, seed in rc.CUT_CASES:
            _, links, true, wrong = _ground_truth(C, P, seed, sigma)
            print(f"sigma {sigma} ({C},{P}) seed {seed}: {len(true)} true links, {len(links & true)} found, {len(wrong)} wrong")
            assert not wrong, (sigma, C, P, seed, wrong)
            if (C, P) == (5, 4):
                found, total = found + len(links & true), total + len(true)
            wrong_without += len(_ground_truth(C, P, seed, sigma, veto=False)[3])
        want = 0.8 * sweep["defaults"]["cut_recall_5x4"][str(sigma)]
        print(f"sigma {sigma}: recall on the 5 x 4 scenes {found}/{total}, gate {want:.3f}")
        assert found / total >= want, (sigma, found, total, want)
    assert wrong_without >= 1


@pytest.mark.parametrize("seed,pair", [(20280701, (2, 3)), (20280707, (0, 1)), (20280703, (0, 1))])
def test_two_people_with_identical_lengths_are_refused_not_swapped(seed, pair):
    """Person pair[1] gets pair[0]'s bone lengths.  Their records' z are then noise against noise, and the veto refuses a link unless
    one z falls below ratio x the other by chance: no link between two people, and what is linked of the twins is true.  The refusal
    is statistical, not certain: of the 32 cases seeds 20280701 .. 20280708 x pairs (0, 1), (2, 3) x sigma 1, 2 cm the restatement
    takes a link between the twins in 2 (seed 20280701, pair (0, 1), both sigmas); these three cases are among the other 30."""
    for sigma in rc.SIGMAS:
        people, links, true, wrong = _ground_truth(5, 4, seed, sigma, same_lengths=pair)
        twins = {l for l in links if people[l[0]] in pair or people[l[1]] in pair}
        print(f"sigma {sigma}: links {sorted(links)}, of the twins {sorted(twins)} of {sum(people[a] in pair for a, _ in true)} true")
        assert not wrong and twins <= true


def test_parameters_and_pack_without_a_gpu():
    from multiview_motion_capture_amd import relinking
    from relink_cases import make_tracklets
    ok = dict(max_z=2.0, ratio=0.7, floor=0.002, min_poses=10, reach=1.0, speed=0.08)
    relinking.check_reid_parameters(**ok)
    relinking.check_reid_parameters(max_gap=5, **ok)
    for bad in (dict(max_z=-1.0), dict(max_z=float("nan")), dict(ratio=1.5), dict(ratio=-0.1), dict(floor=float("inf")), dict(reach=-1.0),
                dict(speed=float("nan")), dict(min_poses=0), dict(min_poses=2.5), dict(max_gap=0), dict(max_gap=1.5)):
        with pytest.raises(ValueError):
            relinking.check_reid_parameters(**dict(ok, **bad))
    recs, _, _ = rc.link_cases()["a chain of three"]
    packed = relinking.pack_reid([make_tracklets(recs), []])
    assert packed["order"][0].tolist() == [0, 1, 2] and packed["rec"].tolist() == [[0, 20], [20, 20], [40, 20]]
    assert packed["frames"].tolist() == [[0, 19], [50, 69], [120, 139]] and packed["seq"].tolist() == [[0, 3, 0, 0], [3, 0, 0, 0]]
    assert np.array_equal(packed["joints"], np.concatenate([r[2] for r in recs])) and packed["sig_work_words"] == 0
    assert relinking.pack_reid([make_tracklets([rc.record(0, 0, 513, rc.BASE)])])["sig_work_words"] == 5130
    t = make_tracklets(recs)[0]
    t.frame_idxs = t.frame_idxs[::-1]
    with pytest.raises(ValueError):
        relinking.pack_reid([[t]])
    assert relinking.reidentify_sequences([[], []]) == [[], []]
    from multiview_motion_capture_amd import _cabi
    lib = _cabi.load()
    assert lib.mvmc_reid_work_words(64) == 0 and lib.mvmc_reid_work_words(65) == 2 * 65 * 65 and lib.mvmc_reid_work_words(513) == -1
