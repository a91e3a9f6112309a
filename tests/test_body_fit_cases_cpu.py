"""CPU: the hand-built cases of the body-fit kernels (tests/body_fit_cases.py) are what they claim to be, on the restatement alone
(tests/body_fit_np.py): the selection rule's answers written out by hand, the length and pose steps' decisions clear of their
thresholds, and the case set's coverage.  tests/test_gpu_body_fit_kernels.py asks the device the same questions."""
import numpy as np
import pytest

import body_fit_cases as bc
import body_fit_np as bf


def _slots(c, members):
    return np.where(members >= 0, members % c["kps17"].shape[2], -1)


@pytest.mark.parametrize("name", list(bc.SELECT_CASES))
def test_selection_cases_end_as_written_by_hand(name):
    c = bc.select_case(name)
    choice, dist, members, nv = bc.select_reference(c)
    assert np.array_equal(nv, (members >= 0).sum(axis=1)) and np.all(np.isinf(dist[choice < 0])) and np.all(np.isfinite(dist[choice >= 0]))
    C, P = c["kps17"].shape[1:3]
    at = choice >= 0
    assert np.array_equal((choice // P)[at], (c["frame_of"][:, None] * C + np.arange(C))[at])      # a pose of its own frame and camera
    if "slots" in c:
        assert _slots(c, members).tolist() == [list(s) for s in c["slots"]]
    for b in c.get("out", []):
        assert choice[b].tolist() == [-1] * C and np.all(dist[b] == np.inf) and members[b].tolist() == [-1] * C and nv[b] == 0
    # the padded restatement is select() wherever select() can be asked: counts within [0, P], frames and rigs in range
    F, R = c["kps17"].shape[0], c["Pm"].shape[0]
    ok = [b for b in range(len(nv)) if 0 <= c["frame_of"][b] < F and 0 <= c["rig_of"][b] < R]
    cnt = np.clip(c["counts"], 0, P)
    views = [[[c["kps17"][f, k, :cnt[f, k]] for k in range(C)] for f in range(F)]] * R
    sel, d2, nv2 = bf.select([(int(c["rig_of"][b]), int(c["frame_of"][b]), int(c["rank"][b]), c["joints"][b]) for b in ok], views, list(c["Pm"]))
    assert np.array_equal(sel, _slots(c, members)[ok]) and np.array_equal(d2, dist[ok]) and np.array_equal(nv2, nv[ok])


def test_selection_bound_is_strict_and_the_problem_order_does_not_matter():
    c = bc.select_case("strict_bound")
    d = bc.select_reference(c)[1][0, 0]
    assert 15.0 < d < 25.0
    assert bc.select_reference(c, max_dist=d)[2][0].tolist()[0] == -1
    assert bc.select_reference(c, max_dist=np.nextafter(d, np.inf))[2][0, 0] == bc.select_reference(c)[2][0, 0] >= 0
    far = bf.reproj_dist(c["joints"][0], c["kps17"][0, 1, 0], c["Pm"][0, 1])
    assert bf.D_MAX < far < 80
    for name in ("conflicts", "many", "out_of_range"):
        c = bc.select_case(name)
        ref = bc.select_reference(c)
        for perm in bc.permutations(len(c["rank"])):
            got = bc.select_reference(bc.permuted(c, perm))
            for a, b in zip(got, ref):
                assert np.array_equal(a, b[perm])


@pytest.mark.parametrize("name", list(bc.LENGTH_CASES))
def test_length_case_margins(name):
    """Every decision of the case's restated step -- a trial's E against E, the predicted reduction against ftol E, |d|_inf against xtol,
    an accepted reduction against ftol E -- is at least 1e-6 (relative) from its threshold: a condition on the inputs, so that a device
    that agrees to 1e-9 cannot legitimately decide otherwise.  A case that violates it gets another seed, not another margin."""
    m, which = bc.length_margin(name)
    print(f"\n{name}: smallest decision margin {m:.3e} ({which}); traces",
          [r["info"][4:4 + int(r["info"][2])].astype(int).tolist() for r in bc.length_reference(name)])
    assert m >= bc.MARGIN, (name, m, which)


def test_length_cases_are_what_they_claim():
    # the fixed mask's run keeps its margins too, and moves only the slots it frees
    m, which = bc.length_margin(bc.FIX_FREE_CASE, bc.mask_bits(bc.FIX_FREE_MASK))
    assert m >= bc.MARGIN, (m, which)
    idn = bc.length_case(bc.FIX_FREE_CASE)["ids"][0]
    r = bc.solve_identity(idn, free=bc.mask_bits(bc.FIX_FREE_MASK), **bc.step_args(bc.FIX_FREE_CASE))
    assert r["mask"] == bc.FIX_FREE_MASK and r["info"][2] >= 1
    assert np.array_equal(r["lens"][~r["free"]], idn["lens0"][~r["free"]]) and np.all(r["lens"][r["free"]] != idn["lens0"][r["free"]])
    r0 = bc.solve_identity(idn, free=np.zeros(11, bool), **bc.step_args(bc.FIX_FREE_CASE))
    assert np.array_equal(r0["lens"], idn["lens0"]) and r0["info"][2] == 0 and r0["info"][0] == r0["info"][1] > 0
    # held slots stay bit-unchanged, free ones move
    for name in bc.LENGTH_CASES:
        for idn, ref in zip(bc.length_case(name)["ids"], bc.length_reference(name)):
            assert np.array_equal(ref["lens"][~ref["free"]], idn["lens0"][~ref["free"]])
            if ref["info"][3] > 0:
                assert np.all(ref["lens"][ref["free"]] != idn["lens0"][ref["free"]])
    e = bc.length_reference("empty_mid")[1]
    assert e["mask"] == 0 and e["info"].tolist() == [0.0] * 4 + [-1.0] * 12
    r = bc.length_reference("it0")[0]
    assert r["info"][0] == r["info"][1] > 0 and r["info"][2] == 0
    # the far starts: reversing the (problem, view) pairs changes rounding only -- the same trials, lengths a few 1e-12 m apart
    for name in bc.FAR:
        a, b = bc.length_reference(name)[0], bc.solve_identity(bc.length_case(name)["ids"][0], reverse=True, **bc.step_args(name))
        assert np.array_equal(a["info"][2:], b["info"][2:])
        print(f"\n{name}: trials {a['info'][4:4 + int(a['info'][2])].astype(int).tolist()}, lengths summed forward and backward differ by "
              f"{np.abs(a['lens'] - b['lens']).max():.2e} m")


def test_pose_case_margins():
    """Every trust-region decision of every pose problem (accept, the ratio's two thresholds, the radius rule, the three stop tests) has a
    relative margin of 1e-6, and no model has an eigenvalue between the null cluster and 1e-6 of its largest."""
    ref = bc.pose_reference()
    worst = min(r[3] for r in ref)
    print("\npose step: smallest decision margin", worst, "costs", np.round([r[1] for r in ref], 2))
    assert worst >= bc.MARGIN
    c = bc.pose_case()
    assert c["rig_of"].tolist() == [0, 1] * 6 and ((c["members"] >= 0).sum(axis=1) >= 2).all() and (c["members"] < 0).any()


def test_coverage():
    rep = bc.check_coverage()
    for k, v in rep.items():
        print(f"\n{k}: {v}")
