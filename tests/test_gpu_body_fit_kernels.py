"""GPU: the body-fit kernels (csrc/mvmc_bodyfit.hip), entry point by entry point, on the hand-built cases of tests/body_fit_cases.py
against the NumPy restatement (tests/body_fit_np.py).  tests/test_body_fit_cases_cpu.py shows on the restatement alone that the cases
reach the branches they are for and that none of their decisions is near a threshold.

Gates (the project's figures): selection exact, its distances within 1.5e-11 px (mvmc_st_affinity's gate on the same reproj_error);
length step: free mask, trial count and accept / reject trace exact, E within 1e-9 relative, lengths within 1e-9 m; pose step: bit-equal
to mvmc_ik_solve_stages, joints within 1e-8 m and cost within 1e-9 relative of the restatement."""
import numpy as np
import pytest
import torch

import body_fit_cases as bc
import body_fit_np as bf

pytestmark = pytest.mark.gpu

D_TOL, E_TOL, L_TOL, J_TOL = 1.5e-11, 1e-9, 1e-9, 1e-8


def _T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- selection --------------------------------------------------------------------------------------------------------------------
def _observe(c, max_dist=bf.D_MAX):
    """-> (choice, dist, members, n_views) of mvmc_body_observe on a case's tables, order / grp_lo / grp_hi from frame_buckets."""
    from multiview_motion_capture_amd import device as dev
    from multiview_motion_capture_amd.sequences import frame_buckets
    order, lo, hi = frame_buckets(c["frame_of"])
    members, nv, choice, dist = dev.body_observe(_T(c["kps17"]), _T(c["counts"]), _T(c["Pm"]), _T(c["frame_of"]), _T(c["rig_of"]),
                                                 _T(c["joints"]), _T(order), _T(lo), _T(hi), _T(c["rank"]), max_dist, bf.MIN_SCORE)
    return choice.cpu().numpy(), dist.cpu().numpy(), members.cpu().numpy(), nv.cpu().numpy()


def _gate_selection(got, exp, what):
    choice, dist, members, nv = got
    e_choice, e_dist, e_members, e_nv = exp
    assert np.array_equal(choice, e_choice), (what, choice.tolist(), e_choice.tolist())
    assert np.array_equal(members, e_members), (what, members.tolist(), e_members.tolist())
    assert np.array_equal(nv, e_nv), what
    none = e_choice < 0
    assert np.all(dist[none] == np.inf), what                  # +inf exactly where nothing was chosen
    worst = float(np.abs(dist[~none] - e_dist[~none]).max()) if (~none).any() else 0.0
    assert worst <= D_TOL, (what, worst)
    return worst


@pytest.mark.parametrize("name", list(bc.SELECT_CASES))
def test_selection_equals_the_restatement(name):
    c = bc.select_case(name)
    got = _observe(c)
    worst = _gate_selection(got, bc.select_reference(c), name)
    print(f"\n{name}: {len(c['rank'])} problems, choice / members / n_views equal; worst |dist - restatement| {worst:.2e} px (gate {D_TOL})")
    P = c["kps17"].shape[2]
    if "slots" in c:                                           # the answers written out by hand
        assert np.where(got[2] >= 0, got[2] % P, -1).tolist() == [list(s) for s in c["slots"]]
    for b in c.get("out", []):
        assert (got[0][b] == -1).all() and (got[1][b] == np.inf).all() and (got[2][b] == -1).all() and got[3][b] == 0


def test_selection_distance_bound_is_strict():
    c = bc.select_case("strict_bound")
    choice, dist, members, _ = _observe(c)
    d = float(dist[0, 0])
    assert abs(d - bc.select_reference(c)[1][0, 0]) <= D_TOL and members[0, 0] == choice[0, 0] >= 0
    at = _observe(c, max_dist=d)                               # the distance as the device wrote it: d < d is false
    assert at[0][0, 0] == -1 and at[1][0, 0] == np.inf and at[2][0, 0] == -1 and at[3][0] == 2
    above = _observe(c, max_dist=float(np.nextafter(d, np.inf)))
    assert above[0][0, 0] == choice[0, 0] and above[1][0, 0] == d and above[3][0] == 3
    assert members[0, 1] == -1 and dist[0, 1] == np.inf        # the 70 px pose, beyond D_MAX
    print(f"\nstrict bound: d = {d!r} px; not chosen at max_dist = d, chosen one ulp above")


@pytest.mark.parametrize("name", ["conflicts", "many", "out_of_range"])
def test_selection_does_not_depend_on_the_problem_order(name):
    c = bc.select_case(name)
    ref = _observe(c)
    for perm in bc.permutations(len(c["rank"])):
        got = _observe(bc.permuted(c, perm))
        for a, b in zip(got, ref):
            assert _same_bits(a, np.ascontiguousarray(b[perm])), name      # per record: the same pose at the same distance, bit for bit


def test_selection_launch_shapes_and_argument_checks():
    c = bc.select_case("many")
    assert (len(c["rank"]) * c["kps17"].shape[1]) % 256 != 0   # (gated above: two blocks, the second ragged)
    none = bc.permuted(c, np.zeros(0, int))
    got = _observe(none)                                       # n_problems = 0: no launch, empty outputs
    assert [x.shape for x in got] == [(0, 4), (0, 4), (0, 4), (0,)]
    one = bc.permuted(c, np.arange(1))
    for key, axis in (("kps17", 0), ("kps17", 2), ("Pm", 0)):    # n_frames, p_max, n_rigs = 0: MVMC_ERR_ARG through the wrapper's check
        bad = dict(one)
        bad[key] = np.take(one[key], [], axis=axis)
        if key == "kps17" and axis == 0:
            bad["counts"] = one["counts"][:0]
        with pytest.raises(ValueError, match="mvmc_body_observe"):
            _observe(bad)
    bad = dict(one, kps17=one["kps17"][:, :0], counts=one["counts"][:, :0], Pm=one["Pm"][:, :0])      # n_views = 0
    with pytest.raises(ValueError, match="mvmc_body_observe"):
        _observe(bad)


# ---- length step ------------------------------------------------------------------------------------------------------------------
def _lengths(c, fix_free=False, mask=0, **step):
    """-> (lens (n_ids,11), free_mask (n_ids,), info (n_ids,16)) of mvmc_body_lengths on a scene's tables."""
    from multiview_motion_capture_amd import device as dev
    lens, free = _T(c["lens0"].copy()), _T(np.full(len(c["lens0"]), mask, np.int32))
    info = dev.body_lengths(_T(c["kps17"]), _T(c["Pm"]), _T(c["rig_of"]), _T(c["members"]), _T(c["params"]), _T(c["id_lo"]), lens, free,
                            fix_free, step["max_iter"], step["mu0"], step["ftol"], step["xtol"])
    return lens.cpu().numpy(), free.cpu().numpy(), info.cpu().numpy()


def _rel(a, b):
    return 0.0 if a == b else abs(a - b) / abs(b)


def _gate_lengths(c, got, refs, what, lens_tol=L_TOL):
    lens, free, info = got
    worst = dict(E=0.0, lens=0.0)
    for i, ref in enumerate(refs):
        assert free[i] == ref["mask"], (what, i, bin(free[i]), bin(ref["mask"]))
        assert np.array_equal(info[i, 2:], ref["info"][2:]), (what, i, info[i].tolist(), ref["info"].tolist())     # trials, accepted, trace, -1 fill
        worst["E"] = max(worst["E"], _rel(info[i, 0], ref["info"][0]), _rel(info[i, 1], ref["info"][1]))
        worst["lens"] = max(worst["lens"], float(np.abs(lens[i] - ref["lens"]).max()))
        held = ~ref["free"]
        assert _same_bits(lens[i][held], c["lens0"][i][held]), (what, i)       # held slots: bit-unchanged
    print(f"\n{what}: free masks, trial counts and traces equal; worst E difference {worst['E']:.2e} relative (gate {E_TOL}), "
          f"worst length difference {worst['lens']:.2e} m (gate {lens_tol:.2e})")
    assert worst["E"] <= E_TOL and worst["lens"] <= lens_tol, (what, worst)
    return worst


@pytest.mark.parametrize("name", [n for n in bc.LENGTH_CASES if n not in bc.FAR])
def test_length_step_equals_the_restatement(name):
    c, refs = bc.length_case(name), bc.length_reference(name)
    got = _lengths(c, **bc.step_args(name))
    _gate_lengths(c, got, refs, f"{name} ({np.diff(c['id_lo']).tolist()} problems)")
    if name == "empty_mid":                                    # the identity without problems: untouched, {0, 0, 0, 0, -1 ..}
        assert _same_bits(got[0][1], c["lens0"][1]) and got[1][1] == 0 and got[2][1].tolist() == [0.0] * 4 + [-1.0] * 12
    if name in bc.HELD:
        assert [s for s in range(11) if not (got[1][0] >> s) & 1] == sorted(set(bc.HELD[name][1]) | {7})
    if name == "it0":                                          # max_iter = 0: E0 alone, the lengths as they came
        assert _same_bits(got[0], c["lens0"]) and got[2][0, 0] == got[2][0, 1] > 0


@pytest.mark.parametrize("name", bc.FAR)
def test_length_step_from_far_starts(name):
    """Lengths 6 and 8 times too long, 65 problems: rejected trials, the cap of 12 trials, and (stop_ftol) an accepted trial below
    ftol E.  The lengths here are metres and E is 1e9 and more, so the bound on the lengths is measured, not the 1e-9 m of the other
    cases: the restatement summed over its (problem, view) pairs forward and backward (rounding alone), times 100, and not below 1e-9 m.
    Measured spread: far6 2.3e-12 m, far8 6.3e-12 m, stop_ftol 2.3e-12 m -- the bound is 1e-9 m after all."""
    c, refs, a = bc.length_case(name), bc.length_reference(name), bc.step_args(name)
    back = bc.solve_identity(c["ids"][0], reverse=True, **a)
    spread = float(np.abs(back["lens"] - refs[0]["lens"]).max())
    bound = max(100.0 * spread, L_TOL)
    trace = refs[0]["info"][4:4 + int(refs[0]["info"][2])].astype(int).tolist()
    print(f"\n{name}: trials {trace}; restatement forward against backward {spread:.2e} m -> bound {bound:.2e} m")
    assert 0 in trace and np.array_equal(back["info"][2:], refs[0]["info"][2:])
    _gate_lengths(c, _lengths(c, **a), refs, name, bound)


def test_length_step_max_iter_cap():
    c = bc.length_case("it0")
    a = bc.step_args("it0")
    assert bc.MAX_ITER_CAP == bc.length_reference("far6")[0]["info"][2]        # 12 is accepted and reached (gated above)
    _lengths(c, **dict(a, max_iter=bc.MAX_ITER_CAP))
    for bad in (bc.MAX_ITER_CAP + 1, -1):
        with pytest.raises(ValueError, match="mvmc_body_lengths"):
            _lengths(c, **dict(a, max_iter=bad))


def test_length_step_with_a_fixed_mask():
    name = bc.FIX_FREE_CASE
    c, a = bc.length_case(name), bc.step_args(name)
    ref = bc.solve_identity(c["ids"][0], free=bc.mask_bits(bc.FIX_FREE_MASK), **a)
    got = _lengths(c, fix_free=True, mask=bc.FIX_FREE_MASK, **a)
    assert got[1][0] == bc.FIX_FREE_MASK                       # honoured (fewer bits than diag(H) > 0 gives) and left as it is
    _gate_lengths(c, got, [ref], f"{name}, mask {bc.FIX_FREE_MASK:#b}")
    moved = got[0][0] != c["lens0"][0]
    assert moved.tolist() == bc.mask_bits(bc.FIX_FREE_MASK).tolist()
    got = _lengths(c, fix_free=True, mask=0, **a)              # mask 0: nothing moves, no trial is made
    assert got[1][0] == 0 and _same_bits(got[0], c["lens0"])
    assert got[2][0, 2:].tolist() == [0.0, 0.0] + [-1.0] * 12 and got[2][0, 0] == got[2][0, 1]
    assert _rel(got[2][0, 0], bc.length_reference(name)[0]["info"][0]) <= E_TOL


def test_length_step_depends_on_nothing_else_in_the_launch():
    c, a = bc.length_case("three"), bc.step_args("three")
    whole = _lengths(c, **a)
    again = _lengths(c, **a)
    assert all(_same_bits(x, y) for x, y in zip(whole, again))                 # run to run
    alone = _lengths(bc.cut(c, [0]), **a)
    last = _lengths(bc.cut(c, [1, 2, 0]), **a)                                 # block 2, the others' problems before its own
    for x, y, z in zip(whole, alone, last):
        assert _same_bits(x[0], y[0]) and _same_bits(x[0], z[2])
        assert _same_bits(x[1], z[0]) and _same_bits(x[2], z[1])
    print("\nidentity 0 of three: lens, free mask and info bit-equal alone, as block 0 of three and as block 2 of three, and run to run")


# ---- pose step --------------------------------------------------------------------------------------------------------------------
def _rigs(c, Pm, rig_of, mask=1, nfev=bc.POSE_NFEV, rows=None, members=None):
    from multiview_motion_capture_amd import device as dev
    rows = np.arange(len(c["init"])) if rows is None else rows
    mem = c["members"] if members is None else members
    out = dev.ik_solve_stages_rigs(_T(c["init"][rows]), mask, nfev, _T(c["kps17"]), _T(Pm), _T(np.asarray(rig_of, np.int32)), _T(mem[rows]))
    return [x.cpu().numpy() for x in out]


def _single(c, P, rows, mask=1, nfev=bc.POSE_NFEV):
    from multiview_motion_capture_amd import device as dev
    out = dev.ik_solve_stages(_T(c["init"][rows]), mask, nfev, _T(c["kps17"]), _T(P), _T(c["members"][rows]))
    return [x.cpu().numpy() for x in out]


@pytest.mark.parametrize("mask", [1, 2, 3])
@pytest.mark.parametrize("nfev", [1, 5])
def test_pose_step_is_ik_solve_stages_with_a_rig_offset(mask, nfev):
    """Three rigs in the launch, the calibration under test in the middle, every problem on it: bit-equal to mvmc_ik_solve_stages."""
    from test_body_fit_cpu import _cameras
    c = bc.pose_case()
    rows = np.flatnonzero(c["rig_of"] == 0)
    Pm = np.array([c["Pm"][1], c["Pm"][0], _cameras(4, dist=8.0)])
    got = _rigs(c, Pm, np.ones(len(rows)), mask, nfev, rows)
    exp = _single(c, c["Pm"][0], rows, mask, nfev)
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    for g, e, what in zip(got, exp, ("params", "joints", "info")):
        assert _same_bits(g, e), (what, mask, nfev, float(np.nanmax(np.abs(g - e))))
    print(f"\nstage mask {mask}, {nfev} evaluations: {len(rows)} problems on rig 1 of 3, params / joints / info bit-equal to ik_solve_stages; "
          f"cost {np.array2string(got[2][:, 0], precision=2)}")


def test_pose_step_with_mixed_rigs_equals_single_rig_launches_and_the_restatement():
    c, ref = bc.pose_case(), bc.pose_reference()
    got = _rigs(c, c["Pm"], c["rig_of"])
    for r in (0, 1):
        rows = np.flatnonzero(c["rig_of"] == r)
        for g, e in zip(got, _single(c, c["Pm"][r], rows)):
            assert _same_bits(np.ascontiguousarray(g[rows]), e), r
    dj = max(float(np.abs(got[1][b] - ref[b][2]).max()) for b in range(len(ref)))
    dc = max(_rel(got[2][b, 0], ref[b][1]) for b in range(len(ref)))
    print(f"\n12 problems alternating between two rigs: bit-equal to their single-rig launches; against the restatement joints {dj:.2e} m "
          f"(gate {J_TOL}), cost {dc:.2e} relative (gate {E_TOL}); smallest decision margin {min(r[3] for r in ref):.1e}")
    assert dj <= J_TOL and dc <= E_TOL


def test_pose_step_out_of_range_rigs_and_fewer_than_two_members():
    c = bc.pose_case()
    base = _rigs(c, c["Pm"], c["rig_of"])
    rig = c["rig_of"].copy()
    rig[3], rig[8] = -1, c["Pm"].shape[0]
    mem = c["members"].copy()
    mem[5, np.flatnonzero(mem[5] >= 0)[1:]] = -1               # one member
    mem[6] = -1                                                # none
    got = _rigs(c, c["Pm"], rig, members=mem)
    bad = [3, 5, 6, 8]
    for g, shape in zip(got, ((68,), (18, 3), (8,))):
        assert g.shape[1:] == shape and np.isnan(g[bad]).all()
    good = np.setdiff1d(np.arange(len(rig)), bad)
    for g, e in zip(got, base):
        assert _same_bits(np.ascontiguousarray(g[good]), np.ascontiguousarray(e[good]))     # the neighbours: as without them
    # v_max = C = 1: accepted, nobody has two views; n_problems = 0: accepted, empty outputs
    one = dict(c, kps17=c["kps17"][:, :1], members=np.zeros((len(rig), 1), np.int32))
    out = _rigs(one, c["Pm"][:, :1], c["rig_of"])
    assert all(np.isnan(x).all() for x in out)
    out = _rigs(c, c["Pm"], np.zeros(0), rows=np.zeros(0, int))
    assert [x.shape for x in out] == [(0, 68), (0, 18, 3), (0, 8)]
