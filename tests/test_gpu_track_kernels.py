"""The temporal-layer kernels (csrc/mvmc_track.hip: mvmc_st_affinity, mvmc_track_assign, mvmc_track_commit,
mvmc_fmats_from_projections) driven directly on the small cases of tests/track_cases.py -- several chains, gathered frames, counts
and table sizes that need clamping, scores at the threshold, poses without a valid joint, graphs at the 80-node limit, clusters with
two tracklets, K / V / table overflow -- against the NumPy restatement tests/track_np.py, which tests/test_track_np_cpu.py pins to the
oracle tracker; and the forms of the same device functions that only the chain kernels run (whole-workgroup graph builder with a
pose-pair block made ahead, 64-lane ballot assignment, multi-lane commit; mvmc_debug_st_affinity_wg, mvmc_debug_track_wave) against
the stand-alone kernels, bit for bit."""
import numpy as np
import pytest
import torch

import oracle_np as o
import track_cases as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    from multiview_motion_capture_amd import device as dev
    d = torch.device("cuda:0")
    return dev, (lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(d))


def N(t):
    return t.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------------------------
# the graph
# ------------------------------------------------------------------------------------------------------------------------------------
def _affinity_args(gpu, name):
    dev, U = gpu
    c = tc.affinity_case(name)
    Pm = U(c["P"])
    return (U(c["kps17"]), U(c["counts"]), U(c["frame_idx"]), U(c["track_joints"]), U(c["n_tracks"]), Pm, dev.fmats_from_projections(Pm))


@pytest.mark.parametrize("name", ["small", "limit"])
def test_st_affinity_vs_restatement(gpu, name):
    """W, D and the group counts of every chain, padding included.  Bars (those of tests/test_gpu_tracker.py): D to
    1e-9 max(1, nanmax |D|) with the NaN pattern exact, W to 1e-10; entries the reference cuts to 0 are 0, the padding is 0.
    Observed on an MI355X: small |dD| 5.1e-12 px (nanmax |D| 805 px), |dW| 6.5e-14; limit |dD| 1.5e-11 px (1284 px), |dW| 1.5e-13."""
    dev, _ = gpu
    c = tc.affinity_case(name)
    W_o, D_o, gc_o = tc.affinity_reference(name)
    W, D, gc = dev.st_affinity(*_affinity_args(gpu, name), want_D=True, min_score=c["min_score"])
    W, D, gc = N(W), N(D), N(gc)
    assert np.array_equal(gc, gc_o)
    assert np.array_equal(np.isnan(D), np.isnan(D_o))
    scale = max(1.0, np.nanmax(np.abs(D_o)))
    dD, dW = np.nanmax(np.abs(D - D_o)), np.abs(W - W_o).max()
    print(f"\nst_affinity {name}: worst |dD| {dD:.3e} px (nanmax |D| {scale:.1f}), worst |dW| {dW:.3e}")
    assert dD <= 1e-9 * scale
    assert dW < 1e-10
    assert not W[W_o == 0].any()                            # cut entries and the padding: exactly 0
    n = gc_o.sum(axis=1)
    for b in range(len(n)):
        assert not D[b, n[b]:].any() and not D[b, :, n[b]:].any()


def test_st_affinity_refuses_a_graph_beyond_the_node_limit(gpu):
    from multiview_motion_capture_amd._cabi import MvmcError
    dev, U = gpu
    kps, cnt, fidx, tj, nt, Pm, F2 = _affinity_args(gpu, "limit")
    tj81 = torch.zeros((tj.shape[0], 17, 18, 3), dtype=torch.float64, device=tj.device)       # NS = 17 + 64 = 81
    for call in (lambda: dev.st_affinity(kps, cnt, fidx, tj81, nt, Pm, F2),
                 lambda: dev.debug_st_affinity_wg(kps, cnt, fidx, tj81, nt, Pm, F2, 512, 2)):
        with pytest.raises(MvmcError, match="status"):
            call()


@pytest.mark.parametrize("n_views", [1, 2, 16])
def test_fmats_from_projections_vs_oracle(gpu, n_views):
    """get_fundamental_matrix for every ordered pair of views, one camera to 256 pairs over several blocks.  The error of these 4 x 4
    determinants scales with their rows, not with their value: for a single camera (F = 0 in exact arithmetic) the scale is that of a
    second camera of the same kind."""
    from multiview_motion_capture_amd import synth
    dev, U = gpu
    _, _, Pm = synth.make_cameras(max(n_views, 2), np.random.default_rng([51, n_views]))
    ref = np.array([[o.fundamental_from_projections(Pm[a], Pm[b]) for b in range(len(Pm))] for a in range(len(Pm))])
    scale = np.abs(ref).max()
    F2 = N(dev.fmats_from_projections(U(Pm[:n_views])))
    assert F2.shape == (n_views, n_views, 3, 3)
    err = np.abs(F2 - ref[:n_views, :n_views]).max()
    print(f"\nfmats_from_projections C = {n_views}: worst error {err / scale:.2e} of the scale")
    assert err <= 1e-12 * scale


# ------------------------------------------------------------------------------------------------------------------------------------
# assignment and commit
# ------------------------------------------------------------------------------------------------------------------------------------
def _assign(gpu, fn, c, overflow=None, **kw):
    dev, U = gpu
    return fn(U(c["labels_sp"]), U(c["ncl_sp"]), U(c["labels_st"]), U(c["ncl_st"]), U(c["counts"]), U(c["frame_idx"]), U(c["n_tracks"]),
              U(c["track_params"]), c["P"], c["K"], c["V"], overflow=overflow, **kw)


def _assert_assign(out, ref, T, what):
    for k, key in enumerate(("members", "cold", "init", "status", "n_new")):
        got, exp = N(out[k]), ref[k]
        if key == "init":
            got = got[:, :T]                                # rows of the new slots are not part of the contract
        assert np.array_equal(got, exp), (what, key)


@pytest.mark.parametrize("name", list(tc.ASSIGN_SHAPES) + ["cut64"])
def test_track_assign_vs_restatement(gpu, name):
    """Every output bit for bit; the overflow word absent, and preset to 4 (bit 0 is OR-ed in).  cut64: a match_spatial cluster of
    more than 64 poses is cut to 64 and must say so in bit 0 (the one-thread walk used to cut it silently)."""
    dev, U = gpu
    c, ref = tc.assign_case(name), tc.assign_reference(name)
    _assert_assign(_assign(gpu, dev.track_assign, c), ref, c["T"], "no overflow word")
    ovf = torch.full((len(ref[5]),), 4, dtype=torch.int32, device="cuda:0")
    _assert_assign(_assign(gpu, dev.track_assign, c, overflow=ovf), ref, c["T"], "overflow preset")
    assert np.array_equal(N(ovf), ref[5] | 4)


def _tables(gpu, c):
    _, U = gpu
    return {k: U(c[k]) for k in ("track_params", "track_joints", "meta", "n_tracks", "next_id", "n_dead")}


def _commit(gpu, fn, c, n_inits, overflow):
    _, U = gpu
    t = _tables(gpu, c)
    B, T = c["status"].shape
    slot_src = torch.full((B, T), 77, dtype=torch.int32, device="cuda:0")
    fn(U(c["status"]), U(c["n_new"]), U(c["ik_params"]), U(c["ik_joints"]), t["track_params"], t["track_joints"], t["meta"],
       t["n_tracks"], t["next_id"], t["n_dead"], c["K"], n_inits=n_inits, slot_src=slot_src, overflow=overflow)
    return dict(params=t["track_params"], joints=t["track_joints"], meta=t["meta"], n_tracks=t["n_tracks"], next_id=t["next_id"],
                n_dead=t["n_dead"], slot_src=slot_src)


def _assert_tables(got, exp, what):
    """The tables up to n_tracks, the whole of the scalars and of slot_src (its -1 tail included)."""
    nt = exp["n_tracks"]
    assert np.array_equal(N(got["n_tracks"]), nt), what
    live = np.arange(exp["meta"].shape[1])[None, :] < nt[:, None]
    for key in ("params", "joints", "meta"):
        assert np.array_equal(N(got[key])[live], exp[key][live]), (what, key)
    for key in ("next_id", "n_dead", "slot_src"):
        assert np.array_equal(N(got[key]), exp[key]), (what, key)


@pytest.mark.parametrize("n_inits", [1, 3])
@pytest.mark.parametrize("name", list(tc.COMMIT_SHAPES))
def test_track_commit_vs_restatement(gpu, name, n_inits):
    dev, _ = gpu
    c, ref = tc.commit_case(name), tc.commit_reference(name, n_inits)
    _assert_tables(_commit(gpu, dev.track_commit, c, n_inits, None), ref, "no overflow word")
    ovf = torch.full((len(ref["overflow"]),), 4, dtype=torch.int32, device="cuda:0")
    _assert_tables(_commit(gpu, dev.track_commit, c, n_inits, ovf), ref, "overflow preset")
    assert np.array_equal(N(ovf), ref["overflow"] | 4)


def _multistep(gpu, name, assign, commit):
    """Six frames of assign -> stand-in solve -> commit on the device; the whole table against the restatement after every frame."""
    _, U = gpu
    C, P, T, K, V = tc.ASSIGN_SHAPES[tc.MULTI_SHAPES[name]]
    start, steps = tc.multistep(name)
    tab = {k: U(start[k]) for k in ("params", "joints", "meta", "n_tracks", "next_id", "n_dead", "overflow")}
    slot_src = torch.full((tc.B_CHAINS, T), 77, dtype=torch.int32, device="cuda:0")
    for k, s in enumerate(steps):
        out = assign(U(s["labels_sp"]), U(s["ncl_sp"]), U(s["labels_st"]), U(s["ncl_st"]), U(s["counts"]), U(s["frame_idx"]),
                     tab["n_tracks"], tab["params"], P, K, V, overflow=tab["overflow"])
        _assert_assign(out, s["assign"], T, f"frame {k}")
        commit(out[3], out[4], U(s["ik_params"]), U(s["ik_joints"]), tab["params"], tab["joints"], tab["meta"], tab["n_tracks"],
               tab["next_id"], tab["n_dead"], K, n_inits=3, slot_src=slot_src, overflow=tab["overflow"])
        _assert_tables(dict(tab, slot_src=slot_src), s["after"], f"frame {k}")
        assert np.array_equal(N(tab["overflow"]), s["after"]["overflow"]), k


@pytest.mark.parametrize("name", list(tc.MULTI_SHAPES))
def test_assign_solve_commit_over_six_frames(gpu, name):
    dev, _ = gpu
    _multistep(gpu, name, dev.track_assign, dev.track_commit)


# ------------------------------------------------------------------------------------------------------------------------------------
# the forms the chain kernels run, against the stand-alone kernels
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "limit"])
def test_workgroup_graph_forms_equal_the_stand_alone_kernel(gpu, name):
    """st_affinity_wave<256 | 512> with the 2-D / 2-D block computed in place, made ahead per pose pair (st_pose_pairs) and by line
    tables from staged keypoints (st_stage_keypoints + st_pose_pairs_lines): W, D (NaN positions included) and the group counts of
    mvmc_st_affinity, bit for bit.  'limit' is the 80-node graph of the big chain layout."""
    dev, _ = gpu
    c = tc.affinity_case(name)
    args = _affinity_args(gpu, name)
    W0, D0, gc0 = (N(t) for t in dev.st_affinity(*args, want_D=True, min_score=c["min_score"]))
    differ = []
    for nt_threads in (256, 512):
        for pair_form in (0, 1, 2):
            W, D, gc = (N(t) for t in dev.debug_st_affinity_wg(*args, nt_threads, pair_form, want_D=True, min_score=c["min_score"]))
            same = np.array_equal(gc, gc0) and np.array_equal(D, D0, equal_nan=True) and np.array_equal(W, W0)
            if not same:
                differ.append((nt_threads, pair_form, int((W != W0).sum()), float(np.nanmax(np.abs(D - D0)))))
    assert not differ, differ


@pytest.mark.parametrize("name", list(tc.ASSIGN_SHAPES))
def test_ballot_assignment_equals_the_one_thread_walk(gpu, name):
    """assign_chain on a 64-lane wave (graph node = lane, nodes 64 .. 79 in a second ballot word) against mvmc_track_assign: every
    output and the overflow word; with n_members, the counts and the rows [0, count) of the member table."""
    dev, _ = gpu
    c = tc.assign_case(name)
    B, T = c["track_params"].shape[:2]
    ovf0 = torch.full((B,), 4, dtype=torch.int32, device="cuda:0")
    ovf1, ovf2 = ovf0.clone(), ovf0.clone()
    ref = [N(t) for t in _assign(gpu, dev.track_assign, c, overflow=ovf0)]
    ref[2] = ref[2][:, :T]
    _assert_assign(_assign(gpu, dev.debug_track_assign_wave, c, overflow=ovf1), ref, T, "padded table")
    _assert_assign(_assign(gpu, dev.debug_track_assign_wave, c), ref, T, "no overflow word")
    out = _assign(gpu, dev.debug_track_assign_wave, c, overflow=ovf2, want_counts=True)
    _assert_assign((torch.from_numpy(ref[0]),) + tuple(out[1:5]), ref, T, "with counts")
    assert torch.equal(ovf1, ovf0) and torch.equal(ovf2, ovf0)
    mem, n_mem = N(out[0]), N(out[5])
    assert np.array_equal(n_mem, (ref[0] >= 0).sum(axis=2))
    valid = np.arange(c["V"])[None, None, :] < n_mem[:, :, None]
    assert np.array_equal(mem[valid], ref[0][valid])


@pytest.mark.parametrize("n_inits", [1, 3])
@pytest.mark.parametrize("name", list(tc.COMMIT_SHAPES))
def test_wave_commit_equals_the_one_thread_commit(gpu, name, n_inits):
    dev, _ = gpu
    c = tc.commit_case(name)
    B = len(c["n_new"])
    ovf0 = torch.full((B,), 4, dtype=torch.int32, device="cuda:0")
    ovf1 = ovf0.clone()
    ref = {k: N(v) for k, v in _commit(gpu, dev.track_commit, c, n_inits, ovf0).items()}
    _assert_tables(_commit(gpu, dev.debug_track_commit_wave, c, n_inits, ovf1), ref, "wave")
    assert torch.equal(ovf0, ovf1)
    _assert_tables(_commit(gpu, dev.debug_track_commit_wave, c, n_inits, None), ref, "wave, no overflow word")


@pytest.mark.parametrize("name", list(tc.MULTI_SHAPES))
def test_wave_forms_over_six_frames(gpu, name):
    dev, _ = gpu
    _multistep(gpu, name, dev.debug_track_assign_wave, dev.debug_track_commit_wave)


def test_wave_forms_refuse_what_the_ballot_words_cannot_hold(gpu):
    """t_max > 16, n_views p_max > 64 (cut64: 80 poses) and n_views > 16 are refused before any launch."""
    from multiview_motion_capture_amd._cabi import MvmcError
    dev, U = gpu
    with pytest.raises(MvmcError, match="status"):
        _assign(gpu, dev.debug_track_assign_wave, tc.assign_case("cut64"))
    z = lambda *s: torch.zeros(s, dtype=torch.int32, device="cuda:0")
    zd = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda:0")
    for C, P, T in ((3, 3, 17), (17, 1, 4)):
        with pytest.raises(MvmcError, match="status"):
            dev.debug_track_assign_wave(z(1, C * P), z(1), z(1, T + C * P), z(1), z(1, C), z(1), z(1), zd(1, T, 68), P, 2, 2)
    with pytest.raises(MvmcError, match="status"):
        dev.debug_track_commit_wave(z(1, 17), z(1), zd(1, 19, 68), zd(1, 19, 18, 3), zd(1, 17, 68), zd(1, 17, 18, 3), z(1, 17, 4), z(1), z(1),
                                    z(1), 2)
