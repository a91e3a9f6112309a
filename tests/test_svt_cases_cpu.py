"""CPU: the graphs of tests/svt_cases.py are what they claim to be.  The float64 restatement of the device's algorithm
(tests/svt_np.py, eigen form) agrees with oracle_np.match_svt (SVD form); the graphs admitted to the device gates
(tests/test_gpu_svt_small.py) have every decision clear of its threshold; and the admitted set covers every path the issue names."""
import numpy as np
import pytest

import svt_cases as sc
import svt_np

COVER = dict(neg_eig="a negative eigenvalue survives the threshold", mu_up="mu doubled", mu_down="mu halved",
             converged="converged before max_iter", max_iter="max_iter reached", tie="simplex projection with two equal entries",
             blk_early="a block stopped before round 10", blk_round10="a block ran round 10")


def _flags(nm, dtype=np.float64):
    rec = sc.restated(nm, dtype)[3]
    return dict({k: rec[k] for k in COVER if k != "max_iter"}, max_iter=not rec["converged"], tie_pos=rec["tie_pos"])


def test_restatement_agrees_with_the_oracle():
    """Call count and x_bin equal, max |dX| <= 1e-9, on every float64 graph whose own decisions are clear of their thresholds."""
    worst = (-1.0, "")
    for nm in sc.names():
        X, xb, calls, rec = sc.restated(nm)
        Xo, xbo, co = sc.oracle(nm)
        dx = float(np.abs(X - Xo).max())
        worst = max(worst, (dx, nm))
        if sc.clear(rec):
            assert calls == co and np.array_equal(xb, xbo) and dx <= sc.X_TOL, (nm, calls, co, dx)
            assert sc.agrees(nm)
    print(f"\nrestatement against oracle_np.match_svt: worst |dX| {worst[0]:.2e} ({worst[1]}) over {len(sc.names())} graphs")


@pytest.mark.parametrize("name", ["n2/0", "n5/2", "gaps/0", "ragged16/2", "degenerate/constant", "degenerate/round10"])
def test_block_projection_is_the_oracles(name):
    """The restatement's block loop reports its rounds; its result is oracle_np._proj2dpam's, bit for bit, on every block met."""
    X, xb, calls, _ = svt_np.match_svt(*sc.case(name), check=True)
    assert np.array_equal(X, sc.restated(name)[0]) and calls == sc.restated(name)[2]


def test_float32_input_is_cast_first():
    for nm in ("n7/0", "four9/1", "degenerate/twins"):
        s32, counts = sc.case_input(nm, np.float32)
        a, b = svt_np.match_svt(s32, counts), svt_np.match_svt(s32.astype(np.float64), counts)
        assert a[0].dtype == np.float64 and np.array_equal(a[0], b[0]) and a[2] == b[2]
    assert sc.restated("n7/2", np.float32) is sc.restated("n7/2")      # a quantised graph is exact in float32


def test_degenerate_graphs_are_what_they_claim():
    S, counts = sc.case("degenerate/twins")
    assert np.array_equal(S[0], S[1]) and np.array_equal(S[3], S[4]) and np.linalg.matrix_rank(S) == 2
    S, counts = sc.case("degenerate/constant")
    lv = np.linalg.eigvalsh(S)
    assert np.sum(np.abs(lv - lv[0]) < 1e-12) >= 2      # a repeated eigenvalue
    assert not sc.case("degenerate/zero")[0].any()
    assert sc.restated("degenerate/fast")[2] <= 3 and sc.restated("degenerate/fast")[3]["converged"]
    assert sc.restated("degenerate/round10")[3]["blk_round10"]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_admission_and_cover(dtype):
    adm = sc.admitted(dtype)
    print(f"\n{np.dtype(dtype).name} input: {len(adm)} of {len(sc.names())} graphs admitted")
    shapes = list(sc.SHAPES) + ["degenerate"]
    for s in shapes:
        mine = [nm for nm in sc.names() if sc.shape_of(nm) == s]
        out = [nm for nm in mine if nm not in adm]
        why = [(nm, "margin %.1e, |X - 0.5| %.1e, oracle %s" % (sc.restated(nm, dtype)[3]["margin"], sc.restated(nm, dtype)[3]["margin_half"],
                                                              sc.agrees(nm))) for nm in out]
        worst = min(min(sc.restated(nm, dtype)[3]["margin"], sc.restated(nm, dtype)[3]["margin_half"]) for nm in mine if nm in adm) if len(out) < len(mine) else 0
        print(f"  {s:13s} {str(sc.SHAPES.get(s, '')):40s} admitted {len(mine) - len(out)}, left out {len(out)}, smallest margin {worst:.1e} {why if why else ''}")
        if s != "degenerate":
            assert len(out) < len(mine), (s, why)
        else:
            assert not out, why        # the hand-built graphs have one instance each: none may fall out
    assert 10 * (len(sc.names()) - len(adm)) <= len(sc.names())
    for nm in adm:
        rec = sc.restated(nm, dtype)[3]
        assert rec["margin"] >= sc.MARGIN and rec["margin_half"] >= sc.MARGIN and sc.agrees(nm)
    print("  cover over the admitted graphs:")
    for k, what in list(COVER.items()) + [("tie_pos", "(two equal POSITIVE entries: not required)")]:
        hit = [nm for nm in adm if _flags(nm, dtype)[k]]
        print(f"    {what:45s} {len(hit):2d} graphs, e.g. {hit[:3]}")
        if k != "tie_pos":
            assert hit, what
    # at least one pair in every shape that has two non-empty groups
    for s, counts in sc.SHAPES.items():
        if sum(c > 0 for c in counts) >= 2:
            pairs = [int(sc.restated(nm, dtype)[1].sum() - sum(counts)) // 2 for nm in adm if sc.shape_of(nm) == s]
            assert max(pairs) >= 1, (s, pairs)
    # both instantiations and both parities of n are in the set
    assert any(max(sc.case(nm)[1]) <= 8 for nm in adm) and any(max(sc.case(nm)[1]) > 8 for nm in adm)
    assert {sum(sc.case(nm)[1]) for nm in adm} >= set(range(1, 10)) | {63, 64}
