"""GPU: the single-wave Householder tridiagonalisation with its row operands by DPP against the same routine with LDS broadcasts.

eightri::tridiag_krylov_w1<N, DPP> (csrc/mvmc_tri_w1.h) takes the row-side values v_i, w_i of a Householder step either as DPP row
broadcasts from replicated registers (the shipped form) or as LDS broadcasts (DPP = false).  Both make the same multiply-adds in the
same order, so everything the IK's model step reads afterwards must agree BIT FOR BIT: d, e, tau, v0, out4, the return value, the
number of steps, the per-lane scv / tauv and the packed reflectors of every lane (mvmc_debug_tridiag_w1, one wave per problem; not
part of include/mvmc.h).

The problems are the smallest at which the DPP form can go wrong -- a wrong lane immediate or row group shows at the boundaries of the
rows of 16 lanes, a wrong execution mask or chunk skip where rows die:
  * N = 30, 40, 50 (the three instances), J^T J = A^T A of random A, fixed seed;
  * full rank (every pivot lane 1 .. N - 1, so 15, 16, 31, 32, 47 and 48 are all crossed);
  * an active size n below N: N - 1, and 17 / 16 / 33 (a row group of 16 partly and wholly dead);
  * a null space, so that the clean collapse (0 < return < n) is hit early and late and AT pivot lanes 15, 16, 17, 31, 32, 33, 47, 48;
  * a block-diagonal matrix with the gradient inside the first block: the Krylov space ends in front of a block that is not null
    (return -1) and the plain Householder steps run on;
  * a gradient along e_0: tau = 0 on the first reflector, whose two-sided update is skipped.
That each kind does what its name says is asserted on the LDS form's results, and on the full-rank problems the tridiagonal matrix
must have the eigenvalues of the input (1e-10 of the largest: an orthogonal similarity in double precision), so that two forms which
were wrong in the same way would not pass.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _gram(rng, n, rank):
    A = rng.standard_normal((rank, n))
    return A.T @ A, A


def _pad(M, g, N):
    n = M.shape[0]
    Mp = np.zeros((N, N)); Mp[:n, :n] = M
    gp = np.zeros(N); gp[:n] = g
    return Mp, gp


def problems(N):
    """-> list of (kind, n, M (N, N), g (N,)); kind in full / small / null / unclean / tau0"""
    rng = np.random.RandomState(20260107 + N)
    out = []
    for _ in range(2):
        M, A = _gram(rng, N, N + 8)
        out.append(("full", N, M, A.T @ rng.standard_normal(N + 8)))
    for n in [m for m in (16, 17, 33, N - 1) if m < N]:
        M, A = _gram(rng, n, n + 8)
        out.append(("small", n) + _pad(M, A.T @ rng.standard_normal(n + 8), N))
    for rank in (3, 15, 16, 17, 31, 32, 33, 47, 48, N - 3):
        if rank <= N - 3:
            M, A = _gram(rng, N, rank)
            out.append(("null", N, M, A.T @ rng.standard_normal(rank)))   # g in range(M): the Krylov space has `rank` dimensions
    M, A = _gram(rng, N - 1, 16)                                           # the same below the full size: rows 16 .. N - 2 null, row N - 1 dead
    out.append(("null", N - 1) + _pad(M, A.T @ rng.standard_normal(16), N))
    for m in (6, 16):
        M1, A1 = _gram(rng, m, m + 4)
        M2, _ = _gram(rng, N - m, N - m + 4)
        M = np.zeros((N, N)); M[:m, :m] = M1; M[m:, m:] = M2
        g = np.zeros(N); g[:m] = A1.T @ rng.standard_normal(m + 4)
        out.append(("unclean", N, M, g))
    M, _ = _gram(rng, N, N + 8)
    g = np.zeros(N); g[0] = -1.7
    out.append(("tau0", N, M, g))
    return out


def _run(N, probs, dpp):
    from multiview_motion_capture_amd import _cabi
    from multiview_motion_capture_amd.device import _p, _stream, check
    fn = _cabi.load().mvmc_debug_tridiag_w1
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    B, H = len(probs), (N - 2) // 2
    dev = torch.device("cuda")
    A = torch.from_numpy(np.stack([p[2] for p in probs])).to(dev).contiguous()
    g = torch.from_numpy(np.stack([p[3] for p in probs])).to(dev).contiguous()
    na = torch.tensor([p[1] for p in probs], dtype=torch.int32, device=dev)
    vec = torch.full((B, 6, 64), np.nan, dtype=torch.float64, device=dev)
    out4 = torch.full((B, 4), np.nan, dtype=torch.float64, device=dev)
    ret = torch.full((B, 2), -99, dtype=torch.int32, device=dev)
    pk = torch.full((B, H, 64), np.nan, dtype=torch.float64, device=dev)
    check(fn(_p(A), _p(g), _p(na), B, N, int(dpp), _p(vec), _p(out4), _p(ret), _p(pk), _stream()), "mvmc_debug_tridiag_w1")
    torch.cuda.synchronize()
    return {"vec": vec.cpu().numpy(), "out4": out4.cpu().numpy(), "ret": ret.cpu().numpy(), "pk": pk.cpu().numpy()}


@pytest.mark.parametrize("N", [30, 40, 50])
def test_dpp_row_operands_are_bit_identical_to_lds_broadcasts(N):
    probs = problems(N)
    ref, new = _run(N, probs, False), _run(N, probs, True)
    # the problems do what they were built for (LDS form)
    for b, (kind, n, M, g) in enumerate(probs):
        kk, ksteps = int(ref["ret"][b, 0]), int(ref["ret"][b, 1])
        d, e = ref["vec"][b, 0], ref["vec"][b, 1]
        assert np.isfinite(ref["vec"][b]).all() and np.isfinite(ref["pk"][b]).all() and np.isfinite(ref["out4"][b]).all(), (N, b, kind)
        if kind in ("full", "small", "tau0"):
            assert kk == n and ksteps == n - 1, (N, b, kind, n, kk, ksteps)
            T = np.diag(d[:n]) + np.diag(e[:n - 1], 1) + np.diag(e[:n - 1], -1)
            lam, lam_t = np.linalg.eigvalsh(M[:n, :n]), np.linalg.eigvalsh(T)
            assert np.abs(lam - lam_t).max() <= 1e-10 * lam[-1], (N, b, kind, np.abs(lam - lam_t).max() / lam[-1])
        if kind == "tau0":
            assert ref["out4"][b, 1] == 0.0 and ref["out4"][b, 0] == g[0], (N, b, ref["out4"][b])
        else:
            assert ref["out4"][b, 1] != 0.0, (N, b, kind)
        if kind == "null":
            rank = np.linalg.matrix_rank(M)
            # the range block, then the null one (a sub-diagonal entry that is small but above the 1e-8 threshold one step earlier
            # can move the split by one: seen in a NumPy restatement at N = 50, rank 17)
            assert 0 < kk < n and abs(kk - rank) <= 1 and ksteps == kk, (N, b, n, rank, kk, ksteps)
        if kind == "unclean":
            assert kk == -1 and ksteps == n - 1, (N, b, kk, ksteps)
    kinds = [p[0] for p in probs]
    assert {"full", "small", "null", "unclean", "tau0"} == set(kinds)
    # bit for bit
    for key in ("ret", "out4", "vec", "pk"):
        same = np.array_equal(ref[key], new[key])
        if not same:
            bad = sorted({int(i) for i in np.argwhere(ref[key] != new[key])[:, 0]})
            pytest.fail(f"N = {N}: {key} differs between the DPP and the LDS form on problems {[(b, kinds[b], probs[b][1]) for b in bad]}")
