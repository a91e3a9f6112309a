"""CPU: the live session pool's host side (multiview_motion_capture_amd/live.py) and its C entry point, mvmc_chain_run_sessions --
what can be checked without a GPU: the declaration, export and binding, the argument errors the launcher reports before any HIP call,
and the pool's input checks, which raise before any device work."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chain_run_sessions_is_declared_exported_and_bound():
    from multiview_motion_capture_amd import _cabi
    header = open(os.path.join(ROOT, "include", "mvmc.h")).read()
    m = re.search(r"int\s+mvmc_chain_run_sessions\s*\(([^)]*)\)", header)
    assert m, "mvmc_chain_run_sessions is not declared in include/mvmc.h"
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1)).split(",")]
    assert len(args) == 6
    assert "int32_t*" in args[2].replace(" ", "") and args[3].startswith("int ") and "uint8_t*" in args[4].replace(" ", "")
    assert "mvmc_chain_run_sessions" in _cabi.SYMBOLS
    lib = _cabi.load()
    fn = lib.mvmc_chain_run_sessions          # AttributeError if the library does not export it
    assert fn.argtypes[2] is ctypes.c_void_p and fn.argtypes[3] is ctypes.c_int and fn.argtypes[4] is ctypes.c_void_p
    assert fn.restype is ctypes.c_int
    # the ABI stays where it was: the struct and the version are those of the multi-rig entry point
    assert _cabi.MVMC_ABI == 6 and len(_cabi.MvmcChainBuffers._INTS) == 14


def _buffers(n_parts):
    """A struct that passes every other check of the launcher, with fake pointers (never dereferenced: the call must refuse first)."""
    from multiview_motion_capture_amd import _cabi
    buf = _cabi.MvmcChainBuffers()
    for name, v in dict(n_chains=4, chain_len=2, n_views=5, p_max=4, t_max=8, k_max=10, v_max=20, max_nfev_cold=50, max_nfev_warm=5,
                        n_inits=3, seed_len=6400, n_parts=n_parts, force_big=0, hand_over=0).items():
        setattr(buf, name, v)
    for k, name in enumerate(_cabi.MvmcChainBuffers._PTRS):
        setattr(buf, name, 0x1000 * (k + 1))
    return buf


def test_chain_run_sessions_argument_errors_come_before_any_hip_call():
    from multiview_motion_capture_amd import _cabi
    fn = _cabi.load().mvmc_chain_run_sessions
    sk = _cabi.MvmcSkeleton()
    fake_active = ctypes.c_void_p(0xdead0000)
    buf = _buffers(n_parts=2)
    assert fn(None, ctypes.byref(buf), None, 1, None, None) == 1                   # NULL skeleton
    assert fn(ctypes.byref(sk), None, None, 1, None, None) == 1                    # NULL buffers
    assert fn(ctypes.byref(sk), None, None, 1, fake_active, None) == 1
    assert fn(ctypes.byref(sk), ctypes.byref(buf), None, 0, None, None) == 1       # n_rigs < 1
    assert fn(ctypes.byref(sk), ctypes.byref(buf), None, 2, None, None) == 1       # no rig_of_chain with two rigs
    # idle chains need one workgroup per chain: an idle chain's part 0 would never hand over to its successors
    assert fn(ctypes.byref(sk), ctypes.byref(buf), None, 1, fake_active, None) == 1
    assert fn(ctypes.byref(sk), ctypes.byref(buf), ctypes.c_void_p(0xbeef0000), 4, fake_active, None) == 1


def test_open_checks():
    from multiview_motion_capture_amd.live import check_open
    check_open(0, 4, 5, 5)
    check_open(3, 4, 5, 5)
    with pytest.raises(ValueError, match="4 cameras, the pool's sessions have 5"):
        check_open(0, 4, 5, 4)
    with pytest.raises(ValueError, match="all 4 session slots are taken"):
        check_open(4, 4, 5, 5)


def test_tick_checks_name_every_bad_input():
    from multiview_motion_capture_amd.live import check_tick
    open_sids = {0, 1, 7}
    ok = [1, 2, 0, 3, 4]
    check_tick(open_sids, 5, 4, [], [])
    check_tick(open_sids, 5, 4, [0, 7], [ok, [4, 4, 4, 4, 4]])
    with pytest.raises(ValueError, match="no open session 3"):
        check_tick(open_sids, 5, 4, [0, 3], [ok, ok])
    with pytest.raises(ValueError, match="session 1's frame has 4 views, the pool's sessions have 5"):
        check_tick(open_sids, 5, 4, [0, 1], [ok, ok[:4]])
    with pytest.raises(ValueError, match="session 7: more than p_max=4 people in view 2"):
        check_tick(open_sids, 5, 4, [7], [[0, 1, 5, 0, 0]])
    with pytest.raises(ValueError, match="session 0 is named twice"):
        check_tick(open_sids, 5, 4, [0, 1, 0], [ok, ok, ok])
    with pytest.raises(ValueError, match="2 sessions, 1 frames"):
        check_tick(open_sids, 5, 4, [0, 1], [ok])


def test_live_session_error_names_the_failed_sessions():
    from multiview_motion_capture_amd.live import LiveSessionError
    e = LiveSessionError({3: ValueError("more than t_max live tracklets"), 1: RuntimeError("x")})
    assert set(e.errors) == {1, 3} and isinstance(e.errors[3], ValueError)
    assert str(e).index("1: x") < str(e).index("3: more than t_max")
