"""CPU: the chain kernel's flag words as the Python side reads them (tracker.ChainFlags, after the comment of mvmcChainBuffers.flags in
include/mvmc.h), the one verdict every caller draws from them (tracker.void_verdict), and the one filler of the argument struct."""
import numpy as np
import pytest
import torch

from multiview_motion_capture_amd import _cabi
from multiview_motion_capture_amd.tracker import ChainFlags, fill_chain_buffers, void_verdict


def test_layout_of_three_chains_in_two_parts():
    B, parts = 3, 2
    assert ChainFlags.length(B, parts) == 17
    words = np.arange(100, 117, dtype=np.int32)
    for w in (words, torch.from_numpy(words.copy())):
        fl = ChainFlags(w, B)
        assert np.array_equal(np.asarray(fl.done), [100, 101, 102])
        assert (int(fl.timeout), int(fl.graph), int(fl.capacity)) == (103, 104, 105)
        assert np.array_equal(np.asarray(fl.status), [103, 104, 105])
        assert np.array_equal(np.asarray(fl.void), [107, 108, 109])
        assert int(fl.tickets) == 110
    fl = ChainFlags(words, B)
    fl.void[1] = 0                      # views, not copies
    assert words[8] == 0


@pytest.mark.parametrize("timeout, bits, kind, parts", [
    (0, 1, ValueError, ("capacity exceeded", "k_max")),
    (0, 2, ValueError, ("capacity exceeded", "t_max")),
    (0, 4, ValueError, ("graph",)),
    (0, 8, RuntimeError, ("IK waves", "void")),
    (0, 16, ValueError, ("rig index",)),
    (1, 0, RuntimeError, ("hand-over", "void")),
])
def test_each_word_alone(timeout, bits, kind, parts):
    exc = void_verdict(timeout, bits, 1, "caller")
    assert type(exc) is kind
    assert str(exc).startswith("caller: ") and all(p in str(exc) for p in parts)
    if bits in (1, 2):
        assert ("t_max" in str(exc)) == (bits == 2)


def test_nothing_set_is_no_verdict():
    assert void_verdict(0, 0, 0, "caller") is None


def test_precedence():
    assert "hand-over" in str(void_verdict(1, 31, 3, "c"))                          # the time-out over everything
    e = void_verdict(0, 8 | 16 | 4 | 3, 3, "c")
    assert type(e) is RuntimeError and "IK waves" in str(e)                         # 8 over 16
    e = void_verdict(0, 16 | 4 | 3, 3, "c")
    assert type(e) is ValueError and "rig index" in str(e)                          # 16 over 4
    e = void_verdict(0, 4 | 3, 3, "c")
    assert "graph" in str(e) and "capacity exceeded" not in str(e)                  # 4 over 1 | 2


def test_a_capacity_verdict_counts_the_void_chains():
    void = np.array([1, 0, 2], dtype=np.int32)
    e = void_verdict(0, int(np.bitwise_or.reduce(void)), int(np.count_nonzero(void)), "c")
    assert type(e) is ValueError and "capacity exceeded" in str(e) and "t_max" in str(e) and "k_max" in str(e)
    assert "2 chain(s)" in str(e)


def _complete():
    S = _cabi.MvmcChainBuffers
    ints = {name: 3 + i for i, name in enumerate(S._INTS)}
    tensors = {name: torch.zeros(4, dtype=torch.float64) for name in S._PTRS}
    return ints, tensors


def test_struct_filler_fills_every_field():
    ints, tensors = _complete()
    tensors["out_info"] = None
    buf = fill_chain_buffers(ints, tensors)
    for name in buf._INTS:
        assert getattr(buf, name) == ints[name], name
    for name in buf._PTRS:
        assert getattr(buf, name) == (None if tensors[name] is None else tensors[name].data_ptr()), name
    assert buf.out_info is None                                                      # None is the explicit NULL


@pytest.mark.parametrize("which", ["ints", "tensors"])
def test_struct_filler_refuses_a_missing_or_an_unknown_name(which):
    for change in ("missing", "unknown"):
        ints, tensors = _complete()
        d = ints if which == "ints" else tensors
        if change == "missing":
            d.pop(next(iter(d)))
        else:
            d["no_such_buffer"] = d[next(iter(d))]
        with pytest.raises(ValueError, match="a chain buffer is not named or not known"):
            fill_chain_buffers(ints, tensors)
