"""CPU: live_smoothing.ReadBack, the one read-back of a live smoother's tick -- the parts come back by name in their registered shapes
with exact values, through one concatenation and one host copy; a name registered twice is an error."""
import numpy as np
import pytest
import torch

from multiview_motion_capture_amd.live_smoothing import ReadBack


def _parts(n=5):
    rng = np.random.default_rng(0)
    return {
        "info": torch.from_numpy(rng.normal(size=(n, 16))),                                    # float64 (n,16)
        "jcov": torch.from_numpy(rng.normal(size=(n, 18, 6))),                                 # float64 (n,18,6)
        "none": torch.zeros((0, 68), dtype=torch.float64),                                     # a zero-row part
        "members": torch.from_numpy(rng.integers(-1, 2 ** 31 - 1, (n, 3)).astype(np.int32)),   # int32, up to the largest
        "labels": torch.from_numpy(rng.integers(0, 2, (n, 2)).astype(np.uint8)),               # uint8
        "flags": torch.from_numpy(rng.integers(0, 2, (n,)).astype(bool)),                      # bool
        "anchors": torch.from_numpy(rng.normal(size=(n, 6))),                                  # registered under another shape
    }


def test_parts_come_back_by_name_with_their_shapes_and_exact_values():
    parts = _parts()
    rb = ReadBack()
    for name, t in parts.items():
        rb.add(name, t, (t.shape[0], 2, 3) if name == "anchors" else None)
    got = rb.fetch()
    assert list(got) == list(parts)
    for name, t in parts.items():
        shape = (5, 2, 3) if name == "anchors" else tuple(t.shape)
        assert got[name].dtype == np.float64 and got[name].shape == shape, name
        assert np.array_equal(got[name], t.numpy().astype(np.float64).reshape(shape)), name
    assert got["none"].shape == (0, 68) and got["members"].astype(np.int32).tolist() == parts["members"].tolist()
    assert ReadBack().fetch() == {}


def test_one_concatenation_and_one_host_copy(monkeypatch):
    calls = dict(cat=0, cpu=0)
    cat = torch.cat

    class OnDevice:      # stands for the concatenated device tensor: counts its copies to the host
        def __init__(self, t):
            self.t = t

        def cpu(self):
            calls["cpu"] += 1
            return self.t

    def counted(tensors, *a, **k):
        calls["cat"] += 1
        assert all(t.dtype == torch.float64 and t.dim() == 1 for t in tensors)
        return OnDevice(cat(tensors, *a, **k))
    monkeypatch.setattr(torch, "cat", counted)
    rb = ReadBack()
    parts = _parts()
    for name, t in parts.items():
        rb.add(name, t)
    got = rb.fetch()
    assert calls == dict(cat=1, cpu=1)
    assert np.array_equal(got["jcov"], parts["jcov"].numpy()) and np.array_equal(got["flags"] != 0, parts["flags"].numpy())


def test_a_name_registered_twice_is_an_error():
    rb = ReadBack()
    rb.add("rows", torch.zeros((2, 68), dtype=torch.float64))
    with pytest.raises(ValueError, match="registered twice"):
        rb.add("rows", torch.zeros((1, 68), dtype=torch.float64))
    assert list(rb.fetch()) == ["rows"]
