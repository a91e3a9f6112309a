"""bench.py host logic that needs no GPU: the multi-rank launcher must not leave ranks behind when one of them dies."""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_a_dead_rank_ends_the_whole_job_quickly():
    # `python bench.py --gpus 2` starts two child ranks.  Here there is no GPU (and on a one-GPU box rank 1 has no device): a rank fails at
    # torch.cuda.set_device.  The launcher has to notice, stop the other rank -- which would otherwise wait in the rendezvous for its
    # time-out -- and return a non-zero code.
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--frames", "64", "--steps", "1",
                        "--warmup", "0", "--cpu-frames", "0", "--sustain", "0"], capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode != 0
    assert "the other ranks were stopped" in r.stderr or "exited with code" in r.stderr
    assert r.stdout.strip() == ""            # no bench line from a failed job
    assert time.time() - t0 < 200


def test_kernel_source_hash_is_stable_and_sensitive():
    sys.path.insert(0, ROOT)
    import bench
    a = bench.kernel_sources_sha()
    assert a == bench.kernel_sources_sha() and len(a) == 16


def test_als_histogram_and_the_defaults_of_the_command_line():
    """The ALS iteration histogram of a bench line and the flags added in round 5."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    h = bench.als_histogram(np.array([[44, 140, 0], [205, 1000, 999]]))
    assert h["graphs"] == 5 and h["min"] == 44 and h["max"] == 1000 and h["share_at_the_1000_cap"] == 0.2
    assert sum(h["histogram"].values()) == 5 and h["histogram"]["1000"] == 1 and h["histogram"]["[500, 1000)"] == 1
    assert bench.als_histogram(np.zeros(4, dtype=np.int32)) is None
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0
    for flag in ("--force-collective", "--dlt-out", "--other-configs", "--frames-total", "--walk"):
        assert flag in r.stdout
    assert "--big-split" not in r.stdout                                    # (retired in round 6)
    # the strong-scaling form refuses a total that does not divide into whole chains per rank
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--frames-total", "1000"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode != 0 and "--frames-total" in r.stderr
    assert bench.OTHER_CONFIGS[-1][1][-2:] == ["--dlt-out", "f64"]           # config 2 with the reference's output dtype rides along
    assert bench.DEFAULT_NCCL_MAX_NCHANNELS == "4" and bench.OTHER_CONFIGS[1][1][:6] == ["--views", "8", "--people", "8", "--frames", "25008"]


def test_a_plain_run_times_the_headline_only_and_full_adds_the_records():
    """A plain command measures its headline figure and nothing else; --full restores every further record, and an option given
    explicitly holds either way."""
    sys.path.insert(0, ROOT)
    import bench
    records = lambda a: (a.full, a.sustain, a.host_io, a.cpu_frames, a.other_configs)
    assert records(bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5"])) == (False, 0, 0, 0, False)
    assert records(bench.parse_args(["--full"])) == (True, 300, 20, 1, True)
    assert records(bench.parse_args(["--full", "--views", "8", "--people", "8", "--frames", "25008"])) == (True, 300, 20, 1, False)
    assert records(bench.parse_args(["--full", "--sustain", "0", "--no-other-configs"])) == (True, 0, 20, 1, False)
    assert records(bench.parse_args(["--host-io", "5", "--other-configs"])) == (False, 0, 5, 0, True)
    r =subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--full" in r.stdout


def test_dump_outputs_writes_float_arrays_within_the_budget(tmp_path, monkeypatch):
    """--dump-outputs: every file float32 / float64, integer tables exact, and a step larger than the budget written as a fixed, seeded
    sample of frames (the same frames on every run) that keeps the files under DUMP_BYTES_MAX."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    F = 640
    per_frame = {"joints": torch.arange(F * 8 * 54, dtype=torch.float64).reshape(F, 8, 18, 3),
                 "meta": torch.arange(F * 8 * 4, dtype=torch.int32).reshape(F, 8, 4),
                 "pts3d": torch.ones((F * 2, 17, 4), dtype=torch.float32)}                 # (frames x people first: reshaped per frame)
    whole = {"next_id": torch.arange(F // 16, dtype=torch.int32)}
    bench.dump_outputs(str(tmp_path / "all"), per_frame, whole, F)
    got = {p.stem: np.load(p) for p in (tmp_path / "all").iterdir()}
    assert set(got) == {"joints", "meta", "pts3d", "next_id", "frame_index"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert np.array_equal(got["meta"], per_frame["meta"].numpy()) and got["pts3d"].shape == (F, 2, 17, 4)
    assert np.array_equal(got["frame_index"], np.arange(F))
    monkeypatch.setattr(bench, "DUMP_BYTES_MAX", 1_000_000)
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), per_frame, whole, F)
    size = sum(p.stat().st_size for p in (tmp_path / "a").iterdir())
    a, b = ({p.stem: np.load(p) for p in (tmp_path / r).iterdir()} for r in ("a", "b"))
    idx = a["frame_index"].astype(np.int64)
    assert size <= 1_000_000 and 0 < len(idx) < F and np.all(np.diff(idx) > 0)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert np.array_equal(a["joints"], per_frame["joints"].numpy()[idx])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--steps" in r.stderr
