"""GPU: the frames the reference and oracle tests use are the frames bench.py times.  bench.py runs one timed step with --dump-outputs;
its tables must be bit-identical to this test's own run of the chain kernel on tests/helpers.bench_step_data -- the function the scene
fixtures (tests/golden/synth_c*_scene_tracker.npz, oracle/gen_golden_scene.py) were recorded from.  A benchmark that timed other
frames, or a race between steps in flight (warm-up and timed steps share no buffers but one stream), would show here."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import bench_step_data

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("F,C,P,seed,extra", [(10000, 5, 4, 20260103, []),
                                              (25008, 8, 8, 20260104, ["--views", "8", "--people", "8", "--frames", "25008",
                                                                       "--seed", "20260104"])], ids=["config4", "config5"])
def test_the_benchmark_times_the_frames_of_bench_step_data(F, C, P, seed, extra, tmp_path):
    from multiview_motion_capture_amd.pipeline import HotPath
    from multiview_motion_capture_amd.tracker import check_chain_flags, run_chains_fused
    dump = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "1", "--sustain", "0",
                        "--host-io", "0", "--cpu-frames", "0", "--no-other-configs", "--dump-outputs", str(dump)] + extra,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    got = {k: np.load(dump / f"{k}.npy") for k in ("frame_index", "meta", "n_tracks", "joints", "params", "n_dead")}
    idx = got["frame_index"].astype(np.int64)
    assert np.array_equal(got["frame_index"], idx) and len(idx) > 0
    L = 16
    data = bench_step_data(F, C, P, seed, 0, L)
    d = torch.device("cuda:0")
    hp = HotPath(data["K"], data["Rt"], device=d)
    out = run_chains_fused(hp, torch.from_numpy(data["kps25"]).to(d), torch.from_numpy(data["counts"]).to(d), L)
    torch.cuda.synchronize()
    check_chain_flags(out)
    print(f"\nbench.py dumped {len(idx)} of {F} frames (C{C} P{P}, seed {seed})")
    for k in ("meta", "n_tracks", "joints", "params"):
        mine = out[k].cpu().numpy()[idx]
        mine = mine if mine.dtype in (np.float32, np.float64) else mine.astype(np.float64)
        assert got[k].shape == mine.shape, (k, got[k].shape, mine.shape)
        assert np.array_equal(got[k], mine, equal_nan=True), f"bench.py's {k} differ from the kernel's on bench_step_data"
    assert np.array_equal(got["n_dead"], out["n_dead"].cpu().numpy().astype(np.float64))
