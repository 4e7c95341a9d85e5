"""bench.py end to end on the GPU: the plain run's line and --dump-outputs (one small run, shared by the tests)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

import bench

pytestmark = pytest.mark.gpu

W, H, K = 640, 360, 1.0      # BASELINE configs[0]: the smallest config, more than one tile row and 3600 tiles
STEPS, WARMUP = 6, 3


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    out = tmp_path_factory.mktemp("dump")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR",
                                                             "MASTER_PORT", "LOCAL_WORLD_SIZE")}
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", str(WARMUP), "--width", str(W), "--height", str(H), "--K", str(K),
                        "--settle-ms", "0", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=120, env=env, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0]), out


def test_plain_line_times_the_steps_only(plain_run):
    """A plain run prints the headline figure of its N timed steps and none of the legs behind --full."""
    line, _ = plain_run
    assert line["metric"] == bench.METRIC and line["unit"] == "Mrays/s" and line["dtype"] == "f32"
    assert line["higher_is_better"] is True and line["full"] is False
    assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["n_gpus"] == 1
    ms = line["ms_per_step"]
    assert ms > 0 and line["frame_ms"] == ms
    # value is W x H rays per ms_per_step (both rounded in the line: ms to 1e-4 ms, value to 0.01)
    assert ms > 1e-3
    assert abs(line["value"] - W * H / ms / 1e3) <= W * H / ms / 1e3 * (0.5e-4 / (ms - 0.5e-4)) + 0.01
    for key in ("check", "cpu_baseline", "fixed_camera", "pipeline", "frame_latency_ms", "first_render_ms",
                "configs", "member_shares", "post", "d2h", "frameless"):
        assert key not in line, key


def test_dump_is_the_last_timed_frame(plain_run):
    """--dump-outputs: float32 position / normal of the last timed frame (frame WARMUP + STEPS - 1 of the camera
    path), every row of this small frame, bit for bit the oracle's."""
    line, out = plain_run
    assert sorted(os.listdir(out)) == ["normal.npy", "position.npy", "rows.npy"]
    pos, nrm, rows = (np.load(os.path.join(out, n + ".npy")) for n in ("position", "normal", "rows"))
    assert pos.dtype == nrm.dtype == np.float32 and rows.dtype == np.float64
    assert pos.shape == nrm.shape == (H, W, 4) and np.array_equal(rows, np.arange(H))
    assert line["dump_outputs"]["rows"] == H
    assert pos.nbytes + nrm.nbytes + rows.nbytes <= 64 * 10 ** 6
    view = bench.frame_camera(W, H, K, WARMUP + STEPS - 1).corners()
    check = np.linspace(0, H - 1, 12).astype(int)
    assert bench.check_oracle_rows(pos, nrm, view, W, H, check)
    other = bench.frame_camera(W, H, K, WARMUP + STEPS - 2).corners()   # (the check tells neighbouring frames apart)
    assert not bench.check_oracle_rows(pos, nrm, other, W, H, check)
