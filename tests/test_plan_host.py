"""CPU: the render schedule (sphereflake-raytracer_amd/csrc/sf_plan.h), checked without a GPU. The header is plain
C++ -- tests/cpp/plan_probe.cpp includes nothing else -- so the probe runs the very function launch() and
sf_render_frames call, render after render, carrying the order state as they do.

The expectations are the schedule's rules worked by hand for 256 CUs, 8 XCD queue groups of 4 queues, one wave per
block, and 32 / 32 / 28 resident blocks per CU of the general, lean and pair kernels (grids of 8 192, 8 192 and 7 168
waves), default knobs and a fresh context:

  pairs       where a plain whole frame has more tiles than 2 x max(8192, 7168), or SF_PAIR=1
  small       units <= 2 x grid;  tiny: 2 x units <= grid;  large: not small   (whole frames only)
  order       tiny or large (SF_ORDER overrides); splits auto, but 0 for pairs and for large frames
  grid        min(the kernel's full grid, ceil(units_max / waves per block), SF_MAX_BLOCKS)
  queues      groups halved until <= grid; x 4 per group from 64 waves per queue
  rebuild     no order of these units yet, or every 3rd render (small) / 64th (large) / SF_ORDER_EVERY
  costs       by every render unless large (SF_ORDER_RECORD overrides), and by a rebuilding one
  lean loop   a plain launch whose schedule has no part units and records no costs; pairs count as lean
"""
import pathlib
import shutil
import subprocess

import pytest

import sphereflake_amd as sf

REPO = pathlib.Path(__file__).resolve().parent.parent
CSRC = REPO / "sphereflake-raytracer_amd" / "csrc"


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path_factory.mktemp("plan") / "plan_probe"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", f"-I{CSRC}", str(REPO / "tests" / "cpp" / "plan_probe.cpp"),
                        "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr[-3000:]   # (-Wall: no warning either)
    return exe


def launch(kernel, units, grid, queues, order, costs, splits, flags="0"):
    return f"{kernel}:{units}:grid={grid}:{queues}:order={order}:costs={costs}:splits={splits}:flags={flags}"


def line(name, launches, rebuild, orders, lean, pair):
    runs = ",".join(f"{what}*{n}" for what, n in launches)
    return f"{name} | {runs} | rebuild={rebuild} | orders={orders} | lean={lean} pair={pair}"


def ordered(name, kernel, units, grid, queues, splits, renders, rebuild, orders, lean=0, pair=0):
    """A case whose every render records costs on one kernel: the first finds no order, the others read one."""
    return line(name, [(launch(kernel, units, grid, queues, "none", 1, splits), 1),
                       (launch(kernel, units, grid, queues, "read", 1, splits), renders - 1)], rebuild, orders, lean, pair)


def periodic(name, units, grid, queues, rebuilding, steady, renders, rebuild, orders, lean, pair):
    """Costs only on the rebuilding renders (1 and 1 + period), which take `rebuilding`; `steady` between."""
    first, second = (int(v) for v in rebuild.split(","))
    return line(name, [(launch(rebuilding, units, grid, queues, "none", 1, 0), 1),
                       (launch(steady, units, grid, queues, "read", 0, 0), second - first - 1),
                       (launch(rebuilding, units, grid, queues, "read", 1, 0), 1),
                       (launch(steady, units, grid, queues, "read", 0, 0), renders - second)], rebuild, orders, lean, pair)


Q1, Q1C, Q1T, Q1G, Q2, FR = ("sf_trace_queue1", "sf_trace_queue1c", "sf_trace_queue1t", "sf_trace_queue1g",
                             "sf_trace_queue2", "sf_trace_frames1")
ONCE = "SF_ORDER=1 SF_SPLIT_BUCKETS=0 SF_ORDER_RECORD=0"

EXPECTED = [
    # the frame sizes (66 renders where the 64-render period matters)
    periodic("1920x1080", "16200pairs", 7168, "8/32", Q1C, Q1, 66, "1,65", "16200p*66", 66, 66),
    line("1280x720", [(launch(Q1T, "14400tiles", 8192, "8/32", "no", 0, -1), 66)], "-", "0t*66", 66, 0),
    ordered("640x360", Q1G, "3600tiles", 8192, "8/32", -1, 7, "1,4,7", "3600t*7"),
    line("1080p share 0/8", [(launch(Q1G, "4080tiles", 4080, "8/32", "no", 0, -1), 66)], "-", "0t*66", 0, 0),
    ordered("96x64", Q1G, "96tiles", 384, "8/8", -1, 5, "1,4", "96t*5"),
    line("16x8 SF_ORDER=0", [(launch(Q1T, "2tiles", 2, "2/2", "no", 0, -1), 5)], "-", "0t*5", 5, 0),
    periodic("1920x1080 x4", "32400tiles", 8192, "8/32", FR, FR, 66, "1,65", "32400t*66", 0, 0),
    # the knobs the GPU tests rely on, at the two smallest sizes
    ordered("96x64 SF_PAIR=1", Q1C, "48pairs", 48, "8/8", 0, 5, "1,4", "48p*5", 5, 5),
    ordered("16x8 SF_PAIR=1", Q1C, "1pairs", 1, "1/1", 0, 5, "1,4", "1p*5", 5, 5),
    line("16x8 SF_PAIR=1 SF_ORDER=0", [(launch(Q1, "1pairs", 1, "1/1", "no", 0, 0), 5)], "-", "0t*5", 5, 5),
    ordered("96x64 SF_PAIR=0", Q1G, "96tiles", 384, "8/8", -1, 5, "1,4", "96t*5"),
    ordered("16x8 SF_PAIR=0", Q1G, "2tiles", 8, "8/8", -1, 5, "1,4", "2t*5"),
    ordered("96x64 SF_LEAN=0", Q1G, "96tiles", 384, "8/8", -1, 5, "1,4", "96t*5"),
    line("16x8 SF_LEAN=0 SF_ORDER=0", [(launch(Q1G, "2tiles", 2, "2/2", "no", 0, -1), 5)], "-", "0t*5", 0, 0),
    # render 1 general (it rebuilds), renders 2 and 3 lean, render 4 rebuilds again
    periodic(f"96x64 {ONCE}", "96tiles", 96, "8/8", Q1G, Q1T, 5, "1,4", "96t*5", 3, 0),
    periodic(f"16x8 {ONCE}", "2tiles", 2, "2/2", Q1G, Q1T, 5, "1,4", "2t*5", 3, 0),
    # halves are a row-major schedule: under the order a tiny frame takes by default they do not apply
    ordered("96x64 SF_HALVES=1", Q1G, "96tiles", 384, "8/8", -1, 5, "1,4", "96t*5"),
    line("96x64 SF_HALVES=1 SF_ORDER=0", [(launch(Q1G, "96tiles", 192, "8/8", "no", 0, -1, "0x4000"), 5)], "-", "0t*5", 0, 0),
    line("16x8 SF_HALVES=1 SF_ORDER=0", [(launch(Q1G, "2tiles", 4, "4/4", "no", 0, -1, "0x4000"), 5)], "-", "0t*5", 0, 0),
    ordered("96x64 SF_MAX_BLOCKS=3", Q1G, "96tiles", 3, "2/2", -1, 5, "1,4", "96t*5"),
    ordered("16x8 SF_MAX_BLOCKS=1", Q1G, "2tiles", 1, "1/1", -1, 5, "1,4", "2t*5"),
    ordered("96x64 SF_TRACE_WAVES=2", Q2, "96tiles", 192, "8/8", -1, 5, "1,4", "96t*5"),
    ordered("16x8 SF_TRACE_WAVES=2", Q2, "2tiles", 4, "4/4", -1, 5, "1,4", "2t*5"),
    # one tile column: 2 pairs, 2 tiles. launch, frames x2, frames x2, launch, launch under a 64-render period: only
    # an order of the other kind of units makes renders 2 and 4 rebuild
    line("8x16 SF_PAIR=1 SF_ORDER=1 SF_ORDER_EVERY=64",
         [(launch(Q1C, "2pairs", 2, "2/2", "none", 1, 0), 1), (launch(FR, "2tiles", 16, "8/8", "none", 1, -1), 1),
          (launch(FR, "2tiles", 16, "8/8", "read", 1, -1), 1), (launch(Q1C, "2pairs", 2, "2/2", "none", 1, 0), 1),
          (launch(Q1C, "2pairs", 2, "2/2", "read", 1, 0), 1)], "1,2,4", "2p*1,2t*2,2p*2", 3, 3),
    # tests/test_gpu_frames.py::test_frames_alternate_with_pair_launches: launch, frames x2, launch
    line("40x16 SF_PAIR=1 SF_ORDER=1 SF_ORDER_EVERY=1",
         [(launch(Q1C, "6pairs", 6, "4/4", "none", 1, 0), 1), (launch(FR, "10tiles", 80, "8/8", "none", 1, -1), 1),
          (launch(Q1C, "6pairs", 6, "4/4", "none", 1, 0), 1)], "1,2,3", "6p*1,10t*1,6p*1", 2, 2),
    # 2^27 tiles: 3 frames in one launch stay below 2^29 unit positions, 4 are refused
    line("131072x65536 x3 x4", [(launch(FR, "134217728tiles", 8192, "8/32", "none", 1, 0), 1), ("refused", 1)],
         "1", "134217728t*1,-*1", 0, 0),
]


def test_schedule_cases(probe):
    got = subprocess.run([str(probe)], capture_output=True, text=True, timeout=60, check=True).stdout.splitlines()
    names = [g.split(" | ")[0] for g in got]
    assert names == [e.split(" | ")[0] for e in EXPECTED]
    for g, e in zip(got, EXPECTED):
        assert g == e


@pytest.mark.parametrize("H,band,n", [(1080, 8, 8), (1080, 64, 3), (45, 8, 2), (7, 8, 4), (16384, 8, 8)])
def test_band_share_equals_slab_rows(probe, H, band, n):
    """test_host.py::test_slab_rows_partition_frame's cases: each member's pixel rows are sf_slab_rows', and the
    members' tile rows sum to the frame's."""
    sf.build()
    out = subprocess.run([str(probe), "share", str(H), str(band), str(n)], capture_output=True, text=True, timeout=60,
                         check=True).stdout.split()
    member, tile_rows, rows = (list(map(int, out[k::3])) for k in range(3))
    assert member == list(range(n))
    assert rows == [sf.lib().sf_slab_rows(H, band, n, i) for i in range(n)]
    assert sum(rows) == H
    assert sum(tile_rows) == (H + 7) // 8


def test_band_share_defaults(probe):
    """0 for band_rows and band_count: one member owns the whole frame, as sf_slab_rows(H, 0, 0, 0) says."""
    out = subprocess.run([str(probe), "share", "45", "0", "0"], capture_output=True, text=True, timeout=60, check=True)
    assert out.stdout.split() == ["0", "6", "45"]
    sf.build()
    assert sf.lib().sf_slab_rows(45, 0, 0, 0) == 45
