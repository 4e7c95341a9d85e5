"""The random views of the lean and pair tile loops' sweep (tests/test_loop_sweep_host.py on the CPU model,
tests/test_gpu_loop_sweep.py on the GPU): sweep_view(seed) is built like seeded_view of tests/test_gpu_depth_seed.py
-- the same draws in the same order: camera scale K log-uniform over [0.05, 2.5], position noise, pitch, yaw, roll,
FOV -- from a generator of its own (9000 + seed) and at a frame size picked by the seed:

  72 x 40   9 tile columns: the last pair of each row has no B tile
  61 x 37   8 columns, the last 5 pixels wide; the bottom tile row 5 pixels high
  96 x 54   12 columns; the bottom row 6 pixels high
  33 x 70   5 columns, the last 1 pixel wide and without a B tile; 9 tile rows, the last 6 high
 136 x 72   17 columns, 9 rows: 81 pair units, 153 tiles
  24 x 16   3 columns, 2 rows
 120 x 9    15 columns, 2 rows, the second 1 pixel high
   8 x 8    one tile
  13 x 7    one pair with invalid lanes in both rays (A: 7 rows; B: 5 columns)
  17 x 64   3 columns, the last 1 pixel wide; 8 tile rows

sweep_reference(seed, variant): the oracle's frame of that view at the variant's LOD constant, computed once."""
import functools

import numpy as np

import sphereflake_amd as sf
from test_gpu_depth_seed import camera_view

SEEDS = range(64)
SIZES = [(72, 40), (61, 37), (96, 54), (33, 70), (136, 72), (24, 16), (120, 9), (8, 8), (13, 7), (17, 64)]
LOD = {"avx": 70.0, "sse": 60.0}


@functools.lru_cache(maxsize=None)
def sweep_view(seed):
    """((origin, tl, tr, bl), the oracle's setup, camera scale K, (W, H)) of view `seed`."""
    rng = np.random.default_rng(9000 + seed)
    W, H = SIZES[seed % len(SIZES)]
    cam = sf.Camera(W, H)
    K = float(np.exp(rng.uniform(np.log(0.05), np.log(2.5))))
    cam.SetPosition(np.asarray(sf.DEFAULT_CAMERA_POSITION, np.float32) * np.float32(K)
                    + rng.normal(0.0, 0.15 * K, 3).astype(np.float32))
    cam.SetPitch(np.float32(sf.DEFAULT_PITCH + rng.uniform(-0.4, 0.4)))
    cam.SetYaw(np.float32(sf.DEFAULT_YAW + rng.uniform(-0.6, 0.6)))
    cam.SetRoll(np.float32(rng.uniform(-0.3, 0.3)))
    cam.SetFOV(float(rng.choice([45.0, 60.0, 90.0])))
    view, setup = camera_view(cam)
    for a in setup.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return view, setup, K, (W, H)


DEEP = 7   # the overflow leg runs on the views of at least this depth
# The levels the overflow leg provisions, below DEEP - 1. A view of depth >= 7 has a node of depth 5 that expands for
# some ray (an ancestor of its deepest node), and with 5 levels the kernels enter no child of a node of depth 4: the
# unit that holds that ray flags itself for sf_fixup_wave's deeper re-trace.
OVERFLOW_LEVELS = 5


@functools.lru_cache(maxsize=None)
def sweep_reference(seed, variant="avx"):
    """The oracle's frame of sweep_view(seed) in `variant` ("avx": LOD 70, "sse": LOD 60), computed once, read-only."""
    from oracle import pyoracle
    ref = pyoracle.render(sweep_view(seed)[1], threads=8, lod=LOD[variant])
    for a in ref.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return ref
