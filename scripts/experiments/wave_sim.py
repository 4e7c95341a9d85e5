#!/usr/bin/env python3
"""Drive wave_sim.c: the product kernel's wave-coherent traversal modelled on the CPU, its work counted per depth
(experiment, not product). Usage: [WAVE_UNIT=16x8] wave_sim.py [setup=c3] [tile_step=1] [mode=0 ...]
WAVE_UNIT: the pixels a wave traces, TWxTH (default 8x8, one tile; 16x8 or 8x16: the pair unit), at most 128 lanes.
WAVE_SIM_DIR: where the model's library is built (default: the system's temporary directory)."""
import ctypes
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "oracle"))
import pyoracle  # noqa: E402

TW, TH = (int(v) for v in os.environ.get("WAVE_UNIT", "8x8").split("x"))
SO = os.path.join(os.environ.get("WAVE_SIM_DIR") or tempfile.gettempdir(), f"wave_sim_{TW}x{TH}.so")
subprocess.check_call(["gcc", "-O2", "-mno-fma", "-ffp-contract=off", f"-DTW={TW}", f"-DTH={TH}", "-shared", "-fPIC", "-o", SO,
                       os.path.join(HERE, "wave_sim.c"), "-lm"])
L = ctypes.CDLL(SO)
NST = 32
FIELDS = ["exp", "iter", "miss", "lodnone", "occlnone", "entered", "leaf", "push", "act", "hitl"]
TAIL = ["tiles", "mismatch", "ties", "maxd"]
EXTRA = ["cone_tested", "cone_culled", "skip_exp", "skip_lost", "cache_hit", "half_exp", "half_iter", "fold_exp", "fold_iter",
         "root_a", "root_b", "root_d", "side_iter", "side_lod",
         "lf_node", "lf_iter", "lf_hit", "lf_ent", "lf_own", "lf_ent_own", "lf_old", "lf_two", "lf_mixed", "lf_empty"]


class Stats(ctypes.Structure):
    _fields_ = [(f, ctypes.c_longlong * NST) for f in FIELDS] + [(f, ctypes.c_longlong) for f in TAIL] + \
               [(f, ctypes.c_longlong * NST) for f in EXTRA]


fp = ctypes.POINTER(ctypes.c_float)
up = ctypes.POINTER(ctypes.c_uint32)
L.wsim_tiles.argtypes = [ctypes.c_uint32, ctypes.c_uint32, fp, fp, fp, fp, fp, fp, up, fp, ctypes.c_uint32,
                         ctypes.c_uint32, ctypes.c_int, fp, up, ctypes.POINTER(Stats), ctypes.c_int, ctypes.c_int,
                         ctypes.POINTER(ctypes.c_double)]
L.wsim_depth8.argtypes = [ctypes.c_float, fp]


def run(name="c3", tile_step=1, mode=0, check=True, split=(0, 0)):
    s = name if isinstance(name, dict) else pyoracle.load_setup(name)   # (a setup of the caller's own, or a fixture's)
    W, H = int(s["W"]), int(s["H"])
    lut = np.ascontiguousarray(pyoracle.load_lut(), np.uint32)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    o, tl, tr, bl, root, child = (f32(s[k]) for k in ("origin", "tl", "tr", "bl", "root", "children"))
    child = child.reshape(-1)
    d8 = np.zeros(NST * 8, np.float32)
    L.wsim_depth8(70.0, d8.ctypes.data_as(fp))
    tw, th = (W + TW - 1) // TW, (H + TH - 1) // TH   # units per row, unit rows
    trows = list(range(0, th, tile_step))
    ref_m = ref_i = None
    if check:
        rows = np.arange(H)
        ref = pyoracle.render(s, rows=rows)
        ref_m = np.ascontiguousarray(ref["minT"], np.float32)
        ref_i = np.ascontiguousarray(ref["index"], np.uint32)
    parts = [Stats() for _ in trows]
    works = [np.zeros(3 * tw) for _ in trows]

    def work(k):
        ty = trows[k]
        L.wsim_tiles(W, H, o.ctypes.data_as(fp), tl.ctypes.data_as(fp), tr.ctypes.data_as(fp), bl.ctypes.data_as(fp),
                     root.ctypes.data_as(fp), child.ctypes.data_as(fp), lut.ctypes.data_as(up), d8.ctypes.data_as(fp),
                     ty * tw, (ty + 1) * tw, mode,
                     ref_m.ctypes.data_as(fp) if check else None, ref_i.ctypes.data_as(up) if check else None,
                     ctypes.byref(parts[k]), split[0], split[1], works[k].ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    with ThreadPoolExecutor(8) as ex:
        list(ex.map(work, range(len(trows))))
    tot = {f: np.sum([np.array(getattr(p, f)[:]) for p in parts], 0) for f in FIELDS + EXTRA}
    for f in TAIL:
        tot[f] = max(getattr(p, f) for p in parts) if f == "maxd" else sum(getattr(p, f) for p in parts)
    tot["scale"] = tile_step
    tot["tile_work"] = np.concatenate(works).reshape(-1, 3)
    return tot


def report(t, label=""):
    sc = t["scale"]
    print(f"{label} tiles {t['tiles']} mismatch {t['mismatch']} ties {t['ties']} maxd {t['maxd']} (x{sc} for frame)")
    print(" d   exp     iter    miss   lodnone occlnone entered  leaf    push   act/it  cone-cull skip-exp lost")
    for d in range(NST):
        if t["exp"][d] == 0:
            continue
        it = t["iter"][d]
        print(f"{d:2d} {t['exp'][d]*sc:7d} {it*sc:8d} {t['miss'][d]*sc:7d} {t['lodnone'][d]*sc:7d} {t['occlnone'][d]*sc:7d}"
              f" {t['entered'][d]*sc:7d} {t['leaf'][d]*sc:7d} {t['push'][d]*sc:7d} {t['act'][d]/max(it,1):6.1f}"
              f"  {t['cone_culled'][d]/max(t['cone_tested'][d],1):.3f}  {t['skip_exp'][d]*sc:7d} {t['skip_lost'][d]*sc:6d}"
              f"  hit {t['cache_hit'][d]/max(t['exp'][d],1):.2f}")
    tot = lambda f: int(t[f].sum()) * sc
    print(f"all {tot('exp'):8d} {tot('iter'):8d} {tot('miss'):7d} {tot('lodnone'):7d} {tot('occlnone'):7d} {tot('entered'):7d}"
          f" {tot('leaf'):7d} {tot('push'):7d} {t['act'].sum()/max(t['iter'].sum(),1):6.1f}")
    print("leaf-level nodes (every kept child an inline leaf), by the node's depth")
    print(" d    nodes  of-exp   child-iter  of-iter  bound-hit  entered  own-hit  ent+own  old-path  two-ray  mixed-lvs  no-child")
    lf = ["lf_node", "exp", "lf_iter", "iter", "lf_hit", "lf_ent", "lf_own", "lf_ent_own", "lf_old", "lf_two", "lf_mixed", "lf_empty"]
    for d in range(NST):
        if t["exp"][d]:
            print(f"{d:2d} " + " ".join(f"{t[f][d]*sc:9d}" for f in lf))
    print("all " + " ".join(f"{tot(f):9d}" for f in lf))
    if TW * TH > 64:   # a unit of more than one tile: what of it is visited by lanes of one 8x8 tile only
        print(f"unit {TW}x{TH}: visited by lanes of one 8x8 tile only")
        print(" d  exp-one-half    of     iter-one-half    of")
        for d in range(NST):
            if t["exp"][d]:
                print(f"{d:2d} {t['half_exp'][d]*sc:9d} {t['exp'][d]*sc:9d} {t['half_iter'][d]*sc:11d} {t['iter'][d]*sc:9d}")
        print(f"all {tot('half_exp'):8d} {tot('exp'):9d} {tot('half_iter'):11d} {tot('iter'):9d}")
    if (TW, TH) == (16, 8):   # the pair unit: what the kernel's one-ray loop takes, and what its two-ray loop still pays
        print("pair unit: under nodes that no hardware lane visits with both tiles (one-tile nodes included)")
        print(" d  exp-fold        of     iter-fold        of   roots: A-only  B-only disjoint")
        for d in range(NST):
            if t["exp"][d]:
                print(f"{d:2d} {t['fold_exp'][d]*sc:9d} {t['exp'][d]*sc:9d} {t['fold_iter'][d]*sc:11d} {t['iter'][d]*sc:9d}"
                      f"  {t['root_a'][d]*sc:13d} {t['root_b'][d]*sc:7d} {t['root_d'][d]*sc:8d}")
        print(f"all {tot('fold_exp'):8d} {tot('exp'):9d} {tot('fold_iter'):11d} {tot('iter'):9d}"
              f"  {tot('root_a'):13d} {tot('root_b'):7d} {tot('root_d'):8d}")
        below = lambda f: int(t[f][1:].sum()) * sc
        print(f"roots entered from a two-ray node (depth >= 1): A-only {below('root_a')} B-only {below('root_b')}"
              f" disjoint {below('root_d')}")
        print("pair unit: two-ray iterations whose bounding hits lie in one tile only")
        print(" d  one-sided  passing-LOD  two-ray-iter")
        for d in range(NST):
            if t["exp"][d]:
                print(f"{d:2d} {t['side_iter'][d]*sc:10d} {t['side_lod'][d]*sc:12d} {(t['iter'][d]-t['fold_iter'][d])*sc:13d}")
        print(f"all {tot('side_iter'):9d} {tot('side_lod'):12d} {tot('iter')-tot('fold_iter'):13d}")


if __name__ == "__main__":
    name = sys.argv[1] if len(sys.argv) > 1 else "c3"
    step = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    modes = [int(m) for m in sys.argv[3:]] or [0]
    for m in modes:
        report(run(name, step, m, check=(step == 1)), f"{name} mode {m}:")
