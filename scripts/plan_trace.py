#!/usr/bin/env python3
"""The launches the render schedule makes (csrc/sf_plan.h), case by case, for comparing two builds of the library.

Run mode (no argument): in one process, every case of tests/test_plan_host.py that fits a device -- the frame sizes
and the knob rows -- each in fresh contexts under its own environment, on the config view: a marker launch
(sf_light_fill), then five renders. Prints one JSON line per case (what the library's counters say afterwards) and
one for the device. Run it under `rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python3
scripts/plan_trace.py`, once per library (SF_LIB / SF_LIB_PARTIAL=1 select another build).

    plan_trace.py --list DIR/.../run_kernel_trace.csv [CUS]

prints that trace as the ordered list of the library's launches per case -- kernel, grid (work-items), workgroup,
group segment bytes -- cut at the markers; two builds make the same launches where these lists are equal. With the
device's CU count it ends with the blocks per CU of the three full grids (general, lean, pair kernel)."""
import csv
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "sphereflake-raytracer_amd")]

ONCE = {"SF_ORDER": "1", "SF_SPLIT_BUCKETS": "0", "SF_ORDER_RECORD": "0"}
# (name, W, H, environment, renders: "0" a launch of its own, "n" n frames in one launch, Render()'s keywords)
CASES = [
    ("1920x1080", 1920, 1080, {}, "00000", {}),
    ("1280x720", 1280, 720, {}, "00000", {}),
    ("640x360", 640, 360, {}, "00000", {}),
    ("1080p share 0/8", 1920, 1080, {}, "00000", dict(band_rows=8, band_count=8, band_index=0)),
    ("96x64", 96, 64, {}, "00000", {}),
    ("16x8 SF_ORDER=0", 16, 8, {"SF_ORDER": "0"}, "00000", {}),
    ("1920x1080 x4", 1920, 1080, {}, "44444", {}),
]
for W, H, blocks in ((96, 64, "3"), (16, 8, "1")):
    for env in ({"SF_PAIR": "1"}, {"SF_PAIR": "1", "SF_ORDER": "0"}, {"SF_PAIR": "0"}, {"SF_LEAN": "0"},
                {"SF_LEAN": "0", "SF_ORDER": "0"}, ONCE, {"SF_HALVES": "1"}, {"SF_HALVES": "1", "SF_ORDER": "0"},
                {"SF_MAX_BLOCKS": blocks}, {"SF_TRACE_WAVES": "2"}):
        CASES.append((f"{W}x{H} " + " ".join(f"{k}={v}" for k, v in env.items()), W, H, env, "00000", {}))
CASES += [
    ("8x16 pairs and frames", 8, 16, {"SF_PAIR": "1", "SF_ORDER": "1", "SF_ORDER_EVERY": "64"}, "02200", {}),
    ("40x16 pairs and frames", 40, 16, {"SF_PAIR": "1", "SF_ORDER": "1", "SF_ORDER_EVERY": "1"}, "02020", {}),
]
KEYS = sorted({k for c in CASES for k in c[3]})
MARKER = "sf_light_fill_px"


def run():
    import sphereflake_amd as sf
    import torch
    print(json.dumps({"cus": torch.cuda.get_device_properties(0).multi_processor_count,
                      "source_sha256": sf.lib().sf_build_id().decode()}))
    for name, W, H, env, renders, kw in CASES:
        for k in KEYS:
            os.environ.pop(k, None)
        os.environ.update(env)
        flakes = [sf.Sphereflake(W, H) for _ in range(max(1, max(int(r) for r in renders)))]
        try:
            for f in flakes:
                f.SetCamera(sf.config_camera(W, H, 1.0))
            flakes[0].light_fill((0.0, 0.0, 0.0))
            for r in renders:
                if r == "0":
                    flakes[0].Render(**kw)
                else:
                    sf.render_frames(flakes[:int(r)], **kw)
            for f in flakes:
                f.Synchronize()
            print(json.dumps({"case": name, "lean_launches": flakes[0].lean_launches(),
                              "pair_launches": flakes[0].pair_launches(),
                              "order_units": int(sf.lib().sf_order_units(flakes[0].ctx))}))
        finally:
            for f in flakes:
                f.close()


def listing(path, cus):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r.get("Dispatch_Id") or r["Start_Timestamp"]))
    col = lambda r, *names: next(r[n] for n in names if n in r)
    case, full = -1, {}
    for r in rows:
        kernel = r["Kernel_Name"].split("(")[0].split(".kd")[0]
        if not kernel.startswith("sf_"):
            continue   # (the runtime's own fill and copy kernels)
        if kernel == MARKER:
            case += 1
            print(f"== {CASES[case][0]}")
            continue
        grid, wg = int(col(r, "Grid_Size_X", "Grid_Size")), int(col(r, "Workgroup_Size_X", "Workgroup_Size"))
        print(f"{kernel} grid {grid} workgroup {wg} lds {col(r, 'LDS_Block_Size', 'Group_Segment_Size')}")
        if case >= 0 and kernel.startswith("sf_trace_queue1"):
            full.setdefault((CASES[case][0], kernel), grid // wg)
    assert case + 1 == len(CASES), (case + 1, len(CASES))
    if cus:   # the full grids: 640x360's general loop, 1280x720's lean loop, 1920x1080's pair loop
        occ = [full[k] / cus for k in (("640x360", "sf_trace_queue1g"), ("1280x720", "sf_trace_queue1t"),
                                       ("1920x1080", "sf_trace_queue1"))]
        print(f"== blocks per CU of {cus}: general {occ[0]:g} lean {occ[1]:g} pair {occ[2]:g}")


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "--list":
        listing(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 0)
    else:
        run()
