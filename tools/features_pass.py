#!/usr/bin/env python3
"""First-hit feature buffers vs a depth-1 render of the same primary rays.  The canonical scene of config 3
(teapot_tri.obj + two mirror disks, octree 10/19) at 2048 x 2048, for 64 and 8 samples per pixel:
  A  rtmi_render_tile_device at maxdepth = 1 (HipRayCaster.walk_tile_device): the same primary rays through k_path_primary
     (with its packet cull), 16 B per pixel out.  The yardstick; it exists before this feature too (--legs A).
  B  rtmi_render_features_device, all three outputs (HipRayCaster.walk_features_device): k_gen_samples, k_trace_oct, k_features.
  R  for context, HipRayCaster.primary_records of sample 0 (the only route to per-pixel hits before): host wall time, once.
Every shape is warmed up first (all legs); then A and B alternate in one process, --reps times.  The time of a repetition is
the call's device time between HIP events (rtmi_stats_t.kernel_ms).  Reported: median [min, max] per leg and the median B / A.
--once runs each leg's call once after the warm-up and nothing else: the shape of a run under a kernel-trace profiler.
--streams N sets rtmi_tuning_t.streams (default: the library's automatic rule); with 1 no two launches of a call overlap.
Usage: tools/features_pass.py [--reps N] [--legs AB|A|B] [--spp 64,8] [--size 2048] [--streams N] [--records] [--once] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from rust_raytrace_amd import raytrace as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--legs", default="AB")
ap.add_argument("--spp", default="64,8")
ap.add_argument("--size", type=int, default=2048)
ap.add_argument("--streams", type=int, default=0)
ap.add_argument("--records", action="store_true")
ap.add_argument("--once", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()

W = H = args.size
scene = R.canonical_scene(os.path.join(ROOT, "tests", "golden", "teapot_tri.obj"), gpu_build=0)
c = R.HipRayCaster(seed=1, tuning={"streams": args.streams} if args.streams else None)
c.upload(scene)
stream = torch.cuda.current_stream().cuda_stream
tile = (0, H, H, 0)
out = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
albedo, normal = torch.zeros_like(out), torch.zeros_like(out)
ids = torch.zeros((H, W), dtype=torch.int32, device="cuda:0")
results = []
for spp in [int(x) for x in args.spp.split(",")]:
    vp = R.canonical_viewport(W, H, 1, spp)
    legs = {}
    if "A" in args.legs:
        legs["A"] = lambda: c.walk_tile_device(vp, scene, tile, out.data_ptr(), stream)
    if "B" in args.legs:
        legs["B"] = lambda: c.walk_features_device(vp, scene, tile, albedo.data_ptr(), normal.data_ptr(), ids.data_ptr(), 0, spp, stream)
    for f in legs.values():  # warm-up: workspaces, code objects
        f()
    torch.cuda.synchronize()
    times = {leg: [] for leg in legs}
    trace = {leg: [] for leg in legs}
    for _ in range(1 if args.once else args.reps):
        for leg, f in legs.items():
            torch.cuda.synchronize()
            st = f().stats
            torch.cuda.synchronize()
            times[leg].append(st["kernel_ms"])
            trace[leg].append(st["trace_ms"])
    r = {"width": W, "height": H, "spp": spp, "paths": W * H * spp}
    line = f"{W}x{H} @{spp}:"
    for leg in legs:
        r[leg + "_ms"] = {"median": statistics.median(times[leg]), "min": min(times[leg]), "max": max(times[leg]),
                          "all": [round(t, 3) for t in times[leg]], "trace_ms_median": statistics.median(trace[leg])}
        line += f"  {leg} {r[leg + '_ms']['median']:.3f} ms [{r[leg + '_ms']['min']:.3f}, {r[leg + '_ms']['max']:.3f}] (trace {r[leg + '_ms']['trace_ms_median']:.3f})"
    if "A" in legs and "B" in legs:
        r["B_over_A_median"] = r["B_ms"]["median"] / r["A_ms"]["median"]
        line += f"  B/A {r['B_over_A_median']:.3f}"
    results.append(r)
    print(line, flush=True)

records = None
if args.records and not args.once:
    vp = R.canonical_viewport(W, H, 1, 64)
    t0 = time.perf_counter()
    rec = c.primary_records(vp, scene, 0, H, 0)
    records = {"wall_ms": (time.perf_counter() - t0) * 1e3, "kernel_ms": rec.stats["kernel_ms"], "rays": W * H}
    print(f"primary_records of sample 0: {records['wall_ms']:.1f} ms wall, {records['kernel_ms']:.3f} ms on the device", flush=True)

if args.out:
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/features_pass.py", "reps": args.reps, "legs": args.legs, "streams": args.streams, "device": torch.cuda.get_device_name(0),
                   "results": results, "primary_records": records}, f, indent=1)
