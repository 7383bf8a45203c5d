#!/usr/bin/env python3
"""Batches of views vs one call per view.  The canonical scene of config 3 (teapot_tri.obj + two mirror
disks, octree 10/19, depth 5) seen by K cameras on an arc around the teapot, each with its own seed.  Per shape:
  seq    K calls of rtmi_render_tile_device (HipRayCaster.walk_rows_device), one per view, into one device buffer
  batch  one call of rtmi_render_views_device (HipRayCaster.walk_views_device) for the whole stack
Both legs go through the same Python + C++ host layer.  Every shape is warmed up first (both legs); then the legs alternate,
--reps times, each timed on the host from a device sync before the leg to a device sync after it.  Reported: median, min
and max milliseconds per leg, the median ratio seq / batch, and whether the two legs' stacks are bit-equal.
Usage: tools/views_batch.py [--reps N] [--out FILE.json]"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from rust_raytrace_amd import raytrace as R  # noqa: E402

# (width, height, spp, K): the reference's interactive 64 x 64 window, a mid-size batch, config 3's frame
SHAPES = [(64, 64, 1, 64), (64, 64, 1, 256), (512, 512, 16, 8), (2048, 2048, 64, 1), (2048, 2048, 64, 2)]
DEPTH = 5

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()


def orbit(w, h, spp, n):
    """n cameras on an arc of +-30 degrees around the teapot (at (0, 0.5, 5)), the canonical field of view"""
    views = []
    for k in range(n):
        a = math.radians(-30.0 + 60.0 * k / max(n - 1, 1))
        pos = [5.0 * math.sin(a), 0.0, 5.0 - 5.0 * math.cos(a)]
        d = R.unit([-pos[0], 0.5 - pos[1], 5.0 - pos[2]])
        aspect = np.float32(h) / np.float32(w)
        views.append(R.create_viewport((w, h), (1.0, float(np.float32(1.0) * aspect)), pos, d, 90.0, R.to_radians(0.0), DEPTH, spp))
    return views


scene = R.canonical_scene(os.path.join(ROOT, "tests", "golden", "teapot_tri.obj"), gpu_build=0)
c = R.HipRayCaster(seed=1)
c.upload(scene)
stream = torch.cuda.current_stream().cuda_stream
results = []
for (w, h, spp, K) in SHAPES:
    views = orbit(w, h, spp, K)
    seeds = [1000 + k for k in range(K)]
    bufs = {leg: torch.zeros((K * h, w, 4), dtype=torch.float32, device="cuda:0") for leg in ("seq", "batch")}
    row_bytes = w * 16

    def seq():
        base = bufs["seq"].data_ptr()
        for k in range(K):
            c.seed = seeds[k]
            c.walk_rows_device(views[k], scene, 0, h, base + k * h * row_bytes, stream)
        c.seed = 1

    def batch():
        c.walk_views_device(views, scene, (0, K * h, K * h, 0), bufs["batch"].data_ptr(), stream, seeds=seeds)

    legs = {"seq": seq, "batch": batch}
    for f in legs.values():  # warm-up: workspaces, view table, code objects
        f()
    torch.cuda.synchronize()
    times = {leg: [] for leg in legs}
    for _ in range(args.reps):
        for leg, f in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            times[leg].append((time.perf_counter() - t0) * 1e3)
    same = torch.equal(bufs["seq"].view(torch.int32), bufs["batch"].view(torch.int32))
    r = {"width": w, "height": h, "spp": spp, "views": K, "paths": K * w * h * spp, "bit_equal": bool(same)}
    for leg in legs:
        r[leg + "_ms"] = {"median": statistics.median(times[leg]), "min": min(times[leg]), "max": max(times[leg]),
                          "all": [round(t, 3) for t in times[leg]]}
    r["speedup_median"] = r["seq_ms"]["median"] / r["batch_ms"]["median"]
    results.append(r)
    print(f"{w}x{h} @{spp} K={K}: seq {r['seq_ms']['median']:.3f} ms [{r['seq_ms']['min']:.3f}, {r['seq_ms']['max']:.3f}]  "
          f"batch {r['batch_ms']['median']:.3f} ms [{r['batch_ms']['min']:.3f}, {r['batch_ms']['max']:.3f}]  "
          f"seq/batch {r['speedup_median']:.2f}  bit-equal {same}", flush=True)
    del bufs
    torch.cuda.empty_cache()

if args.out:
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/views_batch.py", "reps": args.reps, "depth": DEPTH, "device": torch.cuda.get_device_name(0),
                   "results": results}, f, indent=1)
