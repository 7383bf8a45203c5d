#!/usr/bin/env python3
"""What vertex normals cost per frame.  The canonical scene (teapot_tri.obj + two mirror disks, octree 10/19) at the
benchmark's size (--size x --size, S = --spp, maxdepth 5, seed 1), three legs, each on its own scene handle, alternated --reps times
in one process after a warm-up; every leg renders the whole frame into device memory with rtmi_render_tile_device and reports
stats.kernel_ms (HIP events on the caller's stream):
  smooth    the scene with generated normals on the teapot (canonical_scene(smooth=True)): the per-pass pipeline with
            k_shade_smooth (a scene with vertex normals always)
  plain_p1  the same scene without them, tuning.pipeline = 1: the same per-pass pipeline with k_shade
  plain_p3  the same scene without them, tuning.pipeline = 3: the path kernels, what the benchmark runs
plain_p1 and plain_p3 are existing code: the baseline.  The ray counts differ, because normals change where paths go, so both are
reported with the time per ray.
The shading launches' share: further frames of smooth and of plain_p1 each under the library's own timer of the closest-hit
launches (stats.trace_ms) on ONE stream, where frame - trace is the time of everything that is not a walk -- generation, shading,
accumulation -- and the difference of that remainder between the two legs is what 96 B of gathered records per bouncing hit and
the interpolation cost in k_shade_smooth.  (Kernel-by-kernel times need a profiler run of their own.)
Usage: tools/smooth_pass.py [--reps N] [--size 2048] [--spp 64] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from rust_raytrace_amd import raytrace as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--size", type=int, default=2048)
ap.add_argument("--spp", type=int, default=64)
ap.add_argument("--out", default=None)
args = ap.parse_args()

W = H = args.size
S, DEPTH, SEED = args.spp, 5, 1
OBJ = os.path.join(ROOT, "tests", "golden", "teapot_tri.obj")
stream = torch.cuda.current_stream().cuda_stream


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": [round(x, 4) for x in xs]}


smooth_scene = R.canonical_scene(OBJ, gpu_build=0, smooth=True)
plain1, plain3 = R.canonical_scene(OBJ, gpu_build=0), R.canonical_scene(OBJ, gpu_build=0)
out = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda:0")
torch.cuda.synchronize()
vp = R.canonical_viewport(W, H, DEPTH, S)
tile = (0, H, H, 0)
c0 = R.HipRayCaster(seed=SEED)
c1 = R.HipRayCaster(seed=SEED, tuning=dict(pipeline=1))
c3 = R.HipRayCaster(seed=SEED, tuning=dict(pipeline=3))
legs = {
    "smooth": lambda: c0.walk_tile_device(vp, smooth_scene, tile, out.data_ptr(), stream).stats,
    "plain_p1": lambda: c1.walk_tile_device(vp, plain1, tile, out.data_ptr(), stream).stats,
    "plain_p3": lambda: c3.walk_tile_device(vp, plain3, tile, out.data_ptr(), stream).stats,
}
for f in legs.values():  # warm-up: uploads, workspaces, code objects
    f()
st = {k: [] for k in legs}
for _ in range(args.reps):
    for k, f in legs.items():
        st[k].append(f())
torch.cuda.synchronize()
assert st["smooth"][0]["pipeline"] == 1 and st["plain_p1"][0]["pipeline"] == 1 and st["plain_p3"][0]["pipeline"] == 3
assert st["smooth"][0]["slow_paths"] == 0
res = {"tool": "tools/smooth_pass.py", "reps": args.reps, "width": W, "height": H, "samples_per_pixel": S, "maxdepth": DEPTH, "seed": SEED,
       "device": torch.cuda.get_device_name(0), "legs": {}}
for k, v in st.items():
    m = {"kernel_ms": summary([s["kernel_ms"] for s in v]), "rays": v[0]["rays"], "rays_per_path": v[0]["rays"] / (W * H * S),
         "pipeline": v[0]["pipeline"], "streams": v[0]["streams"], "trace_launches": v[0]["trace_launches"],
         "trace_ms": statistics.median([s["trace_ms"] for s in v])}
    m["mrays_per_s"] = m["rays"] / (m["kernel_ms"]["median"] * 1e3)
    m["ns_per_ray"] = m["kernel_ms"]["median"] * 1e6 / m["rays"]
    res["legs"][k] = m
    print(f"{k}: {m['kernel_ms']['median']:.3f} ms [{m['kernel_ms']['min']:.3f}, {m['kernel_ms']['max']:.3f}], {m['rays']} rays "
          f"({m['ns_per_ray']:.4f} ns/ray, {m['mrays_per_s']:.1f} Mrays/s), trace {m['trace_ms']:.3f} ms summed over {m['streams']} stream(s), "
          f"pipeline {m['pipeline']}", flush=True)
e, p1, p3 = (res["legs"][k]["kernel_ms"]["median"] for k in ("smooth", "plain_p1", "plain_p3"))
res["smooth_minus_plain_p1_ms"], res["smooth_over_plain_p1"], res["smooth_over_plain_p3"] = e - p1, e / p1, e / p3
res["rays_smooth_over_plain"] = res["legs"]["smooth"]["rays"] / res["legs"]["plain_p1"]["rays"]
print(f"smooth - plain_p1 = {e - p1:.3f} ms, smooth / plain_p1 = {e / p1:.4f}, smooth / plain_p3 = {e / p3:.4f}, "
      f"rays smooth / plain = {res['rays_smooth_over_plain']:.5f}", flush=True)

# one stream: the launches of a frame run one after the other, so frame - trace is the time of everything that is not a walk
s0 = R.HipRayCaster(seed=SEED, tuning=dict(streams=1))
s1 = R.HipRayCaster(seed=SEED, tuning=dict(pipeline=1, streams=1))
one = {"smooth": lambda: s0.walk_tile_device(vp, smooth_scene, tile, out.data_ptr(), stream).stats,
       "plain_p1": lambda: s1.walk_tile_device(vp, plain1, tile, out.data_ptr(), stream).stats}
for f in one.values():
    f()
rest = {k: [] for k in one}
frame = {k: [] for k in one}
for _ in range(args.reps):
    for k, f in one.items():
        s = f()
        assert s["streams"] == 1
        frame[k].append(s["kernel_ms"])
        rest[k].append(s["kernel_ms"] - s["trace_ms"])
torch.cuda.synchronize()
d_frame = statistics.median(frame["smooth"]) - statistics.median(frame["plain_p1"])
d_rest = statistics.median(rest["smooth"]) - statistics.median(rest["plain_p1"])
res["one_stream"] = {k: {"kernel_ms": summary(frame[k]), "not_trace_ms": summary(rest[k])} for k in one}
res["one_stream"]["frame_difference_ms"] = d_frame
res["one_stream"]["shade_difference_ms"] = d_rest
print(f"one stream: smooth {statistics.median(frame['smooth']):.3f} ms, plain_p1 {statistics.median(frame['plain_p1']):.3f} ms; outside the "
      f"walks {statistics.median(rest['smooth']):.3f} against {statistics.median(rest['plain_p1']):.3f} ms: {d_rest:.3f} of the {d_frame:.3f} ms "
      f"difference", flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
