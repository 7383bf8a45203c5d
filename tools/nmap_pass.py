#!/usr/bin/env python3
"""What normal maps cost per frame.  The canonical scene (teapot_tri.obj + two mirror disks, octree 10/19) with
generated vertex normals on the teapot, box-projected with a --tex x --tex image of seeded random floats, at the benchmark's size
(--size x --size, S = --spp, maxdepth 5, seed 1), two legs, each on its own scene handle, alternated --reps times in one process
after a warm-up; every leg renders the whole frame into device memory with rtmi_render_tile_device and reports stats.kernel_ms
(HIP events on the caller's stream):
  mapped    the teapot also carries a --tex x --tex normal map made by normal_map_from_height from seeded heights
            (canonical_scene(smooth=True, texture=..., normal_map=...)): the per-pass pipeline with k_shade_nmap
  textured  the same scene without the map: the same per-pass pipeline with k_shade_tex
A map moves paths (a bounce leaves about another normal), so the two legs trace different rays: both ray counts are reported and
no ratio is promised.  The shading launches' share: further frames of both legs under the library's own timer of the closest-hit
launches (stats.trace_ms) on ONE stream, where frame - trace is the time of everything that is not a walk -- generation, shading,
accumulation.  (Kernel-by-kernel times need a profiler run of their own.)
Usage: tools/nmap_pass.py [--reps N] [--size 2048] [--spp 64] [--tex 256] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from rust_raytrace_amd import raytrace as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--size", type=int, default=2048)
ap.add_argument("--spp", type=int, default=64)
ap.add_argument("--tex", type=int, default=256)
ap.add_argument("--out", default=None)
args = ap.parse_args()

W = H = args.size
S, DEPTH, SEED = args.spp, 5, 1
OBJ = os.path.join(ROOT, "tests", "golden", "teapot_tri.obj")
stream = torch.cuda.current_stream().cuda_stream


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": [round(x, 4) for x in xs]}


image = (np.random.default_rng(7).random((args.tex, args.tex, 3)) * 2.0).astype(np.float32)
nmap = R.normal_map_from_height(np.random.default_rng(29).random((args.tex, args.tex)).astype(np.float32), 8.0)
map_scene = R.canonical_scene(OBJ, gpu_build=0, smooth=True, texture=image, normal_map=nmap)
tex_scene = R.canonical_scene(OBJ, gpu_build=0, smooth=True, texture=image)
out = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda:0")
torch.cuda.synchronize()
vp = R.canonical_viewport(W, H, DEPTH, S)
tile = (0, H, H, 0)
c0 = R.HipRayCaster(seed=SEED)
legs = {
    "mapped": lambda: c0.walk_tile_device(vp, map_scene, tile, out.data_ptr(), stream).stats,
    "textured": lambda: c0.walk_tile_device(vp, tex_scene, tile, out.data_ptr(), stream).stats,
}
for f in legs.values():  # warm-up: uploads, workspaces, code objects
    f()
st = {k: [] for k in legs}
for _ in range(args.reps):
    for k, f in legs.items():
        st[k].append(f())
torch.cuda.synchronize()
assert all(v[0]["pipeline"] == 1 and v[0]["slow_paths"] == 0 for v in st.values())
res = {"tool": "tools/nmap_pass.py", "reps": args.reps, "width": W, "height": H, "samples_per_pixel": S, "maxdepth": DEPTH, "seed": SEED,
       "texture": [args.tex, args.tex], "normal_map": [args.tex, args.tex], "device": torch.cuda.get_device_name(0), "legs": {}}
for k, v in st.items():
    m = {"kernel_ms": summary([s["kernel_ms"] for s in v]), "rays": v[0]["rays"], "pipeline": v[0]["pipeline"], "streams": v[0]["streams"],
         "trace_launches": v[0]["trace_launches"], "trace_ms": statistics.median([s["trace_ms"] for s in v])}
    m["mrays_per_s"] = m["rays"] / (m["kernel_ms"]["median"] * 1e3)
    res["legs"][k] = m
    print(f"{k}: {m['kernel_ms']['median']:.3f} ms [{m['kernel_ms']['min']:.3f}, {m['kernel_ms']['max']:.3f}], {m['rays']} rays "
          f"({m['mrays_per_s']:.1f} Mrays/s), trace {m['trace_ms']:.3f} ms summed over {m['streams']} stream(s), pipeline {m['pipeline']}", flush=True)
e, p = (res["legs"][k]["kernel_ms"]["median"] for k in ("mapped", "textured"))
res["mapped_minus_textured_ms"], res["mapped_over_textured"] = e - p, e / p
print(f"mapped - textured = {e - p:.3f} ms, mapped / textured = {e / p:.4f} (different rays: {res['legs']['mapped']['rays']} against "
      f"{res['legs']['textured']['rays']})", flush=True)

# one stream: the launches of a frame run one after the other, so frame - trace is the time of everything that is not a walk
s1 = R.HipRayCaster(seed=SEED, tuning=dict(streams=1))
one = {"mapped": lambda: s1.walk_tile_device(vp, map_scene, tile, out.data_ptr(), stream).stats,
       "textured": lambda: s1.walk_tile_device(vp, tex_scene, tile, out.data_ptr(), stream).stats}
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
d_frame = statistics.median(frame["mapped"]) - statistics.median(frame["textured"])
d_rest = statistics.median(rest["mapped"]) - statistics.median(rest["textured"])
res["one_stream"] = {k: {"kernel_ms": summary(frame[k]), "not_trace_ms": summary(rest[k])} for k in one}
res["one_stream"]["frame_difference_ms"] = d_frame
res["one_stream"]["shade_difference_ms"] = d_rest
print(f"one stream: mapped {statistics.median(frame['mapped']):.3f} ms, textured {statistics.median(frame['textured']):.3f} ms; outside the "
      f"walks {statistics.median(rest['mapped']):.3f} against {statistics.median(rest['textured']):.3f} ms: {d_rest:.3f} of the {d_frame:.3f} ms "
      f"difference", flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
