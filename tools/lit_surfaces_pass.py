#!/usr/bin/env python3
"""What box lights cost on a scene with surface features (RTMI_LIT_SURFACES).  The canonical scene (teapot_tri.obj +
two mirror disks, octree 10/19) at the benchmark's size (--size x --size, maxdepth 5), no environment, the teapot with generated
vertex normals, a box-projected --tex x --tex texture and a height-field normal map of the same size.  Two calls on the same scene
handle, both on the per-pass pipeline (the only one a featured scene has):
  lit    rtmi_render_lit_device with RTMI_LIT_SURFACES, the box light A (-3, 6, 1), edge 0.5 and the point light B (4, -6, 4)
  plain  rtmi_render_samples_device
Time: --reps alternated calls of --spp samples of the whole frame each, after a warm-up; stats.kernel_ms per sample, medians.
Reports the shadow-ray count and lit / plain; it reads beside tools/lit_pass.py's ratio on the bare scene.  No ratio is fixed in
advance: the tool reports.
Usage: tools/lit_surfaces_pass.py [--reps 3] [--size 2048] [--spp 16] [--tex 256] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from rust_raytrace_amd import raytrace as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--size", type=int, default=2048)
ap.add_argument("--spp", type=int, default=16)
ap.add_argument("--tex", type=int, default=256)
ap.add_argument("--out", default=None)
args = ap.parse_args()

W = H = args.size
S, DEPTH = args.spp, 5
NTEAPOT = 6320  # triangles 1 .. 6320 of the canonical scene are the teapot's
OBJ = os.path.join(ROOT, "tests", "golden", "teapot_tri.obj")
A = dict(orig=(-3.0, 6.0, 1.0), len2=0.5, color=(1.0, 0.9, 0.8))
B = dict(orig=(4.0, -6.0, 4.0), len2=0.0, color=(0.2, 0.3, 0.5))
stream = torch.cuda.current_stream().cuda_stream
scene = R.canonical_scene(OBJ, gpu_build=0)
rng = np.random.default_rng(3)
image = (0.25 + 0.75 * rng.random((args.tex, args.tex, 3))).astype(np.float32)
heights = rng.random((args.tex, args.tex)).astype(np.float32)
scene.smooth_normals(1, NTEAPOT)
scene.set_textures([image, R.normal_map_from_height(heights, 2.0)], None, None)
scene.project_uvs(1, NTEAPOT, (-1.7, -0.4, 3.1), 0.9, 1)
scene.set_normal_maps(np.full(NTEAPOT, 2, np.uint32))
full = (0, H, H, 0)
acc, out = (torch.zeros(H * W * 4, dtype=torch.float32, device="cuda:0") for _ in range(2))
KINDS = ("lit", "plain")


def call(kind):
    """One call of S samples of a frame of S: stats"""
    c = R.HipRayCaster(seed=1)
    vp = R.canonical_viewport(W, H, DEPTH, S)
    if kind == "lit":
        st = c.walk_rays_lit_device(vp, scene, c.lit_params([A, B], surfaces=True), acc, out, tile=full, stream=stream).stats
    else:
        st = c.walk_samples_device(vp, scene, full, 0, S, acc.data_ptr(), out.data_ptr(), stream).stats
    torch.cuda.synchronize()
    return st


for k in KINDS:
    call(k)  # warm-up: upload, workspaces
runs = {k: [] for k in KINDS}
for _ in range(args.reps):
    for k in KINDS:
        runs[k].append(call(k))
med = lambda k, f: statistics.median(f(st) for st in runs[k])
res = {"tool": "tools/lit_surfaces_pass.py", "device": torch.cuda.get_device_name(0), "width": W, "height": H, "maxdepth": DEPTH,
       "samples_per_call": S, "reps": args.reps, "lights": [A, B], "texture": [args.tex, args.tex], "calls": {}}
for k in KINDS:
    res["calls"][k] = {
        "ms_per_sample": {"median": med(k, lambda st: st["kernel_ms"] / S), "all": [round(st["kernel_ms"] / S, 4) for st in runs[k]]},
        "closest_hit_ms_per_sample": med(k, lambda st: (st["primary_ms"] if k == "lit" else st["trace_ms"]) / S),
        "walk_ms_per_sample": med(k, lambda st: st["bounce_ms"] / S) if k == "lit" else 0.0,
        "rays": runs[k][-1]["rays"], "streams": runs[k][-1]["streams"], "pipeline": runs[k][-1]["pipeline"],
        "trace_launches": runs[k][-1]["trace_launches"]}
t = {k: res["calls"][k]["ms_per_sample"]["median"] for k in KINDS}
res["shadow_rays"] = res["calls"]["lit"]["rays"] - res["calls"]["plain"]["rays"]
res["lit_over_plain_time"] = t["lit"] / t["plain"]
for k in KINDS:
    c = res["calls"][k]
    print(f"{k:6s} {t[k]:.3f} ms per sample {c['ms_per_sample']['all']} (closest hits {c['closest_hit_ms_per_sample']:.3f}, walks "
          f"{c['walk_ms_per_sample']:.3f}, summed over {c['streams']} streams), rays {c['rays']}, pipeline {c['pipeline']}", flush=True)
print(f"lit / plain {res['lit_over_plain_time']:.3f}; shadow rays {res['shadow_rays']} per {S} samples", flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
