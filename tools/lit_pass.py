#!/usr/bin/env python3
"""What box lights inside the path trace cost.  The canonical scene (teapot_tri.obj + two mirror disks, octree
10/19) at the benchmark's size (--size x --size, maxdepth 5), no environment.  Three calls on the same scene handle:
  lit       rtmi_render_lit_device with the box light A (-3, 6, 1), edge 0.5 and the point light B (4, -6, 4)
  plain     rtmi_render_samples_device forced to the per-pass pipeline the other two always run (tuning pipeline = 1), and
  plain3    the same at the library's default (the path kernels): what a user's plain render costs
  shadowed  rtmi_render_shadowed_device with light A alone: the same pass structure with one candidate per surface hit
Time: --reps alternated calls of --spp samples of the whole frame each, after a warm-up; stats.kernel_ms per sample, medians.
Where the time goes: per call primary_ms (the closest-hit launches), bounce_ms (the shadow rays' walks) and the remainder of
kernel_ms (the elementwise kernels, idle gaps), and the rays.  --once KIND runs one call of KIND on ONE stream and nothing else,
for a kernel trace.  No ratio is fixed in advance: the tool reports.
Usage: tools/lit_pass.py [--reps 3] [--size 2048] [--spp 16] [--once lit|plain|shadowed] [--out FILE.json]"""
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
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--size", type=int, default=2048)
ap.add_argument("--spp", type=int, default=16)
ap.add_argument("--once", default=None, choices=["lit", "plain", "shadowed"])
ap.add_argument("--out", default=None)
args = ap.parse_args()

W = H = args.size
S, DEPTH = args.spp, 5
OBJ = os.path.join(ROOT, "tests", "golden", "teapot_tri.obj")
A = dict(orig=(-3.0, 6.0, 1.0), len2=0.5, color=(1.0, 0.9, 0.8))
B = dict(orig=(4.0, -6.0, 4.0), len2=0.0, color=(0.2, 0.3, 0.5))
stream = torch.cuda.current_stream().cuda_stream
scene = R.canonical_scene(OBJ, gpu_build=0)
full = (0, H, H, 0)
acc, out = (torch.zeros(H * W * 4, dtype=torch.float32, device="cuda:0") for _ in range(2))
KINDS = ("lit", "plain", "plain3", "shadowed")


def call(kind, tuning=None):
    """One call of S samples of a frame of S: stats"""
    t = dict(tuning or {})
    if kind == "plain":
        t["pipeline"] = 1
    c = R.HipRayCaster(seed=1, tuning=t) if t else R.HipRayCaster(seed=1)
    vp = R.canonical_viewport(W, H, DEPTH, S)
    if kind == "lit":
        st = c.walk_rays_lit_device(vp, scene, [A, B], acc, out, tile=full, stream=stream).stats
    elif kind == "shadowed":
        st = c.walk_rays_shadowed_device(vp, scene, acc, out, tile=full, orig=A["orig"], len2=A["len2"], stream=stream).stats
    else:
        st = c.walk_samples_device(vp, scene, full, 0, S, acc.data_ptr(), out.data_ptr(), stream).stats
    torch.cuda.synchronize()
    return st


if args.once:
    call(args.once, dict(streams=1))  # warm-up: upload, workspaces
    st = call(args.once, dict(streams=1))
    print(f"{args.once}, one stream: {st['kernel_ms'] / S:.3f} ms per sample, rays {st['rays']}", flush=True)
    sys.exit(0)

for k in KINDS:
    call(k)  # warm-up: upload, workspaces
runs = {k: [] for k in KINDS}
for _ in range(args.reps):
    for k in KINDS:
        runs[k].append(call(k))
R.HipRayCaster().upload(scene)
med = lambda k, f: statistics.median(f(st) for st in runs[k])
res = {"tool": "tools/lit_pass.py", "device": torch.cuda.get_device_name(0), "width": W, "height": H, "maxdepth": DEPTH,
       "samples_per_call": S, "reps": args.reps, "lights": [A, B], "shadowed_light": A, "calls": {}}
for k in KINDS:
    res["calls"][k] = {
        "ms_per_sample": {"median": med(k, lambda st: st["kernel_ms"] / S), "all": [round(st["kernel_ms"] / S, 4) for st in runs[k]]},
        "closest_hit_ms_per_sample": med(k, lambda st: (st["primary_ms"] if k in ("lit", "shadowed") else st["trace_ms"]) / S),
        "walk_ms_per_sample": med(k, lambda st: st["bounce_ms"] / S) if k in ("lit", "shadowed") else 0.0,
        "rays": runs[k][-1]["rays"], "streams": runs[k][-1]["streams"], "pipeline": runs[k][-1]["pipeline"],
        "trace_launches": runs[k][-1]["trace_launches"]}
t = {k: res["calls"][k]["ms_per_sample"]["median"] for k in KINDS}
res["shadow_rays"] = {"lit": res["calls"]["lit"]["rays"] - res["calls"]["plain"]["rays"],
                      "shadowed": res["calls"]["shadowed"]["rays"] - res["calls"]["plain"]["rays"]}
res["lit_over_plain_time"] = t["lit"] / t["plain"]
res["lit_over_plain3_time"] = t["lit"] / t["plain3"]
res["lit_over_shadowed_time"] = t["lit"] / t["shadowed"]
for k in KINDS:
    c = res["calls"][k]
    print(f"{k:9s} {t[k]:.3f} ms per sample {c['ms_per_sample']['all']} (closest hits {c['closest_hit_ms_per_sample']:.3f}, walks "
          f"{c['walk_ms_per_sample']:.3f}, summed over {c['streams']} streams), rays {c['rays']}", flush=True)
print(f"lit / plain {res['lit_over_plain_time']:.3f}, lit / plain (path kernels) {res['lit_over_plain3_time']:.3f}, lit / shadowed "
      f"{res['lit_over_shadowed_time']:.3f}; shadow rays {res['shadow_rays']}", flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
