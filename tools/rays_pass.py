#!/usr/bin/env python3
"""What an explicit-ray render costs beside the camera's own.  The canonical scene (teapot_tri.obj + two mirror
disks, octree 10/19), the canonical view at --size x --size, --spp samples, depth 5.  Legs, all on device buffers, each reporting
stats.kernel_ms (HIP events on the caller's stream around the whole call) and stats.trace_ms:
  rays      rtmi_render_rays_device of the view's own primary rays (orc.primary_rays, uploaded once) into `mean`, group = spp,
            keys from the formula: the per-pass pipeline on one stream, 32 B per ray read instead of a ray generated
  frame1    rtmi_render_device of the same frame with tuning.pipeline = 1 (k_gen, then one closest-hit + one shading launch per
            pass): the same pipeline behind the camera; automatic streams (three)
  frame1s1  the same with tuning.streams = 1: the same pipeline on the same number of streams as `rays`
  frame3    rtmi_render_device as it runs by default (pipeline 3: k_path_primary's packet culling and in-place mirror pass),
            which an explicit-ray render cannot use
After a warm-up the legs alternate in one process, --reps times; reported: median [min, max] per leg and the ratios of the
medians.  The four images are compared bit for bit.  --frame-only runs the three frame legs alone (a build without the call).
Usage: tools/rays_pass.py [--reps N] [--size 1024] [--spp 4] [--frame-only] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from oracle import orc  # noqa: E402  (the primary rays only: the renderer's own ray generation, restated)
from rust_raytrace_amd import raytrace as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--spp", type=int, default=4)
ap.add_argument("--frame-only", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()

W = H = args.size
SPP, DEPTH, SEED = args.spp, 5, 1
OBJ = os.path.join(ROOT, "tests", "golden", "teapot_tri.obj")
sc = R.canonical_scene(OBJ, gpu_build=0)
vp = R.canonical_viewport(W, H, DEPTH, SPP)
stream = torch.cuda.current_stream().cuda_stream
casters = {"frame1": R.HipRayCaster(seed=SEED, tuning={"pipeline": 1}), "frame1s1": R.HipRayCaster(seed=SEED, tuning={"pipeline": 1, "streams": 1}),
           "frame3": R.HipRayCaster(seed=SEED)}
images = {k: torch.zeros(H * W * 4, device="cuda:0") for k in casters}
legs = {k: (lambda k=k: casters[k].walk_rows_device(vp, sc, 0, H, images[k].data_ptr(), stream).stats) for k in casters}
if not args.frame_only:
    o4, d4 = orc.primary_rays(W, H, orc.canonical_viewport(W, H), SPP, SEED)
    to, td = torch.from_numpy(o4).to("cuda:0"), torch.from_numpy(d4).to("cuda:0")
    images["rays"] = torch.zeros(H * W * 4, device="cuda:0")
    rays_caster = R.HipRayCaster(seed=SEED)
    legs["rays"] = lambda: rays_caster.walk_rays_explicit_device(sc, to, td, DEPTH, group=SPP, mean=images["rays"], stream=stream).stats
torch.cuda.synchronize()

for _ in range(2):  # warm-up: workspaces, code objects
    for leg in legs.values():
        leg()
times = {k: {"kernel_ms": [], "trace_ms": []} for k in legs}
last = {}
for _ in range(args.reps):
    for k, leg in legs.items():
        st = leg()
        times[k]["kernel_ms"].append(st["kernel_ms"])
        times[k]["trace_ms"].append(st["trace_ms"])
        last[k] = st
torch.cuda.synchronize()
ref = images["frame3"].cpu().numpy().view(np.uint32)
for k in legs:
    assert np.array_equal(images[k].cpu().numpy().view(np.uint32), ref), k  # one image whichever way it is rendered
    assert last[k]["rays"] == last["frame3"]["rays"], k

res = {}
for k in legs:
    res[k] = {"rays": last[k]["rays"], "pipeline": last[k]["pipeline"], "streams": last[k]["streams"], "trace_launches": last[k]["trace_launches"]}
    for m, xs in times[k].items():
        res[k][m] = {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": [round(x, 4) for x in xs]}
    km, tm = res[k]["kernel_ms"], res[k]["trace_ms"]
    print(f"{k}: {res[k]['rays']} rays, pipeline {res[k]['pipeline']}, {res[k]['streams']} stream(s); kernel {km['median']:.3f} ms "
          f"[{km['min']:.3f}, {km['max']:.3f}], trace {tm['median']:.3f} ms [{tm['min']:.3f}, {tm['max']:.3f}]", flush=True)
ratios = {}
if "rays" in res:
    for k in casters:
        ratios[f"rays/{k}"] = res["rays"]["kernel_ms"]["median"] / res[k]["kernel_ms"]["median"]
    print("ratios of the medians (kernel_ms): " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()), flush=True)

if args.out:
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/rays_pass.py", "reps": args.reps, "width": W, "height": H, "spp": SPP, "maxdepth": DEPTH, "seed": SEED,
                   "device": torch.cuda.get_device_name(0), "legs": res, "ratios": ratios}, f, indent=1)
