#!/usr/bin/env python3
"""What lamps cost a bake.  The canonical scene (teapot_tri.obj + two mirror disks, octree 10/19); the elements
are --elements first hits of the canonical --size x --size view at one sample per pixel (the handle's own rtmi_trace), each with
the normal of the face that was hit.  K = --rays gather rays per element, maxdepth 4, lights A (-3, 6, 1) edge 0.5 and B
(4, -6, 4), a point.  Three legs, alternated --reps times in one process after a warm-up, each reporting stats.kernel_ms (HIP
events on the caller's stream) and its median:
  plain   rtmi_bake_device (light)
  lit     rtmi_bake_lit_device (light and direct)
  direct  rtmi_bake_lit_device (direct alone: no gather ray)
light of `lit` with no lights is compared with `plain` bit for bit before anything is timed.  The shadow-ray counts stand beside
the path-ray count: lit's rays - plain's rays = the live candidates of the paths and of the elements, direct's rays = the elements'.
Usage: tools/bake_lit_pass.py [--reps N] [--size 2048] [--elements 1000000] [--rays 64] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from oracle import orc  # noqa: E402
from rust_raytrace_amd import raytrace as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--size", type=int, default=2048)
ap.add_argument("--elements", type=int, default=1000000)
ap.add_argument("--rays", type=int, default=64)
ap.add_argument("--out", default=None)
args = ap.parse_args()

DEPTH, SEED = 4, 1
F32 = np.float32
LIGHTS = [dict(orig=(-3.0, 6.0, 1.0), len2=0.5, color=(1.0, 0.9, 0.8)), dict(orig=(4.0, -6.0, 4.0), len2=0.0, color=(0.2, 0.3, 0.5))]
OBJ = os.path.join(ROOT, "tests", "golden", "teapot_tri.obj")
sc = R.canonical_scene(OBJ, gpu_build=0)
caster = R.HipRayCaster(seed=SEED)
stream = torch.cuda.current_stream().cuda_stream

o4, d4 = orc.primary_rays(args.size, args.size, orc.canonical_viewport(args.size, args.size), 1)
tri, t, face, _ = caster.trace(sc, o4, d4)
rec, _, _ = sc.triangles()
hit = np.nonzero(tri != 0)[0][: args.elements]
pos = np.ascontiguousarray(((d4[hit] * t[hit, None]).astype(F32) + o4[hit]).astype(F32))
nrm = np.zeros((len(hit), 4), F32)
nrm[:, :3] = rec[tri[hit], 3:6]
nrm[(face[hit] & 1) != 0] *= F32(-1.0)
M, K = len(hit), args.rays
tpos, tnrm = torch.from_numpy(pos).cuda(), torch.from_numpy(nrm).cuda()
params = caster.bake_params("points", rays=K, maxdepth=DEPTH)
lit, none = caster.lit_params(LIGHTS), caster.lit_params(())
light_a, light_b, direct_b, direct_c = (torch.zeros(M * 4, device="cuda") for _ in range(4))


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": [round(x, 4) for x in xs]}


legs = {"plain": lambda: caster.bake_device(sc, tpos, tnrm, params, light=light_a, stream=stream).stats,
        "lit": lambda: caster.bake_lit_device(sc, tpos, tnrm, params, lit, light=light_b, direct=direct_b, stream=stream).stats,
        "direct": lambda: caster.bake_lit_device(sc, tpos, tnrm, params, lit, direct=direct_c, stream=stream).stats}
caster.bake_lit_device(sc, tpos, tnrm, params, none, light=light_b, stream=stream)
legs["plain"]()
torch.cuda.synchronize()
assert torch.equal(light_a.view(torch.int32), light_b.view(torch.int32)), "without lights the lit bake must give the plain bake's bits"
for f in legs.values():  # warm-up: workspaces, code objects
    f()
torch.cuda.synchronize()
assert torch.equal(direct_b.view(torch.int32), direct_c.view(torch.int32)), "direct alone must give the same bits"
st = {k: [] for k in legs}
for _ in range(args.reps):
    for k, f in legs.items():
        st[k].append(f())
torch.cuda.synchronize()
res = {"tool": "tools/bake_lit_pass.py", "reps": args.reps, "view": args.size, "elements": M, "rays_per_element": K, "maxdepth": DEPTH,
       "lights": LIGHTS, "device": torch.cuda.get_device_name(0)}
for k, v in st.items():
    res[k] = summary([s["kernel_ms"] for s in v])
    res[k]["trace_ms"] = statistics.median([s["trace_ms"] for s in v])
    res[k]["rays"] = v[0]["rays"]
    res[k]["trace_launches"] = v[0]["trace_launches"]
res["path_rays"] = res["plain"]["rays"]
res["shadow_rays_paths"] = res["lit"]["rays"] - res["plain"]["rays"] - res["direct"]["rays"]
res["shadow_rays_elements"] = res["direct"]["rays"]
res["ratio_lit_to_plain"] = res["lit"]["median"] / res["plain"]["median"]
res["ratio_direct_to_plain"] = res["direct"]["median"] / res["plain"]["median"]
print(f"{M} elements x {K} rays: {res['path_rays']} path rays, {res['shadow_rays_paths']} shadow rays of the paths, "
      f"{res['shadow_rays_elements']} of the elements")
for k in legs:
    print(f"  {k:6s} {res[k]['median']:9.3f} ms [{res[k]['min']:.3f}, {res[k]['max']:.3f}], walks {res[k]['trace_ms']:.3f} ms")
print(f"  lit / plain = {res['ratio_lit_to_plain']:.3f}, direct alone / plain = {res['ratio_direct_to_plain']:.3f}", flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
