#!/usr/bin/env python3
"""What making the gather rays of a bake on the device saves.  The canonical scene (teapot_tri.obj + two mirror
disks, octree 10/19); the texels are the teapot's first hits of the canonical --size x --size view at one sample per pixel (the
handle's own rtmi_trace), each with the normal of the face that was hit.  For every K of --rays, maxdepth 4, two routes to the
same `light` (compared bit for bit before anything is timed):
  A  rtmi_bake_device: 32 B per texel on the device, everything else made there
  B  the route without it: tests/bake_ref.py builds the K rays per texel on the host (timed once: host_gen_s; a reference
     implementation in NumPy and Python, not a tuned generator), they are uploaded (upload_ms, pageable host memory) and
     rtmi_render_rays_device traces them with keys = NULL, group = K (rays_kernel_ms)
A and B's device leg are alternated --reps times in one process after a warm-up; each reports stats.kernel_ms (HIP events on
the caller's stream).  The traced work is identical, so bake / rays says what the generator costs against reading resident rays,
and bake / (rays + upload) what the removed transfer is worth; host_gen_s is reported beside them, not folded in.
Usage: tools/bake_pass.py [--reps N] [--size 256] [--rays 4,16,64] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from oracle import orc  # noqa: E402
from rust_raytrace_amd import raytrace as R  # noqa: E402
import bake_ref as BR  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--rays", default="4,16,64")
ap.add_argument("--out", default=None)
args = ap.parse_args()

DEPTH, SEED, BIAS = 4, 1, 0.001
F32 = np.float32
OBJ = os.path.join(ROOT, "tests", "golden", "teapot_tri.obj")
sc = R.canonical_scene(OBJ, gpu_build=0)
caster = R.HipRayCaster(seed=SEED)
stream = torch.cuda.current_stream().cuda_stream

# the texels: first hits of the view on the teapot (triangles 1 .. 6320 of the scene), the hit face's normal
o4, d4 = orc.primary_rays(args.size, args.size, orc.canonical_viewport(args.size, args.size), 1)
tri, t, face, _ = caster.trace(sc, o4, d4)
rec, _, _ = sc.triangles()
hit = np.nonzero((tri != 0) & (tri <= 6320))[0]
pos = np.ascontiguousarray(((d4[hit] * t[hit, None]).astype(F32) + o4[hit]).astype(F32))
nrm = np.zeros((len(hit), 4), F32)
nrm[:, :3] = rec[tri[hit], 3:6]
nrm[(face[hit] & 1) != 0] *= F32(-1.0)
M = len(hit)
tpos, tnrm = torch.from_numpy(pos).cuda(), torch.from_numpy(nrm).cuda()


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": [round(x, 4) for x in xs]}


res = {"tool": "tools/bake_pass.py", "reps": args.reps, "view": args.size, "texels": M, "maxdepth": DEPTH, "bias": BIAS,
       "device": torch.cuda.get_device_name(0), "rays_per_texel": {}}
for K in [int(x) for x in args.rays.split(",")]:
    n = M * K
    params = caster.bake_params("points", rays=K, maxdepth=DEPTH, bias=BIAS)
    light_a = torch.zeros(M * 4, device="cuda")
    light_b = torch.zeros(M * 4, device="cuda")
    t0 = time.perf_counter()
    r = BR.rays(orc, SEED, pos, nrm, K, 0, BIAS)
    host_gen_s = time.perf_counter() - t0

    def upload():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a, b = torch.from_numpy(r.orig).cuda(), torch.from_numpy(r.dir).cuda()
        torch.cuda.synchronize()
        return a, b, (time.perf_counter() - t0) * 1e3

    to, td, _ = upload()
    legs = {"bake": lambda: caster.bake_device(sc, tpos, tnrm, params, light=light_a, stream=stream).stats,
            "rays": lambda: caster.walk_rays_explicit_device(sc, to, td, DEPTH, group=K, mean=light_b, stream=stream).stats}
    for f in legs.values():  # warm-up: workspaces, code objects
        f()
    torch.cuda.synchronize()
    assert torch.equal(light_a.view(torch.int32), light_b.view(torch.int32)), "the two routes must give the same bits"
    st = {k: [] for k in legs}
    up = []
    for _ in range(args.reps):
        for k, f in legs.items():
            st[k].append(f())
        up.append(upload()[2])
    torch.cuda.synchronize()
    m = {k: summary([s["kernel_ms"] for s in v]) for k, v in st.items()}
    m["trace_ms"] = {k: statistics.median([s["trace_ms"] for s in v]) for k, v in st.items()}
    m["traced_rays"] = {k: v[0]["rays"] for k, v in st.items()}
    m["upload_ms"] = summary(up)
    m["upload_bytes"] = 32 * n
    m["element_bytes"] = 32 * M
    m["host_gen_s"] = host_gen_s
    m["ratio_bake_to_rays"] = m["bake"]["median"] / m["rays"]["median"]
    m["ratio_bake_to_rays_plus_upload"] = m["bake"]["median"] / (m["rays"]["median"] + m["upload_ms"]["median"])
    res["rays_per_texel"][str(K)] = m
    assert m["traced_rays"]["bake"] == m["traced_rays"]["rays"]
    print(f"K = {K}: {M} texels, {n} gather rays ({m['traced_rays']['bake']} traced); bake {m['bake']['median']:.3f} ms "
          f"[{m['bake']['min']:.3f}, {m['bake']['max']:.3f}], rays resident {m['rays']['median']:.3f} ms [{m['rays']['min']:.3f}, "
          f"{m['rays']['max']:.3f}], upload of {32 * n / 1e6:.1f} MB {m['upload_ms']['median']:.3f} ms, host generation {host_gen_s:.2f} s; "
          f"bake / rays = {m['ratio_bake_to_rays']:.3f}, bake / (rays + upload) = {m['ratio_bake_to_rays_plus_upload']:.3f}", flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
