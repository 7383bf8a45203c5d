#!/usr/bin/env python3
"""What a glass teapot costs.  The canonical scene (teapot_tri.obj + two mirror disks, octree 10/19) at the
benchmark's size (--size x --size, S = --spp, maxdepth 5, seed 1), three legs, each on its own scene handle, alternated --reps
times in one process after a warm-up; every leg renders the whole frame into device memory with rtmi_render_tile_device and reports
stats.kernel_ms (HIP events on the caller's stream):
  glass     the teapot Dielectric(1.5, orange, 0.9): the per-pass pipeline with k_shade_glass (a scene with a dielectric always)
  matte_p1  the teapot Matte as the benchmark has it, tuning.pipeline = 1: the same per-pass pipeline with k_shade
  matte_p3  the teapot Matte, tuning.pipeline = 3: the path kernels, what the benchmark runs
matte_p1 and matte_p3 are existing code: the baseline.  glass / matte_p1 is what the glass arm and the longer glass paths cost on
equal terms, glass / matte_p3 what a caller pays for making the teapot glass.  Per leg: frame time, rays, rays per path, and the
closest-hit launches' time split into primary and bounce passes where the pipeline reports it.
--png FILE also renders a clear-glass teapot (Dielectric(1.5, white, 1.0), --png-size, 64 spp, maxdepth 12) for a human to look at.
Usage: tools/glass_pass.py [--reps N] [--size 2048] [--spp 64] [--out FILE.json] [--png FILE.png]"""
import argparse
import json
import os
import statistics
import struct
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from rust_raytrace_amd import raytrace as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--size", type=int, default=2048)
ap.add_argument("--spp", type=int, default=64)
ap.add_argument("--out", default=None)
ap.add_argument("--png", default=None)
ap.add_argument("--png-size", type=int, default=512)
args = ap.parse_args()

W = H = args.size
S, DEPTH, SEED = args.spp, 5, 1
OBJ = os.path.join(ROOT, "tests", "golden", "teapot_tri.obj")
ORANGE = R.make_color(252, 119, 0)
stream = torch.cuda.current_stream().cuda_stream


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": [round(x, 4) for x in xs]}


def write_png(path, rgb):
    """An 8-bit RGB PNG from an (h, w, 3) uint8 array"""
    h, w, _ = rgb.shape
    raw = b"".join(b"\x00" + rgb[r].tobytes() for r in range(h))
    chunk = lambda tag, data: struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw, 6)) +
                chunk(b"IEND", b""))


glass_scene = R.canonical_scene(OBJ, teapot_surface=R.SurfaceKind.Dielectric(1.5, ORANGE, 0.9), gpu_build=0)
matte1, matte3 = R.canonical_scene(OBJ, gpu_build=0), R.canonical_scene(OBJ, gpu_build=0)
out = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda:0")
torch.cuda.synchronize()
vp = R.canonical_viewport(W, H, DEPTH, S)
tile = (0, H, H, 0)
c0 = R.HipRayCaster(seed=SEED)
c1 = R.HipRayCaster(seed=SEED, tuning=dict(pipeline=1))
c3 = R.HipRayCaster(seed=SEED, tuning=dict(pipeline=3))
legs = {
    "glass": lambda: c0.walk_tile_device(vp, glass_scene, tile, out.data_ptr(), stream).stats,
    "matte_p1": lambda: c1.walk_tile_device(vp, matte1, tile, out.data_ptr(), stream).stats,
    "matte_p3": lambda: c3.walk_tile_device(vp, matte3, tile, out.data_ptr(), stream).stats,
}
for f in legs.values():  # warm-up: uploads, workspaces, code objects
    f()
st = {k: [] for k in legs}
for _ in range(args.reps):
    for k, f in legs.items():
        st[k].append(f())
torch.cuda.synchronize()
assert st["glass"][0]["pipeline"] == 1 and st["matte_p1"][0]["pipeline"] == 1 and st["matte_p3"][0]["pipeline"] == 3
assert st["glass"][0]["slow_paths"] == 0
res = {"tool": "tools/glass_pass.py", "reps": args.reps, "width": W, "height": H, "samples_per_pixel": S, "maxdepth": DEPTH, "seed": SEED,
       "device": torch.cuda.get_device_name(0), "legs": {}}
for k, v in st.items():
    m = {"kernel_ms": summary([s["kernel_ms"] for s in v]), "rays": v[0]["rays"], "rays_per_path": v[0]["rays"] / (W * H * S),
         "pipeline": v[0]["pipeline"], "streams": v[0]["streams"], "trace_launches": v[0]["trace_launches"],
         "trace_ms": statistics.median([s["trace_ms"] for s in v]), "primary_ms": statistics.median([s["primary_ms"] for s in v]),
         "bounce_ms": statistics.median([s["bounce_ms"] for s in v])}
    m["mrays_per_s"] = m["rays"] / (m["kernel_ms"]["median"] * 1e3)
    res["legs"][k] = m
    print(f"{k}: {m['kernel_ms']['median']:.3f} ms [{m['kernel_ms']['min']:.3f}, {m['kernel_ms']['max']:.3f}], {m['rays']} rays "
          f"({m['rays_per_path']:.3f} per path, {m['mrays_per_s']:.1f} Mrays/s), trace {m['trace_ms']:.3f} ms summed over {m['streams']} stream(s) "
          f"(primary {m['primary_ms']:.3f}, bounce {m['bounce_ms']:.3f}), pipeline {m['pipeline']}", flush=True)
g, p1, p3 = (res["legs"][k]["kernel_ms"]["median"] for k in ("glass", "matte_p1", "matte_p3"))
res["glass_over_matte_p1"], res["glass_over_matte_p3"] = g / p1, g / p3
print(f"glass / matte_p1 = {g / p1:.3f}, glass / matte_p3 = {g / p3:.3f}", flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
if args.png:
    n = args.png_size
    clear = R.canonical_scene(OBJ, teapot_surface=R.SurfaceKind.Dielectric(1.5, R.make_color(255, 255, 255), 1.0), gpu_build=0)
    img = np.zeros((n, n, 4), np.float32)
    ctx = c0.walk_rays(R.canonical_viewport(n, n, 12, 64), clear, img)
    write_png(args.png, R.quantize(img).reshape(n, n, 3))
    print(f"{args.png}: {n} x {n} x 64 spp, maxdepth 12, {ctx.total_rays} rays, {ctx.stats['kernel_ms']:.1f} ms", flush=True)
