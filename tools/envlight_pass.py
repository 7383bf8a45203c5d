#!/usr/bin/env python3
"""What sampling the environment at matte hits buys and costs.  The canonical scene (teapot_tri.obj + two mirror
disks, octree 10/19) at the benchmark's size (--size x --size, maxdepth 5) under the default sky of --n x --n texels with the sun
narrowed to --sun-deg degrees of radius (--sun-color R G B replaces its colour; the sun's share of the sampler table's weight is
recorded).  Two calls on the same scene handle:
  envlight  rtmi_render_envlight_device
  plain     rtmi_render_samples_device, the environment path as it was (k_shade_samples_env)
Time: --reps alternated calls of --spp samples of the whole frame each, after a warm-up; stats.kernel_ms per sample.
Error: a crop of --crop x --crop pixels, in the middle of the frame or at --crop-row0 / --crop-col0 (whole rows are rendered, the columns are cut on the host)
against a plain reference of --ref-spp samples (its own seed); the mean squared error over the crop's rgb of each call at --spp
samples (equal samples), and of the plain call at the number of samples it renders in the time envlight needs for --spp (equal
time), each averaged over --seeds seeds.  The one condition: envlight's error at equal time is below the plain call's.
Usage: tools/envlight_pass.py [--reps 3] [--size 2048] [--spp 16] [--n 256] [--sun-deg 1] [--sun-color R G B] [--crop 256] [--crop-row0 R] [--crop-col0 C] [--ref-spp 4096] [--seeds 4] [--out FILE.json]"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from rust_raytrace_amd import raytrace as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--size", type=int, default=2048)
ap.add_argument("--spp", type=int, default=16)
ap.add_argument("--n", type=int, default=256)
ap.add_argument("--sun-deg", type=float, default=1.0)
ap.add_argument("--sun-color", type=float, nargs=3, default=None, help="the sun's colour (default: the sky's own, 40 36 28)")
ap.add_argument("--crop", type=int, default=256)
ap.add_argument("--crop-row0", type=int, default=None, help="first row of the crop (default: centred)")
ap.add_argument("--crop-col0", type=int, default=None, help="first column of the crop (default: centred)")
ap.add_argument("--ref-spp", type=int, default=4096)
ap.add_argument("--seeds", type=int, default=4)
ap.add_argument("--out", default=None)
args = ap.parse_args()

W = H = args.size
S, DEPTH = args.spp, 5
OBJ = os.path.join(ROOT, "tests", "golden", "teapot_tri.obj")
stream = torch.cuda.current_stream().cuda_stream
scene = R.canonical_scene(OBJ, gpu_build=0)
sky = dict(sun_cos=math.cos(math.radians(args.sun_deg)))
if args.sun_color:
    sky["sun_color"] = tuple(args.sun_color)
scene.set_sky(args.n, **sky)
q, total = R.HipRayCaster(seed=1).env_sampler(scene)
sun_share = float(q[q > 524288].astype(np.float64).sum() / total)  # the texels within a factor 2 of the brightest
full = (0, H, H, 0)
r0 = (H - args.crop) // 2 if args.crop_row0 is None else args.crop_row0
c0 = (W - args.crop) // 2 if args.crop_col0 is None else args.crop_col0
band = (r0, args.crop, args.crop, 0)  # the crop's rows


def call(kind, seed, spp, tile):
    """One call of `spp` samples of a frame of `spp`: (image (rows, W, 4) on the host, stats)"""
    c = R.HipRayCaster(seed=seed)
    vp = R.canonical_viewport(W, H, DEPTH, spp)
    n = tile[1] * W * 4
    acc, out = (torch.zeros(n, dtype=torch.float32, device="cuda:0") for _ in range(2))
    if kind == "envlight":
        st = c.walk_rays_envlight_device(vp, scene, acc, out, tile=tile, stream=stream).stats
    else:
        st = c.walk_samples_device(vp, scene, tile, 0, spp, acc.data_ptr(), out.data_ptr(), stream).stats
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(tile[1], W, 4), st


def crop(img):
    return img[:, c0:c0 + args.crop, :3].astype(np.float64)


# ---- time per sample, whole frame
for k in ("envlight", "plain"):
    call(k, 1, S, full)  # warm-up: upload, workspaces, the sampler table
ms = {"envlight": [], "plain": []}
rays = {}
for _ in range(args.reps):
    for k in ms:
        _, st = call(k, 1, S, full)
        ms[k].append(st["kernel_ms"] / S)
        rays[k] = st["rays"]
t_e, t_p = statistics.median(ms["envlight"]), statistics.median(ms["plain"])
print(f"ms per sample: envlight {t_e:.3f} {[round(x, 3) for x in ms['envlight']]}, plain {t_p:.3f} {[round(x, 3) for x in ms['plain']]}, "
      f"ratio {t_e / t_p:.3f}; rays {rays}", flush=True)

# ---- error against the reference
ref = crop(call("plain", 99, args.ref_spp, band)[0])
s_equal_time = max(1, round(S * t_e / t_p))
mse = {"envlight": [], "plain_equal_samples": [], "plain_equal_time": []}
for seed in range(1, args.seeds + 1):
    mse["envlight"].append(float(((crop(call("envlight", seed, S, band)[0]) - ref) ** 2).mean()))
    mse["plain_equal_samples"].append(float(((crop(call("plain", seed, S, band)[0]) - ref) ** 2).mean()))
    mse["plain_equal_time"].append(float(((crop(call("plain", seed, s_equal_time, band)[0]) - ref) ** 2).mean()))
m = {k: statistics.mean(v) for k, v in mse.items()}
print(f"mse over the {args.crop} x {args.crop} crop at {S} spp: envlight {m['envlight']:.5g}, plain {m['plain_equal_samples']:.5g} "
      f"(x {m['plain_equal_samples'] / m['envlight']:.2f}); plain at {s_equal_time} spp (equal time) {m['plain_equal_time']:.5g} "
      f"(x {m['plain_equal_time'] / m['envlight']:.2f})", flush=True)
res = {"tool": "tools/envlight_pass.py", "device": torch.cuda.get_device_name(0), "width": W, "height": H, "maxdepth": DEPTH,
       "samples_per_call": S, "table": args.n, "sun_radius_deg": args.sun_deg, "sun_color": args.sun_color or [40.0, 36.0, 28.0],
       "sun_share_of_sampler_weight": sun_share, "reps": args.reps,
       "ms_per_sample": {k: {"median": statistics.median(v), "all": [round(x, 4) for x in v]} for k, v in ms.items()},
       "envlight_over_plain_time": t_e / t_p, "rays_per_call": rays,
       "crop": args.crop, "crop_row0": r0, "crop_col0": c0, "reference_spp": args.ref_spp, "seeds": args.seeds, "plain_spp_at_equal_time": s_equal_time,
       "mse": {k: {"mean": statistics.mean(v), "all": v} for k, v in mse.items()},
       "plain_over_envlight_mse_equal_samples": m["plain_equal_samples"] / m["envlight"],
       "plain_over_envlight_mse_equal_time": m["plain_equal_time"] / m["envlight"],
       "envlight_wins_at_equal_time": m["envlight"] < m["plain_equal_time"]}
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
sys.exit(0 if res["envlight_wins_at_equal_time"] else 1)
