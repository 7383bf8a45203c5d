#!/usr/bin/env python3
"""What sampling emissive triangles at matte hits buys and costs.  The canonical scene (teapot_tri.obj + two mirror
disks, octree 10/19) plus a Solid quad lamp of 2 --half x 2 --half above the teapot and towards the camera (tests/emissive_cases.py's
recipe_teapot_lamp; radiance --radiance R G B), at the benchmark's size (--size x --size, maxdepth 5).  Two calls on the same scene
handle, both on the per-pass pipeline:
  emissive  rtmi_render_emissive_device
  plain     rtmi_render_samples_device with tuning pipeline = 1
Time: --reps alternated calls of --spp samples of the whole frame each, after a warm-up; stats.kernel_ms per sample.
Error: a crop of --crop x --crop pixels, in the middle of the frame or at --crop-row0 / --crop-col0 (whole rows are rendered, the
columns are cut on the host) against a plain reference of --ref-spp samples (its own seed); the root mean squared error over the
crop's rgb of each call at --spp samples (equal samples), and of the plain call at the number of samples it renders in the time the
emissive call needs for --spp (equal time), each averaged over --seeds seeds.  The reference's own noise is in every figure alike.
The exit status says whether the emissive call's error at equal time is below the plain call's.
Usage: tools/emissive_pass.py [--reps 3] [--size 2048] [--spp 16] [--half 0.75] [--radiance R G B] [--crop 256] [--crop-row0 R]
       [--crop-col0 C] [--ref-spp 4096] [--seeds 4] [--out FILE.json]"""
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
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--size", type=int, default=2048)
ap.add_argument("--spp", type=int, default=16)
ap.add_argument("--half", type=float, default=0.75, help="half the lamp's edge")
ap.add_argument("--radiance", type=float, nargs=3, default=(30.0, 28.0, 26.0))
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


def build():
    s = R.Scene(with_dummy=True)
    s.extend_parse_obj(OBJ, [0.0, 0.5, 5.0], 1.0, R.create_transform(R.unit([0.0, 0.3, 1.0]), R.to_radians(270.0)),
                       R.SurfaceKind.Matte(R.make_color(252, 119, 0), 0.2), 0.05)
    h = args.half
    x = lambda y, z: 4.3 + 0.03 * y - 0.25 * (z - 2.0)
    q = [np.array([x(y, z), y, z], np.float32) for y, z in ((0.3 - h, 2.0 - h), (0.3 + h, 2.0 - h), (0.3 + h, 2.0 + h), (0.3 - h, 2.0 + h))]
    lamp = R.SurfaceKind.Solid(np.asarray(args.radiance, np.float32))
    first = s.num_tris()
    s.push_triangle(np.array([q[0], q[1], q[2]]), lamp, 0.0)
    s.push_triangle(np.array([q[0], q[2], q[3]]), lamp, 0.0)
    side = R.SurfaceKind.Matte(R.make_color(40, 40, 40), 0.2)
    s.extend_make_disk([4.0, 4.0, 7.0], R.unit([-0.3, -0.55, -0.5]), 2.0, 0.1, 50, R.SurfaceKind.Reflective(0.0002, R.make_color(230, 230, 230), 0.7), side, -1.0)
    s.extend_make_disk([4.0, -3.0, 5.0], R.unit([-0.5, 2.0, -0.5]), 1.0, 0.04, 50, R.SurfaceKind.Reflective(0.002, R.make_color(230, 230, 230), 0.7), side, -1.0)
    s.populate_triangle_numbers()
    s.build_bounding_box([0.0, 0.0, 20.1], 20.0, 10, 19, 0, gpu_device=0)
    s.set_emitters(np.array([first, first + 1]))
    return s


scene = build()
full = (0, H, H, 0)
r0 = (H - args.crop) // 2 if args.crop_row0 is None else args.crop_row0
c0 = (W - args.crop) // 2 if args.crop_col0 is None else args.crop_col0
band = (r0, args.crop, args.crop, 0)  # the crop's rows


def call(kind, seed, spp, tile):
    """One call of `spp` samples of a frame of `spp`: (image (rows, W, 4) on the host, stats)"""
    c = R.HipRayCaster(seed=seed, tuning=dict(pipeline=1))
    vp = R.canonical_viewport(W, H, DEPTH, spp)
    n = tile[1] * W * 4
    acc, out = (torch.zeros(n, dtype=torch.float32, device="cuda:0") for _ in range(2))
    if kind == "emissive":
        st = c.walk_rays_emissive_device(vp, scene, acc, out, tile=tile, stream=stream).stats
    else:
        st = c.walk_samples_device(vp, scene, tile, 0, spp, acc.data_ptr(), out.data_ptr(), stream).stats
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(tile[1], W, 4), st


def crop(img):
    return img[:, c0:c0 + args.crop, :3].astype(np.float64)


# ---- time per sample, whole frame
for k in ("emissive", "plain"):
    _, st = call(k, 1, S, full)  # warm-up: upload, workspaces, the lamps' tables
    assert st["pipeline"] == 1
ms = {"emissive": [], "plain": []}
rays = {}
for _ in range(args.reps):
    for k in ms:
        _, st = call(k, 1, S, full)
        ms[k].append(st["kernel_ms"] / S)
        rays[k] = st["rays"]
t_e, t_p = statistics.median(ms["emissive"]), statistics.median(ms["plain"])
print(f"ms per sample: emissive {t_e:.3f} {[round(x, 3) for x in ms['emissive']]}, plain {t_p:.3f} {[round(x, 3) for x in ms['plain']]}, "
      f"ratio {t_e / t_p:.3f}; rays {rays}", flush=True)

# ---- error against the reference
ref = crop(call("plain", 99, args.ref_spp, band)[0])
s_equal_time = max(1, round(S * t_e / t_p))
mse = {"emissive": [], "plain_equal_samples": [], "plain_equal_time": []}
for seed in range(1, args.seeds + 1):
    mse["emissive"].append(float(((crop(call("emissive", seed, S, band)[0]) - ref) ** 2).mean()))
    mse["plain_equal_samples"].append(float(((crop(call("plain", seed, S, band)[0]) - ref) ** 2).mean()))
    mse["plain_equal_time"].append(float(((crop(call("plain", seed, s_equal_time, band)[0]) - ref) ** 2).mean()))
rms = {k: float(np.sqrt(statistics.mean(v))) for k, v in mse.items()}
print(f"rms error over the {args.crop} x {args.crop} crop at {S} spp: emissive {rms['emissive']:.5g}, plain {rms['plain_equal_samples']:.5g} "
      f"(x {rms['plain_equal_samples'] / rms['emissive']:.2f}); plain at {s_equal_time} spp (equal time) {rms['plain_equal_time']:.5g} "
      f"(x {rms['plain_equal_time'] / rms['emissive']:.2f}); mean of the reference crop {ref.mean():.4f}", flush=True)
res = {"tool": "tools/emissive_pass.py", "device": torch.cuda.get_device_name(0), "width": W, "height": H, "maxdepth": DEPTH,
       "samples_per_call": S, "lamp_half_edge": args.half, "radiance": list(args.radiance), "reps": args.reps,
       "ms_per_sample": {k: {"median": statistics.median(v), "all": [round(x, 4) for x in v]} for k, v in ms.items()},
       "emissive_over_plain_time": t_e / t_p, "rays_per_call": rays,
       "crop": args.crop, "crop_row0": r0, "crop_col0": c0, "reference_spp": args.ref_spp, "reference_crop_mean": float(ref.mean()),
       "seeds": args.seeds, "plain_spp_at_equal_time": s_equal_time,
       "mse": {k: {"mean": statistics.mean(v), "all": v} for k, v in mse.items()}, "rms": rms,
       "plain_over_emissive_rms_equal_samples": rms["plain_equal_samples"] / rms["emissive"],
       "plain_over_emissive_rms_equal_time": rms["plain_equal_time"] / rms["emissive"],
       "emissive_wins_at_equal_time": rms["emissive"] < rms["plain_equal_time"]}
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
sys.exit(0 if res["emissive_wins_at_equal_time"] else 1)
