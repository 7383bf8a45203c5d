#!/usr/bin/env python3
"""Cost and quality of adaptive sampling on config 3 (teapot_tri.obj 2048x2048, S = 64 spp at most, depth 5, seed 1, octree
10/19), legs alternated in one process, each timed --reps times (device milliseconds: the sum of the calls' kernel_ms):
  uniform   one rtmi_render_tile_device call at 64 spp (the reference frame)
  8x8       8 progressive passes of 8 samples (rtmi_render_samples_device)
  ad_nan    adaptive, m = 8, p = 8, abs_tol = NaN (every pixel to 64 in 8 passes: the cost of list mode)
  ad_*      adaptive at the tolerances of --tols (rel:abs pairs; 'default' = HipRayCaster's defaults)
  ad_*_s1   the same with one internal stream forced for every pass, pass 0 included (streams = 1)
For each adaptive leg: samples traced as a share of 64 * npix, active pixels per pass (from the count map), the share of
pixels bit-equal to the 64-spp frame and the RMS difference from it.  Usage: tools/adaptive_passes.py [--reps N] [--tols ...]"""
import argparse
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
ap.add_argument("--tols", default="default,0.02:0.004,0.05:0.01")
args = ap.parse_args()
W = H = 2048
S, M, P = 64, 8, 8
NPIX = W * H
scene = R.canonical_scene(os.path.join(ROOT, "tests", "golden", "teapot_tri.obj"), gpu_build=0)
vp = R.canonical_viewport(W, H, 5, S)
casters = {1: R.HipRayCaster(seed=1, tuning={"streams": 1}), 0: R.HipRayCaster(seed=1)}
c = casters[0]
c.upload(scene)
stream = torch.cuda.current_stream().cuda_stream
tile = (0, H, H, 0)
dev = "cuda:0"
buf = {k: torch.zeros((H, W, 4), dtype=torch.float32, device=dev) for k in ("ref", "out", "accum", "sumsq")}
cnt = torch.zeros((H, W), dtype=torch.int32, device=dev)

tols = {"nan": (0.0, float("nan"))}
for t in args.tols.split(","):
    tols[t] = (R.HipRayCaster.ADAPTIVE_REL_TOL, R.HipRayCaster.ADAPTIVE_ABS_TOL) if t == "default" else tuple(float(x) for x in t.split(":"))
legs = ["uniform", "8x8"] + [f"ad_{t}" for t in tols] + [f"ad_{t}_s1" for t in tols if t != "nan"]


def run(leg):
    if leg == "uniform":
        ctx = c.walk_tile_device(vp, scene, tile, buf["ref"].data_ptr(), stream)
        return ctx.stats["kernel_ms"], ctx.total_rays, None
    if leg == "8x8":
        ms, rays = 0.0, 0
        for k0 in range(0, S, 8):
            ctx = c.walk_samples_device(vp, scene, tile, k0, 8, buf["accum"].data_ptr(), buf["out"].data_ptr(), stream)
            ms += ctx.stats["kernel_ms"]
            rays += ctx.total_rays
        return ms, rays, None
    name = leg[3:]
    s1 = name.endswith("_s1")
    rel, ab = tols[name[:-3] if s1 else name]
    cc = casters[1 if s1 else 0]
    ctx = cc.walk_adaptive_device(vp, scene, tile, buf["accum"].data_ptr(), buf["sumsq"].data_ptr(), cnt.data_ptr(),
                                  buf["out"].data_ptr(), stream, M, P, rel, ab)
    return ctx.stats["kernel_ms"], ctx.total_rays, ctx


times = {leg: [] for leg in legs}
info = {}
for leg in legs:
    run(leg)  # warm-up (workspaces, code objects)
for _ in range(max(1, args.reps)):
    for leg in legs:  # alternated
        ms, rays, ctx = run(leg)
        times[leg].append(ms)
        if leg not in info:
            torch.cuda.synchronize()
            d = {"rays": rays}
            if ctx is not None:
                img = buf["out"].cpu().numpy()
                counts = cnt.cpu().numpy().view(np.uint32)
                ref = buf["ref"].cpu().numpy()
                bounds = [0] + list(range(M, S, P))
                d.update(passes=ctx.passes, samples=int(ctx.samples), unconverged=ctx.unconverged,
                         active=[int((counts > b).sum()) for b in bounds][:ctx.passes],
                         equal=float((img.view(np.uint32) == ref.view(np.uint32)).all(-1).mean()),
                         rms=float(np.sqrt(np.mean((img[..., :3].astype(np.float64) - ref[..., :3]) ** 2))),
                         streams=ctx.stats["streams"])
            info[leg] = d
torch.cuda.synchronize()
base = statistics.median(times["uniform"])
print(f"config 3: {W}x{H}, S = {S}, m = {M}, p = {P}; device ms over {args.reps} alternated reps (median [min, max])")
for leg in legs:
    t = times[leg]
    med = statistics.median(t)
    line = f"{leg:>22}: {med:8.1f} ms [{min(t):7.1f}, {max(t):7.1f}]  {med / base:.3f} x uniform  {info[leg]['rays']} rays"
    if "samples" in info[leg]:
        d = info[leg]
        tol = tols[leg[3:-3] if leg.endswith("_s1") else leg[3:]]
        line += (f"\n{'':>24}rel_tol {tol[0]:g} abs_tol {tol[1]:g}: samples {d['samples'] / (S * NPIX):.3f} of 64*npix, {d['passes']} passes, "
                 f"streams {d['streams']}, unconverged {d['unconverged']}\n{'':>24}active per pass {d['active']}\n"
                 f"{'':>24}bit-equal to the 64-spp frame {d['equal']:.4f} of pixels, RMS difference {d['rms']:.3e}")
    print(line)
nan = info["ad_nan"]
assert nan["rays"] == info["uniform"]["rays"] and nan["equal"] == 1.0, "abs_tol = NaN must be the uniform frame"
print("ad_nan: bit-equal to the uniform frame, same rays")
