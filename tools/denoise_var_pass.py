#!/usr/bin/env python3
"""What variance-guided denoising costs.  The canonical scene of config 3 (teapot_tri.obj + two mirror disks,
octree 10/19) at 2048 x 2048: one adaptive render at the default tolerances (S = 32, m = p = 8) with its variance image and the
features of its first 8 samples; everything stays on the device.  Legs:
  V     rtmi_variance_device (52 B per pixel: accum 16 + sumsq 16 + count 4 in, 16 out).
  I<n>  rtmi_denoise_var_device with `n` iterations and var_out, defaults otherwise (n = 1 .. 5); I<n> - I<n-1> is iteration n-1
        alone (tap spacing 2^(n-1)).  I1 is the default call.
  P<n>  the plain rtmi_denoise_device with `n` iterations on the same frame (n = 1, 3): the yardstick.
  A     rtmi_render_adaptive (host variant: the adaptive render and the copy of image and counts to the host), wall ms.
  AD    rtmi_render_adaptive_denoised, wall ms: A plus variance, features, filter.
One scene handle per entry of --lds runs the filter: L<k> = tap spacings up to k staged through LDS (RTMI_DENOISE_VAR_LDS_STEP=k
when the handle is made; 0 = every tap four global loads).  Every leg is warmed up first; then the legs alternate in one
process, --reps times.  Device legs: ms between two HIP events around the call.  Reported: median [min, max] per leg and the
effective bandwidth on the compulsory 112 B per pixel and iteration (colour 16 + variance 16 + guides 32 in; colour 16 + variance
16 out, and 16 more for var_out's ping-pong).
--once runs each leg once after the warm-up: the shape of a run under a kernel-trace profiler.
Usage: tools/denoise_var_pass.py [--reps N] [--size 2048] [--lds 2,1,0] [--once] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from rust_raytrace_amd import raytrace as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--size", type=int, default=2048)
ap.add_argument("--lds", default="2,1,0")
ap.add_argument("--once", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()

W = H = args.size
S, M, P = 32, 8, 8
OBJ = os.path.join(ROOT, "tests", "golden", "teapot_tri.obj")
stream = torch.cuda.current_stream().cuda_stream
tile = (0, H, H, 0)
accum, sumsq, color, var, albedo, normal, out, vout = (torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0") for _ in range(8))
counts = torch.zeros((H, W), dtype=torch.int32, device="cuda:0")

handles = {}
for k in [int(x) for x in args.lds.split(",")]:  # the variable is read once, when a handle is made
    os.environ["RTMI_DENOISE_VAR_LDS_STEP"] = str(k)
    sc = R.canonical_scene(OBJ, gpu_build=0)
    c = R.HipRayCaster(seed=1)
    c.upload(sc)
    handles[k] = (c, sc)
os.environ.pop("RTMI_DENOISE_VAR_LDS_STEP", None)
c0, sc0 = next(iter(handles.values()))
vp = R.canonical_viewport(W, H, 5, S)
ctx = c0.walk_adaptive_device(vp, sc0, tile, accum.data_ptr(), sumsq.data_ptr(), counts.data_ptr(), color.data_ptr(), stream,
                              min_samples=M, pass_samples=P)
c0.walk_features_device(vp, sc0, tile, albedo.data_ptr(), normal.data_ptr(), None, 0, M, stream)
torch.cuda.synchronize()
host_img, host_cnt = np.zeros((H, W, 4), np.float32), np.zeros((H, W), np.uint32)


def timed(call):
    def f():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)
    return f


def wall(call):
    def f():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        return (time.perf_counter() - t0) * 1e3
    return f


legs = {"V": timed(lambda: c0.variance_device(accum.data_ptr(), sumsq.data_ptr(), counts.data_ptr(), W * H, var.data_ptr(), stream=stream, scene=sc0))}
for k, (c, sc) in handles.items():
    for n in range(1, 6):
        legs[f"L{k}.I{n}"] = timed(lambda c=c, sc=sc, n=n: c.denoise_var_device(
            W, H, color.data_ptr(), albedo.data_ptr(), normal.data_ptr(), var.data_ptr(), out.data_ptr(), var_out_ptr=vout.data_ptr(),
            stream=stream, scene=sc, iterations=n))
for n in (1, 3):
    legs[f"P{n}"] = timed(lambda n=n: c0.denoise_device(W, H, color.data_ptr(), albedo.data_ptr(), normal.data_ptr(), out.data_ptr(),
                                                        stream=stream, scene=sc0, iterations=n))
legs["A"] = wall(lambda: c0.walk_rays_adaptive(vp, sc0, host_img, min_samples=M, pass_samples=P, counts=host_cnt))
legs["AD"] = wall(lambda: c0.walk_rays_adaptive_denoised(vp, sc0, host_img, min_samples=M, pass_samples=P, counts=host_cnt))
legs["V"]()  # the variance image the filter legs read
for f in legs.values():  # warm-up: scratch images, code objects, workspaces
    f()
torch.cuda.synchronize()
times = {leg: [] for leg in legs}
for _ in range(1 if args.once else args.reps):
    for leg, f in legs.items():
        torch.cuda.synchronize()
        times[leg].append(f())
torch.cuda.synchronize()

GB = W * H * 112 / 1e9
res = {leg: {"median": statistics.median(t), "min": min(t), "max": max(t), "all": [round(x, 4) for x in t]} for leg, t in times.items()}


def show(leg):
    r = res[leg]
    return f"{r['median']:.3f} ms [{r['min']:.3f}, {r['max']:.3f}]"


print(f"{W}x{H}, adaptive S={S} m=p={M}: {ctx.passes} passes, mean {ctx.samples / (W * H):.2f} spp, {ctx.unconverged} unconverged", flush=True)
print(f"V (k_variance) {show('V')} = {W * H * 52 / 1e9 / (res['V']['median'] * 1e-3):.0f} GB/s on 52 B/pixel", flush=True)
print(f"plain filter: 1 iteration {show('P1')}, default call (3) {show('P3')}", flush=True)
summary = {}
for k in handles:
    per_iter, prev = [], 0.0
    for n in range(1, 6):
        m = res[f"L{k}.I{n}"]["median"]
        per_iter.append(m - prev)
        prev = m
    summary[k] = {"iteration_ms": per_iter, "iteration_GBps": [GB / (t * 1e-3) if t > 0 else None for t in per_iter],
                  "default_call_ms": res[f"L{k}.I1"]["median"], "three_iterations_ms": res[f"L{k}.I3"]["median"],
                  "three_iterations_over_plain": res[f"L{k}.I3"]["median"] / res["P3"]["median"]}
    print(f"LDS up to spacing {k}: default call (1 iteration) {show(f'L{k}.I1')}, 3 iterations {show(f'L{k}.I3')} = "
          f"{summary[k]['three_iterations_over_plain']:.2f} x the plain filter's; iterations " + ", ".join(f"{t:.3f}" for t in per_iter) + " ms = "
          + ", ".join(f"{GB / (t * 1e-3):.0f}" for t in per_iter) + " GB/s on 112 B/pixel", flush=True)
print(f"rtmi_render_adaptive {show('A')}; rtmi_render_adaptive_denoised {show('AD')} (wall, host copies included)", flush=True)

if args.out:
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/denoise_var_pass.py", "reps": 1 if args.once else args.reps, "width": W, "height": H,
                   "device": torch.cuda.get_device_name(0), "bytes_per_pixel_and_iteration": 112, "adaptive": {"S": S, "m": M, "p": P,
                   "passes": ctx.passes, "samples": int(ctx.samples), "unconverged": int(ctx.unconverged)},
                   "legs": res, "by_lds_max_step": summary}, f, indent=1)
