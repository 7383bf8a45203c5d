#!/usr/bin/env python3
"""What the a-trous denoiser costs.  The canonical scene of config 3 (teapot_tri.obj + two mirror disks, octree
10/19) at 2048 x 2048, rendered once at 4 spp with its feature buffers; everything stays on the device.  Legs:
  I<n>  rtmi_denoise_device with `n` iterations at the defaults otherwise (n = 1 .. 5); I<n> - I<n-1> is iteration n-1 alone
        (tap spacing 2^(n-1)).  I3 is the default call.
  M3    the default call with RTMI_DENOISE_DEMODULATE.
  S     rtmi_render_tile_device at depth 5 and 8 spp: one sample per pixel costs S / 8.  The criterion: I3 < S / 8.
One scene handle per entry of --lds runs the filter: L<k> = tap spacings up to k staged through LDS (RTMI_DENOISE_LDS_STEP=k when the handle is
made; 2 is the library's default, 0 = every tap a global load).  Every leg is warmed up first; then the legs alternate in one
process, --reps times.  A repetition's time is the device time between two HIP events around the call on the caller's stream
(S: rtmi_stats_t.kernel_ms, the same thing measured inside the library).  Reported: median [min, max] per leg, the effective
bandwidth on the compulsory 64 B per pixel and iteration (16 colour + 32 guides in, 16 out), and I3 / (S / 8).
--once runs each leg once after the warm-up and nothing else: the shape of a run under a kernel-trace profiler, whose k_accum
and k_atrous rows give the elementwise yardstick and the per-launch times.
--streams N sets rtmi_tuning_t.streams for the renders (default: the library's automatic rule); with 1 no two launches of a
call overlap, which is what a kernel-trace run needs to time k_accum alone.
Usage: tools/denoise_pass.py [--reps N] [--size 2048] [--lds 2,1,0] [--streams N] [--once] [--out FILE.json]"""
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
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--size", type=int, default=2048)
ap.add_argument("--lds", default="2,1,0")
ap.add_argument("--streams", type=int, default=0)
ap.add_argument("--once", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()

W = H = args.size
OBJ = os.path.join(ROOT, "tests", "golden", "teapot_tri.obj")
stream = torch.cuda.current_stream().cuda_stream
tile = (0, H, H, 0)
color, albedo, normal, out = (torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0") for _ in range(4))

handles = {}
for k in [int(x) for x in args.lds.split(",")]:  # the variable is read once, when a handle is made
    os.environ["RTMI_DENOISE_LDS_STEP"] = str(k)
    sc = R.canonical_scene(OBJ, gpu_build=0)
    c = R.HipRayCaster(seed=1, tuning={"streams": args.streams} if args.streams else None)
    c.upload(sc)
    handles[k] = (c, sc)
os.environ.pop("RTMI_DENOISE_LDS_STEP", None)
c0, sc0 = next(iter(handles.values()))
c0.walk_tile_device(R.canonical_viewport(W, H, 5, 4), sc0, tile, color.data_ptr(), stream)
c0.walk_features_device(R.canonical_viewport(W, H, 5, 4), sc0, tile, albedo.data_ptr(), normal.data_ptr(), None, 0, 4, stream)
torch.cuda.synchronize()
vp8 = R.canonical_viewport(W, H, 5, 8)
spp8 = torch.zeros_like(color)


def filt(c, sc, **kw):
    def f():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        c.denoise_device(W, H, color.data_ptr(), albedo.data_ptr(), normal.data_ptr(), out.data_ptr(), stream=stream, scene=sc, **kw)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)
    return f


legs = {}
for k, (c, sc) in handles.items():
    for n in range(1, 6):
        legs[f"L{k}.I{n}"] = filt(c, sc, iterations=n)
    legs[f"L{k}.M3"] = filt(c, sc, iterations=3, demodulate=True)
legs["S"] = lambda: c0.walk_tile_device(vp8, sc0, tile, spp8.data_ptr(), stream).stats["kernel_ms"]
for f in legs.values():  # warm-up: scratch image, code objects, workspaces
    f()
torch.cuda.synchronize()
times = {leg: [] for leg in legs}
for _ in range(1 if args.once else args.reps):
    for leg, f in legs.items():
        torch.cuda.synchronize()
        times[leg].append(f())
torch.cuda.synchronize()

GB = W * H * 64 / 1e9
res = {leg: {"median": statistics.median(t), "min": min(t), "max": max(t), "all": [round(x, 4) for x in t]} for leg, t in times.items()}
sample_ms = res["S"]["median"] / 8.0
print(f"{W}x{H}: S (depth 5, 8 spp) {res['S']['median']:.3f} ms [{res['S']['min']:.3f}, {res['S']['max']:.3f}] -> one sample per pixel {sample_ms:.3f} ms", flush=True)
summary = {}
for k in handles:
    per_iter, prev = [], 0.0
    for n in range(1, 6):
        m = res[f"L{k}.I{n}"]["median"]
        per_iter.append(m - prev)
        prev = m
    i3 = res[f"L{k}.I3"]
    summary[k] = {"iteration_ms": per_iter, "iteration_GBps": [GB / (t * 1e-3) if t > 0 else None for t in per_iter],
                  "default_call_ms": i3["median"], "default_call_GBps": 3 * GB / (i3["median"] * 1e-3),
                  "default_call_over_one_sample": i3["median"] / sample_ms, "demodulated_call_ms": res[f"L{k}.M3"]["median"]}
    print(f"LDS up to spacing {k}: default call {i3['median']:.3f} ms [{i3['min']:.3f}, {i3['max']:.3f}] = {summary[k]['default_call_GBps']:.0f} GB/s"
          f" on 64 B/pixel/iteration, {summary[k]['default_call_over_one_sample']:.3f} of one sample per pixel; demodulated {res[f'L{k}.M3']['median']:.3f} ms;"
          f" iterations " + ", ".join(f"{t:.3f}" for t in per_iter) + " ms", flush=True)

if args.out:
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/denoise_pass.py", "reps": 1 if args.once else args.reps, "width": W, "height": H, "streams": args.streams,
                   "device": torch.cuda.get_device_name(0), "bytes_per_pixel_and_iteration": 64, "one_sample_per_pixel_ms": sample_ms,
                   "legs": res, "by_lds_max_step": summary}, f, indent=1)
