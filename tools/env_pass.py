#!/usr/bin/env python3
"""What an environment costs per frame.  The canonical scene (teapot_tri.obj + two mirror disks, octree 10/19) at the
benchmark's size (--size x --size, S = --spp, maxdepth 5, seed 1), three legs, each on its own scene handle, alternated --reps times
in one process after a warm-up; every leg renders the whole frame into device memory with rtmi_render_tile_device and reports
stats.kernel_ms (HIP events on the caller's stream):
  env       the scene under a generated sky (Scene.set_sky(--n)): the per-pass pipeline with k_shade_env (a scene with an
            environment always)
  plain_p1  the same scene without one, tuning.pipeline = 1: the same per-pass pipeline with k_shade
  plain_p3  the same scene without one, tuning.pipeline = 3: the path kernels, what the benchmark runs
plain_p1 and plain_p3 are existing code: the baseline.  env - plain_p1 is what the lookup costs on equal terms (the rays are the
same: the environment moves colours, not rays), env / plain_p3 what a caller pays for lighting the scene by a map.
The shading launches' share: further frames of env and of plain_p1 each under the library's own timer of the
closest-hit launches (stats.trace_ms, summed over the streams) on ONE stream, where frame - trace is the time of everything that is
not a walk -- generation, shading, accumulation -- and the difference of that remainder between the two legs is the k_shade*_env
kernels' extra time; its share of the frame difference is reported.  (Kernel-by-kernel times need a profiler run of their own.)
Usage: tools/env_pass.py [--reps N] [--size 2048] [--spp 64] [--n 256] [--out FILE.json]"""
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
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--size", type=int, default=2048)
ap.add_argument("--spp", type=int, default=64)
ap.add_argument("--n", type=int, default=256)
ap.add_argument("--out", default=None)
args = ap.parse_args()

W = H = args.size
S, DEPTH, SEED = args.spp, 5, 1
OBJ = os.path.join(ROOT, "tests", "golden", "teapot_tri.obj")
stream = torch.cuda.current_stream().cuda_stream


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": [round(x, 4) for x in xs]}


env_scene = R.canonical_scene(OBJ, gpu_build=0)
env_scene.set_sky(args.n)
plain1, plain3 = R.canonical_scene(OBJ, gpu_build=0), R.canonical_scene(OBJ, gpu_build=0)
out = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda:0")
torch.cuda.synchronize()
vp = R.canonical_viewport(W, H, DEPTH, S)
tile = (0, H, H, 0)
c0 = R.HipRayCaster(seed=SEED)
c1 = R.HipRayCaster(seed=SEED, tuning=dict(pipeline=1))
c3 = R.HipRayCaster(seed=SEED, tuning=dict(pipeline=3))
legs = {
    "env": lambda: c0.walk_tile_device(vp, env_scene, tile, out.data_ptr(), stream).stats,
    "plain_p1": lambda: c1.walk_tile_device(vp, plain1, tile, out.data_ptr(), stream).stats,
    "plain_p3": lambda: c3.walk_tile_device(vp, plain3, tile, out.data_ptr(), stream).stats,
}
for f in legs.values():  # warm-up: uploads, workspaces, code objects
    f()
st = {k: [] for k in legs}
for _ in range(args.reps):
    for k, f in legs.items():
        st[k].append(f())
torch.cuda.synchronize()
assert st["env"][0]["pipeline"] == 1 and st["plain_p1"][0]["pipeline"] == 1 and st["plain_p3"][0]["pipeline"] == 3
assert st["env"][0]["slow_paths"] == 0 and st["env"][0]["rays"] == st["plain_p1"][0]["rays"]
res = {"tool": "tools/env_pass.py", "reps": args.reps, "width": W, "height": H, "samples_per_pixel": S, "maxdepth": DEPTH, "seed": SEED,
       "table": args.n, "device": torch.cuda.get_device_name(0), "legs": {}}
for k, v in st.items():
    m = {"kernel_ms": summary([s["kernel_ms"] for s in v]), "rays": v[0]["rays"], "rays_per_path": v[0]["rays"] / (W * H * S),
         "pipeline": v[0]["pipeline"], "streams": v[0]["streams"], "trace_launches": v[0]["trace_launches"],
         "trace_ms": statistics.median([s["trace_ms"] for s in v])}
    m["mrays_per_s"] = m["rays"] / (m["kernel_ms"]["median"] * 1e3)
    res["legs"][k] = m
    print(f"{k}: {m['kernel_ms']['median']:.3f} ms [{m['kernel_ms']['min']:.3f}, {m['kernel_ms']['max']:.3f}], {m['rays']} rays "
          f"({m['mrays_per_s']:.1f} Mrays/s), trace {m['trace_ms']:.3f} ms summed over {m['streams']} stream(s), pipeline {m['pipeline']}", flush=True)
e, p1, p3 = (res["legs"][k]["kernel_ms"]["median"] for k in ("env", "plain_p1", "plain_p3"))
res["env_minus_plain_p1_ms"], res["env_over_plain_p1"], res["env_over_plain_p3"] = e - p1, e / p1, e / p3
print(f"env - plain_p1 = {e - p1:.3f} ms, env / plain_p1 = {e / p1:.4f}, env / plain_p3 = {e / p3:.4f}", flush=True)

# one stream: the launches of a frame run one after the other, so frame - trace is the time of everything that is not a walk
s0 = R.HipRayCaster(seed=SEED, tuning=dict(streams=1))
s1 = R.HipRayCaster(seed=SEED, tuning=dict(pipeline=1, streams=1))
one = {"env": lambda: s0.walk_tile_device(vp, env_scene, tile, out.data_ptr(), stream).stats,
       "plain_p1": lambda: s1.walk_tile_device(vp, plain1, tile, out.data_ptr(), stream).stats}
for f in one.values():
    f()
rest = {k: [] for k in one}
frame = {k: [] for k in one}
for _ in range(args.reps):
    for k, f in one.items():
        s = f()
        assert s["streams"] == 1
        frame[k].append(s["kernel_ms"])
        rest[k].append(s["kernel_ms"] - s["trace_ms"])
torch.cuda.synchronize()
d_frame = statistics.median(frame["env"]) - statistics.median(frame["plain_p1"])
d_rest = statistics.median(rest["env"]) - statistics.median(rest["plain_p1"])
res["one_stream"] = {k: {"kernel_ms": summary(frame[k]), "not_trace_ms": summary(rest[k])} for k in one}
res["one_stream"]["frame_difference_ms"] = d_frame
res["one_stream"]["shade_difference_ms"] = d_rest
res["one_stream"]["shade_share_of_difference"] = d_rest / d_frame if d_frame else None
print(f"one stream: env {statistics.median(frame['env']):.3f} ms, plain_p1 {statistics.median(frame['plain_p1']):.3f} ms; outside the walks "
      f"{statistics.median(rest['env']):.3f} against {statistics.median(rest['plain_p1']):.3f} ms: {d_rest:.3f} of the {d_frame:.3f} ms difference", flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
