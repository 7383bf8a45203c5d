#!/usr/bin/env python3
"""What a built-in camera model costs.  The canonical scene (teapot_tri.obj + two mirror disks, octree 10/19), a
--size x --size frame, S = 16, maxdepth 5.  For each model three legs on ONE handle per pipeline setting, alternated --reps
times in one process after a warm-up; every leg renders all S samples in one call and reports stats.kernel_ms (HIP events on
the caller's stream):
  A   rtmi_render_camera_device with the model (always the per-pass pipeline)
  B1  rtmi_render_samples_device with tuning.pipeline = 1: the same per-pass pipeline with the pinhole's k_gen_samples
  B3  rtmi_render_samples_device with tuning.pipeline = 3: the path kernels, what a plain render of the view runs by default
B1 and B3 are existing code: the baseline.  A / B1 is what the generator and the model's rays cost on equal terms, A / B3 what a
caller pays for leaving the pinhole.  The pinhole and the thin lens (radius 0.05, focused at --focus world units) use the
canonical view.  The orthographic camera uses the canonical camera tilted by a hair (direction (0.01, 0.02, 1)), and so do its
baselines: with the canonical, axis-aligned camera every orthographic ray has two exactly-zero direction components, the
reference's expensive case, which is measured separately on a --slow-size x --slow-size frame at S = 1 (one call, after one
warm-up call) against the same frame through the tilted camera.  A fourth leg, A with the albedo and normal guides, gives
what k_features adds.
Usage: tools/camera_pass.py [--reps N] [--size 1024] [--slow-size 64] [--out FILE.json]"""
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
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--slow-size", type=int, default=64)
ap.add_argument("--focus", type=float, default=5.0)
ap.add_argument("--out", default=None)
args = ap.parse_args()

W = H = args.size
S, DEPTH, SEED, RADIUS = 16, 5, 1, 0.05
OBJ = os.path.join(ROOT, "tests", "golden", "teapot_tri.obj")
sc = R.canonical_scene(OBJ, gpu_build=0)
stream = torch.cuda.current_stream().cuda_stream


def tilted_viewport(w, h, samples):
    aspect = float(np.float32(h) / np.float32(w))
    return R.create_viewport((w, h), (1.0, aspect), [2.0, 0.0, 0.0], R.unit([0.01, 0.02, 1.0]), 90.0, R.to_radians(0.0), DEPTH, samples)


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": [round(x, 4) for x in xs]}


def buffers(w, h, n=2):
    b = [torch.zeros(w * h * 4, dtype=torch.float32, device="cuda:0") for _ in range(n)]
    torch.cuda.synchronize()
    return b


acc, out, alb, nrm = buffers(W, H, 4)
c1 = R.HipRayCaster(seed=SEED, tuning=dict(pipeline=1))
c3 = R.HipRayCaster(seed=SEED, tuning=dict(pipeline=3))
res = {"tool": "tools/camera_pass.py", "reps": args.reps, "width": W, "height": H, "samples_per_pixel": S, "maxdepth": DEPTH,
       "lens_radius": RADIUS, "focus_distance": args.focus, "device": torch.cuda.get_device_name(0), "models": {}}
canonical = R.canonical_viewport(W, H, DEPTH, S)
for model, vp in (("pinhole", canonical), ("thin_lens", canonical), ("ortho", tilted_viewport(W, H, S))):
    cam = c1.camera_params(vp, model, aperture=RADIUS, focus_distance=args.focus)
    tile = (0, H, H, 0)
    legs = {
        "camera": lambda: c1.walk_rays_camera_device(vp, sc, cam, acc, out, stream=stream).stats,
        "camera_with_guides": lambda: c1.walk_rays_camera_device(vp, sc, cam, acc, out, albedo=alb, normal=nrm, stream=stream).stats,
        "samples_pipeline_1": lambda: c1.walk_samples_device(vp, sc, tile, 0, S, acc.data_ptr(), out.data_ptr(), stream).stats,
        "samples_pipeline_3": lambda: c3.walk_samples_device(vp, sc, tile, 0, S, acc.data_ptr(), out.data_ptr(), stream).stats,
    }
    for f in legs.values():  # warm-up: workspaces, code objects
        f()
    st = {k: [] for k in legs}
    for _ in range(args.reps):
        for k, f in legs.items():
            st[k].append(f())
    torch.cuda.synchronize()
    assert st["samples_pipeline_1"][0]["pipeline"] == 1 and st["samples_pipeline_3"][0]["pipeline"] == 3 and st["camera"][0]["pipeline"] == 1
    m = {k: summary([s["kernel_ms"] for s in v]) for k, v in st.items()}
    m["rays"] = {k: v[0]["rays"] for k, v in st.items()}
    m["streams"] = {k: v[0]["streams"] for k, v in st.items()}
    m["trace_ms"] = {k: statistics.median([s["trace_ms"] for s in v]) for k, v in st.items()}
    m["focus"] = cam.focus
    m["ratio_to_pipeline_1"] = m["camera"]["median"] / m["samples_pipeline_1"]["median"]
    m["ratio_to_pipeline_3"] = m["camera"]["median"] / m["samples_pipeline_3"]["median"]
    m["guides_ms"] = m["camera_with_guides"]["median"] - m["camera"]["median"]
    res["models"][model] = m
    print(f"{model}: camera {m['camera']['median']:.3f} ms [{m['camera']['min']:.3f}, {m['camera']['max']:.3f}] ({m['rays']['camera']} rays), "
          f"with guides {m['camera_with_guides']['median']:.3f}, samples pipeline 1 {m['samples_pipeline_1']['median']:.3f} "
          f"[{m['samples_pipeline_1']['min']:.3f}, {m['samples_pipeline_1']['max']:.3f}], pipeline 3 {m['samples_pipeline_3']['median']:.3f} "
          f"[{m['samples_pipeline_3']['min']:.3f}, {m['samples_pipeline_3']['max']:.3f}]; camera / pipeline 1 = {m['ratio_to_pipeline_1']:.3f}, "
          f"/ pipeline 3 = {m['ratio_to_pipeline_3']:.3f}", flush=True)

# the axis-aligned orthographic camera: every ray is a zero-component ray
w = h = args.slow_size
sacc, sout = buffers(w, h)
slow = {}
for name, vp in (("axis_aligned", R.canonical_viewport(w, h, DEPTH, 1)), ("tilted", tilted_viewport(w, h, 1))):
    cam = c1.camera_params(vp, "ortho")
    c1.walk_rays_camera_device(vp, sc, cam, sacc, sout, stream=stream)
    s = c1.walk_rays_camera_device(vp, sc, cam, sacc, sout, stream=stream).stats
    slow[name] = {"kernel_ms": s["kernel_ms"], "rays": s["rays"]}
res["ortho_zero_component"] = {"width": w, "height": h, "samples_per_pixel": 1, **slow}
print(f"ortho {w} x {h} x 1: axis-aligned {slow['axis_aligned']['kernel_ms']:.3f} ms ({slow['axis_aligned']['rays']} rays), "
      f"tilted {slow['tilted']['kernel_ms']:.3f} ms ({slow['tilted']['rays']} rays)", flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
