#!/usr/bin/env python3
"""What the one-call shaded preview costs against the separate calls it replaces.  The canonical scene
(teapot_tri.obj + two mirror disks, octree 10/19), a --size x --size frame, S = 1 (the centred ray), Ka = 4 AO rays, light A =
the box light at (-3, 6, 1) with edge 0.5 and light B = a point light at (2, 0, -3), K = 4 each.  Two legs, alternated --reps
times in one process after a warm-up:
  A  rtmi_render_preview_device with all seven outputs: one primary pass, one any-hit walk, the per-sample composition
  B  rtmi_render_features_device + rtmi_render_ao_device + two rtmi_render_light_device calls into the same layer buffers:
     four primary passes, three walks, and no composition (a caller cannot make the per-sample one from the per-pixel means)
Both legs report stats.kernel_ms (HIP events on the caller's stream), leg B the sum of its four calls.  Reported: median [min,
max] of each leg; leg A's split into the primary walk (stats.primary_ms), the shared walk (stats.bounce_ms) and the rest
(kernel_ms minus the two: k_gen_samples, k_features, k_preview_rays, k_preview_resolve, the control block's memset); leg B's
four primary_ms; the ray counts; and the one condition: leg A's median may not exceed leg B's median by more than leg B's own
max - min.  The layers of the two legs are compared bit for bit before anything is reported.
Usage: tools/preview_pass.py [--reps N] [--size 1024] [--out FILE.json]"""
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
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--out", default=None)
args = ap.parse_args()

W = H = args.size
SEED, KA = 1, 4
AMBIENT = (0.25, 0.25, 0.3)
LIGHTS = [dict(orig=(-3.0, 6.0, 1.0), len2=0.5, rays=4, color=(1.0, 0.9, 0.8)), dict(orig=(2.0, 0.0, -3.0), len2=0.0, rays=4, color=(0.2, 0.3, 0.5))]
OBJ = os.path.join(ROOT, "tests", "golden", "teapot_tri.obj")
sc = R.canonical_scene(OBJ, gpu_build=0)
c = R.HipRayCaster(seed=SEED)
vp = R.canonical_viewport(W, H, 5, 1)
stream = torch.cuda.current_stream().cuda_stream
dev = "cuda:0"
TILE = (0, H, H, 0)


def buffers():
    f4 = lambda: torch.zeros((H, W, 4), dtype=torch.float32, device=dev)
    f1 = lambda n=1: torch.zeros((n, H, W), dtype=torch.float32, device=dev)
    return dict(color=f4(), albedo=f4(), normal=f4(), ids=torch.zeros((H, W), dtype=torch.int32, device=dev), ao=f1(), shadow=f1(2),
                irradiance=f1(2))


a_buf, b_buf = buffers(), buffers()
torch.cuda.synchronize()


def leg_a():
    return c.walk_rays_preview_device(vp, sc, tile=TILE, ambient=AMBIENT, ao=dict(rays=KA), lights=LIGHTS, color=a_buf["color"],
                                      albedo=a_buf["albedo"], normal=a_buf["normal"], ids=a_buf["ids"], ao_out=a_buf["ao"],
                                      shadow=a_buf["shadow"], irradiance=a_buf["irradiance"], stream=stream).stats


def leg_b():
    b = b_buf
    st = [c.walk_features_device(vp, sc, TILE, b["albedo"].data_ptr(), b["normal"].data_ptr(), b["ids"].data_ptr(), 0, 1, stream).stats,
          c.walk_rays_ao_device(vp, sc, b["ao"].view(-1), rays=KA, stream=stream).stats]
    for l, li in enumerate(LIGHTS):
        kw = {k: v for k, v in li.items() if k != "color"}
        st.append(c.walk_rays_light_device(vp, sc, b["shadow"][l].view(-1), b["irradiance"][l].view(-1), stream=stream, **kw).stats)
    return st


for _ in range(2):  # warm-up: workspaces, code objects
    leg_a()
    leg_b()
sa, sb = [], []
for _ in range(args.reps):
    sa.append(leg_a())
    sb.append(leg_b())
torch.cuda.synchronize()
for name in ("albedo", "normal", "ids", "ao", "shadow", "irradiance"):  # the one call's layers are the separate calls' layers
    assert torch.equal(a_buf[name].view(torch.int32), b_buf[name].view(torch.int32)), name


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": [round(x, 4) for x in xs]}


a_ms = [s["kernel_ms"] for s in sa]
b_ms = [sum(s["kernel_ms"] for s in four) for four in sb]
rest = [s["kernel_ms"] - s["primary_ms"] - s["bounce_ms"] for s in sa]
spread = max(b_ms) - min(b_ms)
names = ("features", "ao", "light_a", "light_b")
res = {"tool": "tools/preview_pass.py", "reps": args.reps, "width": W, "height": H, "samples_per_pixel": 1, "ao_rays": KA,
       "lights": [{k: list(v) if isinstance(v, tuple) else v for k, v in li.items()} for li in LIGHTS], "ambient": list(AMBIENT),
       "device": torch.cuda.get_device_name(0),
       "rays": {"preview_call": sa[0]["rays"], "separate_calls": {n: s["rays"] for n, s in zip(names, sb[0])},
                "separate_calls_total": sum(s["rays"] for s in sb[0]), "primaries": W * H},
       "trace_launches": {"preview_call": sa[0]["trace_launches"], "separate_calls": sum(s["trace_launches"] for s in sb[0])},
       "preview_call_ms": summary(a_ms), "separate_calls_ms": summary(b_ms), "ratio": statistics.median(a_ms) / statistics.median(b_ms),
       "preview_call_split_ms": {"primary_walk": summary([s["primary_ms"] for s in sa]), "shared_walk": summary([s["bounce_ms"] for s in sa]),
                                 "rest": summary(rest)},
       "separate_calls_split_ms": {n: {"kernel": summary([four[k]["kernel_ms"] for four in sb]),
                                       "primary_walk": summary([four[k]["primary_ms"] if k else four[k]["trace_ms"] for four in sb]),
                                       "walk": summary([four[k]["bounce_ms"] for four in sb])} for k, n in enumerate(names)},
       "condition": {"preview_call_median_ms": statistics.median(a_ms), "separate_calls_median_ms": statistics.median(b_ms),
                     "separate_calls_spread_ms": spread, "holds": statistics.median(a_ms) <= statistics.median(b_ms) + spread}}
sp = res["preview_call_split_ms"]
prim_b = [res["separate_calls_split_ms"][n]["primary_walk"]["median"] for n in names]
print(f"{W} x {H}: preview call {res['preview_call_ms']['median']:.3f} ms [{min(a_ms):.3f}, {max(a_ms):.3f}] "
      f"(primary walk {sp['primary_walk']['median']:.3f}, shared walk {sp['shared_walk']['median']:.3f}, rest {sp['rest']['median']:.3f}), "
      f"{res['rays']['preview_call']} rays in {res['trace_launches']['preview_call']} launches; separate calls "
      f"{res['separate_calls_ms']['median']:.3f} ms [{min(b_ms):.3f}, {max(b_ms):.3f}] (primary walks "
      f"{' + '.join(f'{x:.3f}' for x in prim_b)}), {res['rays']['separate_calls_total']} rays in {res['trace_launches']['separate_calls']} launches; "
      f"ratio {res['ratio']:.3f}; condition holds: {res['condition']['holds']}", flush=True)

if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
