#!/usr/bin/env python3
"""What the shadow rays inside the path cost.  The canonical scene (teapot_tri.obj + two mirror disks, octree
10/19), a --size x --size frame, S = 4, maxdepth 5, the box light at (-3, 6, 1) with edge 0.5.  Two legs on ONE handle with
tuning.pipeline = 1, alternated --reps times in one process after a warm-up:
  A  rtmi_render_shadowed_device: every surface hit of every bounce tested against the light
  B  rtmi_render_samples_device: the same per-pass pipeline (k_gen_samples, one closest-hit and one shading launch per pass,
     k_accum_samples) without shadows -- the same paths, the same rays
Both legs report stats.kernel_ms (HIP events on the caller's stream).  Reported: median [min, max] of each leg and their ratio,
at the library's own choice of streams and again on one stream, where the launches of a call do not overlap and the call
splits into its parts: the closest-hit launches (stats.primary_ms of A, stats.trace_ms of B), the shadow walks (A's
stats.bounce_ms) and the rest (kernel_ms minus those: k_gen_samples, the shading kernels, k_accum_samples, the memsets; A's
rest minus B's is what k_shadow_rays and k_shade_shadowed cost beyond k_shade_samples).  Also: shadow rays per path ray, and
(RTMI_OPT_COUNTERS, one more pass of each leg, untimed) the shadow rays' work under the any-hit walk against a closest-hit
trace of the same rays (the same two legs under RTMI_OPT_GENERIC, where the walk is a closest-hit launch).
Usage: tools/shadowed_pass.py [--reps N] [--size 1024] [--out FILE.json]"""
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
S, DEPTH, SEED, LIGHT, LEN2 = 4, 5, 1, (-3.0, 6.0, 1.0), 0.5
OBJ = os.path.join(ROOT, "tests", "golden", "teapot_tri.obj")
sc = R.canonical_scene(OBJ, gpu_build=0)
vp = R.canonical_viewport(W, H, DEPTH, S)
stream = torch.cuda.current_stream().cuda_stream
TILE = (0, H, H, 0)
COUNTERS = ("box_tests", "tri_tests", "full_tests", "nodes", "leaves")
acc, out, out1 = (torch.zeros(W * H * 4, dtype=torch.float32, device="cuda:0") for _ in range(3))
torch.cuda.synchronize()


def leg_a(caster, o=out):
    return caster.walk_rays_shadowed_device(vp, sc, acc, o, orig=LIGHT, len2=LEN2, stream=stream).stats


def leg_b(caster):
    return caster.walk_samples_device(vp, sc, TILE, 0, S, acc.data_ptr(), out.data_ptr(), stream).stats


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": [round(x, 4) for x in xs]}


def alternate(caster):
    for _ in range(2):  # warm-up: workspaces, code objects
        leg_a(caster)
        leg_b(caster)
    sa, sb = [], []
    for _ in range(args.reps):
        sa.append(leg_a(caster))
        sb.append(leg_b(caster))
    torch.cuda.synchronize()
    a_ms, b_ms = [s["kernel_ms"] for s in sa], [s["kernel_ms"] for s in sb]
    return sa, sb, {"streams": sa[0]["streams"], "shadowed_ms": summary(a_ms), "plain_ms": summary(b_ms),
                    "ratio": statistics.median(a_ms) / statistics.median(b_ms)}


res = {"tool": "tools/shadowed_pass.py", "reps": args.reps, "width": W, "height": H, "samples_per_pixel": S, "maxdepth": DEPTH,
       "light": list(LIGHT), "len2": LEN2, "device": torch.cuda.get_device_name(0)}
sa, sb, res["default_streams"] = alternate(R.HipRayCaster(seed=SEED, tuning=dict(pipeline=1)))
leg_a(R.HipRayCaster(seed=SEED, tuning=dict(pipeline=1)), out1)
torch.cuda.synchronize()
sa1, sb1, one = alternate(R.HipRayCaster(seed=SEED, tuning=dict(pipeline=1, streams=1)))
leg_a(R.HipRayCaster(seed=SEED, tuning=dict(pipeline=1, streams=1)))
torch.cuda.synchronize()
assert torch.equal(out.view(torch.int32), out1.view(torch.int32)), "one stream and the default streams differ"
rest_a = [s["kernel_ms"] - s["primary_ms"] - s["bounce_ms"] for s in sa1]
rest_b = [s["kernel_ms"] - s["trace_ms"] for s in sb1]
one["split_ms"] = {"shadowed": {"closest_hit_launches": summary([s["primary_ms"] for s in sa1]), "shadow_walks": summary([s["bounce_ms"] for s in sa1]),
                                "rest": summary(rest_a)},
                   "plain": {"closest_hit_launches": summary([s["trace_ms"] for s in sb1]), "rest": summary(rest_b)},
                   "new_kernels_beyond_k_shade_samples": statistics.median(rest_a) - statistics.median(rest_b)}
res["one_stream"] = one
path_rays, live = sb[0]["rays"], sa[0]["rays"] - sb[0]["rays"]
res["path_rays"], res["shadow_rays"], res["shadow_rays_per_path_ray"] = path_rays, live, live / path_rays
cn = {}
for name, opt in (("any_hit", R.OPT_COUNTERS), ("closest_hit", R.OPT_COUNTERS | R.OPT_GENERIC)):
    cc = R.HipRayCaster(seed=SEED, options=opt, tuning=dict(pipeline=1))
    a, b = leg_a(cc), leg_b(cc)
    assert a["rays"] - b["rays"] == live
    cn[name] = {k: a[k] - b[k] for k in COUNTERS}
    cn[name + "_path_rays"] = {k: b[k] for k in COUNTERS}
res["shadow_ray_counters"] = cn

d, sp = res["default_streams"], one["split_ms"]
print(f"{W} x {H} x {S} spp, depth {DEPTH}: {path_rays} path rays, {live} shadow rays ({live / path_rays:.3f} per path ray); "
      f"{d['streams']} streams: shadowed {d['shadowed_ms']['median']:.3f} ms [{d['shadowed_ms']['min']:.3f}, {d['shadowed_ms']['max']:.3f}], "
      f"plain {d['plain_ms']['median']:.3f} ms [{d['plain_ms']['min']:.3f}, {d['plain_ms']['max']:.3f}], ratio {d['ratio']:.3f}; "
      f"one stream: shadowed {one['shadowed_ms']['median']:.3f}, plain {one['plain_ms']['median']:.3f}, ratio {one['ratio']:.3f}; "
      f"split (one stream): closest-hit {sp['shadowed']['closest_hit_launches']['median']:.3f} (plain {sp['plain']['closest_hit_launches']['median']:.3f}), "
      f"shadow walks {sp['shadowed']['shadow_walks']['median']:.3f}, rest {sp['shadowed']['rest']['median']:.3f} (plain {sp['plain']['rest']['median']:.3f}); "
      f"shadow rays' tri_tests any-hit {cn['any_hit']['tri_tests']} vs closest-hit {cn['closest_hit']['tri_tests']}, "
      f"box_tests {cn['any_hit']['box_tests']} vs {cn['closest_hit']['box_tests']}", flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
