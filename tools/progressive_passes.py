#!/usr/bin/env python3
"""Cost of progressive rendering on config 3 (teapot_tri.obj 2048x2048 @ 64 spp, depth 5, seed 1, octree 10/19): the frame as
one rtmi_render_tile_device call, as 8 passes of 8 samples and as 64 passes of 1 sample (rtmi_render_samples_device, preview
written on every pass), device milliseconds of each (the sum of the calls' kernel_ms, best of --reps).  Asserts that the
three final images are bit-equal.  Usage: tools/progressive_passes.py [--reps N]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from rust_raytrace_amd import raytrace as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
args = ap.parse_args()
W = H = 2048
S = 64
scene = R.canonical_scene(os.path.join(ROOT, "tests", "golden", "teapot_tri.obj"), gpu_build=0)
vp = R.canonical_viewport(W, H, 5, S)
c = R.HipRayCaster(seed=1)
c.upload(scene)
stream = torch.cuda.current_stream().cuda_stream
tile = (0, H, H, 0)
out = {k: torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0") for k in ("1x64", "8x8", "64x1")}
accum = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")


def run(kind):
    if kind == "1x64":
        ctx = c.walk_tile_device(vp, scene, tile, out[kind].data_ptr(), stream)
        return ctx.stats["kernel_ms"], ctx.total_rays
    step = S // int(kind.split("x")[0])
    ms, rays = 0.0, 0
    for k0 in range(0, S, step):
        ctx = c.walk_samples_device(vp, scene, tile, k0, step, accum.data_ptr(), out[kind].data_ptr(), stream)
        ms += ctx.stats["kernel_ms"]
        rays += ctx.total_rays
    return ms, rays


res = {}
for kind in ("1x64", "8x8", "64x1"):
    run(kind)  # warm-up (workspaces, code objects)
    best, rays = min(run(kind) for _ in range(max(1, args.reps)))
    res[kind] = (best, rays)
torch.cuda.synchronize()
base = res["1x64"][0]
for kind, (ms, rays) in res.items():
    print(f"{kind:>5}: {ms:8.1f} ms device ({ms / base:.3f} x one call, {rays / (ms * 1e3):.0f} Mrays/s), {rays} rays")
a, b, d = (out[k].cpu().view(torch.int32) for k in ("1x64", "8x8", "64x1"))
assert torch.equal(a, b) and torch.equal(a, d), "final images differ"
assert res["1x64"][1] == res["8x8"][1] == res["64x1"][1], "ray counts differ"
print("final images of 1 x 64, 8 x 8 and 64 x 1 samples: bit-equal")
