#!/usr/bin/env python3
"""What the one-call direct-light pass costs.  The canonical scene (teapot_tri.obj + two mirror disks, octree
10/19), a --size x --size frame, S = 1 (the centred ray), K = 4 samples of the box light at (-3, 6, 1) with edge 0.5 per hit.
Two legs, alternated --reps times in one process after a warm-up:
  A  rtmi_render_light_device: primaries, candidates, the cull, the live rays' any-hit walk and the per-pixel folds in one
     call, nothing leaves the device
  B  what a caller had to do before, without its host work: rtmi_render_features_device of the same frame followed by
     rtmi_occluded_device on the SAME live rays with the same limits, made once by the NumPy restatement (tests/light_ref.py,
     on this build's own closest hits) and uploaded once; the copies, the host-side ray generation and the host-side reduction
     it also needed are not timed
Both legs report stats.kernel_ms (HIP events on the caller's stream).  Reported: median [min, max] of each leg; leg A's split
into the primary walk (stats.primary_ms), the shadow walk (stats.bounce_ms) and the rest of the call (kernel_ms minus the two:
k_gen_samples, k_light_rays, k_light_resolve and the control block's memset -- an upper bound of the two new kernels); the one
condition (the shadow walk inside the call may not exceed the median of leg B's rtmi_occluded_device by more than that leg's
own max - min); and, with RTMI_OPT_COUNTERS (one more pass, untimed), the live rays' plane tests under the any-hit walk and
under rtmi_trace.
Usage: tools/light_pass.py [--reps N] [--size 1024] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from oracle import orc  # noqa: E402  (the primary rays and the RNG only: the renderer's own, restated)
from rust_raytrace_amd import raytrace as R  # noqa: E402
import light_ref as LR  # noqa: E402
import occluded_ref as OR  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--out", default=None)
args = ap.parse_args()

W = H = args.size
K, SEED, LEN2, BIAS = 4, 1, 0.5, 0.005
F32 = np.float32
OBJ = os.path.join(ROOT, "tests", "golden", "teapot_tri.obj")
sc = R.canonical_scene(OBJ, gpu_build=0)
c = R.HipRayCaster(seed=SEED)
cc = R.HipRayCaster(seed=SEED, options=R.OPT_COUNTERS)
vp = R.canonical_viewport(W, H, 5, 1)
o4, d4 = orc.primary_rays(W, H, orc.canonical_viewport(W, H), 1, SEED)
tri, t, face, _ = c.trace(sc, o4, d4)
rec, _, _ = sc.triangles()
pixel = np.arange(W * H, dtype=np.int64)
hit, o, dirs, r, cdot = LR.candidates(orc, SEED, o4, d4, tri, t, face, rec[:, 3:6].astype(F32), pixel, np.zeros(W * H, np.int64), K, OR.LIGHT,
                                      LEN2, BIAS)
with np.errstate(invalid="ignore"):
    live = cdot > F32(0.0)
l_o, l_d, l_r = (np.ascontiguousarray(a[live]) for a in (o, dirs, r))
n = l_o.shape[0]
print(f"{W} x {H}: {len(hit)} of {W * H} samples hit, {len(hit) * K} candidates, {n} live rays", flush=True)

stream = torch.cuda.current_stream().cuda_stream
dev = "cuda:0"
t_o, t_d, t_tm = torch.from_numpy(l_o).to(dev), torch.from_numpy(l_d).to(dev), torch.from_numpy(l_r).to(dev)
t_occ = torch.zeros(n, dtype=torch.uint8, device=dev)
t_sh, t_ir = (torch.zeros(W * H, dtype=torch.float32, device=dev) for _ in range(2))
t_alb, t_nrm = (torch.zeros((H, W, 4), dtype=torch.float32, device=dev) for _ in range(2))
t_ids = torch.zeros((H, W), dtype=torch.int32, device=dev)
torch.cuda.synchronize()
TILE = (0, H, H, 0)
COUNTERS = ("box_tests", "tri_tests", "full_tests", "nodes", "leaves")


def leg_a(caster=c):
    return caster.walk_rays_light_device(vp, sc, t_sh, t_ir, orig=OR.LIGHT, len2=LEN2, rays=K, bias=BIAS, stream=stream).stats


def leg_b(caster=c):
    f = caster.walk_features_device(vp, sc, TILE, t_alb.data_ptr(), t_nrm.data_ptr(), t_ids.data_ptr(), 0, 1, stream).stats
    oc = caster.occluded_device(sc, n, t_o.data_ptr(), t_d.data_ptr(), t_tm.data_ptr(), t_occ.data_ptr(), stream)
    return f, oc


for _ in range(2):  # warm-up: workspaces, code objects
    leg_a()
    leg_b()
sa, sb = [], []
for _ in range(args.reps):
    sa.append(leg_a())
    sb.append(leg_b())
torch.cuda.synchronize()
# the one call's planes are the two-call leg's bytes resolved per pixel
occ = t_occ.cpu().numpy()
want_sh, want_ir = LR.resolve(tri, live, occ, cdot, W * H, 1, K)
assert np.array_equal(t_sh.cpu().numpy().view(np.uint32), want_sh.view(np.uint32)), "shadow"
assert np.array_equal(t_ir.cpu().numpy().view(np.uint32), want_ir.view(np.uint32)), "irradiance"
ca = leg_a(cc)
cf, co = leg_b(cc)
ct = cc.trace(sc, l_o, l_d)[3]


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": [round(x, 4) for x in xs]}


a_ms = [s["kernel_ms"] for s in sa]
b_ms = [f["kernel_ms"] + oc["kernel_ms"] for f, oc in sb]
rest = [s["kernel_ms"] - s["primary_ms"] - s["bounce_ms"] for s in sa]
walk_a = [s["bounce_ms"] for s in sa]
occ_b = [oc["kernel_ms"] for _, oc in sb]
occ_walk_b = [oc["trace_ms"] for _, oc in sb]
spread = max(occ_b) - min(occ_b)
res = {"tool": "tools/light_pass.py", "reps": args.reps, "width": W, "height": H, "samples_per_pixel": 1, "rays": K, "light": list(OR.LIGHT),
       "len2": LEN2, "device": torch.cuda.get_device_name(0), "hits": int(len(hit)), "candidates": int(len(hit) * K), "live_rays": n,
       "occluded": int(occ.sum()),
       "light_call_ms": summary(a_ms), "features_plus_occluded_ms": summary(b_ms), "ratio": statistics.median(a_ms) / statistics.median(b_ms),
       "light_call_split_ms": {"primary_walk": summary([s["primary_ms"] for s in sa]), "shadow_walk": summary(walk_a),
                               "rest_upper_bound_of_new_kernels": summary(rest)},
       "two_call_split_ms": {"features": summary([f["kernel_ms"] for f, _ in sb]), "features_walk": summary([f["trace_ms"] for f, _ in sb]),
                             "occluded": summary(occ_b), "occluded_walk": summary(occ_walk_b)},
       "condition": {"shadow_walk_median_ms": statistics.median(walk_a), "occluded_median_ms": statistics.median(occ_b),
                     "occluded_spread_ms": spread, "holds": statistics.median(walk_a) <= statistics.median(occ_b) + spread,
                     "holds_against_the_walk_kernel_alone": statistics.median(walk_a) <= statistics.median(occ_walk_b) +
                     (max(occ_walk_b) - min(occ_walk_b))},
       "counters": {k: {"light_call": ca[k], "features": cf[k], "occluded_on_live_rays": co[k], "closest_hit_on_live_rays": ct[k]}
                    for k in COUNTERS}}
sp = res["light_call_split_ms"]
print(f"{res['occluded']} of {n} live rays occluded; light call {res['light_call_ms']['median']:.3f} ms [{min(a_ms):.3f}, {max(a_ms):.3f}], "
      f"features + occluded {res['features_plus_occluded_ms']['median']:.3f} ms [{min(b_ms):.3f}, {max(b_ms):.3f}], ratio {res['ratio']:.3f}; "
      f"split: primary walk {sp['primary_walk']['median']:.3f}, shadow walk {sp['shadow_walk']['median']:.3f}, rest {statistics.median(rest):.3f} ms; "
      f"rtmi_occluded_device {statistics.median(occ_b):.3f} ms [{min(occ_b):.3f}, {max(occ_b):.3f}] (walk {statistics.median(occ_walk_b):.3f}); "
      f"condition holds: {res['condition']['holds']} (walk alone: {res['condition']['holds_against_the_walk_kernel_alone']}); "
      f"live rays' tri_tests any-hit {co['tri_tests']} vs closest-hit {ct['tri_tests']}, box_tests {co['box_tests']} vs {ct['box_tests']}",
      flush=True)

if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
