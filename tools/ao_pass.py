#!/usr/bin/env python3
"""What the one-call ambient-occlusion pass costs and what its any-hit walk saves.  The canonical scene
(teapot_tri.obj + two mirror disks, octree 10/19), a --size x --size frame, S = 1 (the centred ray), K = 4 AO rays per hit,
radius +inf and 1.0.  Two legs per radius, alternated --reps times in one process after a warm-up:
  A  rtmi_render_ao_device: primaries, AO rays, their any-hit walk and the per-pixel count in one call, nothing leaves the device
  B  what a caller had to do before, without its host work: rtmi_render_features_device of the same frame followed by
     rtmi_occluded_device on the SAME AO rays, made once by the NumPy restatement (tests/ao_ref.py, on this build's own closest
     hits) and uploaded once; the copies, the host-side ray generation and the host-side reduction it also needed are not timed
Both legs report stats.kernel_ms (HIP events on the caller's stream).  Reported: median [min, max] of each leg; leg A's split
into the primary walk (stats.primary_ms), the AO walk (stats.bounce_ms) and the rest of the call (kernel_ms minus the two:
k_gen_samples, k_ao_rays, k_ao_count, k_ao_resolve and the control block's memset -- an upper bound of the two new kernels);
and, with RTMI_OPT_COUNTERS (one more pass, untimed), the AO rays' plane tests under the any-hit walk and under rtmi_trace.
Usage: tools/ao_pass.py [--reps N] [--size 1024] [--out FILE.json]"""
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
import ao_ref as AR  # noqa: E402
import occluded_ref as OR  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--out", default=None)
args = ap.parse_args()

W = H = args.size
K, SEED = 4, 1
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
ao_o, ao_d, path = AR.ao_rays(orc, SEED, o4, d4, tri, t, face, rec[:, 3:6].astype(F32), pixel, np.zeros(W * H, np.int64), K, 0.001)
n = ao_o.shape[0]
print(f"{W} x {H}: {int((tri != 0).sum())} of {W * H} samples hit, {n} AO rays", flush=True)

stream = torch.cuda.current_stream().cuda_stream
dev = "cuda:0"
t_o, t_d = torch.from_numpy(ao_o).to(dev), torch.from_numpy(ao_d).to(dev)
t_occ = torch.zeros(n, dtype=torch.uint8, device=dev)
t_ao = torch.zeros(W * H, dtype=torch.float32, device=dev)
t_alb, t_nrm = (torch.zeros((H, W, 4), dtype=torch.float32, device=dev) for _ in range(2))
t_ids = torch.zeros((H, W), dtype=torch.int32, device=dev)
torch.cuda.synchronize()
TILE = (0, H, H, 0)
COUNTERS = ("box_tests", "tri_tests", "full_tests", "nodes", "leaves")
res = {}

for radius in (float("inf"), 1.0):
    t_tm = None if radius == float("inf") else torch.full((n,), radius, dtype=torch.float32, device=dev)
    tm_ptr = None if t_tm is None else t_tm.data_ptr()

    def leg_a(caster=c):
        return caster.walk_rays_ao_device(vp, sc, t_ao, rays=K, radius=radius, stream=stream).stats

    def leg_b(caster=c):
        f = caster.walk_features_device(vp, sc, TILE, t_alb.data_ptr(), t_nrm.data_ptr(), t_ids.data_ptr(), 0, 1, stream).stats
        o = caster.occluded_device(sc, n, t_o.data_ptr(), t_d.data_ptr(), tm_ptr, t_occ.data_ptr(), stream)
        return f, o

    for _ in range(2):  # warm-up: workspaces, code objects
        leg_a()
        leg_b()
    sa, sb = [], []
    for _ in range(args.reps):
        sa.append(leg_a())
        sb.append(leg_b())
    torch.cuda.synchronize()
    # the one call's image is the two-call leg's bytes reduced per pixel
    occ = t_occ.cpu().numpy()
    want = AR.resolve(tri, occ, W * H, 1, K)
    assert np.array_equal(t_ao.cpu().numpy().view(np.uint32), want.view(np.uint32)), radius
    ca = leg_a(cc)
    cf, co = leg_b(cc)
    ct = cc.trace(sc, ao_o, ao_d)[3]

    def summary(xs):
        return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": [round(x, 4) for x in xs]}

    a_ms = [s["kernel_ms"] for s in sa]
    b_ms = [f["kernel_ms"] + o["kernel_ms"] for f, o in sb]
    rest = [s["kernel_ms"] - s["primary_ms"] - s["bounce_ms"] for s in sa]
    r = {"radius": "inf" if radius == float("inf") else radius, "ao_rays": n, "occluded": int(occ.sum()),
         "ao_call_ms": summary(a_ms), "features_plus_occluded_ms": summary(b_ms), "ratio": statistics.median(a_ms) / statistics.median(b_ms),
         "ao_call_split_ms": {"primary_walk": summary([s["primary_ms"] for s in sa]), "ao_walk": summary([s["bounce_ms"] for s in sa]),
                              "rest_upper_bound_of_new_kernels": summary(rest)},
         "two_call_split_ms": {"features": summary([f["kernel_ms"] for f, _ in sb]), "features_walk": summary([f["trace_ms"] for f, _ in sb]),
                               "occluded": summary([o["kernel_ms"] for _, o in sb]), "occluded_walk": summary([o["trace_ms"] for _, o in sb])},
         "counters": {k: {"ao_call": ca[k], "features": cf[k], "occluded_on_ao_rays": co[k], "closest_hit_on_ao_rays": ct[k]} for k in COUNTERS}}
    res[str(r["radius"])] = r
    sp = r["ao_call_split_ms"]
    print(f"radius {r['radius']}: {r['occluded']} of {n} occluded; AO call {r['ao_call_ms']['median']:.3f} ms [{min(a_ms):.3f}, {max(a_ms):.3f}], "
          f"features + occluded {r['features_plus_occluded_ms']['median']:.3f} ms [{min(b_ms):.3f}, {max(b_ms):.3f}], ratio {r['ratio']:.3f}; "
          f"split: primary walk {sp['primary_walk']['median']:.3f}, AO walk {sp['ao_walk']['median']:.3f}, rest {statistics.median(rest):.3f} ms; "
          f"AO rays' tri_tests any-hit {co['tri_tests']} vs closest-hit {ct['tri_tests']}, box_tests {co['box_tests']} vs {ct['box_tests']}",
          flush=True)

if args.out:
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/ao_pass.py", "reps": args.reps, "width": W, "height": H, "samples_per_pixel": 1, "rays": K,
                   "device": torch.cuda.get_device_name(0), "radii": res}, f, indent=1)
