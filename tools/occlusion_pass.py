#!/usr/bin/env python3
"""What the any-hit walk saves.  The canonical scene (teapot_tri.obj + two mirror disks, octree 10/19), the
primary rays of a --size x --size frame (1 spp, centred), three ray sets:
  primary  the primary rays with a NULL tmax: most teapot and disk rays leave the walk at their first hit
  shadow   the shadow segments of the same frame: from every first hit, moved 1e-3 along the hit normal, to the light of
           tests/occluded_ref.py, tmax = the distance to the light
  carry    the primary rays with tmax = 0: no ray leaves early, so this is what carrying the mode costs
Legs per set: A = rtmi_occluded_device (k_occluded_oct), C = rtmi_trace on the same rays (k_trace_oct, the closest-hit launch a
caller had to use before).  Both report stats.trace_ms: HIP events around the walk kernel alone, no copies.  After a warm-up
the two calls alternate in one process, --reps times; reported: median [min, max] per leg, the ratio of the medians and the
spread (max - min) of the closest-hit samples.  With RTMI_OPT_COUNTERS (one more pass, untimed) the work counters of both.
Usage: tools/occlusion_pass.py [--reps N] [--size 1024] [--out FILE.json]"""
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
from oracle import orc  # noqa: E402  (the primary rays only: the renderer's own ray generation, restated)
from rust_raytrace_amd import raytrace as R  # noqa: E402
import occluded_ref as OR  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=11)
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--out", default=None)
args = ap.parse_args()

W = H = args.size
F32 = np.float32
OBJ = os.path.join(ROOT, "tests", "golden", "teapot_tri.obj")
sc = R.canonical_scene(OBJ, gpu_build=0)
c = R.HipRayCaster(seed=1)
cc = R.HipRayCaster(seed=1, options=R.OPT_COUNTERS)
o4, d4 = orc.primary_rays(W, H, orc.canonical_viewport(W, H), 1)
tri, t, face, _ = c.trace(sc, o4, d4)


class ProductHits:
    """occluded_ref.shadow_segments' view of a scene, on the product's own closest hits"""
    def trace(self, o, d):
        return tri, t, face, None

    def triangles(self):
        return sc.triangles()


so4, sd4, dist = OR.shadow_segments(ProductHits(), o4, d4)
sets = {"primary": (o4, d4, None), "shadow": (so4, sd4, dist), "carry": (o4, d4, np.zeros(o4.shape[0], F32))}
stream = torch.cuda.current_stream().cuda_stream
dev, res = {}, {}
for name, (o, d, tm) in sets.items():
    n = o.shape[0]
    dev[name] = (torch.from_numpy(o).to("cuda:0"), torch.from_numpy(d).to("cuda:0"), None if tm is None else torch.from_numpy(tm).to("cuda:0"),
                 torch.zeros(n, dtype=torch.uint8, device="cuda:0"))
torch.cuda.synchronize()


def any_hit(name, caster=c):
    to, td, tt, out = dev[name]
    return caster.occluded_device(sc, to.shape[0], to.data_ptr(), td.data_ptr(), None if tt is None else tt.data_ptr(), out.data_ptr(), stream)


def closest_hit(name, caster=c):
    o, d, _ = sets[name]
    return caster.trace(sc, o, d)


for name, (o, d, tm) in sets.items():
    n = o.shape[0]
    for _ in range(2):  # warm-up: workspaces, code objects
        any_hit(name)
        closest_hit(name)
    ta, tc = [], []
    for _ in range(args.reps):
        ta.append(any_hit(name)["trace_ms"])
        tc.append(closest_hit(name)[3]["trace_ms"])
    torch.cuda.synchronize()
    got = dev[name][3].cpu().numpy()
    htri, ht = closest_hit(name)[:2]
    assert np.array_equal(got, OR.from_hits(htri, ht, tm)), name  # the bytes are the definition's, on this build's own hits
    sa, st = any_hit(name, cc), closest_hit(name, cc)[3]
    ma, mc = statistics.median(ta), statistics.median(tc)
    res[name] = {"rays": n, "occluded": int(got.sum()),
                 "any_hit_ms": {"median": ma, "min": min(ta), "max": max(ta), "all": [round(x, 4) for x in ta]},
                 "closest_hit_ms": {"median": mc, "min": min(tc), "max": max(tc), "all": [round(x, 4) for x in tc]},
                 "ratio": ma / mc, "closest_hit_spread_ms": max(tc) - min(tc), "gain_ms": mc - ma,
                 "counters": {k: {"any_hit": sa[k], "closest_hit": st[k]} for k in ("box_tests", "tri_tests", "full_tests", "nodes", "leaves")}}
    r = res[name]
    print(f"{name}: {n} rays, {r['occluded']} occluded; any-hit {ma:.3f} ms [{min(ta):.3f}, {max(ta):.3f}], closest-hit {mc:.3f} ms "
          f"[{min(tc):.3f}, {max(tc):.3f}] (spread {r['closest_hit_spread_ms']:.3f}); ratio {r['ratio']:.3f}; tri_tests "
          f"{sa['tri_tests']} vs {st['tri_tests']}, box_tests {sa['box_tests']} vs {st['box_tests']}", flush=True)

if args.out:
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/occlusion_pass.py", "reps": args.reps, "width": W, "height": H, "device": torch.cuda.get_device_name(0),
                   "light": list(OR.LIGHT), "sets": res}, f, indent=1)
