#!/usr/bin/env python3
"""Development aid: step statistics of the octree trace kernel (counting build) on the bench scene."""
import ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from rust_raytrace_amd import raytrace as R, _ffi

W = H = int(sys.argv[1]) if len(sys.argv) > 1 else 512
spp = int(sys.argv[2]) if len(sys.argv) > 2 else 16
scene = R.canonical_scene(os.path.join(ROOT, "tests", "golden", "teapot_tri.obj"))
vp = R.canonical_viewport(W, H, 5, spp)
c = R.HipRayCaster(seed=1, options=R.OPT_COUNTERS)
img = np.zeros((H, W, 4), np.float32)

ctx = c.walk_rays(vp, scene, img)
print(ctx.stats)
# the resident scene handle lives inside the C++ caster; fetch the debug counters through a tiny helper
lib = _ffi.lib()
lib.rth_debug_counters_n.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
out = (C.c_ulonglong * 52)()
lib.rth_debug_counters_n(scene.h, out, 52)
d = list(out)
names = ["S steps", "S lanes", "L steps", "L lanes", "refills", "refill lanes", "edge blocks", "edge lanes", "S cycles", "L cycles", "refill cycles", "wave cycles",
         "leaf visits", "memo hits", "planes skipped", "edges skipped",
         "packet L steps", "primary L steps", "packet refs", "refs culled", "violations",
         "mirror rays", "mirror in place", "mirror steps",
         "packet visits", "list culls",
         "cull blocks", "box missed", "blocks culled", "lists culled", "cull violations",
         "cull rays", "rays refused",
         "nodes seen", "nodes missed", "S lanes in missed", "leaves in missed", "node violations"]
for who in ("prim", "refl"):
    names += [f"{who} {x}" for x in ("certified", "refused", "nodes seen", "nodes missed", "S in missed", "leaves in missed", "violations")]
for n, v in zip(names, d):
    print(f"{n:14s} {v}")
rays = ctx.stats["rays"]
print("NOTE: dbg counters cover only the LAST batch/pass sequence of the call (ctrl is reset per batch)")
print(f"S lane util {d[1] / max(d[0] * 64, 1):.3f}   L lane util {d[3] / max(d[2] * 64, 1):.3f}   edge lanes/block {d[7] / max(d[6], 1):.2f}")
print(f"per ray: S steps {d[1] / rays:.1f}  L steps {d[3] / rays:.1f}  wave-steps per ray-wave: S {d[0] * 64 / rays:.1f} L {d[2] * 64 / rays:.1f}")
tot = max(d[11], 1)
print(f"shader-clock cycles of a wave (counting build, all passes of the last batch): SELECT steps {d[8] / tot:.3f}, LEAF steps {d[9] / tot:.3f}, "
      f"refills {d[10] / tot:.3f}, vote/rest {1 - (d[8] + d[9] + d[10]) / tot:.3f} of the wave's lifetime; "
      f"{d[8] / max(d[0], 1):.0f} cycles per SELECT step, {d[9] / max(d[2], 1):.0f} per LEAF step, {d[10] / max(d[4], 1):.0f} per refill")
print(f"leaf memo: {d[13]} of {d[12]} leaf visits take the result of the list the ray scanned last ({d[13] / max(d[12], 1):.3f}); "
      f"plane tests skipped {d[14]} ({d[14] / max(ctx.stats['tri_tests'], 1):.3f} of the call's tri_tests if it was one batch), "
      f"edge tests skipped {d[15]} ({d[15] / max(ctx.stats['full_tests'], 1):.3f} of full_tests)")
print(f"packet cull (k_path_primary, with the mirror reflections it traces in place): {d[16]} of {d[17]} LEAF steps qualify "
      f"({d[16] / max(d[17], 1):.3f}); {d[19]} of their {d[18]} references culled ({d[19] / max(d[18], 1):.3f}); violations {d[20]} (must be 0)")
# dbg[23] packs two step counts: exchange steps with >= 32 mirror lanes (low 32 bits), with 64 (high 32 bits)
print(f"mirror paths (RTMI_MIRROR_INPLACE={os.environ.get('RTMI_MIRROR_INPLACE', 'default')}): {d[21]} primary rays go on through a "
      f"Reflective hit ({d[21] / max(rays, 1):.4f} of all rays), {d[22]} of them traced in place by k_path_primary; exchange steps "
      f"with >= 32 mirror lanes {d[23] & 0xFFFFFFFF}, with 64 {d[23] >> 32}")
# dbg[24]: leaf visits whose first LEAF step is a packet step; dbg[25]: whole-list culls (0 before the whole-list cull existed)
print(f"packet leaf visits (first LEAF step of the visit qualifies): {d[24]}; per such visit: {d[16] / max(d[24], 1):.2f} qualifying "
      f"block steps, {d[18] / max(d[24], 1):.2f} references; whole-list culls {d[25]} ({d[25] / max(d[24], 1):.2f} per visit)")
if d[25]:
    # an estimate: the counting build still steps block by block, so its lanes may line up differently from the fast build's
    print(f"estimated primary LEAF steps of the fast build: {d[17] - d[16] + d[25]} (counting build: {d[17]}; whole-list culls "
          f"replacing its {d[16]} packet block steps)")
# dbg[26..30]: the block cull of k_trace_oct (bounce passes; RTMI_BLOCK_CULL=0: all 0).  The counting build evaluates the
# predicate for the block of every full LEAF step of a lane whose ray is certified and still tests every reference.
# dbg[31..32]: rays k_trace_oct took with the cull on, those of them the sign certificate refused.
print(f"block cull (k_trace_oct, RTMI_BLOCK_CULL={os.environ.get('RTMI_BLOCK_CULL', 'default')}): {d[26]} blocks seen by lanes with a "
      f"qualifying ray ({d[26] / max(d[3], 1):.3f} of all LEAF lane-steps); box missed by the half-line {d[27]} "
      f"({d[27] / max(d[26], 1):.3f}); culled {d[28]} ({d[28] / max(d[26], 1):.3f}); lists ended by a culled block {d[29]}; "
      f"violations {d[30]} (must be 0); sign certificate: {d[32]} of {d[31]} rays refused ({d[32] / max(d[31], 1):.4f})")
st = (C.c_ulonglong * 6)()
lib.rth_debug_cert_stats.argtypes = [C.c_void_p, C.c_void_p]
if lib.rth_debug_cert_stats(scene.h, st) == 0:
    print(f"direction table (G 0: none, the scene keeps the 32-B records): G {st[0]}, {st[1]} distinct normals, {st[2]} list entries ({st[2] / max(3 * st[0] * st[0], 1):.1f} per cell, "
          f"longest {st[3]}), {st[4] / 1e6:.1f} MB, built in {st[5] / 1e6:.3f} s")
# dbg[33..37]: the node cull of k_trace_oct (bounce passes; RTMI_NODE_CULL=0 or no direction table: all 0).  The counting build
# evaluates the node predicate at every first visit of an inner box by a certified lane outside a missed subtree and walks
# the subtree all the same: what it does inside is what the fast build saves.
print(f"node cull (k_trace_oct, RTMI_NODE_CULL={os.environ.get('RTMI_NODE_CULL', 'default')}): {d[33]} inner boxes first visited by "
      f"certified lanes outside a missed subtree, node box missed by the half-line {d[34]} ({d[34] / max(d[33], 1):.3f}); inside "
      f"missed subtrees: {d[35]} SELECT lane-steps ({d[35] / max(d[1], 1):.3f} of all), {d[36]} leaf visits "
      f"({d[36] / max(d[12], 1):.3f} of all); violations {d[37]} (must be 0)")
# DCtrl::hyb: the hybrid bounce passes (hybrid.hpp; RTMI_HYBRID=0 or no direction table: all 0).  The counting launch walks the
# octree as ever and runs the hybrid into scratch records; violations = records the hybrid stands by that differ from the walk's.
hy, hon = (C.c_ulonglong * 12)(), C.c_int(0)
lib.rth_debug_hybrid_counters.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
if lib.rth_debug_hybrid_counters(scene.h, hy, C.byref(hon)) == 0:
    h = list(hy)
    n = max(h[0], 1)
    print(f"hybrid passes (RTMI_HYBRID={os.environ.get('RTMI_HYBRID', 'default')}, on {hon.value}; last batch of each stream): "
          f"{h[0]} rays offered; certificate refusals {h[1]} ({h[1] / n:.4f}); BVH misses {h[2]} ({h[2] / n:.4f}); ties {h[3]} "
          f"({h[3] / n:.6f}); descents failed: absent child {h[4]}, no collision {h[5]}, tmin >= t* {h[6]} "
          f"({(h[4] + h[5] + h[6]) / n:.6f}); lists without the hit {h[7]} ({h[7] / n:.6f}); out of bounds {h[10]} (must be 0); "
          f"confirmed {h[11]} ({h[11] / n:.4f}); fallbacks {h[8]} ({h[8] / n:.4f}); violations {h[9]} (must be 0)")
ns = (C.c_ulonglong * 3)()
lib.rth_debug_node_cull_stats.argtypes = [C.c_void_p, C.c_void_p]
if lib.rth_debug_node_cull_stats(scene.h, ns) == 0:
    print(f"node cull records (0: none): {ns[0]}, {ns[1] / 1e6:.2f} MB, built in {ns[2] / 1e6:.3f} s")
# dbg[38..44] / dbg[45..51]: the node cull of k_path_primary (RTMI_PRIMARY_NODE_CULL=0, RTMI_NODE_CULL=0 or no direction
# table: all 0), for primary rays and for the mirror reflections it traces in place: lanes that took a ray with / without the
# certificate (CERT_KAPPA_PRIMARY), then the five of dbg[33..37].  d[1] and d[12] count all passes: the shares below are of
# the whole frame's SELECT lane-steps and leaf visits.
for who, b in (("primary rays", 38), ("mirror reflections in place", 45)):
    p = d[b:b + 7]
    print(f"node cull (k_path_primary, {who}, RTMI_PRIMARY_NODE_CULL={os.environ.get('RTMI_PRIMARY_NODE_CULL', 'default')}): lanes "
          f"certified {p[0]}, refused {p[1]} ({p[1] / max(p[0] + p[1], 1):.4f}); {p[2]} inner boxes first visited by certified lanes "
          f"outside a missed subtree, missed {p[3]} ({p[3] / max(p[2], 1):.3f}); inside missed subtrees: {p[4]} SELECT lane-steps "
          f"({p[4] / max(p[0] + p[1], 1):.1f} per ray, {p[4] / max(d[1], 1):.3f} of the frame's), {p[5]} leaf visits "
          f"({p[5] / max(p[0] + p[1], 1):.1f} per ray, {p[5] / max(d[12], 1):.3f} of the frame's); violations {p[6]} (must be 0)")
