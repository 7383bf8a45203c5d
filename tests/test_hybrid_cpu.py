"""Hybrid bounce passes (hybrid.hpp, bvh_fast.hpp; DESIGN.md 4.1 "Hybrid pass"): the BVH proposes a ray's closest hit, a guided
descent through the reference's octree confirms it, everything else is walked exactly.  CPU only: the rtmi_debug_hybrid_* hooks
run the kernels' own __host__ __device__ functions on the host.  Checked here: a proposal the descent accepts is what the octree
oracle returns, bit for bit, and the descent accepts nearly every hit; the BVH's boxes come from the records alone; the child
slab equals BoundingBox::collides; the tie flag."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN, TEAPOT_TRI
from test_block_cull_cpu import mkrays, unit
from test_ray_cert_cpu import G

f32 = np.float32
HV_OK, HV_ABSENT, HV_NOCOLLIDE, HV_TMIN, HV_NOTRI, HV_BOUNDS = range(6)


def _lib():
    from rust_raytrace_amd import _ffi
    return _ffi.lib()


def hybrid_verify(geo, topo, refs, recs, rays, t, tri, g=G):
    """A flattened tree (the layout test_node_cull_cpu.node_cull takes), plane records (m, 8), rays (n, 8) and per ray a
    proposed hit -> (cert (n,) bool: the certificate AND the origin bound, out (n,) u8: HV_*, the scene's origin bound)."""
    L = _lib()
    vp = C.c_void_p
    L.rtmi_debug_hybrid_verify.restype = C.c_int
    L.rtmi_debug_hybrid_verify.argtypes = [vp, C.c_uint64, vp, C.c_uint64, C.c_uint64, vp, vp, C.c_uint64, C.c_uint32, vp, vp, vp, vp, vp]
    boxes = np.ascontiguousarray(np.concatenate([np.ascontiguousarray(geo, f32).view(np.uint32), np.asarray(topo, np.uint32)], axis=1),
                                 np.uint32)
    refs = np.ascontiguousarray(refs, np.uint32)
    recs, rays = np.ascontiguousarray(recs, f32), np.ascontiguousarray(rays, f32)
    t, tri = np.ascontiguousarray(t, f32), np.ascontiguousarray(tri, np.uint32)
    cert, out = np.zeros(len(rays), np.uint8), np.zeros(len(rays), np.uint8)
    omax = C.c_float(0)
    rc = L.rtmi_debug_hybrid_verify(boxes.ctypes.data, len(boxes), refs.ctypes.data, len(refs), len(recs), recs.ctypes.data,
                                    rays.ctypes.data, len(rays), g, t.ctypes.data, tri.ctypes.data, cert.ctypes.data, out.ctypes.data, C.byref(omax))
    assert rc == 0, L.rtmi_last_error()
    return cert.astype(bool), out, f32(omax.value)


# ---------------------------------------------------------------- verify against the oracle
@pytest.fixture(scope="module")
def canonical_rays():
    """The canonical scene with the octree and with the linear list; 96 x 96 primary rays at 1 spp and two seeded bounce rays
    from every hit point (uniform over the hemisphere on the ray's side of the triangle)."""
    from oracle import orc
    so, sl = orc.canonical_scene(TEAPOT_TRI), orc.canonical_scene(TEAPOT_TRI, accel="trivial")
    raw, _, _ = so.triangles()
    o4, d4 = orc.primary_rays(96, 96, orc.canonical_viewport(96, 96), 1)
    tri, t, face, _ = so.trace(o4, d4)
    hit = tri != 0
    p = (d4[hit, :3] * t[hit, None] + o4[hit, :3]).astype(f32)  # the hit point as shade_hit forms it
    n = raw[tri[hit], 3:6].astype(np.float64)
    n[(face[hit] & 1) != 0] *= -1.0  # a back-face hit leaves on the other side
    rng = np.random.default_rng(96)
    bo, bd = [], []
    for _ in range(2):
        d = unit(rng.normal(size=(len(p), 3)))
        flip = (d.astype(np.float64) * n).sum(axis=1) < 0
        d[flip] = -d[flip]
        bo.append(p); bd.append(d)
    rays = np.concatenate([np.concatenate([o4, d4], axis=1), mkrays(np.concatenate(bo), np.concatenate(bd))]).astype(f32)
    return so, sl, raw, rays, int(hit.sum())


def test_accepted_proposals_are_the_octree_oracles_hits(canonical_rays):
    from oracle import orc
    so, sl, raw, rays, nprim_hits = canonical_rays
    o4, d4 = np.ascontiguousarray(rays[:, 0:4]), np.ascontiguousarray(rays[:, 4:8])
    orc.set_finite_hits_only(1)
    try:
        ltri, lt, lface, _ = sl.trace(o4, d4)  # the closest hit over ALL triangles: what k_hybrid_bvh proposes
    finally:
        orc.set_finite_hits_only(0)
    otri, ot, oface, _ = so.trace(o4, d4)
    recs = np.zeros((len(raw), 8), f32)
    recs[:, 0:3], recs[:, 3], recs[:, 4:7] = raw[:, 0:3], raw[:, 6], raw[:, 3:6]
    geo, topo, refs = so.tree_flatten()
    cert, out, omax = hybrid_verify(geo, topo, refs, recs, rays, lt, ltri)
    assert omax == origin_max(raw[1:]) and omax > 40
    hit = ltri != 0
    acc = hit & cert & (out == HV_OK)
    print(f"\n{len(rays)} rays ({96 * 96} primary, {len(rays) - 96 * 96} bounce), {hit.sum()} hit; certificate refuses "
          f"{(hit & ~cert).sum()}; descent: absent {(hit & (out == HV_ABSENT)).sum()}, no collision {(hit & (out == HV_NOCOLLIDE)).sum()}, "
          f"tmin >= t {(hit & (out == HV_TMIN)).sum()}, list without the triangle {(hit & (out == HV_NOTRI)).sum()}, "
          f"bounds {(hit & (out == HV_BOUNDS)).sum()}; accepted {acc.sum()} ({acc.sum() / hit.sum():.4f})")
    assert nprim_hits > 1000 and hit.sum() > 3000
    assert not (out[hit] == HV_BOUNDS).any()
    bad = acc & ((otri != ltri) | (ot.view(np.uint32) != lt.view(np.uint32)) | (oface != lface))
    assert not bad.any(), (f"{bad.sum()} accepted rays differ from the octree oracle, first {np.nonzero(bad)[0][:5]}: "
                           f"{ltri[bad][:5]} vs {otri[bad][:5]}")
    assert acc.sum() >= 0.95 * hit.sum(), f"only {acc.sum()} of {hit.sum()} hit rays accepted"
    # a miss of the linear list is a miss of the octree
    assert not (otri[~hit] != 0).any()
    # a wrong proposal is not accepted: the true hit's time with another triangle of the scene
    wrong = ltri.copy()
    wrong[hit] = (ltri[hit] % (len(raw) - 1)) + 1
    _, wout, _ = hybrid_verify(geo, topo, refs, recs, rays[hit][:2000], lt[hit][:2000], wrong[hit][:2000])
    assert (wout != HV_OK).mean() > 0.5


# ---------------------------------------------------------------- the origin bound
def origin_max(rec):
    """hybrid_origin_max (hybrid.hpp): 16 (m + 1), m = the smallest |c|_1 + r of the records, in f32"""
    c = np.abs(rec[:, 0:3]).astype(f32)
    m = (((c[:, 0] + c[:, 1]) + c[:, 2]) + np.sqrt(rec[:, 6].astype(f32))).min()
    return f32(16.0) * (m + f32(1.0))


def intersects_f32(rec, o, d):
    """Triangle::intersects (raytrace.rs:400-439) of record rec (29,) for rays o, d (n, 3), lane 3 zero, in f32 in the kernels'
    operation order -> (accepted (n,), t (n,))"""
    c, nrm, r2 = rec[0:3], rec[3:6], rec[6]
    z = f32(0)
    with np.errstate(all="ignore"):
        a = c - o
        num = ((z + nrm[0] * a[:, 0]) + nrm[1] * a[:, 1]) + nrm[2] * a[:, 2]
        den = ((z + nrm[0] * d[:, 0]) + nrm[1] * d[:, 1]) + nrm[2] * d[:, 2]
        t = num / den
        p = d * t[:, None] + o
        ip = p - c
        l2 = (ip[:, 0] * ip[:, 0] + ip[:, 1] * ip[:, 1]) + ip[:, 2] * ip[:, 2]
        ok = ~(t < 0) & ~(l2 > r2)
        for k in range(3):
            s = rec[7 + 3 * k: 10 + 3 * k]
            ok &= ~(((ip[:, 0] * s[0] + ip[:, 1] * s[1]) + ip[:, 2] * s[2]) > rec[16 + k])
    assert t.dtype == f32 and p.dtype == f32
    return ok & np.isfinite(t), t


def bvh_slab_f32(lo, hi, o, d, tbest):
    """bvh_slab (bvh_fast.hpp) in f32: the box [lo, hi] against rays o, d on [0, tbest]"""
    with np.errstate(all="ignore"):
        inv = f32(1) / d
        t0, t1 = (lo - o) * inv, (hi - o) * inv
        tmin = np.fmax(np.fmin(t0, t1).max(axis=1), f32(0))
        tmax = np.fmax(t0, t1).min(axis=1) * f32(1.0000003)
    return (tmin <= tmax) & (tmin <= tbest) & (tmin < np.inf)


def edge_rays(rec, rng, n, dist):
    """n rays per call aimed at points on the edges of record rec's triangle (and a hair to either side), from `dist` away,
    every direction component well away from zero"""
    cor = rec[20:29].reshape(3, 3).astype(np.float64)
    k = rng.integers(0, 3, n)
    w = rng.uniform(0, 1, (n, 1))
    q = cor[k] * w + cor[(k + 1) % 3] * (1 - w)
    q += (cor.mean(axis=0) - q) * rng.uniform(-1e-4, 1e-3, (n, 1))
    u = unit(rng.normal(size=(n, 3))).astype(np.float64)
    u = np.where(np.abs(u) < 0.05, 0.05, u)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = (q - u * dist).astype(f32)
    d = (q - o.astype(np.float64))
    return o, (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)


def test_origin_bound_keeps_every_accepted_hit_inside_its_clip_box():
    """The hybrid's proof needs the BVH to reach every triangle the reference accepts.  The reference decides on the rounded hit
    point, the slab test on the line: from far away they part (the model finds accepted rays that miss the triangle's own clip
    box at 10^5 .. 10^6), within the origin bound they must not -- and the slab must be entered no later than the hit."""
    rec = np.load(os.path.join(GOLDEN, "canonical_triangle_records.npz"))["rec"]
    _, box, derived = record_boxes(rec[:, :20])
    assert (derived == 1).all()
    omax = origin_max(rec)
    assert 20 < omax < 100
    rng = np.random.default_rng(41)
    n = 40000
    inside = far = far_missed = 0
    for i in range(len(rec)):
        lo, hi = box[i, 0:3], box[i, 3:6]
        for dist in (0.5, 3.0, float(omax) / 4, float(omax) / 2, 1e5, 1e6):
            o, d = edge_rays(rec[i], rng, n, dist)
            ok, t = intersects_f32(rec[i], o, d)
            ok &= (np.abs(d) > 1e-3).all(axis=1)
            reach = bvh_slab_f32(lo, hi, o, d, t)
            within = np.abs(o).astype(f32).sum(axis=1) <= omax
            bad = ok & within & ~reach
            assert not bad.any(), f"record {i}, distance {dist}: {bad.sum()} accepted rays within the bound miss the clip box"
            inside += int((ok & within).sum())
            far += int((ok & ~within).sum()); far_missed += int((ok & ~within & ~reach).sum())
    print(f"\n{inside} accepted rays within the bound (|o|_1 <= {omax:.1f}), all reach their clip box; beyond it {far_missed} of {far} do not")
    assert inside > 500000 and far > 100000
    assert far_missed > 0, "the model no longer shows what the bound is for"


# ---------------------------------------------------------------- boxes from the records
def record_boxes(rec20):
    L = _lib()
    vp = C.c_void_p
    L.rtmi_debug_record_boxes.restype = C.c_int
    L.rtmi_debug_record_boxes.argtypes = [vp, C.c_uint64, vp, vp, vp]
    rec20 = np.ascontiguousarray(rec20, f32)
    n = len(rec20)
    corners, box, derived = np.zeros((n, 3, 3), f32), np.zeros((n, 6), f32), np.zeros(n, np.uint8)
    assert L.rtmi_debug_record_boxes(rec20.ctypes.data, n, corners.ctypes.data, box.ctypes.data, derived.ctypes.data) == 0
    return corners, box, derived


def _margin(rec):
    """the builder's widening (bvh_clip_box): 2e-5 (|c|_1 + r + 1)"""
    return 2e-5 * (np.abs(rec[:, 0:3]).sum(axis=1) + np.sqrt(rec[:, 6]) * 1.00001 + 1.0)


def _disc_box(rec):
    r = np.sqrt(rec[:, 6].astype(np.float64)) * 1.00001
    half = r[:, None] * np.sqrt(np.maximum(1.0 - rec[:, 3:6].astype(np.float64) ** 2, 0.0)) * 1.0001 + _margin(rec)[:, None]
    return rec[:, 0:3] - half, rec[:, 0:3] + half


def _check_corners(rec):
    corners, box, derived = record_boxes(rec[:, :20])
    assert (derived == 1).all()
    want = rec[:, 20:29].reshape(-1, 3, 3).astype(np.float64)
    m = _margin(rec)
    # (the records do not say which corner is which: every true corner has a solved one within the margin, and vice versa)
    dist = np.linalg.norm(want[:, :, None, :] - corners[:, None, :, :].astype(np.float64), axis=3)
    assert (dist.min(axis=2) <= m[:, None]).all() and (dist.min(axis=1) <= m[:, None]).all(), dist.min(axis=2).max()
    # the box holds the corners, lies inside the disc box, and is no wider than the corners' box plus the scaled margin
    lo, hi = box[:, 0:3], box[:, 3:6]
    assert (lo <= want.min(axis=1)).all() and (hi >= want.max(axis=1)).all()
    dlo, dhi = _disc_box(rec)
    assert (lo >= dlo - 1e-6).all() and (hi <= dhi + 1e-6).all()
    return lo, hi, want


def test_boxes_from_records_golden_triangles():
    rec = np.load(os.path.join(GOLDEN, "canonical_triangle_records.npz"))["rec"]
    _check_corners(rec)


def test_boxes_from_records_whole_canonical_scene_and_degenerate():
    from oracle import orc
    raw, _, _ = orc.canonical_scene(TEAPOT_TRI).triangles()
    rec = raw[1:]
    lo, hi, want = _check_corners(rec)
    dlo, dhi = _disc_box(rec)
    # the corners' boxes are a real tightening of the disc boxes
    assert ((hi - lo).prod(axis=1) < 0.8 * (dhi - dlo).prod(axis=1)).mean() > 0.5
    # degenerate records keep the disc box: two parallel edge tests, a zero edge direction, an unbounded region (one test
    # turned round), NaN in an edge test
    bad = np.repeat(rec[:1], 4, axis=0).copy()
    bad[0, 10:13] = bad[0, 7:10]
    bad[1, 7:10] = 0.0
    bad[2, 7:10] *= -1.0
    bad[3, 16] = np.nan
    corners, box, derived = record_boxes(bad[:, :20])
    assert (derived == 0).all() and (corners == 0).all()
    blo, bhi = _disc_box(bad)
    assert np.allclose(box[:, 0:3], blo, rtol=0, atol=1e-6) and np.allclose(box[:, 3:6], bhi, rtol=0, atol=1e-6)
    # a record that is not finite where the disc needs it: no BVH at all
    nf = rec[:1].copy()
    nf[0, 6] = np.inf
    assert record_boxes(nf[:, :20])[2][0] == 2


# ---------------------------------------------------------------- the shared slab function
def collides_f32(c, half, o, inv):
    """BoundingBox::collides (raytrace.rs:860-907) in f32 for rays without a zero direction component: (tmin, tmin < tmax)"""
    with np.errstate(all="ignore"):
        a = ((c - o) * inv).astype(f32)
        b = (inv * half[:, None]).astype(f32)
        t1, t2 = (a - b).astype(f32), (a + b).astype(f32)
        near, far = np.where(inv > 0, t1, t2), np.where(inv > 0, t2, t1)
        tmin = np.fmax(np.fmax(near[:, 0], near[:, 1]), near[:, 2])
        tmax = np.fmin(np.fmin(far[:, 0], far[:, 1]), far[:, 2])
    return tmin, tmin < tmax


def test_child_slab_equals_collides():
    L = _lib()
    vp = C.c_void_p
    L.rtmi_debug_hybrid_slab.restype = C.c_int
    L.rtmi_debug_hybrid_slab.argtypes = [vp, vp, vp, C.c_uint64, vp, vp]
    rng = np.random.default_rng(5)
    n = 200000
    parent = np.zeros((n, 4), f32)
    parent[:, 0:3] = rng.uniform(-20, 20, (n, 3))
    parent[:, 3] = np.ldexp(f32(20.0), -rng.integers(1, 12, n)).astype(f32)  # the children's half edge: root_half 2^-(lvl + 1)
    parent[n // 2:, 3] = rng.uniform(1e-3, 10, n - n // 2)
    octs = rng.integers(0, 8, n).astype(np.uint32)
    rays = np.zeros((n, 6), f32)
    rays[:, 0:3] = rng.uniform(-25, 25, (n, 3))
    d = rng.normal(size=(n, 3))
    d[: n // 4] *= 10.0 ** rng.uniform(-12, 0, (n // 4, 3))  # tiny components of either sign
    d[n // 4: n // 3, rng.integers(0, 3)] *= 1e-30
    rays[:, 3:6] = unit(d)
    dd = rays[:, 3:6]
    dd[dd == 0] = f32(2e-38)
    rays[: n // 8, 0:3] = parent[: n // 8, 0:3]  # origins on the centre planes
    tmin, hit = np.zeros(n, f32), np.zeros(n, np.uint8)
    assert L.rtmi_debug_hybrid_slab(parent.ctypes.data, octs.ctypes.data, rays.ctypes.data, n, tmin.ctypes.data, hit.ctypes.data) == 0
    hc = parent[:, 3]
    sign = np.stack([np.where(octs & 1, hc, -hc), np.where(octs & 2, hc, -hc), np.where(octs & 4, hc, -hc)], axis=1).astype(f32)
    c = (parent[:, 0:3] + sign).astype(f32)  # the builder's child centre: orig + (+-newlen2)
    with np.errstate(all="ignore"):
        inv = (f32(1.0) / rays[:, 3:6]).astype(f32)
    wmin, whit = collides_f32(c, hc, rays[:, 0:3], inv)
    assert (rays[:, 3:6] < 0).any() and (np.abs(rays[:, 3:6]) < 1e-20).any()
    assert np.array_equal(hit.astype(bool), whit)
    ok = ~np.isnan(wmin)
    assert np.array_equal(tmin[ok].view(np.uint32), wmin[ok].view(np.uint32)) and np.isnan(tmin[~ok]).all()
    assert 0.02 < whit.mean() < 0.98


# ---------------------------------------------------------------- the tie rule
def tie_flag(t, tri):
    L = _lib()
    vp = C.c_void_p
    L.rtmi_debug_hybrid_tie.restype = C.c_int
    L.rtmi_debug_hybrid_tie.argtypes = [vp, vp, C.c_uint64, vp, vp, vp]
    t, tri = np.ascontiguousarray(t, f32), np.ascontiguousarray(tri, np.uint32)
    flag, btri, bt = C.c_uint8(0), C.c_uint32(0), C.c_float(0)
    assert L.rtmi_debug_hybrid_tie(t.ctypes.data, tri.ctypes.data, len(t), C.byref(flag), C.byref(btri), C.byref(bt)) == 0
    return bool(flag.value), btri.value, f32(bt.value)


def test_tie_rule_model():
    """Whatever the order the triangles are met in: the flag is set at the end iff two different triangles share the smallest
    time (+0 == -0), and the best is the lowest index among them."""
    rng = np.random.default_rng(9)
    pool = np.array([0.0, -0.0, 1.0, 1.0, 2.5, 2.5, 3.0, np.nextafter(f32(1.0), f32(2.0))], f32)
    nset = nclear = 0
    for it in range(4000):
        n = int(rng.integers(1, 9))
        tri = rng.integers(1, 6, n).astype(np.uint32)
        t = pool[rng.integers(2 if it % 2 else 0, len(pool), n)]
        # one triangle, one time: a triangle met again (it is in one leaf only, but the rule must not depend on that)
        for k in range(n):
            t[k] = t[np.nonzero(tri == tri[k])[0][0]]
        flag, btri, bt = tie_flag(t, tri)
        tm = t.min()
        winners = np.unique(tri[t == tm])
        assert flag == (len(winners) > 1), (t, tri, flag)
        assert btri == winners.min() and bt == tm
        nset += flag; nclear += not flag
    assert nset > 200 and nclear > 200
    assert tie_flag([0.0, -0.0], [2, 1]) == (True, 1, f32(0.0))
    assert tie_flag([5.0, 5.0, 3.0], [1, 2, 3])[0] is False
    assert tie_flag([3.0, 5.0, 5.0], [1, 2, 3])[0] is False
    assert tie_flag([], [])[0:2] == (False, 0)
