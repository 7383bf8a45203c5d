"""Packet cull of k_path_primary (trace_oct.hpp, packet_culls): whenever the predicate says "cull" for a packet of 64 rays
and a triangle, the exact test rejects that triangle for every ray of the packet.  CPU only: rtmi_debug_packet_cull runs
the kernel's own __host__ __device__ functions on the host."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "tests", "golden", "teapot_tri.obj")
f32 = np.float32


def _orc():
    from oracle import orc
    return orc


def _cull(rays, recs):
    """rays (n, 8) f32 (o.xyzw, d.xyzw), recs (m, 8) f32 (incenter.xyz, r2, norm.xyz, 0) -> (on, cull (m,) bool)"""
    from rust_raytrace_amd import _ffi
    L = _ffi.lib()
    L.rtmi_debug_packet_cull.restype = C.c_int
    L.rtmi_debug_packet_cull.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    rays = np.ascontiguousarray(rays, f32)
    recs = np.ascontiguousarray(recs, f32)
    on = C.c_int(0)
    out = np.zeros(len(recs), np.uint8)
    assert L.rtmi_debug_packet_cull(rays.ctypes.data, len(rays), recs.ctypes.data, len(recs), C.byref(on), out.ctypes.data) == 0
    return on.value == 1, out.astype(bool)


def _plane_pass(rays, recs):
    """The plane part of Triangle::intersects (raytrace.rs:400-439) in f32, in the operation order of the oracle and the
    kernels (lane 3 included): True where `t >= 0` (or NaN) and `len2(ip) <= r2` (or NaN), shape (m, n)."""
    o, d = rays[None, :, 0:4], rays[None, :, 4:8]
    c, r2, n = recs[:, None, 0:3], recs[:, None, 3], recs[:, None, 4:7]
    with np.errstate(all="ignore"):
        a = c - o[..., :3]
        num = ((((f32(0) + n[..., 0] * a[..., 0]) + n[..., 1] * a[..., 1]) + n[..., 2] * a[..., 2])
               + f32(0) * (f32(0) - o[..., 3]))
        den = ((((f32(0) + n[..., 0] * d[..., 0]) + n[..., 1] * d[..., 1]) + n[..., 2] * d[..., 2]) + f32(0) * d[..., 3])
        t = num / den
        p = d * t[..., None] + o
        ip = p[..., :3] - c
        pw = p[..., 3]
        l2 = ((ip[..., 0] * ip[..., 0] + ip[..., 1] * ip[..., 1]) + ip[..., 2] * ip[..., 2]) + pw * pw
        return ~(t < 0) & ~(l2 > r2)


def _check(rays, recs):
    on, cull = _cull(rays, recs)
    bad = cull & _plane_pass(rays, recs).any(axis=1)
    assert not bad.any(), f"culled but passed for some ray: records {np.nonzero(bad)[0][:10]}"
    return on, cull


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(f32)


def _packet(rng, o0, d0, so, sd, n=64):
    o = (np.asarray(o0, f32) + rng.uniform(-so, so, (n, 3)).astype(f32)).astype(f32)
    d = _unit(np.asarray(d0, np.float64) + rng.uniform(-sd, sd, (n, 3)))
    o[0], d[0] = o0, _unit(d0)
    rays = np.zeros((n, 8), f32)
    rays[:, 0:3], rays[:, 4:7] = o, d
    return rays


def _rec(c, r, nrm):
    rec = np.zeros(8, f32)
    with np.errstate(over="ignore"):
        rec[0:3], rec[3], rec[4:7] = c, f32(r) * f32(r), _unit(nrm)
    return rec


@pytest.fixture(scope="module")
def canonical():
    orc = _orc()
    so = orc.canonical_scene(OBJ, accel="trivial")
    n = so.num_tris()
    raw = np.zeros((n, 29), f32)
    lib = orc.lib()
    kinds, surf = np.zeros(n, np.int32), np.zeros((n, 5), f32)
    lib.orc_get_triangles(so.h, raw.ctypes.data_as(C.c_void_p), kinds.ctypes.data_as(C.c_void_p), surf.ctypes.data_as(C.c_void_p))
    recs = np.zeros((n, 8), f32)
    recs[:, 0:3], recs[:, 3], recs[:, 4:7] = raw[:, 0:3], raw[:, 6], raw[:, 3:6]
    return so, raw, recs[1:]  # (triangle 0 is the sentinel)


def test_camera_pixel_packets(canonical):
    """The samples of one pixel from the canonical camera against every triangle of the canonical scene; the
    predicate must be sound and must reject most triangles (it is not vacuous)."""
    orc = _orc()
    so, raw, recs = canonical
    w = h = 256
    vp = orc.canonical_viewport(w, h)
    total = culled = 0
    for row in (3, 100, 128, 200):
        o4, d4 = orc.primary_rays(w, h, vp, 64, seed=7, row0=row, nrows=1)
        for col in (5, 64, 127, 250):
            rays = np.concatenate([o4[col * 64:(col + 1) * 64], d4[col * 64:(col + 1) * 64]], axis=1)
            on, cull = _check(rays, recs)
            assert on, f"pixel ({row}, {col}): packet cull off"
            total += len(cull); culled += int(cull.sum())
    assert culled > 0.9 * total, f"only {culled} of {total} (pixel, triangle) pairs culled"


def test_oracle_rejects_culled(canonical):
    """For a sample of culled (pixel packet, triangle) pairs, the oracle's own trace of a one-triangle scene misses
    with all 64 rays."""
    orc = _orc()
    so, raw, recs = canonical
    w = h = 512
    vp = orc.canonical_viewport(w, h)
    o4, d4 = orc.primary_rays(w, h, vp, 64, seed=3, row0=240, nrows=1)
    rays = np.concatenate([o4[17 * 64:18 * 64], d4[17 * 64:18 * 64]], axis=1)
    on, cull = _check(rays, recs)
    assert on
    # the triangles closest to the packet's line: the ones nearest to the threshold
    c = recs[:, 0:3].astype(np.float64) - rays[0, 0:3]
    dist = np.linalg.norm(np.cross(c, rays[0, 4:7].astype(np.float64)), axis=1) - np.sqrt(recs[:, 3])
    pick = [int(j) for j in np.argsort(dist) if cull[j]][:40]
    assert pick
    for j in pick:
        one = orc.Scene(with_dummy=True)
        pts = raw[j + 1, 20:29]
        one.add_triangle(pts, orc.Surface(orc.MATTE, orc.make_color(1, 2, 3), 0.2), float(raw[j + 1, 19]))
        one.build_trivial_bounding_box([0.0, 0.0, 20.1], 20.0)
        tri, t, face, _ = one.trace(rays[:, 0:4], rays[:, 4:8])
        assert (tri == 0).all(), f"triangle {j + 1} culled but hit by the oracle"


def test_random_packets():
    rng = np.random.default_rng(1)
    for it in range(200):
        scale = f32(10.0 ** rng.uniform(-3, 3))
        o0 = rng.uniform(-1, 1, 3).astype(f32) * scale
        d0 = _unit(rng.normal(size=3))
        rays = _packet(rng, o0, d0, float(scale) * 1e-3 * rng.uniform(0, 1), 1e-3 * rng.uniform(0, 1))
        c = (o0[None] + rng.normal(size=(300, 3)) * float(scale)).astype(f32)
        recs = np.stack([_rec(c[k], rng.uniform(0, 0.5) * float(scale), rng.normal(size=3)) for k in range(300)])
        on, cull = _check(rays, recs)
        assert on


def test_adversarial_threshold_grazing_and_planes():
    rng = np.random.default_rng(2)
    nculled = 0
    for it in range(150):
        o0 = rng.uniform(-3, 3, 3).astype(f32)
        d0 = _unit(rng.normal(size=3))
        rays = _packet(rng, o0, d0, 1e-3, 5e-4)
        perp = _unit(np.cross(d0, rng.normal(size=3)))
        recs = []
        for _ in range(60):
            s = rng.uniform(0.1, 20.0)
            r = rng.uniform(0.01, 1.0)
            # incenter at (r + tiny) from the reference line: right at the reject threshold
            dist = r + rng.choice([0.0, 1e-7, 1e-5, 1e-3, 1e-2]) * rng.choice([-1, 1])
            c = (o0 + d0 * s + perp * dist).astype(f32)
            nrm = rng.normal(size=3)
            kind = rng.integers(4)
            if kind == 1:  # grazing / edge-on: normal (almost) perpendicular to the direction, den of a few ulp
                nrm = _unit(np.cross(d0, rng.normal(size=3))).astype(np.float64)
                nrm = nrm + d0 * rng.choice([0.0, 1e-7, 1e-6, 1e-4])
            elif kind == 2:  # the reference origin on the plane
                c = (o0 + perp * dist).astype(f32)
                nrm = _unit(np.cross(perp, rng.normal(size=3)))
            recs.append(_rec(c, r, nrm))
        on, cull = _check(rays, np.stack(recs))
        assert on
        nculled += int(cull.sum())
    assert nculled > 0


def test_extreme_coordinates_and_lane3():
    rng = np.random.default_rng(3)
    for scale in (1e-30, 1e-12, 1e-6, 1e6, 1e12, 1e14, 1e16, 1e20, 1e30):
        o0 = (rng.uniform(-1, 1, 3) * scale).astype(f32)
        d0 = _unit(rng.normal(size=3))
        rays = _packet(rng, o0, d0, scale * 1e-4, 1e-4)
        c = (o0[None] + rng.normal(size=(200, 3)) * scale).astype(f32)
        recs = np.stack([_rec(c[k], rng.uniform(0, 0.5) * scale, rng.normal(size=3)) for k in range(200)])
        recs[::7, 3] = np.inf
        recs[1::7, 4:7] = 0.0
        recs[2::7, 0] = np.nan
        _check(rays, recs)
    rays = _packet(rng, [0.0, 0.0, 0.0], [0.0, 0.0, 1.0], 1e-3, 1e-3)
    recs = np.stack([_rec([5.0, 5.0, 5.0], 0.1, [0.0, 0.0, 1.0])])
    on, cull = _check(rays, recs)
    assert on and cull.all()
    for lane3 in ((5, 3), (17, 7)):
        r3 = rays.copy()
        r3[lane3[0], lane3[1]] = f32(1e-3)
        on, cull = _check(r3, recs)
        assert not on and not cull.any(), "a nonzero lane 3 must turn the packet cull off"
    wide = _packet(rng, [0.0, 0.0, 0.0], [0.0, 0.0, 1.0], 1e-3, 0.2)  # a wide cone: off
    assert not _cull(wide, recs)[0]


# ---------------------------------------------------------------- -m gpu
_RENDER = r"""
import ctypes as C, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from rust_raytrace_amd import raytrace as R, _ffi
counting = sys.argv[3] == "1"
sp = R.canonical_scene(os.path.join(sys.argv[1], "tests", "golden", "teapot_tri.obj"))
w = h = 512
img = np.zeros((h, w, 4), np.float32)
c = R.HipRayCaster(seed=5, options=R.OPT_COUNTERS) if counting else R.HipRayCaster(seed=5)
ctx = c.walk_rays(R.canonical_viewport(w, h, 5, 64), sp, img)
np.save(sys.argv[2], img)
if counting:
    L = _ffi.lib()
    L.rth_debug_counters_n.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    out = (C.c_ulonglong * 24)()
    L.rth_debug_counters_n(sp.h, out, 24)
    np.save(sys.argv[2] + ".dbg.npy", np.array(list(out), np.uint64))
"""


def _render(tmp_path, name, cull, counting):
    env = dict(os.environ, RTMI_PACKET_CULL="1" if cull else "0")
    out = str(tmp_path / name)
    subprocess.run([sys.executable, "-c", _RENDER, ROOT, out, "1" if counting else "0"], env=env, check=True, timeout=600)
    return np.load(out + ".npy")


@pytest.mark.gpu
def test_packet_cull_bit_exact_on_gpu(tmp_path):
    """512x512 @ 64 spp on the canonical scene, in fresh processes: the image with the packet cull equals the image
    without it bit for bit; the counting build evaluates the predicate and finds no violation."""
    a = _render(tmp_path, "on", True, False)
    b = _render(tmp_path, "off", False, False)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    c = _render(tmp_path, "count", True, True)
    assert np.array_equal(a.view(np.uint32), c.view(np.uint32))
    d = np.load(str(tmp_path / "count") + ".dbg.npy")
    print(f"\npacket LEAF steps {d[16]} of {d[17]}, references culled {d[19]} of {d[18]}, violations {d[20]}")
    assert d[16] > 0 and d[19] > 0
    assert d[20] == 0
