"""Any-hit occlusion (rtmi_occluded / rtmi_occluded_device): the entry points exist and are declared, they refuse bad arguments
before any HIP call and before the scene is used, the Python methods validate their arguments, and the expectations the GPU
tests compare with (tests/occluded_ref.py, from the oracle alone) are not trivial.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import occluded_ref as OR

RTMI_OK, RTMI_ERR_INVALID, RTMI_ERR_UNSUPPORTED = 0, 1, 3
NAMES = ("rtmi_occluded", "rtmi_occluded_device", "rth_caster_occluded", "rth_caster_occluded_device")
BOGUS = C.c_void_p(0x10)  # a dangling scene handle: never dereferenced when a check fails
ORIG, DIR, TMAX, OUT = (0x100000 * k for k in range(1, 5))  # never touched: every call fails or is empty


def _lib():
    from rust_raytrace_amd import _ffi
    return _ffi, _ffi.lib()


def _both(n=48, bufs=(ORIG, DIR, TMAX, OUT), scene=BOGUS):
    """(rc, message, stats.rays) of the device and of the host variant for the same arguments"""
    ffi, L = _lib()
    o, d, tm, out = (C.c_void_p(p) if p else None for p in bufs)
    res = []
    for dev in (True, False):
        st = ffi.Stats()
        st.rays = 123
        if dev:
            rc = L.rtmi_occluded_device(scene, n, o, d, tm, out, None, C.byref(st))
        else:
            rc = L.rtmi_occluded(scene, n, o, d, tm, out, C.byref(st))
        res.append((rc, L.rtmi_last_error(), st.rays))
    return res


def test_entry_points_are_exported_declared_and_listed():
    ffi, L = _lib()
    text = open(os.path.join(ROOT, "include", "rtmi.h")).read() + open(os.path.join(ROOT, "include", "rtmi_host.h")).read()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in ffi.RTMI_SYMBOLS + ffi.RTH_SYMBOLS, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name


def test_null_scene_and_buffers_are_refused_and_stats_cleared():
    for rc, msg, rays in _both(scene=None):
        assert rc == RTMI_ERR_INVALID and b"scene" in msg and rays == 0, msg
    for rc, msg, rays in _both(scene=None, n=0):  # the scene comes before the empty set
        assert rc == RTMI_ERR_INVALID and b"scene" in msg and rays == 0, msg
    for k in (0, 1, 3):
        bufs = [ORIG, DIR, TMAX, OUT]
        bufs[k] = 0
        for rc, msg, rays in _both(bufs=bufs):
            assert rc == RTMI_ERR_INVALID and b"NULL" in msg and rays == 0, msg
    # a NULL tmax is +inf for every ray, not an error: the next check that fails is reached
    for rc, msg, _ in _both(bufs=(ORIG, DIR, 0, ORIG)):
        assert rc == RTMI_ERR_INVALID and b"alias" in msg, msg


def test_an_empty_set_is_ok_and_touches_nothing():
    for bufs in ((ORIG, DIR, TMAX, OUT), (0, 0, 0, 0), (ORIG, DIR, 0, ORIG)):
        for rc, _, rays in _both(n=0, bufs=bufs):
            assert rc == RTMI_OK and rays == 0


def test_an_output_that_aliases_an_input_is_refused():
    for k, word in ((0, b"orig4"), (1, b"dir4"), (2, b"tmax")):
        bufs = [ORIG, DIR, TMAX, OUT]
        bufs[3] = bufs[k]
        for rc, msg, rays in _both(bufs=bufs):
            assert rc == RTMI_ERR_INVALID and b"alias" in msg and word in msg and rays == 0, msg
    n = 48
    # overlapping byte ranges: the output starts inside an input (16 n, 16 n, 4 n bytes), or an input inside the output (n bytes)
    for bufs, word in (((ORIG, DIR, TMAX, ORIG + 16 * n - 1), b"orig4"), ((ORIG, DIR, TMAX, DIR + 5), b"dir4"),
                       ((ORIG, DIR, TMAX, TMAX + 4 * n - 1), b"tmax"), ((OUT + n - 1, DIR, TMAX, OUT), b"orig4"),
                       ((ORIG, DIR, OUT + 1, OUT), b"tmax")):
        for rc, msg, _ in _both(n=n, bufs=bufs):
            assert rc == RTMI_ERR_INVALID and b"alias" in msg and word in msg, (bufs, msg)
    # adjacent is not aliased: the next check that fails is the ray count
    for rc, msg, _ in _both(n=1 << 31, bufs=(0x1000, 0x1000 + (16 << 31), 0, 0x1000 + (32 << 31))):
        assert rc == RTMI_ERR_UNSUPPORTED, msg


def test_too_many_rays_are_unsupported():
    big = 1 << 40
    for n in (1 << 31, (1 << 31) + 5, 1 << 33):
        for rc, msg, rays in _both(n=n, bufs=(big, 2 * big, 3 * big, 4 * big)):
            assert rc == RTMI_ERR_UNSUPPORTED and b"2^31" in msg and rays == 0, msg


def test_python_api_validates_its_arguments(canonical_pair):
    from rust_raytrace_amd import raytrace as R
    _, sp = canonical_pair
    c = R.HipRayCaster()
    o4, d4 = np.zeros((5, 4), np.float32), np.zeros((5, 4), np.float32)
    with pytest.raises(ValueError):
        c.occluded(sp, o4, d4[:4])
    with pytest.raises(ValueError):
        c.occluded(sp, o4, d4, tmax=np.zeros(4, np.float32))
    for ptrs in ((0, 8192, 0, 12288), (4096, None, 0, 12288), (4096, 8192, 0, 0), (4096, 8192, 0, 4096), (4096, 8192, 0, 8192),
                 (4096, 8192, 12288, 12288)):
        with pytest.raises(ValueError):
            c.occluded_device(sp, 5, *ptrs)
    with pytest.raises(ValueError):
        c.occluded_device(sp, -1, 4096, 8192, 0, 12288)


# ---------------------------------------------------------------- the expectations, on the oracle alone
@pytest.fixture(scope="module")
def primary(canonical_pair):
    from oracle import orc
    so, _ = canonical_pair
    o4, d4 = orc.primary_rays(64, 64, orc.canonical_viewport(64, 64), 1)
    tri, t, _ = OR.closest_hits(so, o4, d4)
    return so, o4, d4, tri, t


def test_the_rule_on_known_values():
    nan, inf = np.nan, np.inf
    tri = np.array([0, 3, 3, 3, 3, 3, 3, 3, 3, 0], np.uint32)
    t = np.array([0, 1, 1, 1, nan, inf, 0, 0, 1, 0], np.float32)
    tmax = np.array([inf, 1, np.nextafter(np.float32(1), np.float32(2)), nan, inf, inf, 0, -0.0, -1, 5], np.float32)
    assert OR.from_hits(tri, t, tmax).tolist() == [0, 0, 1, 0, 0, 0, 0, 0, 0, 0]
    assert OR.from_hits(tri, t, None).tolist() == [0, 1, 1, 1, 0, 0, 1, 1, 1, 0]  # NULL = +inf: finite hits only


def test_shadow_segments_are_a_mixed_set(primary):
    """Light at occluded_ref.LIGHT = (-3, 6, 1): 274 of the 825 segments (33 %) are occluded, the rest see the light."""
    so, o4, d4, tri, t = primary
    so4, sd4, dist = OR.shadow_segments(so, o4, d4)
    assert so4.shape[0] == int((tri != 0).sum()) > 500 and np.isfinite(dist).all() and (dist > 1.0).all()
    assert np.allclose(np.linalg.norm(sd4[:, :3], axis=1), 1.0, atol=1e-6)
    occ = OR.expected(so, so4, sd4, dist)
    frac = float(occ.mean())
    print(f"shadow segments to {OR.LIGHT}: {int(occ.sum())} of {occ.size} occluded ({frac:.3f})")
    assert 0.05 <= frac <= 0.95
    # without the limit more segments are blocked (geometry behind the light counts), never fewer
    unlimited = OR.expected(so, so4, sd4, None)
    assert (unlimited >= occ).all()


def test_nextafter_flips_every_hit_ray(primary):
    so, o4, d4, tri, t = primary
    hit = tri != 0
    assert hit.sum() > 500 and np.isfinite(t[hit]).all()
    fam = OR.tmax_families(t)
    at_t = OR.from_hits(tri, t, fam["t"])
    after = OR.from_hits(tri, t, fam["nextafter"])
    assert not at_t.any()  # a hit at t == tmax does not occlude
    assert np.array_equal(after != 0, hit)  # one ulp further and every hit ray is occluded; a miss never is
    for name in ("zero", "nan", "minus_one"):
        assert not OR.from_hits(tri, t, fam[name]).any(), name
    assert np.array_equal(OR.from_hits(tri, t, fam["null"]), OR.from_hits(tri, t, fam["inf"]))
    assert np.array_equal(OR.from_hits(tri, t, None) != 0, hit)
    mix = OR.from_hits(tri, t, fam["mix"])
    assert 0 < mix[hit].sum() < hit.sum()  # neighbouring rays get different answers
