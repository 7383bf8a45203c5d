"""Path tracing of caller-supplied rays (rtmi_render_rays / rtmi_render_rays_device) and rtmi_trace_device: the entry points
exist and are declared, they refuse bad arguments before any HIP call and before the scene is used, the Python methods validate
their arguments, and the expectations the GPU tests compare with (tests/rays_ref.py, from the oracle alone) are not trivial.
No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, build_pair, recipe_axis_box
import rays_ref as RR

RTMI_OK, RTMI_ERR_INVALID, RTMI_ERR_UNSUPPORTED = 0, 1, 3
NAMES = ("rtmi_render_rays", "rtmi_render_rays_device", "rtmi_trace_device", "rth_caster_walk_rays_explicit",
         "rth_caster_walk_rays_explicit_device", "rth_caster_trace_device")
BOGUS = C.c_void_p(0x10)  # a dangling scene handle: never dereferenced when a check fails
ORIG, DIR, KEYS, COLOR, MEAN, ALBEDO, NORMAL, IDS = (0x100000 * k for k in range(1, 9))  # never touched: every call fails or is empty
OUTS = ("color", "mean", "albedo", "normal", "ids")


def _lib():
    from rust_raytrace_amd import _ffi
    return _ffi, _ffi.lib()


def _both(n=48, orig=ORIG, dirs=DIR, keys=KEYS, scene=BOGUS, rays=(5, 4, 0, 0), out=(COLOR, MEAN, ALBEDO, NORMAL, IDS)):
    """(rc, message, stats.rays) of the device and of the host variant for the same arguments; rays / out None: a NULL struct"""
    ffi, L = _lib()
    r = C.byref(ffi.Rays(*rays)) if rays is not None else None
    o = C.byref(ffi.RaysOut(*[p or None for p in out])) if out is not None else None
    ptr = lambda p: C.c_void_p(p) if p else None
    res = []
    for dev in (True, False):
        st = ffi.Stats()
        st.rays = 123
        if dev:
            rc = L.rtmi_render_rays_device(scene, n, ptr(orig), ptr(dirs), ptr(keys), 7, r, o, None, C.byref(st))
        else:
            rc = L.rtmi_render_rays(scene, n, ptr(orig), ptr(dirs), ptr(keys), 7, r, o, C.byref(st))
        res.append((rc, L.rtmi_last_error(), st.rays))
    return res


def _refused(code, word, **kw):
    for rc, msg, rays in _both(**kw):
        assert rc == code and word in msg and rays == 0, (kw, rc, msg)


def test_entry_points_are_exported_declared_and_listed():
    ffi, L = _lib()
    text = open(os.path.join(ROOT, "include", "rtmi.h")).read() + open(os.path.join(ROOT, "include", "rtmi_host.h")).read()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in ffi.RTMI_SYMBOLS + ffi.RTH_SYMBOLS, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
    assert C.sizeof(ffi.Rays) == 16 and C.sizeof(ffi.RaysOut) == 5 * C.sizeof(C.c_void_p)
    assert re.search(r"\}\s*rtmi_rays_t;\s*/\* 16 bytes \*/", text)
    assert re.search(r"RTMI_RAYS_MAKE_RAY\s*=\s*1u << 0", text)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES[:3]:
        assert re.search(r"pub fn " + name + r"\(", doc), name


def test_null_arguments_are_refused_and_stats_cleared():
    _refused(RTMI_ERR_INVALID, b"scene", scene=None)
    _refused(RTMI_ERR_INVALID, b"scene", scene=None, n=0)  # the scene comes before the empty set
    _refused(RTMI_ERR_INVALID, b"(rays)", rays=None)
    _refused(RTMI_ERR_INVALID, b"(out)", out=None)
    _refused(RTMI_ERR_INVALID, b"(orig4)", orig=0)
    _refused(RTMI_ERR_INVALID, b"(dir4)", dirs=0)
    _refused(RTMI_ERR_INVALID, b"outputs", out=(0, 0, 0, 0, 0))
    # NULL keys are the formula, not an error: the next check that fails is reached
    _refused(RTMI_ERR_UNSUPPORTED, b"maxdepth", keys=0, rays=(33, 4, 0, 0))
    # one output is enough
    for k in range(5):
        out = [0] * 5
        out[k] = COLOR
        _refused(RTMI_ERR_UNSUPPORTED, b"maxdepth", out=out, rays=(33, 4, 0, 0))


def test_group_flags_and_key_range_are_checked():
    _refused(RTMI_ERR_INVALID, b"group", rays=(5, 0, 0, 0))
    _refused(RTMI_ERR_INVALID, b"group", rays=(5, 0, 0, 0), n=0)  # the parameter struct comes before the empty set
    _refused(RTMI_ERR_INVALID, b"multiple", rays=(5, 5, 0, 0))  # 48 % 5
    _refused(RTMI_ERR_INVALID, b"flag", rays=(5, 4, 0, 2))
    _refused(RTMI_ERR_INVALID, b"flag", rays=(5, 4, 0, 0x80000001))
    _refused(RTMI_ERR_UNSUPPORTED, b"maxdepth", rays=(33, 4, 0, 1))  # RTMI_RAYS_MAKE_RAY alone is known
    # keys == NULL: the last group's pixel is pixel0 + n / G - 1
    _refused(RTMI_ERR_INVALID, b"pixel0", keys=0, rays=(5, 4, 0xFFFFFFFF - 10, 0))  # 12 groups: the last one would be 2^32
    _refused(RTMI_ERR_UNSUPPORTED, b"maxdepth", keys=0, rays=(33, 4, 0xFFFFFFFF - 11, 0))  # the last one is 2^32 - 1: allowed
    _refused(RTMI_ERR_UNSUPPORTED, b"maxdepth", rays=(33, 4, 0xFFFFFFFF, 0))  # with keys pixel0 is not used


def test_limits_are_unsupported():
    big = 1 << 40
    far = dict(orig=big, dirs=2 * big, keys=3 * big, out=tuple(k * big for k in range(4, 9)))
    for n in (1 << 31, (1 << 31) + 4, 1 << 33):
        _refused(RTMI_ERR_UNSUPPORTED, b"2^31", n=n, **far)
    _refused(RTMI_ERR_UNSUPPORTED, b"maxdepth", rays=(33, 4, 0, 0))
    _refused(RTMI_ERR_UNSUPPORTED, b"group", n=65537 * 2, rays=(5, 65537, 0, 0), **far)
    # the invalid-argument checks come first
    _refused(RTMI_ERR_INVALID, b"multiple", n=(1 << 31) + 1, rays=(33, 4, 0, 0), **far)


def test_overlapping_buffers_are_refused():
    n, g = 48, 12
    bufs = dict(orig=ORIG, dirs=DIR, keys=KEYS, color=COLOR, mean=MEAN, albedo=ALBEDO, normal=NORMAL, ids=IDS)
    size = dict(orig=16 * n, dirs=16 * n, keys=8 * n, color=16 * n, mean=16 * g, albedo=16 * g, normal=16 * g, ids=4 * g)
    word = dict(orig=b"orig4", dirs=b"dir4")

    def call(b):
        return dict(n=n, orig=b["orig"], dirs=b["dirs"], keys=b["keys"], out=tuple(b[k] for k in OUTS))

    names = list(bufs)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            for start in (bufs[a], bufs[a] + size[a] - 1):  # the same buffer, and one that begins on the other's last byte
                moved = dict(bufs)
                moved[b] = start
                for rc, msg, rays in _both(**call(moved)):
                    assert rc == RTMI_ERR_INVALID and b"overlap" in msg and rays == 0, (a, b, msg)
                    assert word.get(a, a.encode()) in msg and word.get(b, b.encode()) in msg, (a, b, msg)
            moved = dict(bufs)
            moved[b] = bufs[a] + size[a]  # adjacent is not overlapping: the next check that fails is reached
            for rc, msg, _ in _both(rays=(33, 4, 0, 0), **call(moved)):
                assert rc == RTMI_ERR_UNSUPPORTED and b"maxdepth" in msg, (a, b, msg)


def test_an_empty_set_is_ok_and_touches_nothing():
    for kw in (dict(), dict(orig=0, dirs=0, keys=0, out=(0, 0, 0, 0, 0)), dict(out=(COLOR, COLOR, COLOR, COLOR, COLOR)),
               dict(rays=(33, 70000, 0, 0))):
        for rc, _, rays in _both(n=0, **kw):
            assert rc == RTMI_OK and rays == 0, kw


def _trace_device(n=48, bufs=(ORIG, DIR, COLOR, MEAN, IDS), scene=BOGUS):
    ffi, L = _lib()
    st = ffi.Stats()
    st.rays = 123
    rc = L.rtmi_trace_device(scene, n, *[C.c_void_p(p) if p else None for p in bufs], None, C.byref(st))
    return rc, L.rtmi_last_error(), st.rays


def test_trace_device_checks_are_rtmi_traces_plus_overlap():
    rc, msg, rays = _trace_device(scene=None)
    assert rc == RTMI_ERR_INVALID and b"scene" in msg and rays == 0
    rc, msg, rays = _trace_device(scene=None, n=0)
    assert rc == RTMI_ERR_INVALID and b"scene" in msg and rays == 0
    assert _trace_device(n=0, bufs=(0, 0, 0, 0, 0)) == (RTMI_OK, _trace_device(n=0)[1], 0)
    for k in range(5):
        bufs = [ORIG, DIR, COLOR, MEAN, IDS]
        bufs[k] = 0
        rc, msg, rays = _trace_device(bufs=bufs)
        assert rc == RTMI_ERR_INVALID and b"NULL" in msg and rays == 0, msg
    names = (b"orig4", b"dir4", b"tri", b"t", b"face")
    n = 48
    size = (16 * n, 16 * n, 4 * n, 4 * n, 4 * n)
    for i in range(5):
        for j in range(i + 1, 5):
            bufs = [ORIG, DIR, COLOR, MEAN, IDS]
            bufs[j] = bufs[i] + size[i] - 1
            rc, msg, rays = _trace_device(bufs=bufs)
            assert rc == RTMI_ERR_INVALID and b"overlap" in msg and names[i] in msg and names[j] in msg and rays == 0, msg
    big = 1 << 40
    rc, msg, rays = _trace_device(n=1 << 31, bufs=tuple(k * big for k in range(1, 6)))
    assert rc == RTMI_ERR_UNSUPPORTED and b"2^31" in msg and rays == 0


def test_python_api_validates_its_arguments(canonical_pair):
    import torch
    from rust_raytrace_amd import raytrace as R
    _, sp = canonical_pair
    c = R.HipRayCaster()
    o4, d4 = np.zeros((6, 4), np.float32), np.zeros((6, 4), np.float32)
    d4[:, 2] = 1.0
    bad = (dict(orig4=o4, dir4=d4[:5], maxdepth=3), dict(orig4=o4, dir4=d4, maxdepth=33), dict(orig4=o4, dir4=d4, maxdepth=-1),
           dict(orig4=o4, dir4=d4, maxdepth=3, group=0), dict(orig4=o4, dir4=d4, maxdepth=3, group=4),
           dict(orig4=o4, dir4=d4, maxdepth=3, group=65537), dict(orig4=o4, dir4=d4, maxdepth=3, keys=np.zeros((5, 2), np.uint32)),
           dict(orig4=o4, dir4=d4, maxdepth=3, pixel0=(1 << 32) - 5), dict(orig4=o4, dir4=d4, maxdepth=3, pixel0=-1),
           dict(orig4=o4, dir4=d4, maxdepth=3, color=False))
    for kw in bad:
        with pytest.raises(ValueError):
            c.walk_rays_explicit(sp, **kw)
    # the device variants take torch tensors on the device: NumPy arrays, host tensors and wrong shapes never reach the library
    to, td = torch.zeros(24), torch.zeros(24)
    col = torch.zeros(24)
    for kw in (dict(orig4=o4, dir4=d4, color=o4), dict(orig4=to, dir4=td, color=col), dict(orig4=to.double(), dir4=td, color=col),
               dict(orig4=torch.zeros(23), dir4=td, color=col)):
        with pytest.raises(ValueError):
            c.walk_rays_explicit_device(sp, maxdepth=3, **kw)
    for args in ((o4, d4, o4, o4, o4), (to, td, torch.zeros(6, dtype=torch.int32), torch.zeros(6), torch.zeros(6, dtype=torch.int32))):
        with pytest.raises(ValueError):
            c.trace_device(sp, *args)

    class FakeDeviceTensor:  # enough of a device tensor to reach the checks behind "is it on the device"
        is_cuda = True

        def __init__(self, n, dtype="torch.float32", ptr=0x1000, contiguous=True):
            self._n, self.dtype, self._ptr, self._c = n, dtype, ptr, contiguous

        def data_ptr(self):
            return self._ptr

        def numel(self):
            return self._n

        def is_contiguous(self):
            return self._c

    T = FakeDeviceTensor
    o, d = T(24, ptr=0x10000), T(24, ptr=0x20000)
    for kw in (dict(color=T(20, ptr=0x30000)), dict(color=T(24, "torch.float64", 0x30000)), dict(color=T(24, ptr=0x30000, contiguous=False)),
               dict(mean=T(24, ptr=0x30000), group=2), dict(ids=T(6, "torch.float32", 0x30000)), dict(color=T(24, ptr=0x30000), keys=T(12, "torch.float32", 0x40000)),
               dict(color=T(24, ptr=0x30000), keys=T(10, "torch.int32", 0x40000)), dict(), dict(color=T(24, ptr=0x10000 + 95)),
               dict(color=T(24, ptr=0x30000), ids=T(6, "torch.int32", 0x30000 + 95))):
        with pytest.raises(ValueError):
            c.walk_rays_explicit_device(sp, o, d, 3, **kw)


# ---------------------------------------------------------------- the expectations, on the oracle alone
def _orc():
    from oracle import orc
    return orc


def test_centred_rays_expectations_are_not_trivial(canonical_pair):
    """The canonical 33 x 33 view at 1 spp: 65 rays with a zero direction component (the camera's row and column), 218 hits,
    20 of them edge faces, 1 518 `Rays` at depth 5."""
    orc = _orc()
    so, _ = canonical_pair
    c = RR.CENTRED
    vo = orc.canonical_viewport(c["w"], c["h"])
    o4, d4, keys = RR.camera_rays(orc, vo, **c)
    assert o4.shape == (33 * 33, 4) and keys[-1].tolist() == [33 * 33 - 1, 0]
    assert RR.zero_component_rays(d4) == 65
    tri, t, face, _ = so.trace(o4, d4)
    assert int((tri != 0).sum()) == 218 and int(((face & 2) != 0)[tri != 0].sum()) == 20
    img, cn = so.render(c["w"], c["h"], vo, c["maxdepth"], c["spp"], seed=c["seed"])
    assert cn["rays"] == 1518
    # depth 1 from the hits alone equals the oracle's depth-1 render: the formula of rays_ref is the renderer's
    _, kinds, surf = so.triangles()
    img1, _ = so.render(c["w"], c["h"], vo, 1, 1, seed=c["seed"])
    assert np.array_equal(RR.depth1_color(tri, face, kinds, surf).view(np.uint32), img1.reshape(-1, 4).view(np.uint32))
    assert len(np.unique(img.reshape(-1, 4), axis=0)) >= 10  # a few surfaces and depths: a palette, but not one colour


def test_jittered_rays_expectations_are_not_trivial(canonical_pair):
    """24 x 24 at 4 spp, seed 7: 3 271 `Rays` for 2 304 samples; the second camera sees the scene too."""
    orc = _orc()
    so, _ = canonical_pair
    c = RR.JITTERED
    vo = orc.canonical_viewport(c["w"], c["h"])
    o4, d4, keys = RR.camera_rays(orc, vo, **c)
    assert o4.shape[0] == 2304 and keys[5].tolist() == [1, 1]
    img, cn = so.render(c["w"], c["h"], vo, c["maxdepth"], c["spp"], seed=c["seed"])
    assert cn["rays"] == 3271
    s = RR.SECOND
    img2, cn2 = so.render(s["w"], s["h"], RR.second_viewport(orc), s["maxdepth"], s["spp"], seed=s["seed"])
    assert cn2["rays"] > s["w"] * s["h"] * s["spp"] and len(np.unique(img2.reshape(-1, 4), axis=0)) >= 10


def test_fold_and_vunit_on_known_values():
    col = np.array([[1, 2, 3, 0], [0.5, 0.25, 0.125, 0], [1e-8, 3, 0, 0], [np.inf, np.nan, 1, 0]], np.float32)
    assert np.array_equal(RR.fold(col, 1).view(np.uint32), col.view(np.uint32))
    m = RR.fold(col, 2)
    assert m[0].tolist() == [0.75, 1.125, 1.5625, 0.0] and np.isinf(m[1, 0]) and np.isnan(m[1, 1]) and m[1, 2] == 0.5
    third = RR.fold(np.ones((3, 4), np.float32), 3)  # (1 + 1 + 1) * (1.f / 3.f), not 3 / 3
    assert third[0, 0] == np.float32(3.0) * (np.float32(1.0) / np.float32(3.0))
    d = np.array([[3, 0, 4, 0], [0, 0, 2, 0], [1, 1, 1, 1], [0, 0, 0, 0]], np.float32)
    u = RR.vunit(d)
    assert u[0].tolist() == [np.float32(3) * np.float32(0.2), 0.0, np.float32(4) * np.float32(0.2), 0.0]
    assert u[1].tolist() == [0.0, 0.0, 1.0, 0.0] and u[2].tolist() == [0.5] * 4 and np.isnan(u[3]).all()


def test_arbitrary_rays_cover_every_depth1_case():
    so, _ = build_pair(recipe_axis_box())
    o4, d4 = RR.arbitrary_rays()
    assert o4.shape[0] == 1666 and o4.shape[0] % 256 != 0
    tri, t, face, _ = so.trace(o4, d4)
    _, kinds, surf = so.triangles()
    hit = tri != 0
    assert 100 < hit.sum() < o4.shape[0] - 100
    assert ((face & 2) != 0)[hit].any() and (kinds[tri[hit]] == 0).any() and (kinds[tri[hit]] == 1).any()
    assert not np.isfinite(t[hit]).all()  # the degenerate "hits" of rays parallel to a plane are in the set
    col = RR.depth1_color(tri, face, kinds, surf)
    assert len(np.unique(col, axis=0)) >= 4
    un = RR.unnormalised(d4)
    back = RR.vunit(un)
    ok = np.isfinite(d4).all(axis=1) & (np.abs(d4).sum(axis=1) > 0)
    assert np.allclose(back[ok], d4[ok], atol=1e-6) and not np.array_equal(back[ok], d4[ok])
