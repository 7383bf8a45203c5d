"""Adaptive sampling (rtmi_render_adaptive / rtmi_render_adaptive_device): the entry points exist and refuse bad arguments
before any HIP call, so these checks run without a GPU.  The float32 replay of the stop rule that the GPU tests use is
checked here too."""
import ctypes as C

import numpy as np
import pytest

RTMI_ERR_INVALID = 1
NAN = float("nan")


class Vp(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("orig", C.c_float * 3), ("cam", C.c_float * 3), ("vu", C.c_float * 3),
                ("vv", C.c_float * 3), ("maxdepth", C.c_uint32), ("samples_per_pixel", C.c_uint32)]


def _lib():
    from rust_raytrace_amd import _ffi
    return _ffi, _ffi.lib()


def test_adaptive_entry_points_are_exported():
    ffi, L = _lib()
    for name in ("rtmi_render_adaptive", "rtmi_render_adaptive_device", "rth_caster_walk_adaptive", "rth_caster_walk_adaptive_device"):
        assert hasattr(L, name), name
        assert name in ffi.RTMI_SYMBOLS + ffi.RTH_SYMBOLS, name


def test_adaptive_struct_layout():
    ffi, _ = _lib()
    assert C.sizeof(ffi.Adaptive) == 32 and ffi.Adaptive.samples.offset == 24 and ffi.Adaptive.passes.offset == 16


# (spp, min_samples, pass_samples): every one is refused whatever the buffers are
BAD_SCHEDULES = [(4, 1, 2), (4, 0, 2), (4, 5, 2), (4, 2, 0), (1, 1, 1), (1, 2, 1), (0, 2, 1)]


@pytest.mark.parametrize("spp,m,p", BAD_SCHEDULES)
def test_bad_schedule_is_refused_before_the_scene_is_used(spp, m, p):
    """A dangling scene handle is never dereferenced: the checks come first.  Stats are cleared, the message is set."""
    ffi, L = _lib()
    vp = Vp(8, 8, maxdepth=5, samples_per_pixel=spp)
    out = np.zeros((8, 8, 4), np.float32)
    cnt = np.zeros((8, 8), np.uint32)
    bogus = C.c_void_p(0x10)
    ad = ffi.Adaptive(m, p, 0.0, NAN)
    st = ffi.Stats()
    st.rays = 123
    rc = L.rtmi_render_adaptive(bogus, C.byref(vp), 1, 0, 8, C.byref(ad), out.ctypes.data_as(C.c_void_p),
                                cnt.ctypes.data_as(C.c_void_p), C.byref(st))
    assert rc == RTMI_ERR_INVALID
    assert L.rtmi_last_error(), "no message"
    assert st.rays == 0
    tile = ffi.Tile(0, 8, 8, 0)
    st.rays = 123
    rc = L.rtmi_render_adaptive_device(bogus, C.byref(vp), 1, C.byref(tile), C.byref(ad), C.c_void_p(4096), C.c_void_p(8192),
                                       C.c_void_p(12288), None, None, C.byref(st))
    assert rc == RTMI_ERR_INVALID, L.rtmi_last_error()
    assert st.rays == 0


def test_null_scene_viewport_or_parameters_are_refused():
    ffi, L = _lib()
    vp = Vp(8, 8, maxdepth=5, samples_per_pixel=4)
    out = np.zeros((8, 8, 4), np.float32)
    cnt = np.zeros((8, 8), np.uint32)
    po, pc = out.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p)
    ad = ffi.Adaptive(2, 2, 0.0, NAN)
    bogus = C.c_void_p(0x10)
    assert L.rtmi_render_adaptive(None, C.byref(vp), 1, 0, 8, C.byref(ad), po, pc, None) == RTMI_ERR_INVALID
    assert b"NULL" in L.rtmi_last_error()
    assert L.rtmi_render_adaptive(bogus, None, 1, 0, 8, C.byref(ad), po, pc, None) == RTMI_ERR_INVALID
    assert L.rtmi_render_adaptive(bogus, C.byref(vp), 1, 0, 8, None, po, pc, None) == RTMI_ERR_INVALID
    assert b"rtmi_adaptive_t" in L.rtmi_last_error()
    tile = ffi.Tile(0, 8, 8, 0)
    b = [C.c_void_p(4096 * (i + 1)) for i in range(4)]
    assert L.rtmi_render_adaptive_device(bogus, C.byref(vp), 1, C.byref(tile), None, b[0], b[1], b[2], b[3], None, None) == RTMI_ERR_INVALID
    assert L.rtmi_render_adaptive_device(bogus, C.byref(vp), 1, None, C.byref(ad), b[0], b[1], b[2], b[3], None, None) == RTMI_ERR_INVALID
    assert b"tile" in L.rtmi_last_error()


@pytest.mark.parametrize("which", [0, 1, 2])
def test_null_device_buffer_is_refused(which):
    ffi, L = _lib()
    vp = Vp(8, 8, maxdepth=5, samples_per_pixel=4)
    ad = ffi.Adaptive(2, 2, 0.0, NAN)
    tile = ffi.Tile(0, 8, 8, 0)
    b = [C.c_void_p(4096 * (i + 1)) for i in range(4)]
    b[which] = None
    rc = L.rtmi_render_adaptive_device(C.c_void_p(0x10), C.byref(vp), 1, C.byref(tile), C.byref(ad), b[0], b[1], b[2], b[3], None, None)
    assert rc == RTMI_ERR_INVALID
    assert b"NULL buffer" in L.rtmi_last_error()


@pytest.mark.parametrize("i,j", [(0, 1), (0, 2), (1, 2), (0, 3), (1, 3), (2, 3)])
def test_aliased_buffers_are_refused(i, j):
    ffi, L = _lib()
    vp = Vp(8, 8, maxdepth=5, samples_per_pixel=4)
    ad = ffi.Adaptive(2, 2, 0.0, NAN)
    tile = ffi.Tile(0, 8, 8, 0)
    b = [C.c_void_p(4096 * (k + 1)) for k in range(4)]
    b[j] = b[i]
    rc = L.rtmi_render_adaptive_device(C.c_void_p(0x10), C.byref(vp), 1, C.byref(tile), C.byref(ad), b[0], b[1], b[2], b[3], None, None)
    assert rc == RTMI_ERR_INVALID
    assert b"alias" in L.rtmi_last_error()
    if j < 2:  # the host variant's two buffers: out and counts
        out = np.zeros((8, 8, 4), np.float32)
        p = out.ctypes.data_as(C.c_void_p)
        assert L.rtmi_render_adaptive(C.c_void_p(0x10), C.byref(vp), 1, 0, 8, C.byref(ad), p, p, None) == RTMI_ERR_INVALID
        assert L.rtmi_render_adaptive(C.c_void_p(0x10), C.byref(vp), 1, 0, 8, C.byref(ad), p, None, None) == RTMI_ERR_INVALID


def test_adaptive_python_api_validates_its_arguments(canonical_pair):
    from rust_raytrace_amd import raytrace as R
    _, sp = canonical_pair
    vp = R.canonical_viewport(8, 8, 5, 16)
    c = R.HipRayCaster()
    img = np.zeros((8, 8, 4), np.float32)
    with pytest.raises(ValueError):
        c.walk_rays_adaptive(vp, sp, np.zeros((8, 8, 3), np.float32))
    with pytest.raises(ValueError):
        c.walk_rays_adaptive(vp, sp, img, counts=np.zeros((8, 8), np.int64))
    for kw in ({"min_samples": 1}, {"min_samples": 17}, {"pass_samples": 0}):
        with pytest.raises(ValueError):
            c.walk_rays_adaptive(vp, sp, img, **kw)
    with pytest.raises(ValueError):
        c.walk_rays_adaptive(R.canonical_viewport(8, 8, 5, 1), sp, img, min_samples=1)
    with pytest.raises(ValueError):
        c.walk_adaptive_device(vp, sp, (0, 8, 8, 0), 4096, 8192, 12288, min_samples=1)
    assert 0 < c.ADAPTIVE_REL_TOL and 0 < c.ADAPTIVE_ABS_TOL


def test_replay_of_the_stop_rule():
    """The numpy replay the GPU tests compare against: NaN never stops, +inf stops everything at m, a constant pixel stops."""
    from test_adaptive import replay, stop_rule
    rng = np.random.default_rng(5)
    cols = rng.random((16, 3, 5, 4), dtype=np.float32)
    cols[..., 3] = 0
    cols[:, 0, 0] = np.float32(0.25)  # zero variance
    counts, acc, sq, passes, unconverged = replay(cols, 4, 4, 0.0, NAN)
    assert (counts == 16).all() and passes == 4 and unconverged == 15
    assert np.array_equal(acc, np.cumsum(cols, axis=0, dtype=np.float32)[-1])
    counts, _, _, passes, unconverged = replay(cols, 4, 4, 0.0, float("inf"))
    assert (counts == 4).all() and passes == 1 and unconverged == 0
    counts, _, _, _, unconverged = replay(cols, 4, 4, 0.0, 1e-6)
    assert counts[0, 0] == 4 and (counts[1:] == 16).all() and unconverged == 14
    # the schedule's edges: m == S is one pass whose failing pixels are all unconverged; a last pass clamped to S; S = m = 2
    counts, _, _, passes, unconverged = replay(cols[:6], 6, 4, 0.0, 1e-6)
    assert (counts == 6).all() and passes == 1 and unconverged == 14
    counts, _, _, passes, _ = replay(cols[:7], 2, 3, 0.0, 1e-6)
    assert passes == 3 and set(np.unique(counts).tolist()) == {2, 7}
    counts, _, _, passes, unconverged = replay(cols[:2], 2, 2, 0.0, NAN)
    assert (counts == 2).all() and passes == 1 and unconverged == 15
    counts, _, _, passes, _ = replay(cols[:9], 2, 1, 0.0, NAN)
    assert (counts == 9).all() and passes == 8
    s = np.array([np.nan, 0, 0, 0], np.float32)
    assert not stop_rule(s, s, 4, 0.0, np.inf)
