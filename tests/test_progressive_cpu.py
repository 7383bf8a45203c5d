"""Progressive rendering (rtmi_render_samples / rtmi_render_samples_device): the entry points exist and refuse bad arguments
before any HIP call, so these checks run without a GPU."""
import ctypes as C

import numpy as np
import pytest

RTMI_ERR_INVALID = 1


class Vp(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("orig", C.c_float * 3), ("cam", C.c_float * 3), ("vu", C.c_float * 3),
                ("vv", C.c_float * 3), ("maxdepth", C.c_uint32), ("samples_per_pixel", C.c_uint32)]


def _lib():
    from rust_raytrace_amd import _ffi
    return _ffi, _ffi.lib()


def test_progressive_entry_points_are_exported():
    ffi, L = _lib()
    for name in ("rtmi_render_samples", "rtmi_render_samples_device", "rth_caster_walk_samples", "rth_caster_walk_samples_device"):
        assert hasattr(L, name), name
        assert name in ffi.RTMI_SYMBOLS + ffi.RTH_SYMBOLS, name


def test_null_scene_is_refused_with_a_message():
    ffi, L = _lib()
    vp = Vp(8, 8, maxdepth=5, samples_per_pixel=4)
    acc = np.zeros((8, 8, 4), np.float32)
    st = ffi.Stats()
    st.rays = 123
    rc = L.rtmi_render_samples(None, C.byref(vp), 1, 0, 8, 0, 4, acc.ctypes.data_as(C.c_void_p), None, C.byref(st))
    assert rc == RTMI_ERR_INVALID
    assert L.rtmi_last_error(), "no message"
    assert st.rays == 0  # stats describe this call: cleared even when it is refused
    tile = ffi.Tile(0, 8, 8, 0)
    rc = L.rtmi_render_samples_device(None, C.byref(vp), 1, C.byref(tile), 0, 4, C.c_void_p(16), None, None, None)
    assert rc == RTMI_ERR_INVALID
    assert b"NULL" in L.rtmi_last_error()


@pytest.mark.parametrize("sample0,nsamples,spp", [(0, 0, 4), (3, 2, 4), (0xFFFFFFFF, 2, 4), (0, 1, 0)])
def test_sample_range_is_checked_before_the_scene_is_used(sample0, nsamples, spp):
    """A bad sample range is refused before the scene handle is touched (a dangling handle is never dereferenced here);
    the end of the range is computed in 64 bits, so sample0 + nsamples cannot wrap round."""
    ffi, L = _lib()
    vp = Vp(8, 8, maxdepth=5, samples_per_pixel=spp)
    acc = np.zeros((8, 8, 4), np.float32)
    bogus = C.c_void_p(0x10)  # never dereferenced: the checks come first
    rc = L.rtmi_render_samples(bogus, C.byref(vp), 1, 0, 8, sample0, nsamples, acc.ctypes.data_as(C.c_void_p), None, None)
    assert rc == RTMI_ERR_INVALID, L.rtmi_last_error()
    tile = ffi.Tile(0, 8, 8, 0)
    rc = L.rtmi_render_samples_device(bogus, C.byref(vp), 1, C.byref(tile), sample0, nsamples, C.c_void_p(16), None, None, None)
    assert rc == RTMI_ERR_INVALID, L.rtmi_last_error()


def test_null_or_aliased_accumulator_is_refused():
    ffi, L = _lib()
    vp = Vp(8, 8, maxdepth=5, samples_per_pixel=4)
    bogus = C.c_void_p(0x10)
    assert L.rtmi_render_samples(bogus, C.byref(vp), 1, 0, 8, 0, 4, None, None, None) == RTMI_ERR_INVALID
    assert b"accumulator" in L.rtmi_last_error()
    tile = ffi.Tile(0, 8, 8, 0)
    assert L.rtmi_render_samples_device(bogus, C.byref(vp), 1, C.byref(tile), 0, 4, None, None, None, None) == RTMI_ERR_INVALID
    buf = C.c_void_p(4096)
    assert L.rtmi_render_samples_device(bogus, C.byref(vp), 1, C.byref(tile), 0, 4, buf, buf, None, None) == RTMI_ERR_INVALID


def test_progressive_python_api_validates_its_arguments(canonical_pair):
    from rust_raytrace_amd import raytrace as R
    _, sp = canonical_pair
    vp = R.canonical_viewport(8, 8, 5, 4)
    c = R.HipRayCaster()
    with pytest.raises(ValueError):
        c.walk_rays_progressive(vp, sp, np.zeros((8, 8, 3), np.float32))
    with pytest.raises(ValueError):
        c.walk_rays_progressive(vp, sp, np.zeros((8, 8, 4), np.float32), pass_samples=0)
    with pytest.raises(ValueError):
        c.walk_samples(vp, sp, 0, 8, 0, 4, np.zeros((8, 8, 4), np.float64))
