"""Batches of views (rtmi_render_views / rtmi_render_views_device): the entry points exist and refuse bad arguments before
any HIP call and before the scene is used, so these checks run without a GPU."""
import ctypes as C

import numpy as np
import pytest

RTMI_ERR_INVALID, RTMI_ERR_UNSUPPORTED = 1, 3
NAMES = ("rtmi_render_views", "rtmi_render_views_device", "rth_caster_walk_views", "rth_caster_walk_views_device")


class Vp(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("orig", C.c_float * 3), ("cam", C.c_float * 3), ("vu", C.c_float * 3),
                ("vv", C.c_float * 3), ("maxdepth", C.c_uint32), ("samples_per_pixel", C.c_uint32)]


def _lib():
    from rust_raytrace_amd import _ffi
    return _ffi, _ffi.lib()


def _views(n, w=8, h=6, depth=5, spp=4):
    vps = (Vp * n)()
    for k in range(n):
        vps[k] = Vp(w, h, (C.c_float * 3)(1.0 + k, 0.5, 0.0), (C.c_float * 3)(2.0, 0.0, -1.0), (C.c_float * 3)(0.0, 0.0, 1.0),
                    (C.c_float * 3)(0.0, 0.75, 0.0), depth, spp)
    return vps


BOGUS = C.c_void_p(0x10)  # a dangling scene handle: never dereferenced when a check fails


def _both(vps, seeds, n, tile=None, out_host=None, out_dev=C.c_void_p(4096), scene=BOGUS):
    """rc and message of the host and the device variant for the same batch; stats must come back cleared."""
    ffi, L = _lib()
    h = vps[0].height if n and vps is not None else 1
    w = vps[0].width if n and vps is not None else 1
    if out_host is None:
        out_host = np.zeros((max(n, 1), h, w, 4), np.float32)
    if tile is None:
        tile = ffi.Tile(0, max(n, 1) * h, max(n, 1) * h, 0)
    res = []
    st = ffi.Stats()
    st.rays = 123
    ph = out_host.ctypes.data_as(C.c_void_p) if isinstance(out_host, np.ndarray) else out_host
    rc = L.rtmi_render_views(scene, vps, seeds, n, ph, C.byref(st))
    res.append((rc, L.rtmi_last_error()))
    assert st.rays == 0
    st.rays = 123
    rc = L.rtmi_render_views_device(scene, vps, seeds, n, C.byref(tile), out_dev, None, C.byref(st))
    res.append((rc, L.rtmi_last_error()))
    assert st.rays == 0
    return res


def _seeds(n):
    return (C.c_uint64 * max(n, 1))(*range(1, max(n, 1) + 1))


def test_views_entry_points_are_exported_and_listed():
    ffi, L = _lib()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in ffi.RTMI_SYMBOLS + ffi.RTH_SYMBOLS, name


def test_zero_views_is_refused():
    for rc, msg in _both(_views(1), _seeds(1), 0):
        assert rc == RTMI_ERR_INVALID and b"nviews" in msg, msg


def test_null_arguments_are_refused():
    ffi, L = _lib()
    vps, seeds = _views(2), _seeds(2)
    for rc, msg in _both(None, seeds, 2):
        assert rc == RTMI_ERR_INVALID and b"NULL" in msg, msg
    for rc, msg in _both(vps, None, 2):
        assert rc == RTMI_ERR_INVALID and b"NULL" in msg, msg
    for rc, msg in _both(vps, seeds, 2, scene=None):
        assert rc == RTMI_ERR_INVALID and b"NULL" in msg and b"scene" in msg, msg
    for rc, msg in _both(vps, seeds, 2, out_host=C.c_void_p(0), out_dev=None):
        assert rc == RTMI_ERR_INVALID and b"output" in msg, msg
    assert L.rtmi_render_views_device(BOGUS, vps, seeds, 2, None, C.c_void_p(4096), None, None) == RTMI_ERR_INVALID
    assert b"tile" in L.rtmi_last_error()


@pytest.mark.parametrize("field,value", [("width", 9), ("height", 7), ("maxdepth", 4), ("samples_per_pixel", 2)])
def test_a_view_that_differs_in_a_shared_field_is_named(field, value):
    vps = _views(4)
    setattr(vps[2], field, value)
    setattr(vps[3], field, value)
    for rc, msg in _both(vps, _seeds(4), 4):
        assert rc == RTMI_ERR_INVALID, msg
        assert msg.startswith(b"view 2: " + field.encode()), msg  # the FIRST view that differs


def test_cameras_and_seeds_may_differ():
    """orig/cam/vu/vv and the seed are per view: such a batch passes every check.  With an empty tile nothing is rendered and
    the call returns RTMI_OK without touching the (bogus) scene."""
    ffi, L = _lib()
    vps = _views(3)
    for k in range(3):
        vps[k].orig[0] = 10.0 * k
        vps[k].vv[1] = 0.1 * (k + 1)
    tile = ffi.Tile(0, 0, 1, 0)
    assert L.rtmi_render_views_device(BOGUS, vps, _seeds(3), 3, C.byref(tile), C.c_void_p(4096), None, None) == 0


@pytest.mark.parametrize("vals,code,word", [
    (dict(samples_per_pixel=0), RTMI_ERR_INVALID, b"samples_per_pixel"),
    (dict(width=0), RTMI_ERR_INVALID, b"empty viewport"),
    (dict(height=0), RTMI_ERR_INVALID, b"empty viewport"),
    (dict(maxdepth=33), RTMI_ERR_UNSUPPORTED, b"maxdepth"),
])
def test_single_view_checks_apply_and_name_the_view(vals, code, word):
    vps = _views(3)
    for k in range(3):
        for f, v in vals.items():
            setattr(vps[k], f, v)
    for rc, msg in _both(vps, _seeds(3), 3):
        assert rc == code, msg
        assert msg.startswith(b"view 0: ") and word in msg, msg


@pytest.mark.parametrize("tile", [(0, 19, 19, 0), (15, 4, 4, 0), (0, 12, 4, 8), (0, 8, 4, 2), (0, 4, 0, 0)])
def test_a_tile_outside_the_stack_is_refused(tile):
    """3 views of 6 rows: the stack has 18 rows; stripes may cross views but must stay inside it and not overlap."""
    ffi, L = _lib()
    t = ffi.Tile(*tile)
    rc = L.rtmi_render_views_device(BOGUS, _views(3), _seeds(3), 3, C.byref(t), C.c_void_p(4096), None, None)
    assert rc == RTMI_ERR_INVALID
    assert b"stack of 3 views" in L.rtmi_last_error()


def test_more_than_2_32_stacked_pixels_is_unsupported():
    # 4096 x 4096 per view is fine alone (2^24 pixels); 256 of them are 2^32
    for rc, msg in _both(_views(256, w=4096, h=4096), _seeds(256), 256, out_host=C.c_void_p(4096)):
        assert rc == RTMI_ERR_UNSUPPORTED and b"2^32" in msg, msg


def test_python_api_validates_its_arguments(canonical_pair):
    from rust_raytrace_amd import raytrace as R
    _, sp = canonical_pair
    c = R.HipRayCaster()
    v = R.canonical_viewport(8, 6, 5, 4)
    with pytest.raises(ValueError):
        c.walk_rays_views([], sp)
    with pytest.raises(ValueError):
        c.walk_rays_views([v, R.canonical_viewport(8, 6, 5, 2)], sp)
    with pytest.raises(ValueError):
        c.walk_rays_views([v, R.canonical_viewport(8, 7, 5, 4)], sp)
    with pytest.raises(ValueError):
        c.walk_rays_views([v, v], sp, seeds=[1])
    for bad in (np.zeros((2, 6, 8, 3), np.float32), np.zeros((1, 6, 8, 4), np.float32), np.zeros((2, 6, 8, 4), np.float64),
                np.zeros((2, 8, 6, 4), np.float32)):
        with pytest.raises(ValueError):
            c.walk_rays_views([v, v], sp, bad)
    sp.debug_en = True
    try:
        with pytest.raises(ValueError):
            c.walk_rays_views([v, v], sp)
    finally:
        sp.debug_en = False
    with pytest.raises(ValueError):
        c.walk_views_device([], sp, (0, 6, 6, 0), 4096)
    with pytest.raises(ValueError):
        c.walk_views_device([v, R.canonical_viewport(8, 6, 4, 4)], sp, (0, 12, 12, 0), 4096)
