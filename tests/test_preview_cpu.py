"""The shaded preview (rtmi_render_preview / rtmi_render_preview_device): the entry points exist and are declared, the two
structures have the layout the header states, the calls refuse bad arguments before any HIP call and before the scene is used,
the Python methods validate their arguments, and the restatement the GPU tests compare with (tests/preview_ref.py, from the
oracle and the layers' restatements alone) gives what geometry says on hand-made scenes and the recorded counts on the
canonical one.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import ao_ref as AR
import features_ref as FR
import light_ref as LR
import occluded_ref as OR
import preview_ref as PR

RTMI_OK, RTMI_ERR_INVALID, RTMI_ERR_UNSUPPORTED = 0, 1, 3
NAMES = ("rtmi_render_preview", "rtmi_render_preview_device", "rth_caster_walk_preview", "rth_caster_walk_preview_device")
BOGUS = C.c_void_p(0x10)  # a dangling scene handle: never dereferenced when a check fails
FIELDS = ("color", "albedo", "normal", "ids", "ao", "shadow", "irradiance")
OUTS = {n: 0x1000000 * (k + 1) for k, n in enumerate(FIELDS)}  # never touched: every call fails or is empty
F32 = np.float32
INF = float("inf")
NAN = float("nan")


def _lib():
    from rust_raytrace_amd import _ffi
    return _ffi, _ffi.lib()


class Vp(C.Structure):
    """rtmi_viewport_t (include/rtmi.h)"""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("orig", C.c_float * 3), ("cam", C.c_float * 3), ("vu", C.c_float * 3),
                ("vv", C.c_float * 3), ("maxdepth", C.c_uint32), ("samples_per_pixel", C.c_uint32)]


def _vp(w=8, h=8, spp=4, maxdepth=5):
    v = Vp()
    v.width, v.height, v.maxdepth, v.samples_per_pixel = w, h, maxdepth, spp
    return v


def _both(scene=BOGUS, vp="dflt", tile=(0, 8, 8, 0), sample0=0, nsamples=4, preview="dflt", out="dflt", nlights=1, edit=None, device_only=False,
          **outs):
    """(rc, message, stats.rays) of the device and of the host variant for the same arguments.  edit(p): changes the
    rtmi_preview_t (defaults with `nlights` lights); outs: pointer overrides of the outputs (0 = NULL)"""
    ffi, L = _lib()
    v = _vp() if vp == "dflt" else vp
    p = o = None
    if preview == "dflt":
        p = ffi.Preview()
        L.rtmi_preview_defaults(C.byref(p))
        p.nlights = nlights
        if edit:
            edit(p)
    if out == "dflt":
        ptr = dict(OUTS, **outs)
        if preview == "dflt" and p.nlights == 0 and "shadow" not in outs and "irradiance" not in outs:
            ptr["shadow"] = ptr["irradiance"] = 0
        if preview == "dflt" and p.ao.rays == 0 and "ao" not in outs:
            ptr["ao"] = 0
        o = ffi.PreviewOut(*[ptr[n] or None for n in FIELDS])
    res = []
    for dev in ((True, False) if tile is not None and not device_only else (True,)):  # the host variant takes rows, not a tile
        st = ffi.Stats()
        st.rays = 123
        vp_p, p_p, o_p = (C.byref(x) if x is not None else None for x in (v, p, o))
        if dev:
            t = ffi.Tile(*tile) if tile is not None else None
            rc = L.rtmi_render_preview_device(scene, vp_p, 7, C.byref(t) if t is not None else None, sample0, nsamples, p_p, o_p, None,
                                              C.byref(st))
        else:
            rc = L.rtmi_render_preview(scene, vp_p, 7, tile[0], tile[1], sample0, nsamples, p_p, o_p, C.byref(st))
        res.append((rc, L.rtmi_last_error(), st.rays))
    return res


def test_entry_points_are_exported_declared_and_listed():
    ffi, L = _lib()
    text = open(os.path.join(ROOT, "include", "rtmi.h")).read() + open(os.path.join(ROOT, "include", "rtmi_host.h")).read()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in ffi.RTMI_SYMBOLS + ffi.RTH_SYMBOLS, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
    assert hasattr(L, "rtmi_preview_defaults") and "rtmi_preview_defaults" in ffi.RTMI_SYMBOLS
    assert re.search(r"\bvoid\s+rtmi_preview_defaults\s*\(", text)
    assert re.search(r"RTMI_PREVIEW_MAX_LIGHTS\s*=\s*4", text) and ffi.PREVIEW_MAX_LIGHTS == 4


def test_structure_layouts():
    ffi, _ = _lib()
    P, O = ffi.Preview, ffi.PreviewOut
    assert C.sizeof(P) == 196
    assert (P.ambient.offset, P.nlights.offset, P.flags.offset, P.ao.offset, P.lights.offset, P.light_color.offset) == (0, 12, 16, 20, 36, 148)
    assert C.sizeof(O) == 7 * C.sizeof(C.c_void_p)
    assert [getattr(O, n).offset for n in FIELDS] == [k * C.sizeof(C.c_void_p) for k in range(7)]


def test_defaults():
    ffi, L = _lib()
    p = ffi.Preview()
    C.memset(C.byref(p), 0x5A, C.sizeof(p))
    L.rtmi_preview_defaults(C.byref(p))
    assert [F32(x) for x in p.ambient] == [F32(0.3)] * 3 and (p.nlights, p.flags) == (0, 0)
    a, li = ffi.Ao(), ffi.Light()
    L.rtmi_ao_defaults(C.byref(a))
    L.rtmi_light_defaults(C.byref(li))
    assert bytes(p.ao) == bytes(a)
    for l in range(4):
        assert bytes(p.lights[l]) == bytes(li) and tuple(p.light_color[l]) == (1.0, 1.0, 1.0)
    L.rtmi_preview_defaults(None)  # tolerated


def test_null_arguments_are_refused_and_stats_cleared():
    for kw in (dict(scene=None), dict(vp=None), dict(tile=None), dict(preview=None), dict(out=None), {n: 0 for n in FIELDS}):
        for rc, msg, rays in _both(**kw):
            assert rc == RTMI_ERR_INVALID and b"NULL" in msg and rays == 0, (kw, msg)


def test_overlapping_outputs_are_refused():
    npix = 64
    for outs in (dict(albedo=OUTS["color"]), dict(ids=OUTS["ao"]), dict(normal=OUTS["color"] + 16 * npix - 4), dict(ao=OUTS["ids"] - 4 * npix + 4),
                 dict(irradiance=OUTS["shadow"] + 4 * npix * 2 - 4), dict(color=OUTS["shadow"] - 16 * npix + 4)):
        for rc, msg, rays in _both(nlights=2, **outs):
            assert rc == RTMI_ERR_INVALID and b"overlap" in msg and rays == 0, (outs, msg)
    # touching ranges are fine: the call gets as far as the sample range check
    for outs in (dict(normal=OUTS["color"] + 16 * npix), dict(irradiance=OUTS["shadow"] + 4 * npix * 2), dict(ao=OUTS["ids"] - 4 * npix)):
        for rc, msg, _ in _both(nlights=2, nsamples=5, **outs):
            assert rc == RTMI_ERR_INVALID and b"sample0 + nsamples" in msg, (outs, msg)


def _set(path, value):
    def edit(p):
        obj = p
        for name in path[:-1]:
            obj = obj[name] if isinstance(name, int) else getattr(obj, name)
        if isinstance(path[-1], int):
            obj[path[-1]] = value
        else:
            setattr(obj, path[-1], value)
    return edit


BAD = [(("nlights",), 5, b"nlights"), (("nlights",), 1 << 31, b"nlights"), (("flags",), 1, b"flags"), (("flags",), 1 << 31, b"flags"),
       (("ambient", 0), NAN, b"ambient"), (("ambient", 2), INF, b"ambient"), (("ambient", 1), -INF, b"ambient"),
       (("light_color", 0, 1), NAN, b"light 0"), (("light_color", 1, 2), INF, b"light 1"),
       (("ao", "rays"), 257, b"ao.rays"), (("ao", "flags"), 1, b"ao.flags"), (("ao", "radius"), NAN, b"radius"), (("ao", "radius"), -1.0, b"radius"),
       (("ao", "bias"), NAN, b"bias"), (("ao", "bias"), INF, b"bias"),
       (("lights", 0, "rays"), 0, b"light 0: rays"), (("lights", 1, "rays"), 257, b"light 1: rays"), (("lights", 1, "flags"), 2, b"light 1: unknown flags"),
       (("lights", 0, "len2"), NAN, b"light 0: len2"), (("lights", 1, "len2"), -1.0, b"light 1: len2"), (("lights", 1, "len2"), INF, b"light 1: len2"),
       (("lights", 0, "bias"), NAN, b"light 0: bias"), (("lights", 1, "bias"), -INF, b"light 1: bias"),
       (("lights", 1, "orig", 0), NAN, b"light 1: orig"), (("lights", 0, "orig", 2), INF, b"light 0: orig")]


@pytest.mark.parametrize("path,value,word", BAD, ids=[".".join(str(x) for x in b[0]) + "=" + str(b[1]) for b in BAD])
def test_bad_parameters_are_refused(path, value, word):
    for rc, msg, rays in _both(nlights=2, edit=_set(path, value)):
        assert rc == RTMI_ERR_INVALID and word in msg and rays == 0, msg


def test_unused_lights_are_ignored():
    """Entries >= nlights are not checked: garbage in lights[1] and its colour with nlights = 1 reaches the next check"""
    def edit(p):
        p.lights[1].rays = 0
        p.lights[1].len2 = NAN
        p.light_color[1][0] = NAN
        p.lights[3].flags = 99
    for rc, msg, _ in _both(nlights=1, nsamples=5, edit=edit):
        assert rc == RTMI_ERR_INVALID and b"sample0 + nsamples" in msg, msg


def test_outputs_that_need_a_layer_that_is_off():
    for rc, msg, rays in _both(edit=_set(("ao", "rays"), 0), ao=OUTS["ao"]):
        assert rc == RTMI_ERR_INVALID and b"ao" in msg and rays == 0, msg
    for outs in (dict(shadow=OUTS["shadow"], irradiance=0), dict(irradiance=OUTS["irradiance"], shadow=0)):
        for rc, msg, rays in _both(nlights=0, **outs):
            assert rc == RTMI_ERR_INVALID and b"nlights" in msg and rays == 0, msg


def test_valid_edge_parameters_reach_the_next_check():
    """ao.rays 0 (without its plane), nlights 0 and 4, the unbounded flag, len2 0, a zero radius, each output alone: with them
    the call gets as far as the sample range check"""
    cases = [dict(edit=_set(("ao", "rays"), 0)), dict(nlights=0), dict(nlights=4), dict(nlights=0, edit=_set(("ao", "rays"), 0)),
             dict(edit=_set(("lights", 0, "flags"), 1)), dict(edit=_set(("lights", 0, "len2"), 0.0)), dict(edit=_set(("lights", 0, "len2"), 1e30)),
             dict(edit=_set(("ao", "radius"), 0.0)), dict(edit=_set(("ao", "radius"), INF)), dict(edit=_set(("ao", "rays"), 256)),
             dict(edit=_set(("lights", 0, "rays"), 256)), dict(edit=_set(("ambient", 0), -2.0)), dict(edit=_set(("light_color", 0, 0), -1.0))]
    cases += [dict({m: 0 for m in FIELDS if m != n}) for n in FIELDS]
    for kw in cases:
        for rc, msg, _ in _both(nsamples=5, **kw):
            assert rc == RTMI_ERR_INVALID and b"sample0 + nsamples" in msg, (kw, msg)


def test_sample_range_viewport_and_tile_checks():
    for kw, word in ((dict(nsamples=0), b"nsamples"), (dict(sample0=3, nsamples=2), b"sample0 + nsamples"),
                     (dict(sample0=0xFFFFFFFF, nsamples=2), b"sample0 + nsamples"), (dict(vp=_vp(spp=0)), b"samples_per_pixel")):
        for rc, msg, rays in _both(**kw):
            assert rc == RTMI_ERR_INVALID and word in msg and rays == 0, (kw, msg)
    for kw, word in ((dict(vp=_vp(w=0)), b"empty viewport"), (dict(tile=(4, 8, 8, 0)), b"outside"), (dict(tile=(0, 9, 9, 0)), b"outside")):
        for rc, msg, rays in _both(**kw):
            assert rc == RTMI_ERR_INVALID and word in msg and rays == 0, (kw, msg)
    for tile, word in (((0, 4, 0, 0), b"stripe_rows"), ((0, 8, 2, 1), b"overlap"), ((0, 8, 2, 4), b"outside")):
        rc, msg, rays = _both(tile=tile, device_only=True)[0]
        assert rc == RTMI_ERR_INVALID and word in msg and rays == 0, tile
    # vp->maxdepth is not consulted: a depth the renderer refuses is fine here (the empty tile is reached)
    for rc, _, rays in _both(vp=_vp(maxdepth=1000), tile=(0, 0, 1, 0)):
        assert rc == RTMI_OK and rays == 0


def test_an_empty_tile_is_ok_and_touches_nothing():
    for tile in ((0, 0, 1, 0), (100, 0, 0, 0)):
        for rc, _, rays in _both(tile=tile):
            assert rc == RTMI_OK and rays == 0


def test_sample_times_rays_of_2_pow_24_is_unsupported():
    big = _vp(spp=1 << 20)
    for kw in (dict(nsamples=1 << 16, edit=_set(("ao", "rays"), 256)), dict(nsamples=1 << 20, edit=_set(("lights", 0, "rays"), 16)),
               dict(nsamples=1 << 20, nlights=2, edit=_set(("lights", 1, "rays"), 17)),
               dict(nsamples=1 << 16, edit=_set(("ao", "rays"), 256), tile=(0, 0, 1, 0))):  # refused before the empty tile is looked at
        for rc, msg, rays in _both(vp=big, **kw):
            assert rc == RTMI_ERR_UNSUPPORTED and b"2^24" in msg and rays == 0, (kw, msg)
    # one below: valid, the empty tile is reached
    for rc, _, _ in _both(vp=big, nsamples=(1 << 16) - 1, edit=_set(("ao", "rays"), 256), tile=(0, 0, 1, 0)):
        assert rc == RTMI_OK


def test_python_api_validates_its_arguments(canonical_pair):
    from rust_raytrace_amd import raytrace as R
    _, sp = canonical_pair
    c = R.HipRayCaster()
    vp = R.canonical_viewport(8, 8, 5, 4)
    li = dict(orig=(-3, 6, 1), len2=0.5)
    img = np.zeros((8, 8, 4), np.float32)
    for kw in (dict(ambient=(0.1, 0.2)), dict(ambient=(0.1, NAN, 0.2)), dict(ao=dict(rays=257)), dict(ao=dict(radius=-1.0)), dict(ao=dict(bias=INF)),
               dict(ao=dict(depth=3)), dict(lights=[li] * 5), dict(lights=[dict(li, rays=0)]), dict(lights=[dict(li, len2=NAN)]),
               dict(lights=[dict(li, color=(1.0, INF, 0.0))]), dict(lights=[dict(li, color=(1.0, 0.0))]), dict(lights=[dict(li, power=2)]),
               dict(nsamples=0), dict(sample0=3, nsamples=2), dict(sample0=-1), dict(color=False), dict(color=None, albedo=None),
               dict(ao=False, ao_out=True), dict(ao=dict(rays=0), ao_out=True), dict(shadow=True), dict(irradiance=True),
               dict(color=np.zeros((8, 8, 4), np.float64)), dict(color=np.zeros((8, 9, 4), np.float32)), dict(ids=np.zeros((8, 8), np.int32)),
               dict(lights=[li], shadow=np.zeros((8, 8), np.float32)), dict(color=img, albedo=img),
               dict(color=np.zeros((8, 8, 8), np.float32)[:, :, ::2])):
        with pytest.raises(ValueError):
            c.walk_rays_preview(vp, sp, **kw)
    big = R.canonical_viewport(8, 8, 5, 1 << 20)
    with pytest.raises(ValueError):
        c.walk_rays_preview(big, sp, ao=dict(rays=256), nsamples=1 << 16)
    with pytest.raises(ValueError):
        c.walk_rays_preview(big, sp, lights=[dict(li, rays=256)], nsamples=1 << 16)
    for bad in (None, img):  # nothing at all, or not a device tensor
        with pytest.raises(ValueError):
            c.walk_rays_preview_device(vp, sp, color=bad)
    p = R.HipRayCaster.preview_params(ambient=(0.25, 0.25, 0.5), ao=dict(rays=3, radius=2.0), lights=[dict(li, rays=7, unbounded=True, color=(1, 0.5, 0.25)), li])
    assert tuple(p.ambient) == (0.25, 0.25, 0.5) and (p.nlights, p.flags, p.ao.rays, p.ao.radius) == (2, 0, 3, 2.0)
    assert tuple(p.lights[0].orig) == (-3.0, 6.0, 1.0) and (p.lights[0].rays, p.lights[0].flags) == (7, 1) and tuple(p.light_color[0]) == (1.0, 0.5, 0.25)
    assert (p.lights[1].rays, p.lights[1].flags) == (4, 0) and tuple(p.light_color[1]) == (1.0, 1.0, 1.0)
    assert R.HipRayCaster.preview_params(ao=False).ao.rays == 0 and R.HipRayCaster.preview_params().ao.rays == 4


# ---------------------------------------------------------------- the restatement, on the oracle alone
def _orc():
    from oracle import orc
    return orc


def _down_view(orc, w, h, y=5.0):
    """A camera y above the plane y = 0 looking straight down at it"""
    return orc.create_viewport(w, h, (1.0, 1.0), [0.0, y, 0.0], orc.unit([0.0, -1.0, 0.0]), 90.0, 0.0)


GREY = (200, 200, 200)


def _floor_scene(orc, ceiling, half=False):
    """A grey floor at y = 0 (half: only where x <= 0, edge on the camera's axis), optionally a ceiling 2 above it"""
    s = orc.Scene(with_dummy=True)
    grey = orc.Surface(orc.MATTE, orc.make_color(*GREY), 0.5)
    if half:
        s.add_triangle(np.array([[0, 0, -60], [0, 0, 60], [-90, 0, 0]], F32), grey, 0.0)
    else:
        s.add_triangle(np.array([[-60, 0, -60], [60, 0, -60], [0, 0, 90]], F32), grey, 0.0)
    if ceiling:  # far larger than the floor seen from any point of it, 2 above it
        s.add_triangle(np.array([[-4000, 2, -4000], [4000, 2, -4000], [0, 2, 6000]], F32), grey, 0.0)
    s.populate_triangle_numbers()
    s.build_trivial_bounding_box([0.0, 0.0, 0.0], 8000.0)
    return s


def _fold(x):
    """(npix, n) float32 -> the ordered sum over axis 1 from 0.f, one rounding per term"""
    acc = np.zeros(x.shape[0], F32)
    for k in range(x.shape[1]):
        acc = (acc + x[:, k]).astype(F32)
    return acc


def test_an_open_floor_under_a_light():
    """Nothing occludes: f = 1 and per sample e = a * (ambient + colour * mean c)"""
    orc = _orc()
    so = _floor_scene(orc, ceiling=False)
    amb, col = (0.25, 0.5, 0.125), (1.0, 0.75, 0.5)
    li = dict(orig=(-0.5, 10.0, -0.5), len2=1.0, rays=4, color=col)
    r = PR.preview_ref(orc, so, 12, 10, _down_view(orc, 12, 10), 2, 5, amb, None, [li])
    assert r.nhit == r.npaths == 240 and r.ao_occ == 0 and r.nculled == [0] and r.nocc == [0] and (r.f == 1.0).all()
    assert r.rays == 240 + 960 + 960
    one = LR.light_ref(orc, so, 12, 10, _down_view(orc, 12, 10), 2, 5, 4, li["orig"], 1.0)
    g = (_fold(one.c.reshape(240, 4)) * F32(0.25)).astype(F32)  # per sample: its four c in k order
    a = (np.array(GREY, F32) / F32(255.0)).astype(F32)
    assert np.array_equal(r.a[..., :3].reshape(-1, 3), np.broadcast_to(a, (240, 3)))
    for ch in range(3):
        L = (F32(amb[ch]) * F32(1.0) + (F32(col[ch]) * g).astype(F32)).astype(F32)
        e = (a[ch] * L).astype(F32).reshape(120, 2)
        want = (_fold(e) * F32(0.5)).astype(F32)
        assert np.array_equal(r.color[..., ch].reshape(-1).view(np.uint32), want.view(np.uint32)), ch
    assert (r.color[..., 3] == 0).all() and (r.color[..., :3] > 0).all()


def test_a_floor_under_a_ceiling_keeps_no_term():
    """Enclosed: every AO ray and every shadow ray is occluded, f = 0 and g = 0, the colour is a * (ambient * 0) = 0"""
    orc = _orc()
    so = _floor_scene(orc, ceiling=True)
    li = dict(orig=(-0.5, 10.0, -0.5), len2=1.0, rays=4)
    r = PR.preview_ref(orc, so, 12, 10, _down_view(orc, 12, 10, 1.0), 2, 5, (0.5, 0.5, 0.5), None, [li])  # the camera between the two
    assert r.nhit == 240 and r.ao_occ == 960 and r.nocc == [960] and (r.f == 0.0).all() and (r.g == 0.0).all()
    assert np.array_equal(r.color, np.zeros((10, 12, 4), F32)) and np.array_equal(r.ao, np.zeros((10, 12), F32))
    # a limited radius lets the ambient term through alone: e = a * ambient
    r2 = PR.preview_ref(orc, so, 12, 10, _down_view(orc, 12, 10, 1.0), 2, 5, (0.5, 0.5, 0.5), dict(radius=1.0), [li])
    a = (np.array(GREY, F32) / F32(255.0)).astype(F32)
    e = (a * F32(0.5)).astype(F32)
    assert r2.ao_occ == 0 and r2.nocc == [960]
    assert np.array_equal(r2.color[..., :3], np.broadcast_to(((e + e).astype(F32) * F32(0.5)).astype(F32), (10, 12, 3)))


def test_the_sky_half_of_a_half_covered_pixel_stays_sky():
    """The floor ends on the camera's axis, which runs through the middle pixels of a 13 x 11 frame.  With 8 jittered samples a
    middle pixel has samples on both sides: it is the mean of lit samples and of samples that are exactly the sky, where the
    product of the per-pixel means lights the sky half and dims it by the ambient factor."""
    orc = _orc()
    so = _floor_scene(orc, ceiling=False, half=True)
    amb = (0.5, 0.5, 0.5)
    li = dict(orig=(-0.5, 10.0, -0.5), len2=1.0, rays=4)
    r = PR.preview_ref(orc, so, 13, 11, _down_view(orc, 13, 11), 8, 5, amb, None, [li])
    tri = r.tri.reshape(143, 8)
    hits = (tri != 0).sum(axis=1)
    part = (hits > 0) & (hits < 8)
    assert part.sum() >= 10 and (hits == 0).sum() >= 50 and (hits == 8).sum() >= 50
    miss = tri == 0
    assert np.array_equal(r.e[miss], np.broadcast_to(FR.SKY, (int(miss.sum()), 3)))  # every sky sample is exactly the sky
    col = r.color[..., :3].reshape(143, 3)
    sky8 = (_fold(np.broadcast_to(FR.SKY[:, None], (3, 8))) * F32(0.125)).astype(F32)  # the sky's own mean over 8 samples
    assert np.array_equal(col[hits == 0], np.broadcast_to(sky8, (int((hits == 0).sum()), 3))) and np.allclose(sky8, FR.SKY, rtol=1e-6)
    # a partly covered pixel: the ordered mean of its lit samples and of the sky, sample by sample
    lit = r.e[hits == 8].reshape(-1, 3)
    assert (lit > 0).all() and (lit != FR.SKY).all()
    for p in np.nonzero(part)[0][:3]:
        acc = np.zeros(3, F32)
        for s_ in range(8):
            acc = (acc + (FR.SKY if miss[p, s_] else r.e[p, s_])).astype(F32)
        assert np.array_equal(col[p].view(np.uint32), (acc * F32(0.125)).astype(F32).view(np.uint32))
    prod = (r.albedo[..., :3] * ((np.asarray(amb, F32) * r.ao[..., None]).astype(F32) + r.irradiance[0][..., None])).astype(F32).reshape(143, 3)
    assert (prod[part] != col[part]).any(axis=1).all()  # the product of the means is wrong in every partly covered pixel
    assert (prod[hits == 0] != col[hits == 0]).any(axis=1).all()  # ... and dims the sky itself


@pytest.fixture(scope="module")
def canonical_32(canonical_pair):
    orc = _orc()
    so, _ = canonical_pair
    vp12 = orc.canonical_viewport(32, 32)
    A = dict(orig=OR.LIGHT, len2=0.5, rays=4, color=(1.0, 0.9, 0.8))
    B = dict(orig=(2.0, 0.0, -3.0), len2=0.0, rays=4, color=(0.2, 0.3, 0.5))
    amb = (0.25, 0.25, 0.3)
    return so, vp12, amb, A, B, PR.preview_ref(orc, so, 32, 32, vp12, 2, 1, amb, None, [A, B])


def test_canonical_counts(canonical_32):
    """32 x 32, S = 2, seed 1, Ka = 4, light A = (-3, 6, 1) / 0.5 / K 4, light B = a point light at (2, 0, -3) / K 4"""
    so, vp12, amb, A, B, r = canonical_32
    assert OR.LIGHT == (-3.0, 6.0, 1.0)
    assert r.npaths == 2048 and r.nhit == 417
    assert r.n_ao == 1668 and r.ao_occ == 195
    assert (r.nculled[0], r.nlive[0], r.nocc[0]) == (385, 1283, 224)
    assert (r.nculled[1], r.nlive[1], r.nocc[1]) == (0, 1668, 0)
    hits = (r.tri.reshape(1024, 2) != 0).sum(axis=1)
    assert (int((hits == 0).sum()), int((hits == 1).sum()), int((hits == 2).sum())) == (797, 37, 190)
    assert r.nedge == 17
    assert np.isfinite(r.color).all() and (r.color[..., 3] == 0).all()
    assert r.rays == 2048 + 1668 + 1283 + 1668 == 6667
    # the product of the per-pixel means is not the preview
    prod = (r.albedo[..., :3] * ((np.asarray(amb, F32) * r.ao[..., None]).astype(F32) + (np.asarray(A["color"], F32) * r.irradiance[0][..., None]).astype(F32)
                                 + (np.asarray(B["color"], F32) * r.irradiance[1][..., None]).astype(F32))).astype(F32)
    differ = (prod != r.color[..., :3]).any(axis=2).reshape(-1)
    print(f"product of means differs in {int(differ[hits > 0].sum())} of {int((hits > 0).sum())} covered pixels and {int(differ[hits == 0].sum())} sky pixels")
    assert differ[hits > 0].sum() >= 1 and differ[hits == 0].all()
    # an edge face's sample is black, a sky sample is the sky
    edge = ((r.face & 2) != 0) & (r.tri != 0)
    assert (r.e.reshape(-1, 3)[edge] == 0).all() and np.array_equal(r.e.reshape(-1, 3)[r.tri == 0], np.broadcast_to(FR.SKY, (2048 - 417, 3)))


def test_the_layers_are_the_layers_restatements(canonical_32):
    so, vp12, amb, A, B, r = canonical_32
    orc = _orc()
    alb, nrm, ids, _ = FR.features_ref(orc, so, 32, 32, vp12, 2, 1)
    for got, want in ((r.albedo, alb), (r.normal, nrm)):
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(r.ids, ids)
    assert np.array_equal(r.ao.view(np.uint32), AR.ao_ref(orc, so, 32, 32, vp12, 2, 1, 4).ao.view(np.uint32))
    for l, li in enumerate((A, B)):
        one = LR.light_ref(orc, so, 32, 32, vp12, 2, 1, 4, li["orig"], li["len2"])
        assert np.array_equal(r.shadow[l].view(np.uint32), one.shadow.view(np.uint32))
        assert np.array_equal(r.irradiance[l].view(np.uint32), one.irradiance.view(np.uint32))
        assert (r.nlive[l], r.nculled[l]) == (one.nlive, one.nculled)


def test_sample_ranges_and_tiles_select_the_same_samples(canonical_32):
    so, vp12, amb, A, B, r = canonical_32
    orc = _orc()
    s1 = PR.preview_ref(orc, so, 32, 32, vp12, 2, 1, amb, None, [A, B], sample0=1, nsamples=1)
    assert np.array_equal(s1.e[:, 0].view(np.uint32), r.e[:, 1].view(np.uint32))
    tile = (1, 12, 3, 8)
    t = PR.preview_ref(orc, so, 32, 32, vp12, 2, 1, amb, None, [A, B], tile=tile)
    assert np.array_equal(t.color.view(np.uint32), r.color[FR.tile_rows(tile)].view(np.uint32))
    off = PR.preview_ref(orc, so, 32, 32, vp12, 2, 1, amb, False, [])
    assert off.rays == 2048 and off.ao is None and off.shadow is None
    hit = off.tri != 0  # neither AO nor lights: a flat preview, every sample that hit is a * ambient
    assert (off.f == 1.0).all() and np.array_equal(off.e.reshape(-1, 3)[hit], (off.a.reshape(-1, 4)[hit, :3] * np.asarray(amb, F32)).astype(F32))
