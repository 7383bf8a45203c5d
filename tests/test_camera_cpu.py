"""The built-in camera models (rtmi_render_camera / rtmi_render_camera_device): the restatement the GPU tests compare with
(tests/camera_ref.py, from the oracle alone) is pinned -- its pinhole rays ARE orc.primary_rays, its path tracer over them IS
Scene.render -- the lens samples and the thin-lens geometry are what the header says (checked in float64), the orthographic rays
are parallel, and the entry points exist, are declared and refuse bad arguments before any HIP call and before the scene is
used.  No GPU needed."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import camera_ref as CR
from rays_ref import second_viewport

RTMI_OK, RTMI_ERR_INVALID, RTMI_ERR_UNSUPPORTED = 0, 1, 3
NAMES = ("rtmi_render_camera", "rtmi_render_camera_device", "rth_caster_walk_camera", "rth_caster_walk_camera_device")
F32 = np.float32


def _orc():
    from oracle import orc
    return orc


# ---------------------------------------------------------------- the restatement, on the oracle alone
@pytest.mark.parametrize("spp", [1, 4])
def test_pinhole_rays_are_the_oracles_primary_rays(spp):
    orc = _orc()
    w, h = 33, 17
    vp12 = orc.canonical_viewport(w, h)
    cr = CR.camera_rays(orc, vp12, w, h, spp, 7, CR.cam(CR.PINHOLE))
    o4, d4 = orc.primary_rays(w, h, vp12, spp, 7)
    assert np.array_equal(cr.o4.view(np.uint32), o4.view(np.uint32))
    assert np.array_equal(cr.d4.view(np.uint32), d4.view(np.uint32))
    assert np.array_equal(cr.keys[:, 0], np.repeat(np.arange(w * h, dtype=np.uint32), spp))
    assert np.array_equal(cr.keys[:, 1], np.tile(np.arange(spp, dtype=np.uint32), w * h))
    # a pass and a row subset select the same rays
    if spp == 4:
        sub = CR.camera_rays(orc, vp12, w, h, spp, 7, CR.cam(CR.PINHOLE), 1, 3, rows=[2, 9])
        want = o4.reshape(h, w, spp, 4)[[2, 9]][:, :, 1:4].reshape(-1, 4)
        assert np.array_equal(sub.o4.view(np.uint32), np.ascontiguousarray(want).view(np.uint32)) and (sub.npix, sub.n) == (2 * w, 3)


def test_path_trace_over_the_pinhole_rays_is_the_oracles_render(canonical_pair):
    orc = _orc()
    so, _ = canonical_pair
    w = h = 16
    vp12 = orc.canonical_viewport(w, h)
    r = CR.render(orc, so, vp12, w, h, 2, 1, CR.cam(CR.PINHOLE), 5)
    ref, cn = so.render(w, h, vp12, 5, 2, seed=1, threads=4)
    assert np.array_equal(r.image.view(np.uint32), ref.view(np.uint32))
    assert r.rays == cn["rays"] and len(r.passes) == 5 and r.passes[0] == w * h * 2 and r.passes[2] > 0


# ---------------------------------------------------------------- lens samples
class _Recorder:
    """orc with every rng_block call recorded"""

    def __init__(self, orc):
        self.orc, self.calls = orc, []

    def rng_block(self, seed, pixel, sample, blk):
        self.calls.append((seed, pixel, sample, blk))
        return self.orc.rng_block(seed, pixel, sample, blk)


def test_lens_samples():
    orc = _orc()
    n = 4096
    pixel, sample = np.arange(n, dtype=np.int64) * 7 + 3, np.arange(n, dtype=np.int64) % 5
    rec = _Recorder(orc)
    x, y, taken = CR.lens_samples(rec, 11, pixel, sample)
    assert x.dtype == np.float32 and y.dtype == np.float32
    # all inside the unit disc (in float64: the float32 test x*x + y*y <= 1 can round up to 1 from at most 1 + 2^-23)
    assert (x.astype(np.float64) ** 2 + y.astype(np.float64) ** 2 <= 1.0 + 2.0 ** -22).all()
    # the fallbacks: Binomial(n, p), p = (1 - pi/4)^4; both tails together below 1e-6
    p = CR.P_FALLBACK
    assert abs(p - 0.0021) < 5e-5
    pmf = [math.exp(math.lgamma(n + 1) - math.lgamma(k + 1) - math.lgamma(n - k + 1) + k * math.log(p) + (n - k) * math.log1p(-p))
           for k in range(n + 1)]
    lo = 0
    while sum(pmf[:lo + 1]) < 5e-7:
        lo += 1
    hi = n
    while sum(pmf[hi:]) < 5e-7:
        hi -= 1
    nfall = int((taken == 4).sum())
    print(f"fallback samples: {nfall} of {n}, expected {p * n:.2f}, accepted [{lo}, {hi}]")
    assert lo <= nfall <= hi
    assert (x[taken == 4] == 0).all() and (y[taken == 4] == 0).all()
    # the candidates are taken in order, about pi/4 of the keys take the first one, and every candidate index occurs
    assert abs((taken == 0).mean() - math.pi / 4) < 0.03 and set(np.unique(taken)) == {0, 1, 2, 3, 4}
    # every draw comes from the stated blocks ...
    assert {c[3] for c in rec.calls} == {0x40000000, 0x40000001}
    assert {(c[0], c[1], c[2]) for c in rec.calls} == {(11, int(a), int(b)) for a, b in zip(pixel, sample)}
    # ... and words: the sample of key i is candidate taken[i] = 2 k + j, words 2 j and 2 j + 1 of block 0x40000000 | k
    for i in list(range(64)) + list(np.nonzero(taken >= 2)[0][:32]):
        if taken[i] == 4:
            continue
        k, j = divmod(int(taken[i]), 2)
        wds = orc.rng_block(11, int(pixel[i]), int(sample[i]), 0x40000000 | k)
        u = [F32(orc.u32_to_unit_f32(int(wds[2 * j + c]))) for c in (0, 1)]
        assert x[i] == F32(F32(2.0) * u[0] - F32(1.0)) and y[i] == F32(F32(2.0) * u[1] - F32(1.0))
        for kk, jj in [divmod(q, 2) for q in range(int(taken[i]))]:  # the earlier candidates lie outside
            wq = orc.rng_block(11, int(pixel[i]), int(sample[i]), 0x40000000 | kk)
            a, b = (2.0 * orc.u32_to_unit_f32(int(wq[2 * jj + c])) - 1.0 for c in (0, 1))
            assert a * a + b * b > 1.0 - 1e-6


# ---------------------------------------------------------------- thin-lens geometry, in float64
@pytest.mark.parametrize("view", ["canonical", "second"])
def test_thin_lens_geometry(view):
    orc = _orc()
    if view == "canonical":
        w, h, spp = 24, 24, 4
        vp12 = orc.canonical_viewport(w, h)
    else:
        w, h, spp = 20, 16, 2
        vp12 = second_viewport(orc)
    radius, focus = 0.05, 4.0
    cr = CR.camera_rays(orc, vp12, w, h, spp, 7, CR.cam(CR.THIN_LENS, radius, focus))
    vp = np.asarray(vp12, np.float64)
    orig, eye, vu, vv = (vp[3 * i:3 * i + 3] for i in range(4))
    O, D, F, p = (a[:, :3].astype(np.float64) for a in (cr.o4, cr.d4, cr.F, cr.p))
    assert (cr.o4[:, 3] == 0).all() and (cr.d4[:, 3] == 0).all()
    assert np.abs(np.linalg.norm(D, axis=1) - 1.0).max() < 1e-6
    # every ray passes within a relative 1e-5 of its F
    tF = ((F - O) * D).sum(axis=1)
    miss = np.linalg.norm(O + tF[:, None] * D - F, axis=1)
    assert (miss <= 1e-5 * np.linalg.norm(F - eye, axis=1)).all() and (tF > 0).all()
    # every ray crosses the lens plane (through the eye, parallel to the image plane) within lens_radius (1 + 1e-5) of the eye
    nrm = np.cross(vu, vv)
    nrm /= np.linalg.norm(nrm)
    tl = ((eye - O) @ nrm) / (D @ nrm)
    rl = np.linalg.norm(O + tl[:, None] * D - eye, axis=1)
    assert (rl <= radius * (1 + 1e-5)).all() and rl.max() > 0.9 * radius
    # every ray starts in the image plane
    dist = np.abs((O - orig) @ nrm)
    assert (dist <= 1e-5 * np.linalg.norm(orig - eye)).all()
    # the image-plane point p lies on the segment lens point -> F (which is what makes focus = 1 start at p)
    assert ((tl < 0) & (tF > 0)).all()
    # focus = 1: the rays start at p, bit for bit
    one = CR.camera_rays(orc, vp12, w, h, spp, 7, CR.cam(CR.THIN_LENS, radius, 1.0))
    assert np.array_equal(one.o4.view(np.uint32), one.p.view(np.uint32)) and not np.array_equal(cr.o4, cr.p)
    # lens_radius = 0 is the pinhole's picture: same directions to rounding, origins equal as numbers
    zero = CR.camera_rays(orc, vp12, w, h, spp, 7, CR.cam(CR.THIN_LENS, 0.0, focus))
    pin = CR.camera_rays(orc, vp12, w, h, spp, 7, CR.cam(CR.PINHOLE))
    assert np.array_equal(zero.o4, pin.o4) and np.abs(zero.d4.astype(np.float64) - pin.d4).max() < 1e-6


@pytest.mark.parametrize("view", ["canonical", "second"])
def test_ortho_directions_are_all_the_same(view):
    orc = _orc()
    w, h, spp = (8, 8, 1) if view == "canonical" else (16, 16, 2)
    vp12 = orc.canonical_viewport(w, h) if view == "canonical" else second_viewport(orc)
    cr = CR.camera_rays(orc, vp12, w, h, spp, 7, CR.cam(CR.ORTHO))
    assert (cr.d4.view(np.uint32) == cr.d4.view(np.uint32)[0]).all()
    assert np.array_equal(cr.o4.view(np.uint32), cr.p.view(np.uint32))
    vp = np.asarray(vp12, np.float64)
    axis = vp[0:3] + 0.5 * vp[6:9] + 0.5 * vp[9:12] - vp[3:6]
    assert np.abs(cr.d4[0, :3] - axis / np.linalg.norm(axis)).max() < 1e-6
    if view == "canonical":  # the axis-aligned camera: every ray has two zero components
        assert ((cr.d4[:, :3] == 0).sum(axis=1) == 2).all()
    else:
        assert (cr.d4[:, :3] != 0).all()


# ---------------------------------------------------------------- the built library
def _lib():
    from rust_raytrace_amd import _ffi
    return _ffi, _ffi.lib()


def test_entry_points_are_exported_declared_and_listed():
    ffi, L = _lib()
    text = open(os.path.join(ROOT, "include", "rtmi.h")).read() + open(os.path.join(ROOT, "include", "rtmi_host.h")).read()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in ffi.RTMI_SYMBOLS + ffi.RTH_SYMBOLS, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
    assert hasattr(L, "rtmi_camera_defaults") and "rtmi_camera_defaults" in ffi.RTMI_SYMBOLS
    assert re.search(r"\bvoid\s+rtmi_camera_defaults\s*\(", text)
    assert re.search(r"RTMI_CAMERA_PINHOLE = 0, RTMI_CAMERA_THIN_LENS = 1, RTMI_CAMERA_ORTHO = 2", text)
    assert (ffi.CAMERA_PINHOLE, ffi.CAMERA_THIN_LENS, ffi.CAMERA_ORTHO) == (CR.PINHOLE, CR.THIN_LENS, CR.ORTHO) == (0, 1, 2)
    assert C.sizeof(ffi.Camera) == 16 and ffi.Camera.lens_radius.offset == 8 and ffi.Camera.focus.offset == 12
    assert C.sizeof(ffi.CameraOut) == 3 * C.sizeof(C.c_void_p)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES[:2]:
        assert re.search(r"pub fn " + name + r"\(", doc), name


def test_defaults():
    ffi, L = _lib()
    c = ffi.Camera(9, 9, 9.0, 9.0)
    L.rtmi_camera_defaults(C.byref(c))
    assert (c.model, c.flags, c.lens_radius, c.focus) == (0, 0, 0.0, 1.0)
    L.rtmi_camera_defaults(None)  # tolerated


class Vp(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("orig", C.c_float * 3), ("cam", C.c_float * 3), ("vu", C.c_float * 3),
                ("vv", C.c_float * 3), ("maxdepth", C.c_uint32), ("samples_per_pixel", C.c_uint32)]


def _vp(w=8, h=8, spp=4, maxdepth=5):
    v = Vp()
    v.width, v.height, v.maxdepth, v.samples_per_pixel = w, h, maxdepth, spp
    return v


BOGUS, ACC, OUT, G0, G1, G2 = 0x10, 0x100000, 0x200000, 0x300000, 0x400000, 0x500000


def _both(scene=BOGUS, view="dflt", tile=(0, 8, 8, 0), sample0=0, nsamples=4, camera="dflt", accum=ACC, outp=OUT, guides=None,
          variants=(True, False), **fields):
    """(rc, message, stats.rays) of the device and the host variant; the scene is a dangling handle no failing check may use"""
    ffi, L = _lib()
    v = _vp() if view == "dflt" else view
    cam = None
    if camera == "dflt":
        cam = ffi.Camera()
        L.rtmi_camera_defaults(C.byref(cam))
        for k, x in fields.items():
            setattr(cam, k, x)
    g = ffi.CameraOut(*[C.c_void_p(p) if p else None for p in guides]) if guides is not None else None
    res = []
    for dev in variants:
        st = ffi.Stats()
        st.rays = 123
        args = dict(vp=C.byref(v) if v is not None else None, cam=C.byref(cam) if cam is not None else None,
                    acc=C.c_void_p(accum) if accum else None, out=C.c_void_p(outp) if outp else None, g=C.byref(g) if g is not None else None)
        sc = C.c_void_p(scene) if scene else None
        if dev:
            t = ffi.Tile(*tile) if tile is not None else None
            rc = L.rtmi_render_camera_device(sc, args["vp"], 7, C.byref(t) if t is not None else None, args["cam"], sample0, nsamples,
                                             args["acc"], args["out"], args["g"], None, C.byref(st))
        else:
            row0, nrows = (tile[0], tile[1]) if tile is not None else (0, 8)
            rc = L.rtmi_render_camera(sc, args["vp"], 7, row0, nrows, args["cam"], sample0, nsamples, args["acc"], args["out"], args["g"],
                                      C.byref(st))
        res.append((rc, L.rtmi_last_error(), st.rays))
    return res


def _refused(word, code=RTMI_ERR_INVALID, **kw):
    for rc, msg, rays in _both(**kw):
        assert rc == code and word in msg and rays == 0, (kw, rc, msg, rays)


def test_bad_arguments_are_refused_before_the_scene_is_used():
    """Every refusal of the header, both variants, through a dangling scene handle, with stats cleared.  (Fails on a library
    without the feature: the symbol is missing.)"""
    nan, inf = float("nan"), float("inf")
    # everything rtmi_render_samples[_device] refuses
    for kw in (dict(scene=None), dict(view=None), dict(accum=0)):
        _refused(b"NULL", **kw)
    _refused(b"different buffers", accum=ACC, outp=ACC)
    _refused(b"nsamples", nsamples=0)
    _refused(b"sample0 + nsamples", sample0=3, nsamples=2)
    _refused(b"sample0 + nsamples", sample0=0xFFFFFFFF, nsamples=2)
    _refused(b"samples_per_pixel", view=_vp(spp=0))
    _refused(b"empty viewport", view=_vp(w=0))
    _refused(b"outside", tile=(4, 8, 8, 0))
    _refused(b"outside", tile=(0, 9, 9, 0))
    rc, msg, rays = _both(tile=None, variants=(True,))[0]
    assert rc == RTMI_ERR_INVALID and b"tile" in msg and rays == 0
    for tile, word in (((0, 4, 0, 0), b"stripe_rows"), ((0, 8, 2, 1), b"overlap"), ((0, 8, 2, 4), b"outside")):
        rc, msg, rays = _both(tile=tile, variants=(True,))[0]  # (what the host variant cannot express)
        assert rc == RTMI_ERR_INVALID and word in msg and rays == 0, (tile, msg)
    _refused(b"maxdepth", code=RTMI_ERR_UNSUPPORTED, view=_vp(maxdepth=33))
    # the camera
    _refused(b"NULL", camera=None)
    for m in (3, 4, 0xFFFFFFFF):
        _refused(b"model", model=m)
    for m in (0, 1, 2):
        for f in (1, 2, 1 << 31):
            _refused(b"flags", model=m, flags=f)
    for r in (-1.0, -1e-30, nan, inf, -inf):
        _refused(b"lens_radius", model=1, lens_radius=r)
    for f in (0.0, -0.0, -1.0, nan, inf, -inf):
        _refused(b"focus", model=1, focus=f)
    # a guide buffer that is another buffer of the call
    for g in ((ACC, 0, 0), (0, OUT, 0), (0, 0, ACC), (G0, G0, 0), (G0, 0, G0), (0, G1, G1), (OUT, G1, G2)):
        _refused(b"aliases", guides=g)
    # what is valid reaches the next check: ORTHO and PINHOLE ignore lens_radius and focus; edge values of the thin lens; guides
    for kw in (dict(model=0, lens_radius=nan, focus=-1.0), dict(model=2, lens_radius=-1.0, focus=nan), dict(model=1, lens_radius=0.0),
               dict(model=1, lens_radius=-0.0, focus=1e-30), dict(model=1, lens_radius=1e30, focus=1e30), dict(outp=0),
               dict(guides=(G0, G1, G2)), dict(guides=(0, 0, 0)), dict(guides=(0, G1, 0), outp=0)):
        _refused(b"sample0 + nsamples", nsamples=5, **kw)
    # an empty tile is fine and touches nothing
    for tile in ((0, 0, 1, 0), (100, 0, 0, 0)):
        for rc, _, rays in _both(tile=tile, model=1, lens_radius=0.1, focus=2.0, guides=(G0, G1, G2)):
            assert rc == RTMI_OK and rays == 0


def test_python_api_validates_its_arguments_and_converts_the_focus(canonical_pair):
    from rust_raytrace_amd import raytrace as R
    orc = _orc()
    _, sp = canonical_pair
    c = R.HipRayCaster()
    vp = R.canonical_viewport(8, 8, 5, 4)
    cam = c.camera_params(vp)
    assert (cam.model, cam.flags, cam.lens_radius, cam.focus) == (0, 0, 0.0, 1.0)
    assert c.camera_params(vp, "ortho", aperture=3.0, focus_distance=9.0).model == 2
    with pytest.raises(ValueError):
        c.camera_params(vp, "fisheye")
    # focus = focus_distance / |c - cam| in float64, rounded once
    v64 = np.asarray(orc.canonical_viewport(8, 8), np.float64)
    d = float(np.linalg.norm(v64[0:3] + 0.5 * v64[6:9] + 0.5 * v64[9:12] - v64[3:6]))
    lens = c.camera_params(vp, "thin_lens", aperture=0.05, focus_distance=5.0)
    assert lens.model == 1 and lens.lens_radius == float(F32(0.05)) and lens.focus == float(F32(5.0 / d))
    assert c.camera_params(vp, "thin_lens", aperture=0.05).focus == 1.0
    img = np.zeros((8, 8, 4), F32)
    for kw in (dict(data=np.zeros((8, 8, 4), np.float64)), dict(data=np.zeros((8, 9, 4), F32)), dict(pass_samples=0),
               dict(albedo=np.zeros((8, 8, 3), F32)), dict(ids=np.zeros((8, 8), np.int64))):
        kw.setdefault("data", img)
        with pytest.raises(ValueError):
            c.walk_rays_camera(vp, sp, camera=lens, **kw)
    for bad in (None, img):  # not a device tensor, or nothing at all
        with pytest.raises((ValueError, TypeError)):
            c.walk_rays_camera_device(vp, sp, lens, bad)
