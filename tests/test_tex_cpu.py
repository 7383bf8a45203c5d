"""Textures without a GPU (include/rtmi.h "TEXTURES OF A SCENE"): what pins tests/tex_ref.py, the restatement that
tests/test_tex.py holds the device against, and the host side of the feature.
 1. The conditions on tests/tex_cases.py's inputs, as counts: hits with u or v below 0 and above 1, texel indices -1 and W - 1
    (H - 1), an untextured triangle beside a textured one, every kind textured, the Solid.
 2. With no textures, and with all-ones textures, tex_ref is smooth_ref bit for bit, with and without normals and an environment.
 3. tex_ref.lookup against a float64 textbook evaluation at the patch hits and at 4 000 random (u, v) per texture: the largest
    error as measured, asserted at twice that.
 4. Continuity across the repeat seam at u, v = k -+ 1e-6.
 5. rtmi_project_uvs and the host Scene's stored tables are tex_ref.project's and the given ones bit for bit, ties of the axis
    rule included.
 6. The loader: uvs="file" on tests/golden/quad_uv.obj, uvs="box", a corner without a vt index raises, the default is untouched.
 7. Every refusal that needs no device."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import conftest as CT
import env_ref as ER
import glass_cases as GC
import smooth_cases as SC
import smooth_ref as SR
import tex_cases as TC
import tex_ref as TR
from conftest import ROOT, assert_bits_equal

F32 = np.float32
SEED = 5
LOOKUP_MEASURED = 5.976e-7  # largest |lookup_f32 - textbook_f64| (a component, texels in [0, 2]) over the sample, as measured
SUN = dict(sun_dir=(-0.75, 0.25, 0.6), sun_cos=0.8, sun_color=(30.0, 24.0, 16.0))
QUAD_UV = os.path.join(ROOT, "tests", "golden", "quad_uv.obj")


def _orc():
    from oracle import orc
    return orc


def _R():
    from rust_raytrace_amd import raytrace as R
    return R


def _lib():
    from rust_raytrace_amd import _ffi
    return _ffi.lib()


@pytest.fixture(scope="module")
def patch():
    so, sp = GC.build_pair(TC.recipe_patch())
    uvs, tot = TC.patch_uvs(len(so.triangles()[0]))
    o4, d4 = TC.rays()
    return so, sp, uvs, tot, o4, d4


def _hits(so, uvs, tot, o4, d4):
    """colour()'s detail at the surface hits of the rays, and the hit triangles"""
    recs, kinds, surf = so.triangles()
    tri, t, face, _ = so.trace(o4, d4)
    tri, face, t = np.asarray(tri, np.int64), np.asarray(face, np.uint32), np.asarray(t, F32)
    ok = (tri != 0) & ((face & 2) == 0)
    point = ((d4[ok] * t[ok, None]).astype(F32) + o4[ok]).astype(F32)
    rec = TR.records(recs[:, 20:29], uvs, tot)
    _, d = TR.colour(rec, TC.images(), tri[ok], point, surf[tri[ok], :3], detail=True)
    return d, tri[ok], kinds[tri[ok]], rec


# ---------------------------------------------------------------- 1
def test_the_patchs_rays_meet_every_condition(patch):
    so, sp, uvs, tot, o4, d4 = patch
    d, tri, kind, rec = _hits(so, uvs, tot, o4, d4)
    T = d.textured
    counts = {"u<0": (T & (d.u < 0)).sum(), "v<0": (T & (d.v < 0)).sum(), "u>1": (T & (d.u > 1)).sum(), "v>1": (T & (d.v > 1)).sum(),
              "ix==-1": (T & (d.ix == -1)).sum(), "ix+1==W": (T & (d.ix + 1 == d.w)).sum(), "iy==-1": (T & (d.iy == -1)).sum(),
              "iy+1==H": (T & (d.iy + 1 == d.h)).sum(), "untextured": (~T).sum(), "solid": (T & (tri == TC.SOLID_TRI)).sum()}
    assert min(counts.values()) >= 20, counts
    for k in (SR.MATTE, SR.REFLECTIVE, TR.DIELECTRIC):
        assert (T & (kind == k)).sum() >= 100, (k, counts)
    # an untextured triangle beside a textured one: 2 shares an edge with 1, 8 with 7
    assert tot[1] and not tot[2] and tot[7] and not tot[8] and (tri == 2).sum() >= 20 and (tri == 8).sum() >= 20
    assert set(np.unique(d.tex[T])) == {1, 2, 3, 4}  # every texture size is looked up
    # the sliver: accepted by make_triangle, den exactly 0, so stored without the texture it was given
    assert rec.den[TC.SLIVER_TRI] == 0 and tot[TC.SLIVER_TRI] != 0 and rec.tex[TC.SLIVER_TRI] == 0 and (rec.den[1:11] > 0).all()


# ---------------------------------------------------------------- 2
@pytest.mark.parametrize("with_env", [False, True])
@pytest.mark.parametrize("with_normals", [False, True])
def test_without_textures_and_with_all_ones_the_restatement_is_smooth_ref(patch, with_normals, with_env):
    so, sp, uvs, tot, o4, d4 = patch
    orc = _orc()
    n = len(o4)
    nrm = None
    if with_normals:
        nrm = np.zeros((len(uvs), 3, 3), F32)
        nrm[:SC.NTRI_PATCH + 1] = SC.patch_normals(so.triangles()[0])[:SC.NTRI_PATCH + 1]
    env = SimpleNamespace(table=ER.sky_table(8, SUN), frame=None) if with_env else None
    args = (orc, so, o4, d4, np.arange(n), np.zeros(n, np.int64), 3, SEED)
    want = SR.path_trace(*args, env=env, normals=nrm)
    none = TR.path_trace(*args, env=env, normals=nrm)
    ones = TR.path_trace(*args, env=env, normals=nrm, tex=TR.textures(TC.images(ones=True), uvs, tot))
    real = TR.path_trace(*args, env=env, normals=nrm, tex=TR.textures(TC.images(), uvs, tot))
    for got, what in ((none, "no textures"), (ones, "all-ones textures")):
        assert_bits_equal(got.color, want.color, what)
        assert got.rays == want.rays and got.passes == want.passes and got.total == want.total
    assert ones.tex["matte"] >= 100 and (real.color != want.color).any(axis=1).sum() >= 500 and real.rays == want.rays
    vo = orc.canonical_viewport(16, 16)
    a = SR.render(orc, so, vo, 16, 16, 2, SEED, 4, env=env, normals=nrm)
    b = TR.render(orc, so, vo, 16, 16, 2, SEED, 4, env=env, normals=nrm, tex=TR.textures(TC.images(ones=True), uvs, tot))
    assert_bits_equal(b.image, a.image, "render, all-ones textures")
    assert_bits_equal(b.accum, a.accum, "render, all-ones textures: accum")


# ---------------------------------------------------------------- 3
def _textbook(img, u, v):
    """Bilinear, repeating lookup in float64 of float32 inputs: texel centres at (i + 0.5) / W"""
    img = np.asarray(img, np.float64)
    h, w = img.shape[:2]
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    x, y = (u - np.floor(u)) * w - 0.5, (v - np.floor(v)) * h - 0.5
    x0, y0 = np.floor(x), np.floor(y)
    tx, ty = (x - x0)[:, None], (y - y0)[:, None]
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    T = lambda i, j: img[j % h, i % w]
    return (T(x0, y0) * (1 - tx) + T(x0 + 1, y0) * tx) * (1 - ty) + (T(x0, y0 + 1) * (1 - tx) + T(x0 + 1, y0 + 1) * tx) * ty


def test_lookup_against_a_float64_textbook_evaluation(patch):
    so, sp, uvs, tot, o4, d4 = patch
    d, _, _, _ = _hits(so, uvs, tot, o4, d4)
    rng = np.random.default_rng(11)
    worst = 0.0
    for k, img in enumerate(TC.images(), start=1):
        sel = d.textured & (d.tex == k)
        u = np.concatenate([d.u[sel], (rng.random(4000) * 8.0 - 4.0).astype(F32)])
        v = np.concatenate([d.v[sel], (rng.random(4000) * 8.0 - 4.0).astype(F32)])
        got = TR.lookup(img, u, v)
        assert not got[:, 3].any()  # lane 3 is the texels' +0
        worst = max(worst, float(np.abs(got[:, :3].astype(np.float64) - _textbook(img, u, v)).max()))
    print(f"largest |lookup_f32 - textbook_f64| = {worst:.3e} (recorded: {LOOKUP_MEASURED:.3e})")
    assert worst <= 2 * LOOKUP_MEASURED, worst


# ---------------------------------------------------------------- 4
def test_the_repeat_seam_is_continuous_and_a_period_apart_is_equal():
    # across u = k the lookup moves by at most |d fx| * (largest texel difference, 2): d fx <= W * (2e-6 + 2 ulp(4)), W <= 8,
    # plus the rounding of the lookup itself (item 3)
    bound = 8 * (2e-6 + 2 * 4.8e-7) * 2 + 4 * LOOKUP_MEASURED
    for img in TC.images():
        for k in (-3, -1, 0, 1, 2, 4):
            other = np.linspace(-1.3, 2.7, 41).astype(F32)
            lo, hi = np.full(41, k - 1e-6, F32), np.full(41, k + 1e-6, F32)
            assert np.abs(TR.lookup(img, lo, other) - TR.lookup(img, hi, other)).max() <= bound
            assert np.abs(TR.lookup(img, other, lo) - TR.lookup(img, other, hi)).max() <= bound
    # u and u + 1 where both are exact in float32 give the same texels and weights
    u = (np.arange(64) / 64.0).astype(F32)
    for img in TC.images():
        assert_bits_equal(TR.lookup(img, u, u[::-1].copy()), TR.lookup(img, (u + F32(1.0)).astype(F32), (u[::-1] - F32(2.0)).astype(F32)), "a period apart")
    # a 1 x 1 texture is its texel everywhere (up to the rounding of the two mix_color levels); NaN coordinates stay in bounds
    one = TC.images()[0]
    got = TR.lookup(one, (np.arange(50) * 0.37 - 7).astype(F32), (np.arange(50) * 0.11).astype(F32))
    assert np.abs(got[:, :3] - one[0, 0]).max() <= 4 * LOOKUP_MEASURED
    bad = TR.lookup(TC.images()[2], np.array([np.nan, 0.5, np.inf], F32), np.array([0.5, np.nan, 0.25], F32))
    assert np.isnan(bad[:, :3]).all()


# ---------------------------------------------------------------- 5
def _library_project(corners, facenorm, lo, scale):
    c, f = np.ascontiguousarray(corners, F32).reshape(-1, 9), np.ascontiguousarray(facenorm, F32).reshape(-1, 3)
    out = np.full((len(c), 3, 2), 7.0, F32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = _lib().rtmi_project_uvs(p(c), p(f), len(c), p(np.asarray(lo, F32)), C.c_float(scale), p(out))
    assert rc == 0, _lib().rtmi_last_error()
    return out


def test_project_uvs_and_the_scenes_tables_are_the_restatements():
    rng = np.random.default_rng(3)
    corners = (rng.random((40, 3, 3)) * 6 - 3).astype(F32)
    fn = rng.standard_normal((40, 3)).astype(F32)
    # the ties of the axis rule: x wins |x| == |y| and |x| == |z|, y wins |y| == |z|, whatever the signs
    fn[:8] = [(1, 1, 0), (1, -1, 0.5), (-2, 0, 2), (0.5, 1, -1), (0, -3, 3), (1, 1, 1), (-1, -1, -1), (0, 0, 0)]
    lo, scale = (-0.7, 0.3, 1.1), 0.37
    want = TR.project(corners, fn, lo, scale)
    assert_bits_equal(_library_project(corners, fn, lo, scale), want, "rtmi_project_uvs")
    c64 = corners.astype(np.float64)
    for i, (j, k) in enumerate(((1, 2), (1, 2), (1, 2), (2, 0), (2, 0), (1, 2), (1, 2), (1, 2))):
        assert np.allclose(want[i, :, 0], (c64[i, :, j] - lo[j]) * scale, atol=1e-5) and np.allclose(want[i, :, 1], (c64[i, :, k] - lo[k]) * scale, atol=1e-5)
    # the Scene mirror on the canonical scene: the teapot projected, the images, a range set by hand
    R = _R()
    s = R.canonical_scene(CT.TEAPOT_TRI, texture=TC.images()[3])
    rec = s.triangles()[0]
    n = len(rec)
    images, uvs, tot = s.textures()
    assert len(images) == 1 and uvs.shape == (n, 3, 2) and tot.shape == (n,)
    assert_bits_equal(images[0], TC.images()[3], "the image")
    assert_bits_equal(uvs[1:6321], TR.project(rec[1:6321, 20:29], rec[1:6321, 3:6], (0, 0, 0), 1.0), "Scene.project_uvs")
    assert (tot[1:6321] == 1).all() and tot[0] == 0 and not tot[6321:].any() and not uvs[6321:].any() and not uvs[0].any()
    hand, ht = rng.random((5, 3, 2)).astype(F32), np.array([1, 0, 2, 2, 1], np.uint32)
    s.set_textures(TC.images()[:2], hand, ht, first=6400, flip_v=True)
    images, uvs2, tot2 = s.textures()
    for a, b in zip(images, TC.images()[:2]):
        assert_bits_equal(a, np.ascontiguousarray(b[::-1]), "flip_v stores the rows bottom first")
    assert_bits_equal(uvs2[6400:6405], hand, "set_textures' uvs")
    assert np.array_equal(tot2[6400:6405], ht) and np.array_equal(tot2[:6400], tot[:6400])
    assert_bits_equal(uvs2[:6400], uvs[:6400], "the other triangles keep their uvs")
    rr = TR.records(rec[:, 20:29], uvs2, tot2)  # the per-triangle table the device will hold of them
    assert np.array_equal(rr.tex, tot2) and (rr.den[1:] > 0).all()
    s.clear_textures()
    assert s.textures() is None


# ---------------------------------------------------------------- 6
def test_the_loader_reads_vt_and_the_default_is_untouched(tmp_path):
    R = _R()
    tr = R.create_transform(R.unit([0.2, 0.3, 1.0]), R.to_radians(40.0))
    surf = R.SurfaceKind.Matte(R.make_color(10, 20, 30), 0.5)

    def load(path=QUAD_UV, **kw):
        s = R.Scene(with_dummy=True)
        s.extend_parse_obj(str(path), [0.5, -0.25, 3.0], 2.0, tr, surf, 0.0, **kw)
        return s
    plain = load()
    assert plain.textures() is None and plain.num_tris() == 3  # the reference's loader: a face's first three corners
    vt = np.array([(0, 0), (1.5, 0), (1.5, 2.25), (0, 2.25), (-0.5, 0.75)], F32)
    s = load(uvs="file", texture=2)
    for a, b in zip(s.triangles(), plain.triangles()):
        assert a.tobytes() == b.tobytes()  # the triangles are the default loader's, byte for byte
    images, uvs, tot = s.textures()
    assert images == [] and not uvs[0].any() and list(tot) == [0, 2, 2]
    assert_bits_equal(uvs[1:], vt[np.array([(0, 1, 2), (1, 4, 2)])], "vt through a/b and a/b/c corners")
    s = load(uvs="file", robust=True)  # the quad is fanned: (1, 2, 3), (1, 3, 4)
    images, uvs, tot = s.textures()
    assert s.num_tris() == 4 and list(tot) == [0, 1, 1, 1]
    assert_bits_equal(uvs[1:], vt[np.array([(0, 1, 2), (0, 2, 3), (1, 4, 2)])], "vt, fanned")
    b = load(uvs="box", texture=3)
    rec = b.triangles()[0]
    images, uvs, tot = b.textures()
    assert_bits_equal(uvs[1:], TR.project(rec[1:, 20:29], rec[1:, 3:6], (0, 0, 0), 1.0), "uvs='box' through the loader")
    assert list(tot) == [0, 3, 3]
    bad = tmp_path / "bad.obj"
    bad.write_text(open(QUAD_UV).read().replace("f 2/2/1 5/5/1 3/3/1", "f 2/2/1 5//1 3/3/1"))
    with pytest.raises(RuntimeError, match="texture coordinate index"):
        load(bad, uvs="file")
    assert load(bad).num_tris() == 3  # the default mode never looks at the second field
    with pytest.raises(ValueError):
        load(uvs="vt")
    with pytest.raises(ValueError):
        load(uvs="file", normals="file")
    # neither of the project's own teapots has a vt line
    with pytest.raises(RuntimeError, match="texture coordinate index"):
        R.Scene(with_dummy=True).extend_parse_obj(CT.TEAPOT_TRI, [0.0, 0.5, 5.0], 1.0, tr, surf, 0.05, uvs="file")


# ---------------------------------------------------------------- 7
def test_interface_refusals_that_need_no_gpu():
    from rust_raytrace_amd import _ffi
    R, L = _R(), _lib()
    s = R.canonical_scene(CT.TEAPOT_TRI)
    n = s.num_tris()
    img = TC.images()[2]
    uv, tt = np.zeros((3, 3, 2), F32), np.ones(3, np.uint32)
    with pytest.raises(ValueError):
        s.set_textures([np.zeros((4, 4), F32)], uv, tt)
    with pytest.raises(ValueError):
        s.set_textures([img], np.zeros((3, 6), F32), tt)
    with pytest.raises(ValueError):
        s.set_textures([], uv, tt)
    with pytest.raises(RuntimeError, match="above ntex"):
        s.set_textures([img], uv, np.array([1, 2, 1], np.uint32), first=4)
    assert s.textures() is None
    with pytest.raises(RuntimeError, match="8192"):
        s.set_textures([np.zeros((1, 8193, 3), F32)], uv, tt)
    with pytest.raises(RuntimeError, match="256"):
        s.set_textures([img] * 257, uv, tt)
    assert s.textures() is None  # none of them left anything behind
    s.set_textures([img], None, None)
    for bad in (np.nan, np.inf):
        x = uv.copy()
        x[1, 2, 0] = bad
        with pytest.raises(RuntimeError, match="uv of triangle 8 is not finite"):
            s.set_textures([img], x, tt, first=7)
        x[1, 2, 0] = 0
        x[2, 0, 1] = bad
        s.set_textures([img], x, np.array([1, 1, 0], np.uint32), first=7)  # an untextured triangle's uvs may hold anything
    with pytest.raises(RuntimeError, match="first"):
        s.set_textures([img], uv, tt, first=0)
    with pytest.raises(RuntimeError, match="beyond"):
        s.set_textures([img], uv, tt, first=n - 1)
    with pytest.raises(RuntimeError, match="first"):
        s.project_uvs(0, 10)
    with pytest.raises(RuntimeError, match="beyond"):
        s.project_uvs(5, n)
    with pytest.raises(RuntimeError, match="above ntex"):
        s.project_uvs(1, 10, texture=2)
    with pytest.raises(RuntimeError, match="not finite"):
        s.project_uvs(1, 10, scale=float("inf"))
    with pytest.raises(RuntimeError, match="above ntex"):
        s.set_textures([img], uv, np.array([1, 2, 1], np.uint32), first=4)
    s.clear_textures()
    assert s.textures() is None
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    c9, f3, o6 = np.zeros((2, 9), F32), np.zeros((2, 3), F32), np.zeros((2, 6), F32)
    lo = np.zeros(3, F32)
    assert L.rtmi_project_uvs(None, p(f3), 2, p(lo), C.c_float(1.0), p(o6)) != 0
    assert L.rtmi_project_uvs(p(c9), p(f3), 2, None, C.c_float(1.0), p(o6)) != 0
    assert L.rtmi_project_uvs(None, None, 0, None, C.c_float(1.0), None) == 0
    t = (_ffi.Texture * 1)(_ffi.Texture(img.ctypes.data, 5, 3, 0))
    n64, w32 = C.c_uint64(0), C.c_uint32(0)
    assert L.rtmi_scene_set_textures(None, t, 1, p(c9), p(o6), p(np.zeros(2, np.uint32)), 2) != 0
    assert L.rtmi_scene_get_uvs(None, None, None, C.byref(n64)) != 0 and L.rtmi_scene_get_texture(None, 1, None, C.byref(w32), C.byref(w32)) != 0


def test_header_symbols_and_documents():
    from rust_raytrace_amd import _ffi
    text = open(os.path.join(ROOT, "include", "rtmi.h")).read()
    assert "TEXTURES OF A SCENE" in text and "rtmi_texture_t" in text
    for name in ("rtmi_scene_set_textures", "rtmi_scene_get_uvs", "rtmi_scene_get_texture", "rtmi_project_uvs"):
        assert re.search(r"\bint %s\(" % name, text) and name in _ffi.RTMI_SYMBOLS and hasattr(_ffi.lib(), name)
    host = open(os.path.join(ROOT, "include", "rtmi_host.h")).read()
    for name in ("rth_scene_set_textures", "rth_scene_set_uvs", "rth_scene_project_uvs", "rth_scene_textures_size", "rth_scene_get_uvs",
                 "rth_scene_get_texture", "rth_caster_uvs", "rth_caster_texture", "rth_add_obj_uvs"):
        assert name in host and name in _ffi.RTH_SYMBOLS and hasattr(_ffi.lib(), name)
    assert "4.25" in open(os.path.join(ROOT, "DESIGN.md")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "rtmi_scene_set_textures" in doc and "rtmi_project_uvs" in doc
