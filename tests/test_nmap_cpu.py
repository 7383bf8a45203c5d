"""Normal maps without a GPU (include/rtmi.h "NORMAL MAPS OF A SCENE"): what pins tests/nmap_ref.py, the restatement
that tests/test_nmap.py holds the device against, and the host side of the feature.
 1. The conditions on tests/nmap_cases.py's inputs, as counts over the patch rays at depth 3 (wild map, hand-set vertex normals).
 2. With no maps, and with maps on degenerate triangles only, nmap_ref is tex_ref bit for bit, with and without normals and an
    environment.
 3. nmap_ref.normal against a float64 textbook evaluation (TBN from the uv derivatives, Gram-Schmidt against the shading normal,
    decode, scale, normalise) at the patch's mapped hits under the tame maps and at 4 000 random (N, texel) pairs per mapped
    triangle: the largest deviation of a component of nm as measured (1.593e-7), asserted at twice that (3.186e-7).  No hit is
    excluded.
 4. Continuity of nm across the repeat seam at u, v = k -+ 1e-6.
 5. rtmi_normal_map_from_height and the host Scene's stored tables are the restatement's bit for bit, hand on a mirrored uv layout
    (negative det) included.
 6. Every refusal that needs no device.
 7. Symbols and documents."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import env_ref as ER
import glass_cases as GC
import nmap_cases as NC
import nmap_ref as NR
import smooth_cases as SC
import smooth_ref as SR
import tex_ref as TR
from conftest import ROOT, assert_bits_equal
from rays_ref import vunit

F32 = np.float32
SEED = 5
NM_MEASURED = 1.593e-7  # largest |nm_f32 - textbook_f64| (a component) over the sample, as measured
LOOKUP_MEASURED = 5.976e-7  # tests/test_tex_cpu.py's, of the bilinear lookup
SUN = dict(sun_dir=(-0.75, 0.25, 0.6), sun_cos=0.8, sun_color=(30.0, 24.0, 16.0))


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
    so, sp = GC.build_pair(NC.recipe_patch())
    n = len(so.triangles()[0])
    uvs, tot = NC.patch_uvs(n)
    o4, d4 = NC.rays()
    nrm = np.zeros((n, 3, 3), F32)
    nrm[:SC.NTRI_PATCH + 1] = SC.patch_normals(so.triangles()[0])[:SC.NTRI_PATCH + 1]
    sp.set_textures(NC.images(), uvs[1:], tot[1:])  # the product's scene carries what the restatement is given
    sp.set_normal_maps(NC.patch_nmaps(n)[1:])
    return SimpleNamespace(so=so, sp=sp, uvs=uvs, tot=tot, nm=NC.patch_nmaps(n), o4=o4, d4=d4, normals=nrm, n=n)


def _trace(p, depth, wild=False, normals=None, env=None, nm="patch", tex=True):
    n = len(p.o4)
    t = TR.textures(NC.images(wild), p.uvs, p.tot) if tex else None
    m = NR.maps(p.nm) if isinstance(nm, str) else nm
    return NR.path_trace(_orc(), p.so, p.o4, p.d4, np.arange(n), np.zeros(n, np.int64), depth, SEED, env=env, normals=normals, tex=t, nm=m)


# ---------------------------------------------------------------- 1
def test_the_patchs_rays_meet_every_condition(patch):
    p = patch
    c = _trace(p, 3, wild=True, normals=p.normals).nmap
    for k in ("usem", "away_from_ray", "away_from_ng", "nan", "retry_usem", "back_usem", "flat_usem", "mapped_matte", "mapped_reflective",
              "mapped_glass"):
        assert c[k] >= 20, (k, c)
    # use false but usem true on the flat triangle (8) itself, from the primary rays
    hn = NR.hit_normals(p.so, p.normals, TR.textures(NC.images(True), p.uvs, p.tot), NR.maps(p.nm), p.o4, p.d4)
    sn = SR.hit_normals(p.so, p.normals, p.o4, p.d4)
    assert (hn.usem & ~sn.use & (hn.tri == 8)).sum() >= 20
    # the inputs of the float64 comparison are well conditioned: |det| of the uv layout, and the two degenerate triangles
    recs = p.so.triangles()[0]
    fr = NR.frames(recs[:, 20:29], p.uvs, recs[:, 3:6], p.nm)
    good = [i for i in range(1, 11) if i != NC.COLLINEAR_TRI]
    assert (np.abs(fr.det[good]) >= 2.39).all() and fr.det[NC.COLLINEAR_TRI] == 0 and fr.den[11] == 0
    assert p.nm[NC.COLLINEAR_TRI] and p.nm[11] and not fr.nmap[NC.COLLINEAR_TRI] and not fr.nmap[11] and not fr.nmap[12:].any()
    assert np.array_equal(fr.nmap[good], p.nm[good])
    T, hand, stored = p.sp.normal_map_frames()  # and the product's scene stores the same
    assert np.array_equal(stored, fr.nmap) and np.array_equal(hand, fr.hand) and T.tobytes() == np.ascontiguousarray(fr.T[:, :3]).tobytes()
    wild = NC.wild_map()
    assert (wild == F32(0.5)).all(axis=2).any() and (wild[..., 2] < 0.5).any() and wild.min() >= -1 and wild.max() <= 2
    for m in NC.tame_maps():
        assert m[..., :2].min() >= 0.25 and m[..., :2].max() <= 0.75 and m[..., 2].min() >= 0.75 and m[..., 2].max() <= 1


# ---------------------------------------------------------------- 2
@pytest.mark.parametrize("with_env", [False, True])
@pytest.mark.parametrize("with_normals", [False, True])
def test_without_maps_the_restatement_is_tex_ref(patch, with_normals, with_env):
    p = patch
    n = len(p.o4)
    nrm = p.normals if with_normals else None
    env = SimpleNamespace(table=ER.sky_table(8, SUN), frame=None) if with_env else None
    tex = TR.textures(NC.images(), p.uvs, p.tot)
    want = TR.path_trace(_orc(), p.so, p.o4, p.d4, np.arange(n), np.zeros(n, np.int64), 3, SEED, env=env, normals=nrm, tex=tex)
    only_degenerate = np.zeros(p.n, np.uint32)
    only_degenerate[[NC.COLLINEAR_TRI, 11]] = 8
    zeros = np.zeros(p.n, np.uint32)
    for nm, what in ((None, "no maps"), (NR.maps(zeros), "all map 0"), (NR.maps(only_degenerate), "maps on degenerate triangles only")):
        got = _trace(p, 3, normals=nrm, env=env, nm=nm)
        assert_bits_equal(got.color, want.color, what)
        assert got.rays == want.rays and got.passes == want.passes and got.total == want.total and got.tex == want.tex
        assert got.nmap["usem"] == 0 and got.nmap["mapped_matte"] == 0
    real = _trace(p, 3, normals=nrm, env=env)
    assert (real.color != want.color).any(axis=1).sum() >= 200 and real.nmap["usem"] >= 500
    vo = _orc().canonical_viewport(16, 16)
    a = TR.render(_orc(), p.so, vo, 16, 16, 2, SEED, 4, env=env, normals=nrm, tex=tex)
    b = NR.render(_orc(), p.so, vo, 16, 16, 2, SEED, 4, env=env, normals=nrm, tex=tex, nm=NR.maps(only_degenerate))
    assert_bits_equal(b.image, a.image, "render, maps on degenerate triangles only")
    fa = TR.features(_orc(), p.so, nrm, tex, 16, 16, vo, 2, SEED)
    fb = NR.features(_orc(), p.so, nrm, tex, NR.maps(only_degenerate), 16, 16, vo, 2, SEED)
    for x, y in zip(fa, fb):
        assert x.tobytes() == y.tobytes()


# ---------------------------------------------------------------- 3
def _textbook(corners, uvs, ngeom, M, strength, back, N):
    """nm in float64 of float32 inputs: the tangent and bitangent of the uv layout, the handedness of (T, B, ngeom), T made
    orthogonal to the shading normal N, the bitangent cross(N, t) with that handedness (N is on the hit side: the sign flips on a
    back face so that b is the same world vector), the decoded texel in that frame, normalised"""
    c, uv, ngeom, M, N = (np.asarray(a, np.float64) for a in (corners, uvs, ngeom, M, N))
    e1, e2 = c[:, 1] - c[:, 0], c[:, 2] - c[:, 0]
    du1, du2, dv1, dv2 = uv[:, 1, 0] - uv[:, 0, 0], uv[:, 2, 0] - uv[:, 0, 0], uv[:, 1, 1] - uv[:, 0, 1], uv[:, 2, 1] - uv[:, 0, 1]
    det = du1 * dv2 - du2 * dv1
    T = (e1 * dv2[:, None] - e2 * dv1[:, None]) / det[:, None]  # d position / d u
    B = (e2 * du1[:, None] - e1 * du2[:, None]) / det[:, None]  # d position / d v
    hand = np.sign(np.einsum("ij,ij->i", np.cross(ngeom, T), B))
    t = T - N * np.einsum("ij,ij->i", N, T)[:, None]
    t /= np.linalg.norm(t, axis=1)[:, None]
    b = np.cross(N, t) * (hand * np.where(back, -1.0, 1.0))[:, None]
    x, y, z = (2 * M[:, 0] - 1) * strength, (2 * M[:, 1] - 1) * strength, 2 * M[:, 2] - 1
    nm = t * x[:, None] + b * y[:, None] + N * z[:, None]
    return nm / np.linalg.norm(nm, axis=1)[:, None], np.linalg.norm(np.cross(N, T), axis=1) / np.linalg.norm(T, axis=1), np.sqrt(x * x + y * y + z * z)


def test_normal_against_a_float64_textbook_evaluation(patch):
    p = patch
    recs = p.so.triangles()[0]
    corners, ngeom = recs[:, 20:29].reshape(-1, 3, 3), recs[:, 3:6]
    fr = NR.frames(corners, p.uvs, ngeom, p.nm)
    rng = np.random.default_rng(13)
    worst, sin_min, len_min, total = 0.0, 9.0, 9.0, 0
    for strength in (1.0, 0.6):
        nm = NR.maps(p.nm, strength)
        tex = TR.textures(NC.images(), p.uvs, p.tot)
        cases = []
        # the patch's mapped hits under the tame maps, with the hand-set vertex normals: every one of them
        hn = NR.hit_normals(p.so, p.normals, tex, nm, p.o4, p.d4)
        m = hn.mapped
        trec = TR.records(corners, p.uvs, p.tot)
        point = ((p.d4[m] * hn.t[m, None]).astype(F32) + p.o4[m]).astype(F32)
        u, v, _ = TR.hit_uv(trec, hn.tri[m], point)
        cases.append((hn.tri[m], (hn.face[m] & 1) != 0, hn.N[m], NR.lookup_maps(tex.images, fr.nmap[hn.tri[m]], u, v), hn.ng[m], p.d4[m]))
        assert m.sum() >= 500
        # 4 000 random (N, texel) pairs per mapped triangle: N tilted off the geometric normal by up to 64 degrees (asin 0.9)
        for tri in np.nonzero(fr.nmap)[0]:
            k = 4000
            back = rng.random(k) < 0.5
            ng = SR.v4(np.repeat(ngeom[tri][None], k, axis=0))
            ng[back] *= F32(-1.0)
            tilt = rng.standard_normal((k, 3))
            tilt *= (0.9 * rng.random(k) ** (1 / 3) / np.linalg.norm(tilt, axis=1))[:, None]  # uniform in a ball of radius 0.9
            N = vunit((ng + SR.v4(tilt)).astype(F32))
            M = np.zeros((k, 4), F32)
            M[:, :2] = 0.25 + 0.5 * rng.random((k, 2))
            M[:, 2] = 0.75 + 0.25 * rng.random(k)
            cases.append((np.full(k, tri), back, N, M, ng, (ng * F32(-1.0)).astype(F32)))
        for tri, back, N, M, ng, rd in cases:
            got = NR.normal(fr, M, nm.strength, tri, back, N, ng, rd)
            assert not got.nan.any() and not got.nm[:, 3].any()  # lane 3 is +0
            want, sin_nt, length = _textbook(corners[tri], p.uvs[tri], ngeom[tri], M[:, :3], float(nm.strength), back, N[:, :3])
            worst = max(worst, float(np.abs(got.nm[:, :3].astype(np.float64) - want).max()))
            sin_min, len_min, total = min(sin_min, float(sin_nt.min())), min(len_min, float(length.min())), total + len(tri)
    print(f"largest |nm_f32 - textbook_f64| = {worst:.3e} over {total} evaluations (recorded: {NM_MEASURED:.3e}); "
          f"smallest sin(N, T) = {sin_min:.3f}, smallest |(x, y, z)| = {len_min:.3f}")
    assert sin_min > 0.19 and len_min >= 0.5  # the float64 evaluation is well conditioned on every input: nothing is excluded
    assert worst <= 2 * NM_MEASURED, worst


# ---------------------------------------------------------------- 4
def test_nm_is_continuous_across_the_repeat_seam(patch):
    p = patch
    recs = p.so.triangles()[0]
    fr = NR.frames(recs[:, 20:29], p.uvs, recs[:, 3:6], p.nm)
    tri = np.full(41, 1)
    ng = SR.v4(np.repeat(recs[1, 3:6][None], 41, axis=0))
    N = vunit((ng + SR.v4(np.array([0.2, -0.1, 0.15]))).astype(F32))
    rd = (ng * F32(-1.0)).astype(F32)
    back = np.zeros(41, bool)

    def nm_at(img, u, v):
        return NR.normal(fr, TR.lookup(img, u, v), F32(1.0), tri, back, N, ng, rd).nm
    # across u = k the lookup moves by at most |d fx| * (largest texel difference: 0.5 in x and y, 0.25 in z) plus its own rounding
    # (tests/test_tex_cpu.py item 4); the decoded vector by twice that per component, and normalising a vector of length >= 0.5
    # scales a move of it by at most 1 / 0.5; plus the rounding of the rule (item 3) at both points
    d_lookup = 8 * (2e-6 + 2 * 4.8e-7) * 0.5 + 4 * LOOKUP_MEASURED
    bound = 2 * np.sqrt(3.0) * d_lookup / 0.5 + 4 * NM_MEASURED
    for img in NC.tame_maps():
        for k in (-3, -1, 0, 1, 2, 4):
            other = np.linspace(-1.3, 2.7, 41).astype(F32)
            lo, hi = np.full(41, k - 1e-6, F32), np.full(41, k + 1e-6, F32)
            assert np.abs(nm_at(img, lo, other) - nm_at(img, hi, other)).max() <= bound
            assert np.abs(nm_at(img, other, lo) - nm_at(img, other, hi)).max() <= bound


# ---------------------------------------------------------------- 5
def test_from_height_and_the_scenes_tables_are_the_restatements(patch):
    R, L = _R(), _lib()
    p = patch
    for w, h in NC.MAP_SIZES + ((7, 2),):
        for scale in (1.0, 3.5):
            hh = NC.heights(w, h, seed=w * 10 + h)
            got = R.normal_map_from_height(hh, scale)
            assert got.shape == (h, w, 3)
            assert_bits_equal(got, NR.from_height(hh, scale), f"rtmi_normal_map_from_height {w} x {h}")
    flat = R.normal_map_from_height(np.ones((3, 3), F32))
    assert (flat == np.array([0.5, 0.5, 1.0], F32)).all()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    out = np.zeros(3, F32)
    assert L.rtmi_normal_map_from_height(None, 1, 1, C.c_float(1.0), ptr(out)) != 0
    assert L.rtmi_normal_map_from_height(ptr(out), 1, 1, C.c_float(1.0), None) != 0
    assert L.rtmi_normal_map_from_height(None, 0, 5, C.c_float(1.0), None) == 0 and L.rtmi_normal_map_from_height(None, 5, 0, C.c_float(1.0), None) == 0
    # the Scene mirror on the patch, and on a mirrored uv layout (u -> 1 - u on the odd triangles: det < 0, hand -1)
    recs = p.so.triangles()[0]
    sp = GC.build_pair(NC.recipe_patch())[1]
    for mirrored in (False, True):
        uvs = p.uvs.copy()
        if mirrored:
            uvs[1::2, :, 0] = (F32(1.0) - uvs[1::2, :, 0]).astype(F32)
        sp.set_textures(NC.images(), uvs[1:], p.tot[1:])
        assert sp.normal_maps() is None
        sp.set_normal_maps(p.nm[1:], strength=0.75)
        back, strength = sp.normal_maps()
        assert np.array_equal(back, p.nm) and strength == 0.75
        want = NR.frames(recs[:, 20:29], uvs, recs[:, 3:6], p.nm)
        T, hand, stored = sp.normal_map_frames()
        assert_bits_equal(T, want.T[:, :3], "T")
        assert np.array_equal(hand, want.hand) and np.array_equal(stored, want.nmap)
        assert stored[NC.COLLINEAR_TRI] == 0 and stored[11] == 0 and stored[1] == 8
        if mirrored:
            odd = [1, 3, 5, 9]  # (7 has no map: its record is zeros and reads as +1)
            assert (want.det[1:11:2] < 0).all() and (want.hand[odd] == -1).all() and (want.hand[2:11:2] == 1).all()
        else:
            assert (want.hand == 1).all()
    # the raw function: no sentinel, map 0 gives zeros
    corners = np.ascontiguousarray(recs[1:12, 20:29])
    uv6, fn, nm = np.ascontiguousarray(p.uvs[1:12]), np.ascontiguousarray(recs[1:12, 3:6]), np.ascontiguousarray(p.nm[1:12])
    fr = np.full((11, 4), 7.0, F32)
    assert L.rtmi_normal_map_frames(ptr(corners), ptr(uv6), ptr(fn), ptr(nm), 11, ptr(fr)) == 0
    want = NR.frames(recs[1:12, 20:29], p.uvs[1:12], recs[1:12, 3:6], p.nm[1:12])
    assert_bits_equal(fr[:, :3], want.T[:, :3], "rtmi_normal_map_frames")
    assert np.array_equal(np.ascontiguousarray(fr[:, 3]).view(np.uint32), want.nmap.astype(np.uint32))
    assert L.rtmi_normal_map_frames(None, ptr(uv6), ptr(fn), ptr(nm), 11, ptr(fr)) != 0
    assert L.rtmi_normal_map_frames(None, None, None, None, 0, None) == 0
    sp.clear_normal_maps()
    assert sp.normal_maps() is None and sp.textures() is not None


def test_canonical_scene_with_a_normal_map():
    import conftest as CT
    R = _R()
    nmap = R.normal_map_from_height(NC.heights())
    s = R.canonical_scene(CT.TEAPOT_TRI, normal_map=nmap)
    images, uvs, tot = s.textures()
    nm, strength = s.normal_maps()
    rec = s.triangles()[0]
    assert len(images) == 1 and not tot.any() and strength == 1.0
    assert (nm[1:6321] == 1).all() and nm[0] == 0 and not nm[6321:].any()
    assert_bits_equal(uvs[1:6321], TR.project(rec[1:6321, 20:29], rec[1:6321, 3:6], (0, 0, 0), 1.0), "the teapot is box-projected")
    s = R.canonical_scene(CT.TEAPOT_TRI, texture=NC.images()[3], normal_map=nmap, smooth=True)
    images, uvs, tot = s.textures()
    nm, _ = s.normal_maps()
    assert len(images) == 2 and (tot[1:6321] == 1).all() and (nm[1:6321] == 2).all()
    assert_bits_equal(images[1], nmap, "the map is the second image")
    T, hand, stored = s.normal_map_frames()
    want = NR.frames(rec[:, 20:29], uvs, rec[:, 3:6], nm)
    assert_bits_equal(T, want.T[:, :3], "the teapot's tangents")
    assert np.array_equal(hand, want.hand) and np.array_equal(stored, want.nmap)
    assert (hand[1:6321] == -1).sum() >= 1000 and (hand[1:6321] == 1).sum() >= 1000  # a box projection mirrors half of the faces


# ---------------------------------------------------------------- 6
def test_interface_refusals_that_need_no_gpu():
    import conftest as CT
    from rust_raytrace_amd import _ffi
    R, L = _R(), _lib()
    s = R.canonical_scene(CT.TEAPOT_TRI)
    n = s.num_tris()
    one = np.ones(5, np.uint32)
    with pytest.raises(RuntimeError, match="no textures"):
        s.set_normal_maps(one)
    assert s.normal_maps() is None
    s.set_textures(NC.images()[:2], None, None)
    s.project_uvs(1, 100)
    with pytest.raises(RuntimeError, match="above ntex"):
        s.set_normal_maps(np.array([1, 2, 3], np.uint32), first=4)
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(RuntimeError, match="strength"):
            s.set_normal_maps(one, strength=bad)
    with pytest.raises(RuntimeError, match="first"):
        s.set_normal_maps(one, first=0)
    with pytest.raises(RuntimeError, match="beyond"):
        s.set_normal_maps(one, first=n - 2)
    with pytest.raises(ValueError):
        s.set_normal_maps(np.zeros(0, np.uint32))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    with pytest.raises(RuntimeError, match="flags"):
        R._chk(L.rth_scene_set_normal_maps(s.h, p(one), 1, 5, 1.0, 1))
    assert s.normal_maps() is None  # none of them left anything behind
    s.set_normal_maps(np.array([2, 0, 1], np.uint32), first=7, strength=2.0)
    nm, strength = s.normal_maps()
    assert list(nm[6:11]) == [0, 2, 0, 1, 0] and strength == 2.0 and len(nm) == n
    s.set_textures(NC.images()[:3], None, None)  # new images: the numbers the maps named are gone
    assert s.normal_maps() is None and s.textures() is not None
    s.set_normal_maps(one)
    s.clear_textures()
    assert s.normal_maps() is None and s.textures() is None
    # null pointers through the raw ABI
    c9, nm = np.zeros((2, 9), F32), np.ones(2, np.uint32)
    n64, f = C.c_uint64(0), C.c_float(0)
    opt = _ffi.NormalMaps(0.0, 7)
    L.rtmi_normal_maps_defaults(C.byref(opt))
    assert opt.strength == 1.0 and opt.flags == 0
    L.rtmi_normal_maps_defaults(None)
    assert L.rtmi_scene_set_normal_maps(None, p(c9), p(nm), 2, None) != 0 and b"NULL" in L.rtmi_last_error()
    assert L.rtmi_scene_get_normal_maps(None, None, C.byref(f), C.byref(n64)) != 0


# ---------------------------------------------------------------- 7
def test_header_symbols_and_documents():
    from rust_raytrace_amd import _ffi
    text = open(os.path.join(ROOT, "include", "rtmi.h")).read()
    assert "NORMAL MAPS OF A SCENE" in text and "rtmi_normal_maps_t" in text
    assert text.index("TEXTURES OF A SCENE") < text.index("NORMAL MAPS OF A SCENE")
    for name in ("rtmi_scene_set_normal_maps", "rtmi_scene_get_normal_maps", "rtmi_normal_map_from_height", "rtmi_normal_map_frames"):
        assert re.search(r"\bint %s\(" % name, text) and name in _ffi.RTMI_SYMBOLS and hasattr(_ffi.lib(), name)
    assert re.search(r"\bvoid rtmi_normal_maps_defaults\(", text) and "rtmi_normal_maps_defaults" in _ffi.RTMI_SYMBOLS
    host = open(os.path.join(ROOT, "include", "rtmi_host.h")).read()
    for name in ("rth_scene_set_normal_maps", "rth_scene_normal_maps_size", "rth_scene_get_normal_maps", "rth_scene_normal_map_frames",
                 "rth_caster_normal_maps", "rth_normal_map_from_height"):
        assert name in host and name in _ffi.RTH_SYMBOLS and hasattr(_ffi.lib(), name)
    assert "4.26" in open(os.path.join(ROOT, "DESIGN.md")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "rtmi_scene_set_normal_maps" in doc and "rtmi_normal_map_from_height" in doc and "rtmi_normal_maps_t" in doc
    assert "normal map" in open(os.path.join(ROOT, "README.md")).read().lower()
