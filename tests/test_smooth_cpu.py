"""No GPU: the restatement of a scene's vertex normals (tests/smooth_ref.py) is pinned before tests/test_smooth.py trusts it, and
the host side of the feature -- the generator, the loader, the interface -- is tested where it runs.
 1. With no normals smooth_ref.path_trace is env_ref.path_trace, bit for bit, on the glass slab and on the canonical scene.
 2. `shading_normal` agrees with an independent float64 textbook evaluation -- barycentric coordinates by areas, the corner normals
    interpolated and normalised -- at random points of random non-degenerate triangles.  The margin is measured, not guessed:
    NORMAL_MEASURED is the largest deviation on the machine the test was written on and the test asserts 8 x that.
 3. At a corner the normal is that corner's within that margin; on a shared edge the two triangles agree (continuity).
 4. `generate` against the library's rtmi_smooth_normals, bit for bit: the teapot, a closed UV sphere from a shared vertex array
    (radial within a measured margin), a cube with crease_cos = 0.5 (every corner normal its face's within 1e-6), a mesh with
    one flipped face, crease_cos = 1 and -1, -0 against +0 and a NaN corner.
 5. The loader: normals="file" on a small OBJ written by the test (a/b/c and a//c), a missing index raises, the default mode
    returns byte-identical triangles.
 6. The interface: refusals that need no GPU, the header, the symbol lists.
 7. On a tessellated sphere the restated normal guide deviates from the analytic radial direction less with normals than without.
 8. The patch's rays (tests/smooth_cases.py) make every branch of the definition run: the condition tests/test_smooth.py asserts."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import conftest as CT
import env_ref as ER
import glass_cases as GC
import smooth_cases as SC
import smooth_ref as SR
from conftest import ROOT, assert_bits_equal
from rays_ref import vunit

F32 = np.float32
NORMAL_MEASURED = 3.647e-6  # largest |shading_normal_f32 - textbook_f64| (a component) over the sample, as measured
SPHERE_MEASURED = 4.748e-2  # largest |generated normal - radial direction| on the 12 x 16 UV sphere, as measured
GUIDE_RATIO_MEASURED = 0.323 # mean angular error of the smooth guide / of the flat one on that sphere, as measured


def _orc():
    from oracle import orc
    return orc


def _R():
    from rust_raytrace_amd import raytrace as R
    return R


def _lib():
    from rust_raytrace_amd import _ffi
    return _ffi.lib()


def _library_generate(corners, facenorm, crease_cos):
    c, f = np.ascontiguousarray(corners, F32).reshape(-1, 9), np.ascontiguousarray(facenorm, F32).reshape(-1, 3)
    out = np.full((len(c), 3, 3), 7.0, F32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = _lib().rtmi_smooth_normals(p(c), p(f), len(c), crease_cos, p(out))
    assert rc == 0, _lib().rtmi_last_error()
    return out


def _face_normals(corners):
    """Unit face normals in float32 from float64 cross products: what a record's `norm` is, up to rounding"""
    c = np.asarray(corners, np.float64)
    x = np.cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0])
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(F32)


# ---------------------------------------------------------------- 1
def _same(a, b, what):
    assert_bits_equal(a.color, b.color, what)
    assert_bits_equal(a.image, b.image, what + ": the images")
    assert a.rays == b.rays and a.passes == b.passes and a.pt.total == b.pt.total


def test_without_normals_the_restatement_is_env_ref_on_the_slab():
    orc = _orc()
    so, _ = GC.build_pair(GC.recipe_slab())
    w, h, spp, seed, maxdepth = 16, 16, 2, 5, 6
    vo = orc.canonical_viewport(w, h)
    want = ER.render(orc, so, vo, w, h, spp, seed, maxdepth)
    got = SR.render(orc, so, vo, w, h, spp, seed, maxdepth)
    _same(got, want, "smooth_ref against env_ref, the slab")
    assert want.pt.total["refract_in"] > 0 and not any(got.pt.smooth.values())
    # and all-zero normals: every triangle flat, the same bits through the smooth line
    zero = np.zeros((len(so.triangles()[0]), 3, 3), F32)
    flat = SR.render(orc, so, vo, w, h, spp, seed, maxdepth, normals=zero)
    _same(flat, want, "all-zero normals")
    assert flat.pt.smooth["flat"] > 0 and flat.pt.smooth["smooth"] == 0


def test_without_normals_the_restatement_is_env_ref_on_the_canonical_scene(canonical_pair):
    orc = _orc()
    so, _ = canonical_pair
    w, h, spp, seed, maxdepth = 16, 12, 2, 5, 5
    vo = orc.canonical_viewport(w, h)
    _same(SR.render(orc, so, vo, w, h, spp, seed, maxdepth), ER.render(orc, so, vo, w, h, spp, seed, maxdepth),
          "smooth_ref against env_ref, the canonical scene")


# ---------------------------------------------------------------- 2, 3
def _random_triangles(n, rng):
    """Non-degenerate triangles (smallest angle above ~10 degrees) with unit corner normals within 60 degrees of the face's"""
    out_c, out_n = [], []
    while len(out_c) < n:
        c = rng.uniform(-3, 3, (3, 3))
        e = [c[(k + 1) % 3] - c[k] for k in range(3)]
        ang = [np.arccos(np.clip(np.dot(-e[k - 1], e[k]) / np.linalg.norm(e[k - 1]) / np.linalg.norm(e[k]), -1, 1)) for k in range(3)]
        if min(ang) < 0.18:
            continue
        fn = np.cross(e[0], -e[2])
        fn /= np.linalg.norm(fn)
        nn = fn + rng.uniform(-0.8, 0.8, (3, 3))
        out_c.append(c)
        out_n.append(nn / np.linalg.norm(nn, axis=1, keepdims=True))
    return np.array(out_c).astype(F32), np.array(out_n).astype(F32)


def _textbook64(corners, normals, point):
    """Barycentric coordinates as ratios of signed areas, the corner normals interpolated and normalised: float64"""
    c, nn, p = np.asarray(corners, np.float64), np.asarray(normals, np.float64), np.asarray(point, np.float64)
    full = np.cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0])
    a2 = (full * full).sum(axis=1)
    area = lambda u, v, w: (np.cross(v - u, w - u) * full).sum(axis=1) / a2
    b0, b1, b2 = area(p, c[:, 1], c[:, 2]), area(c[:, 0], p, c[:, 2]), area(c[:, 0], c[:, 1], p)
    s = nn[:, 0] * b0[:, None] + nn[:, 1] * b1[:, None] + nn[:, 2] * b2[:, None]
    return s / np.linalg.norm(s, axis=1, keepdims=True)


def _eval(corners, normals, bary):
    """shading_normal's ns at the points of barycentric coordinates `bary` (n, 3), front face, and those points in float32"""
    rec = SR.records(corners, normals)
    p = (np.asarray(corners, np.float64) * np.asarray(bary, np.float64)[:, :, None]).sum(axis=1).astype(F32)
    n = len(p)
    ng = SR.v4(np.zeros((n, 3), F32))
    sn = SR.shading_normal(rec, np.arange(n), np.zeros(n, bool), SR.v4(p), SR.v4(np.zeros((n, 3), F32)), ng)
    return sn, p


def test_shading_normal_against_a_float64_textbook_evaluation():
    rng = np.random.default_rng(11)
    corners, normals = _random_triangles(4000, rng)
    bary = rng.dirichlet((1, 1, 1), len(corners))
    sn, p = _eval(corners, normals, bary)
    want = _textbook64(corners, normals, p)
    dev = np.abs(sn.ns[:, :3].astype(np.float64) - want).max()
    print(f"shading_normal: largest deviation from the float64 evaluation {dev:.3e} (recorded {NORMAL_MEASURED:.3e})")
    assert dev <= 8 * NORMAL_MEASURED
    assert (sn.ns[:, 3] == 0).all()


def test_at_a_corner_the_normal_is_the_corners_and_a_shared_edge_is_continuous():
    rng = np.random.default_rng(12)
    corners, normals = _random_triangles(600, rng)
    for k in range(3):
        bary = np.zeros((len(corners), 3))
        bary[:, k] = 1.0
        sn, _ = _eval(corners, normals, bary)
        # a corner rounded to float32 is the corner, so only the arithmetic's rounding is left
        assert np.abs(sn.ns[:, :3] - normals[:, k]).max() <= 8 * NORMAL_MEASURED
    # the neighbour over edge (c1, c2): corners (c2, c1, d) with the shared corners' normals
    d = (corners[:, 1] + corners[:, 2] - corners[:, 0] + rng.uniform(-0.3, 0.3, (len(corners), 3))).astype(F32)
    nd = normals[:, 0]
    other_c = np.stack([corners[:, 2], corners[:, 1], d], axis=1)
    other_n = np.stack([normals[:, 2], normals[:, 1], nd], axis=1)
    t = rng.uniform(0.05, 0.95, len(corners))
    p = (corners[:, 1].astype(np.float64) * (1 - t)[:, None] + corners[:, 2].astype(np.float64) * t[:, None]).astype(F32)
    z = np.zeros(len(p), bool)
    zero4 = SR.v4(np.zeros((len(p), 3), F32))
    a = SR.shading_normal(SR.records(corners, normals), np.arange(len(p)), z, SR.v4(p), zero4, zero4).ns
    b = SR.shading_normal(SR.records(other_c, other_n), np.arange(len(p)), z, SR.v4(p), zero4, zero4).ns
    # the same point, rounded once, seen from both triangles: both are within the margin of the same float64 value, and a point
    # that is a rounding error off the edge moves the normal by |dn/dp| * 1e-7, far below it
    assert np.abs(a - b).max() <= 16 * NORMAL_MEASURED


# ---------------------------------------------------------------- 4
def test_generate_is_the_librarys_on_the_teapot(canonical_pair):
    so, sp = canonical_pair
    rec = so.triangles()[0]
    corners, fn = rec[1:6321, 20:29], rec[1:6321, 3:6]
    want = SR.generate(corners, fn, 0.5)
    assert_bits_equal(_library_generate(corners, fn, 0.5), want, "rtmi_smooth_normals on the teapot")
    assert np.isfinite(want).all() and np.abs(np.linalg.norm(want.astype(np.float64), axis=2) - 1).max() < 1e-6
    # 6 320 faces over 3 644 shared vertices: nearly every corner's normal differs from its face's
    assert (np.abs(want - fn[:, None, :]).max(axis=2) > 1e-4).mean() > 0.95
    # through the scene: Scene.smooth_normals on a range, the rest flat; appended triangles flat
    R = _R()
    s = R.canonical_scene(CT.TEAPOT_TRI, smooth=True)
    got = s.vertex_normals()
    assert got.shape == (s.num_tris(), 3, 3) and not got[0].any() and not got[6321:].any()
    assert_bits_equal(got[1:6321], want, "canonical_scene(smooth=True)")
    s.push_triangle(np.array([[0, 0, 1], [1, 0, 1], [0, 1, 1.5]], F32), R.SurfaceKind.Solid(R.make_color(1, 2, 3)), 0.0)
    again = s.vertex_normals()
    assert again.shape == (s.num_tris(), 3, 3) and not again[-1].any()
    assert R.canonical_scene(CT.TEAPOT_TRI).vertex_normals() is None


def test_generate_on_a_closed_sphere_is_radial():
    corners = SC.uv_sphere(12, 16)
    fn = _face_normals(corners)
    want = SR.generate(corners, fn, 0.5)
    assert_bits_equal(_library_generate(corners, fn, 0.5), want, "rtmi_smooth_normals on the UV sphere")
    radial = corners.astype(np.float64) / np.linalg.norm(corners.astype(np.float64), axis=2, keepdims=True)
    dev = np.abs(want - radial).max()
    print(f"UV sphere 12 x 16: largest deviation of a generated normal from the radial direction {dev:.3e} (recorded {SPHERE_MEASURED:.3e})")
    assert dev <= 8 * SPHERE_MEASURED
    assert np.abs(fn[:, None, :] - radial).max() > 3 * dev  # the faces' own normals are much further from it


def test_generate_on_a_cube_keeps_the_creases():
    corners = np.array(GC.box_triangles((-1.0, -2.0, 0.5), (2.0, 1.0, 3.0)), F32)
    fn = _face_normals(corners)
    want = SR.generate(corners, fn, 0.5)
    assert_bits_equal(_library_generate(corners, fn, 0.5), want, "the cube, crease_cos = 0.5")
    assert np.abs(want - fn[:, None, :]).max() <= 1e-6
    for cc in (1.0, -1.0):
        w = SR.generate(corners, fn, cc)
        assert_bits_equal(_library_generate(corners, fn, cc), w, f"the cube, crease_cos = {cc}")
    assert np.abs(SR.generate(corners, fn, 1.0) - fn[:, None, :]).max() <= 1e-6
    # crease_cos = -1: a corner's normal is the mean of the faces that meet there, weighted by area and by how many triangles of
    # a face touch the corner; it always points out of the corner's octant
    soft = SR.generate(corners, fn, -1.0)
    centre = np.array([0.5, -0.5, 1.75])
    assert (np.sign(soft) == np.sign(corners - centre)).all()


def test_generate_with_a_flipped_face_minus_zero_and_nan():
    corners = SC.uv_sphere(6, 8).copy()
    fn = _face_normals(corners)
    corners[5] = corners[5][[0, 2, 1]]  # one face wound the other way ...
    fn[5] = -fn[5]                      # ... and its record normal with it
    for cc in (0.5, -1.0):
        want = SR.generate(corners, fn, cc)
        assert_bits_equal(_library_generate(corners, fn, cc), want, f"a flipped face, crease_cos = {cc}")
    kept = SR.generate(corners, fn, 0.5)
    assert np.abs(kept[5] - fn[5]).max() <= 1e-6  # the flipped face is a crease to all its neighbours: it keeps its own normal
    # -0 == +0: the poles (0, 0, +-1) written with -0 in one triangle still share their corner; a NaN corner shares nothing
    c2 = SC.uv_sphere(6, 8).copy()
    f2 = _face_normals(c2)
    pole = np.argwhere((c2[:, :, 0] == 0) & (c2[:, :, 1] == 0))
    assert len(pole) >= 8
    c2[pole[0][0], pole[0][1], 0] = F32(-0.0)
    base = SR.generate(SC.uv_sphere(6, 8), f2, 0.5)
    w2 = SR.generate(c2, f2, 0.5)
    assert_bits_equal(w2, base, "-0 in a corner changes nothing")
    assert_bits_equal(_library_generate(c2, f2, 0.5), w2, "-0 in a corner, the library")
    c2[3, 1, 2] = np.nan
    with np.errstate(all="ignore"):
        w3 = SR.generate(c2, f2, 0.5)
    got = _library_generate(c2, f2, 0.5)
    assert np.isnan(w3[3, 1]).all() and np.isnan(got[3, 1]).all()
    ok = ~np.isnan(w3)
    assert (np.isnan(got) == np.isnan(w3)).all() and (got[ok].view(np.uint32) == w3[ok].view(np.uint32)).all()


# ---------------------------------------------------------------- 5
OBJ = """# a quad and a triangle
v 0 0 0
v 1 0 0
v 1 1 0.2
v 0 1 0.1
v 2 0.5 0.4
vn 0 0 2
vn 0.3 0 1
vn 0 0.4 1
vn -0.2 -0.2 1
vt 0 0
f 1/1/1 2/1/2 3/1/3
f 1//1 3//3 4//4
f 2//2 5//4 3//3
"""


def test_the_loader_reads_vn_and_the_default_is_untouched(tmp_path):
    R = _R()
    path = tmp_path / "mesh.obj"
    path.write_text(OBJ)
    tr = R.create_transform(R.unit([0.2, 0.3, 1.0]), R.to_radians(40.0))
    surf = R.SurfaceKind.Matte(R.make_color(10, 20, 30), 0.5)

    def load(**kw):
        s = R.Scene(with_dummy=True)
        s.extend_parse_obj(str(path), [0.5, -0.25, 3.0], 2.0, tr, surf, 0.0, **kw)
        return s
    plain = load()
    assert plain.vertex_normals() is None and plain.num_tris() == 4
    for robust in (False, True):
        s = load(normals="file", robust=robust)
        for a, b in zip(s.triangles(), plain.triangles()):
            assert a.tobytes() == b.tobytes()  # the triangles are the default loader's, byte for byte
        got = s.vertex_normals()
        vn = np.array([[0, 0, 2], [0.3, 0, 1], [0, 0.4, 1], [-0.2, -0.2, 1]], F32)
        basis = np.asarray(tr, F32).reshape(3, 3)
        want = np.zeros((4, 3, 3), F32)
        for f, idx in enumerate(((1, 2, 3), (1, 3, 4), (2, 4, 3)), start=1):
            for k, i in enumerate(idx):
                v = basis.astype(np.float64) @ vn[i - 1].astype(np.float64)  # change_basis: (b0 . v, b1 . v, b2 . v)
                want[f, k] = v / np.linalg.norm(v)
        assert np.abs(got - want).max() < 1e-6 and not got[0].any()
        assert np.abs(np.linalg.norm(got[1:].astype(np.float64), axis=2) - 1).max() < 1e-6  # unit: no scale, no offset
    sm = load(normals="smooth", crease_cos=-1.0)
    rec = sm.triangles()[0]
    assert_bits_equal(sm.vertex_normals()[1:], SR.generate(rec[1:, 20:29], rec[1:, 3:6], -1.0), "normals='smooth' through the loader")
    # a corner without a normal index
    bad = tmp_path / "bad.obj"
    bad.write_text(OBJ.replace("f 2//2 5//4 3//3", "f 2//2 5 3//3"))
    s = R.Scene(with_dummy=True)
    with pytest.raises(RuntimeError, match="normal index"):
        s.extend_parse_obj(str(bad), [0, 0, 3.0], 1.0, tr, surf, 0.0, normals="file")
    s.extend_parse_obj(str(bad), [0, 0, 3.0], 1.0, tr, surf, 0.0)  # the default mode never looks at the third field
    assert s.num_tris() == 4
    with pytest.raises(ValueError):
        s.extend_parse_obj(str(path), [0, 0, 3.0], 1.0, tr, surf, 0.0, normals="vn")
    # the project's own file: 4 441 vn lines, every face naming one of them at all three corners
    t = R.Scene(with_dummy=True)
    t.extend_parse_obj(CT.TEAPOT_TRI, [0.0, 0.5, 5.0], 1.0, tr, surf, 0.05, normals="file")
    n = t.vertex_normals()
    assert n.shape == (6321, 3, 3) and (n[1:, 0] == n[1:, 1]).all() and (n[1:, 0] == n[1:, 2]).all()


# ---------------------------------------------------------------- 6
def test_interface_refusals_that_need_no_gpu():
    R, L = _R(), _lib()
    s = R.canonical_scene(CT.TEAPOT_TRI)
    n = s.num_tris()
    for cc in (1.5, -1.5, float("nan")):
        with pytest.raises(RuntimeError, match="crease_cos"):
            s.smooth_normals(1, 10, crease_cos=cc)
    with pytest.raises(RuntimeError, match="first"):
        s.smooth_normals(0, 10)
    with pytest.raises(RuntimeError, match="beyond"):
        s.smooth_normals(5, n)
    with pytest.raises(ValueError):
        s.set_vertex_normals(np.zeros((4, 9), F32))
    bad = np.zeros((3, 3, 3), F32)
    bad[1, 2, 0] = np.inf
    with pytest.raises(RuntimeError, match="not finite"):
        s.set_vertex_normals(bad, first=7)
    with pytest.raises(RuntimeError, match="beyond"):
        s.set_vertex_normals(np.zeros((3, 3, 3), F32), first=n - 1)
    assert s.vertex_normals() is None  # none of them left anything behind
    s.set_vertex_normals(np.full((2, 3, 3), 0.5, F32), first=3)
    got = s.vertex_normals()
    assert got.shape == (n, 3, 3) and (got[3:5] == 0.5).all() and not got[:3].any() and not got[5:].any()
    s.clear_vertex_normals()
    assert s.vertex_normals() is None
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    c9, f3, o9 = np.zeros((2, 9), F32), np.zeros((2, 3), F32), np.zeros((2, 9), F32)
    assert L.rtmi_smooth_normals(p(c9), p(f3), 2, 2.0, p(o9)) != 0 and b"crease_cos" in L.rtmi_last_error()
    assert L.rtmi_smooth_normals(None, p(f3), 2, 0.5, p(o9)) != 0
    assert L.rtmi_smooth_normals(None, None, 0, 0.5, None) == 0
    assert L.rtmi_scene_set_normals(None, p(c9), p(o9), 2) != 0 and L.rtmi_scene_get_normals(None, None, None) != 0


def test_header_symbols_and_documents():
    from rust_raytrace_amd import _ffi
    text = open(os.path.join(ROOT, "include", "rtmi.h")).read()
    assert "VERTEX NORMALS OF A SCENE" in text
    for name in ("rtmi_scene_set_normals", "rtmi_scene_get_normals", "rtmi_smooth_normals"):
        assert re.search(r"\bint %s\(" % name, text) and name in _ffi.RTMI_SYMBOLS and hasattr(_ffi.lib(), name)
    host = open(os.path.join(ROOT, "include", "rtmi_host.h")).read()
    for name in ("rth_scene_set_normals", "rth_scene_smooth_normals", "rth_scene_normals_size", "rth_scene_get_normals", "rth_caster_normals",
                 "rth_add_obj_normals"):
        assert name in host and name in _ffi.RTH_SYMBOLS and hasattr(_ffi.lib(), name)
    assert "4.24" in open(os.path.join(ROOT, "DESIGN.md")).read()


# ---------------------------------------------------------------- 7
def test_the_smooth_guide_is_closer_to_the_true_sphere_than_the_flat_one():
    orc = _orc()
    centre = np.array([2.0, 0.0, 4.0])
    corners = SC.uv_sphere(12, 16, 1.5, centre)

    def recipe(api):
        s = api.scene()
        for t in corners:
            api.add_triangle(s, t, api.matte((200, 200, 200), 0.5), 0.0)
        s.populate_triangle_numbers()
        s.build_bounding_box([2.0, 0.0, 4.0], 4.0, 4, 8)
        return s
    so = recipe(CT.OracleApi(orc))
    rec = so.triangles()[0]
    nrm = np.zeros((len(rec), 3, 3), F32)
    nrm[1:] = SR.generate(rec[1:, 20:29], rec[1:, 3:6], 0.5)
    w = h = 48
    vo = orc.canonical_viewport(w, h)
    o4, d4, npix, n = SR.FR.tile_rays(orc, w, h, vo, 1, 5)
    hn = SR.hit_normals(so, nrm, o4, d4)
    hit = hn.ok
    assert hit.sum() > 100 and hn.use[hit].mean() > 0.95
    point = o4[hit, :3].astype(np.float64) + d4[hit, :3].astype(np.float64) * hn.t[hit, None]
    radial = (point - centre) / np.linalg.norm(point - centre, axis=1, keepdims=True)
    ang = lambda v: np.degrees(np.arccos(np.clip((v[:, :3].astype(np.float64) * radial).sum(axis=1), -1, 1)))
    smooth, flat = ang(hn.norm[hit]).mean(), ang(hn.ng[hit]).mean()
    print(f"UV sphere 12 x 16: mean angle to the radial direction {smooth:.3f} deg smooth, {flat:.3f} deg flat, ratio {smooth / flat:.3f} "
          f"(recorded {GUIDE_RATIO_MEASURED})")
    assert smooth < flat


# ---------------------------------------------------------------- 8
def test_the_patchs_rays_run_every_branch():
    orc = _orc()
    so, sp = GC.build_pair(SC.recipe_patch())
    for a, b in zip(so.triangles(), sp.triangles()):
        assert a.tobytes() == b.tobytes()
    nrm = SC.patch_normals(so.triangles()[0])
    assert not nrm[8].any() and not nrm[SC.NTRI_PATCH + 1:].any() and nrm[1:8].any(axis=(1, 2)).all()
    # the shared corners B and C carry one normal in both triangles of a pair
    for k in range(3):
        assert (nrm[1 + 2 * k, 1] == nrm[2 + 2 * k, 0]).all() and (nrm[1 + 2 * k, 2] == nrm[2 + 2 * k, 2]).all()
    ng = so.triangles()[0][1:8, 3:6]
    tilt = np.degrees(np.arccos((nrm[1:8].astype(np.float64) * ng[:, None, :]).sum(axis=2)))
    assert tilt.min() > 20 and tilt.max() < 75  # strongly tilted
    o4, d4 = SC.patch_rays()
    hn = SR.hit_normals(so, nrm, o4, d4)
    assert hn.use.sum() >= 100 and hn.flat.sum() >= 50 and hn.away_from_ng.sum() >= 20 and hn.away_from_ray.sum() >= 50
    assert ((hn.face & 1) != 0).sum() >= 100 and (hn.tri == 0).any() and not (hn.face & 2).any()
    hit = np.bincount(hn.tri, minlength=SC.NTRI_PATCH + 1)
    assert (hit[1:SC.NTRI_PATCH + 1] >= 50).all()
    n = len(o4)
    pt = SR.path_trace(orc, so, o4, d4, np.arange(n), np.zeros(n, np.int64), 3, 5, normals=nrm)
    c = pt.smooth
    assert c["smooth"] >= 100 and c["flat"] >= 100 and c["away_from_ng"] >= 20 and c["away_from_ray"] >= 50, c
    assert min(c["fallback_matte"], c["fallback_reflective"], c["fallback_glass_reflect"], c["fallback_glass_refract"]) >= 1, c
    # a path that fell back left the surface on the side it should: its next ray starts there
    assert pt.total["refract_in"] >= 1 and pt.total["refract_out"] >= 1
