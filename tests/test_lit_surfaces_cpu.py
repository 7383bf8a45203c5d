"""No GPU: box lights on shaded surfaces (RTMI_LIT_SURFACES; include/rtmi.h "BOX LIGHTS ON SHADED SURFACES") as
tests/lit_surfaces_ref.py restates them.  First the flag through the raw ABI.  Then the restatement's footing: on an unfeatured scene
it is lit_ref's, with the lamps off it is nmap_ref's, bit for bit.  Then what the definition must mean physically, held by a float64
referee on a smooth sphere: a point light gives light_color * g with g from the interpolated normal.  Last, the case mix of the
recipes tests/test_lit_surfaces.py renders (tests/lit_surfaces_cases.py), checked on the restatement alone."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import conftest as CT
import glass_cases as GC
import lit_ref as LT
import lit_surfaces_cases as LC
import lit_surfaces_ref as LS
import nmap_cases as NC
import nmap_ref as NR
import smooth_cases as SC

F32 = np.float32
SEED = LC.SEED
DARK = SimpleNamespace(table=np.zeros((4, 4, 3), F32), frame=None)  # an all-zero environment: a path that escapes brings nothing
# test_a_point_light_on_a_smooth_sphere_is_the_float64_formula: the largest relative deviation measured there, times 4
REL_F32 = 4 * 1.33e-5


def _orc():
    from oracle import orc
    return orc


@pytest.fixture(scope="module")
def teapot():
    so = CT.recipe_canonical()(CT.OracleApi(_orc()))
    return so, LC.teapot_inputs(so)


@pytest.fixture(scope="module")
def patch():
    so = NC.recipe_patch()(CT.OracleApi(_orc()))
    return so, LC.patch_inputs(so)


# ---------------------------------------------------------------- the flag, before any HIP call
def test_the_flag_is_declared_accepted_and_bit_1_is_still_refused():
    import test_bake_lit_cpu as TB
    from rust_raytrace_amd import _ffi
    from rust_raytrace_amd import raytrace as R
    L = _ffi.lib()
    assert _ffi.LIT_SURFACES == 4 == LS.SURFACES == R.HipRayCaster.LIT_SURFACES
    text = open(CT.os.path.join(CT.ROOT, "include", "rtmi.h")).read()
    assert "RTMI_LIT_SURFACES = 1u << 2" in text and "BOX LIGHTS ON SHADED SURFACES" in text
    c = R.HipRayCaster
    assert c.lit_params([LT.A]).flags == 0 and c.lit_params([LT.A], surfaces=True).flags == 4
    assert c.lit_params([LT.A], True, True).flags == 5 and c.lit_params([LT.A], inverse_square=True).flags == 1
    bogus, acc, out = C.c_void_p(0x10), C.c_void_p(0x100000), C.c_void_p(0x200000)

    class Vp(C.Structure):
        _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("orig", C.c_float * 3), ("cam", C.c_float * 3), ("vu", C.c_float * 3),
                    ("vv", C.c_float * 3), ("maxdepth", C.c_uint32), ("samples_per_pixel", C.c_uint32)]
    v = Vp()
    v.width, v.height, v.maxdepth, v.samples_per_pixel = 8, 8, 4, 4

    def frame(flags):
        """(rc, message, stats.rays) of both frame variants on an EMPTY tile: reached only past every parameter check, and the
        dangling scene handle is never dereferenced"""
        a = TB._lit(lit_flags=flags)
        res = []
        for dev in (True, False):
            st = _ffi.Stats()
            st.rays = 123
            if dev:
                t = _ffi.Tile(0, 0, 1, 0)
                rc = L.rtmi_render_lit_device(bogus, C.byref(v), 7, C.byref(t), 0, 4, C.byref(a), acc, out, None, C.byref(st))
            else:
                rc = L.rtmi_render_lit(bogus, C.byref(v), 7, 0, 0, 0, 4, C.byref(a), acc, out, C.byref(st))
            res.append((rc, L.rtmi_last_error(), st.rays))
        return res
    for flags in (0, 1, 4, 5):
        for rc, _, rays in frame(flags):
            assert rc == 0 and rays == 0, flags
    for flags in (2, 3, 6, 7, 8, 12, 1 << 31, (1 << 31) | 4):  # bit 1 and every bit above bit 2 stay unknown, with or without the new one
        for rc, msg, rays in frame(flags):
            assert rc == 1 and b"lit: unknown flags" in msg and rays == 0, (flags, msg)
        for rc, msg, rays in TB.rays_both(lit=TB._lit(lit_flags=flags)) + TB.bake_both(lit=TB._lit(lit_flags=flags)):
            assert rc == 1 and b"lit: unknown flags" in msg and rays == 0, (flags, msg)


# ---------------------------------------------------------------- the restatement against the old definitions
def test_on_an_unfeatured_scene_the_restatement_is_lit_refs(teapot):
    orc = _orc()
    so, _ = teapot
    vo = orc.canonical_viewport(32, 32)
    for lights, inv in ((LC.AB, False), (LC.FOUR, True)):
        old = LT.render(orc, so, vo, 32, 32, 4, SEED, 4, lights, inv)
        new = LS.render(orc, so, vo, 32, 32, 4, SEED, 4, lights, inv)
        CT.assert_bits_equal(new.image, old.image, "unfeatured scene: image")
        CT.assert_bits_equal(new.accum, old.accum, "unfeatured scene: accum")
        assert (new.rays, new.nlive, new.passes) == (old.rays, old.nlive, old.passes) and new.pt.live == old.live
        assert new.pt.occluded == old.occluded and LS.total(new.pt, "differs") == 0 and LS.total(new.pt, "culled_ng") == 0
    sky = SimpleNamespace(table=LT.ER.sky_table(8, dict(sun_dir=(-0.75, 0.25, 0.6), sun_cos=0.95, sun_color=(30.0, 24.0, 16.0))), frame=None)
    old = LT.render(orc, so, vo, 32, 32, 2, SEED, 3, LC.AB, env=sky)
    new = LS.render(orc, so, vo, 32, 32, 2, SEED, 3, LC.AB, env=sky)
    CT.assert_bits_equal(new.image, old.image, "unfeatured scene under a sky")


def test_with_the_lamps_off_the_restatement_is_nmap_refs(teapot, patch):
    orc = _orc()
    so, t = teapot
    vo = orc.canonical_viewport(32, 32)
    old = NR.render(orc, so, vo, 32, 32, 4, SEED, 4, normals=t.normals, tex=t.tex, nm=t.nm)
    new = LS.render(orc, so, vo, 32, 32, 4, SEED, 4, (), normals=t.normals, tex=t.tex, nm=t.nm)
    lit = LS.render(orc, so, vo, 32, 32, 4, SEED, 4, LC.AB, normals=t.normals, tex=t.tex, nm=t.nm)
    CT.assert_bits_equal(new.image, old.image, "featured teapot, no lamps")
    assert new.rays == old.rays == lit.rays and new.passes == old.passes == lit.passes  # the lamps move no path
    assert not np.array_equal(lit.image, old.image)
    so, p = patch
    vo = LC.patch_view(orc)
    old = NR.render(orc, so, vo, 16, 16, 2, SEED, 3, normals=p.normals, tex=p.tex, nm=p.nm)
    new = LS.render(orc, so, vo, 16, 16, 2, SEED, 3, (), normals=p.normals, tex=p.tex, nm=p.nm)
    CT.assert_bits_equal(new.image, old.image, "featured patch (glass among its kinds), no lamps")
    assert new.rays == old.rays


# ---------------------------------------------------------------- the float64 referee on a smooth sphere
CENTRE, RADIUS = np.array([2.0, 0.0, 4.0]), 1.5
SPHERE_LIGHT = (2.4, 0.5, -3.0)  # behind the camera, a little off its axis: it sees more of the sphere than the camera does
SPHERE_COLOR = (0.9, 0.7, 0.5)
SPHERE_COLOR_SQ = (45.0, 35.0, 25.0)  # ... with RTMI_LIT_INVERSE_SQUARE: d2 is about 30 to 50 here


def _sphere():
    corners = SC.uv_sphere(12, 16, RADIUS, CENTRE)

    def recipe(api):
        s = api.scene()
        for t in corners:
            api.add_triangle(s, t, api.matte((200, 200, 200), 1.0), 0.0)
        s.populate_triangle_numbers()
        s.build_bounding_box([2.0, 0.0, 4.0], 4.0, 4, 8)
        return s
    so = recipe(CT.OracleApi(_orc()))
    rec = so.triangles()[0]
    nrm = np.zeros((len(rec), 3, 3), F32)
    c = rec[1:, 20:29].reshape(-1, 3, 3).astype(np.float64) - CENTRE
    nrm[1:] = (c / np.linalg.norm(c, axis=2, keepdims=True)).astype(F32)  # exact vertex normals: radial
    return so, nrm


@pytest.mark.parametrize("inverse_square", [False, True], ids=["cosine", "inverse square"])
def test_a_point_light_on_a_smooth_sphere_is_the_float64_formula(inverse_square):
    """S = 1 (no jitter), depth 2, alpha = 1, an all-zero environment: a covered pixel whose candidate is live is light_color * g (the
    convex sphere shadows nothing; what the bounce brings back is 0, escaped or black at the exhausted level).  g in float64 from the
    float64 interpolated normal (the definition's N, with `use` evaluated in float64) at the float64 hit point; live in float64 when
    N . dir > 0 and ng . dir > 0.  Pixels whose float32 and float64 liveness (or `use`) disagree are left out; their share is printed
    and capped at 2 % of the covered pixels.  Measured on the 64 x 64 frame: 392 covered pixels, 387 compared (the other 5 are
    back-face hits through the seam between two facets), none left out; the largest relative deviation over the compared pixels and
    three channels is 1.24e-5 (g = c) and 1.32e-5 (g = c / d2), at the rim, where c falls to 0.085 and the float32 hit point's
    error moves the interpolated normal; asserted at four times the largest, REL_F32 = 5.32e-5.  The flat normal's g is off by
    more than a thousand times that."""
    orc = _orc()
    so, nrm = _sphere()
    w = h = 64
    li = LT.light(SPHERE_LIGHT, 0.0, SPHERE_COLOR_SQ if inverse_square else SPHERE_COLOR)
    r = LS.render(orc, so, orc.canonical_viewport(w, h), w, h, 1, SEED, 2, [li], inverse_square, env=DARK, normals=nrm, keep=True)
    tri, _, face = r.pt.hits0
    cov = (tri != 0) & ((face & 2) == 0)
    cand = r.pt.cand[0][0]
    assert np.array_equal(cand["idx"], np.nonzero(cov)[0]) and cov.sum() > 300  # every covered pixel is a Matte hit that bounces
    # (a few rays slip between two facets and meet the sphere from inside: back-face hits, shadowed by the sphere itself)
    seen = np.ones(len(cand["live"]), bool)
    seen[np.nonzero(cand["live"])[0][cand["occ"] != 0]] = False
    assert LS.total(r.pt, "occluded") <= 0.02 * cov.sum() and LS.total(r.pt, "occluded") == LS.total(r.pt, "back")
    # float64: the hit point on the triangle's plane, its barycentrics, the interpolated normal
    rec = so.triangles()[0]
    k = tri[cov]
    c0, c1, c2 = (rec[k, 20 + 3 * i:23 + 3 * i].astype(np.float64) for i in range(3))
    o, d = r.o4[cov, :3].astype(np.float64), r.d4[cov, :3].astype(np.float64)
    e1, e2 = c1 - c0, c2 - c0
    ng = np.cross(e1, e2)
    ng /= np.linalg.norm(ng, axis=1, keepdims=True)
    t = ((c0 - o) * ng).sum(1) / (d * ng).sum(1)
    p = o + t[:, None] * d
    ng = np.where(((ng * d).sum(1) > 0)[:, None], -ng, ng)
    wv = p - c0
    d00, d01, d11, d20, d21 = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1), (wv * e1).sum(1), (wv * e2).sum(1)
    den = d00 * d11 - d01 * d01
    b1, b2 = (d11 * d20 - d01 * d21) / den, (d00 * d21 - d01 * d20) / den
    n0, n1, n2 = (nrm[k, i].astype(np.float64) for i in range(3))
    ns = n0 * (1 - b1 - b2)[:, None] + n1 * b1[:, None] + n2 * b2[:, None]
    ns /= np.linalg.norm(ns, axis=1, keepdims=True)
    ns = np.where((face[cov] & 1 != 0)[:, None], -ns, ns)
    use64 = ((ns * ng).sum(1) > 0) & ((d * ns).sum(1) < 0)
    N = np.where(use64[:, None], ns, ng)
    v = np.asarray(li["orig"], np.float64) - p
    d2 = (v * v).sum(1)
    dirs = v / np.sqrt(d2)[:, None]
    c = (N * dirs).sum(1)
    live64 = (c > 0) & ((ng * dirs).sum(1) > 0)
    use32 = (cand["N"].view(np.uint32) != cand["ng"].view(np.uint32)).any(axis=1)
    both = live64 & cand["live"] & (use32 == use64) & seen
    out = (live64 != cand["live"]) | (use32 != use64)
    print(f"smooth sphere, inverse_square={inverse_square}: {int(cov.sum())} covered, {int(both.sum())} compared, left out {out.mean():.4f}, "
          f"shading normal used at {use32.mean():.3f}, smallest c {c[both].min():.3f}")
    assert out.mean() <= 0.02 and both.mean() > 0.9 and use32.mean() > 0.9
    g = c / d2 if inverse_square else c
    want = np.asarray(li["color"], np.float64)[None, :] * g[:, None]
    got = r.image.reshape(-1, 4)[cov, :3].astype(np.float64)
    dev = float(np.abs(got[both] / want[both] - 1).max())
    print(f"point light on a smooth sphere, inverse_square={inverse_square}: largest relative deviation {dev:.3e}")
    assert dev <= REL_F32
    # the flat normal would not do: the referee tells the two apart by far more than the bound
    gflat = (ng * dirs).sum(1) / (d2 if inverse_square else 1.0)
    assert np.abs(gflat[both] / g[both] - 1).max() > 1000 * REL_F32


# ---------------------------------------------------------------- the case mix of the GPU file's recipes
def _mix(pt):
    n = LS.total(pt, "candidates", 0)
    return n, {k: LS.total(pt, k, 0) / n for k in ("culled_n", "occluded", "visible", "differs")}


def test_the_gpu_cases_conditions_hold_on_the_restatement(teapot, patch):
    orc = _orc()
    kinds = dict(culled_ng=0, mapped=0, back=0)
    # the featured patch at 16 x 16, 2 samples, depths 1, 2, 3
    so, p = patch
    vo = LC.patch_view(orc)
    c = LC.PATCH
    for depth in c["depths"]:
        r = LS.render(orc, so, vo, c["w"], c["h"], c["spp"], SEED, depth, LC.AB, normals=p.normals, tex=p.tex, nm=p.nm)
        assert LS.total(r.pt, "candidates", depth - 1) == 0 and LS.total(r.pt, "live", depth - 1) == 0  # none at the exhausted level
        if depth == 1:
            assert r.nlive == 0
    n, share = _mix(r.pt)
    print(f"patch, depth 3: {n} level-0 candidates, shares {share}; live per level {[sum(x) for x in r.pt.live]}; kinds {r.pt.kinds[0]}; "
          f"textured Matte levels with light {r.pt.lit_textured}")
    assert n > 200 and share["culled_n"] >= 0.05 and share["occluded"] >= 0.05 and share["visible"] >= 0.05 and share["differs"] >= 0.25
    assert LS.total(r.pt, "live", 1) > 0 and r.pt.kinds[0]["reflective"] > 0 and r.pt.kinds[0]["glass"] > 0 and r.pt.lit_textured[0] > 0
    for k in kinds:
        kinds[k] += LS.total(r.pt, k)
    # the featured teapot at 32 x 32, 4 samples, lights A and B
    so, t = teapot
    c = LC.TEAPOT
    r = LS.render(orc, so, orc.canonical_viewport(c["w"], c["h"]), c["w"], c["h"], c["spp"], SEED, c["depth"], LC.AB, normals=t.normals, tex=t.tex,
                  nm=t.nm)
    n, share = _mix(r.pt)
    print(f"teapot: {n} level-0 candidates, shares {share}; live per level {[sum(x) for x in r.pt.live]}; kinds {r.pt.kinds[0]}; "
          f"textured Matte levels with light {r.pt.lit_textured}")
    assert n > 300 and share["culled_n"] >= 0.05 and share["occluded"] >= 0.05 and share["visible"] >= 0.05 and share["differs"] >= 0.25
    assert LS.total(r.pt, "live", 1) > 0 and LS.total(r.pt, "live", 2) > 0
    assert LS.total(r.pt, "candidates", c["depth"] - 1) == 0 and LS.total(r.pt, "live", c["depth"] - 1) == 0
    assert r.pt.kinds[0]["reflective"] > 0 and sum(r.pt.lit_textured) > 0
    for k in kinds:
        kinds[k] += LS.total(r.pt, k)
    print(f"both recipes: {kinds}")
    assert all(x >= 8 for x in kinds.values()), kinds
    four = LS.render(orc, so, orc.canonical_viewport(32, 32), 32, 32, 4, SEED, 4, LC.FOUR, True, normals=t.normals, tex=t.tex, nm=t.nm)
    assert all(four.pt.live[0][l] > 0 and four.pt.visible[0][l] > 0 for l in range(4))
    # the glass slab: a Dielectric level carries direct = 0, and every candidate whose segment crosses the slab is occluded
    # (the linear list: in the reference's octree a shadow ray can miss the slab's large faces, which reach outside the root box)
    so = GC.recipe_slab(accel="trivial")(CT.OracleApi(orc))
    c = LC.SLAB
    r = LS.render(orc, so, orc.canonical_viewport(c["w"], c["h"]), c["w"], c["h"], c["spp"], SEED, c["depth"], [LC.SLAB_LAMP], keep=True)
    assert r.pt.kinds[0]["glass"] > 20 and r.pt.kinds[0]["matte"] > 20
    ncross = 0
    for j in range(c["depth"] - 1):
        cd = r.pt.cand[j][0]
        if cd is None:
            continue
        lamp = cd["o"][:, :3].astype(np.float64) + cd["dir"][:, :3].astype(np.float64) * cd["r"][:, None].astype(np.float64)
        cross = LC.crosses_slab(cd["o"][:, :3], lamp, shrink=1e-3)[cd["live"]]
        ncross += int(cross.sum())
        assert (cd["occ"][cross] != 0).all()
    print(f"slab: kinds {r.pt.kinds[0]}, {ncross} live candidates cross the slab, visible per level {[sum(x) for x in r.pt.visible]}")
    assert ncross >= 20 and LS.total(r.pt, "visible") >= 20
