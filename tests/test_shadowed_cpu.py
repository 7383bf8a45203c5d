"""The shadowed path-trace (rtmi_render_shadowed / rtmi_render_shadowed_device): the entry points exist and are declared, they
refuse bad arguments before any HIP call and before the scene is used, the Python methods validate their arguments, and the
restatement the GPU tests compare with (tests/shadowed_ref.py, from the oracle alone) is pinned: with the light off it IS the
oracle's render, on hand-made scenes it gives what geometry says, and the canonical case exercises every class of hit.  No GPU
needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, OracleApi, recipe_circles
import occluded_ref as OR
import shadowed_ref as SR

RTMI_OK, RTMI_ERR_INVALID, RTMI_ERR_UNSUPPORTED = 0, 1, 3
NAMES = ("rtmi_render_shadowed", "rtmi_render_shadowed_device", "rth_caster_walk_shadowed", "rth_caster_walk_shadowed_device")
F32 = np.float32
# the canonical case: 32 x 32, S = 2, maxdepth 5, seed 1, the light at occluded_ref.LIGHT = (-3, 6, 1) with len2 = 0.5.
# Per pass (tested, culled, live, occluded) of the restatement on the oracle; 2901 path rays and 587 live shadow rays in all.
CANONICAL_PASSES = ((400, 93, 307, 56), (191, 106, 85, 53), (150, 62, 88, 48), (112, 60, 52, 34), (91, 36, 55, 41))
CANONICAL_RAYS, CANONICAL_LIVE = 2901, 587


def _orc():
    from oracle import orc
    return orc


def test_entry_points_are_exported_declared_and_listed():
    from rust_raytrace_amd import _ffi
    L = _ffi.lib()
    text = open(os.path.join(ROOT, "include", "rtmi.h")).read() + open(os.path.join(ROOT, "include", "rtmi_host.h")).read()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in _ffi.RTMI_SYMBOLS + _ffi.RTH_SYMBOLS, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name


def test_bad_arguments_are_refused_before_the_scene_is_used():
    """Every RTMI_ERR_INVALID case of the header, both variants, through a dangling handle, with stats cleared"""
    SR.check_refusals()


def test_python_api_validates_its_arguments(canonical_pair):
    from rust_raytrace_amd import raytrace as R
    _, sp = canonical_pair
    c = R.HipRayCaster()
    vp = R.canonical_viewport(8, 8, 5, 4)
    img = np.zeros((8, 8, 4), F32)
    nan, inf = float("nan"), float("inf")
    for kw in (dict(), dict(orig=(0.0, nan, 0.0)), dict(orig=(0.0, 0.0)), dict(orig=OR.LIGHT, len2=-1.0), dict(orig=OR.LIGHT, len2=nan),
               dict(orig=OR.LIGHT, len2=inf), dict(orig=OR.LIGHT, bias=nan), dict(orig=OR.LIGHT, nsamples=0),
               dict(orig=OR.LIGHT, sample0=3, nsamples=2), dict(orig=OR.LIGHT, sample0=-1), dict(orig=OR.LIGHT, sample0=1),
               dict(orig=OR.LIGHT, data=np.zeros((8, 8, 4), np.float64)), dict(orig=OR.LIGHT, accum=np.zeros((8, 9, 4), F32)),
               dict(orig=OR.LIGHT, data=img, accum=img)):
        with pytest.raises(ValueError):
            c.walk_rays_shadowed(vp, sp, **kw)
    for bad in (None, img):  # not a device tensor, or nothing at all
        with pytest.raises(ValueError):
            c.walk_rays_shadowed_device(vp, sp, bad, orig=OR.LIGHT)


# ---------------------------------------------------------------- the restatement, on the oracle alone
def test_with_the_light_off_the_restatement_is_the_oracles_render(canonical_pair):
    orc = _orc()
    so, _ = canonical_pair
    vp12 = orc.canonical_viewport(32, 32)
    r = SR.shadowed_ref(orc, so, 32, 32, vp12, 5, 2, 1)
    ref, cn = so.render(32, 32, vp12, 5, 2, seed=1, threads=4)
    assert np.array_equal(r.image.view(np.uint32), ref.view(np.uint32))
    assert r.rays == cn["rays"] == CANONICAL_RAYS and r.nlive == 0 and all(p["tested"] == 0 for p in r.passes)
    # ... and on a scene with Solid, Matte and Reflective balls, edge faces and another seed
    sc = recipe_circles()(OracleApi(orc))
    vpc = orc.canonical_viewport(24, 24)
    r = SR.shadowed_ref(orc, sc, 24, 24, vpc, 5, 2, 3)
    ref, cn = sc.render(24, 24, vpc, 5, 2, seed=3, threads=4)
    assert np.array_equal(r.image.view(np.uint32), ref.view(np.uint32)) and r.rays == cn["rays"]
    # a depth of 1 and a centred-ray frame
    r = SR.shadowed_ref(orc, sc, 24, 24, vpc, 1, 1, 3)
    ref, cn = sc.render(24, 24, vpc, 1, 1, seed=3)
    assert np.array_equal(r.image.view(np.uint32), ref.view(np.uint32)) and r.rays == cn["rays"] == 576


@pytest.fixture(scope="module")
def canonical_lit(canonical_pair):
    orc = _orc()
    so, _ = canonical_pair
    return SR.shadowed_ref(orc, so, 32, 32, orc.canonical_viewport(32, 32), 5, 2, 1, OR.LIGHT, 0.5)


def test_canonical_case_exercises_every_class(canonical_pair, canonical_lit):
    orc = _orc()
    so, _ = canonical_pair
    r = canonical_lit
    assert OR.LIGHT == (-3.0, 6.0, 1.0)
    got = tuple((p["tested"], p["culled"], p["live"], p["occluded"]) for p in r.passes)
    print(got, r.rays, r.nlive, [p["refl_shadowed"] for p in r.passes])
    p0 = r.passes[0]
    assert p0["shadowed"] > 0 and p0["tested"] - p0["shadowed"] > 0                                   # both kinds at pass 0
    assert any(p["shadowed"] > 0 and p["tested"] - p["shadowed"] > 0 for p in r.passes[1:])           # ... and at a later pass
    assert sum(p["culled"] for p in r.passes) > 0 and sum(p["occluded"] for p in r.passes) > 0
    assert sum(p["refl_shadowed"] for p in r.passes) > 0                                              # a shadowed Reflective level
    assert all(p["shadowed"] == p["culled"] + p["occluded"] and p["tested"] == p["culled"] + p["live"] for p in r.passes)
    assert got == CANONICAL_PASSES and (r.rays, r.nlive) == (CANONICAL_RAYS, CANONICAL_LIVE)
    # the paths are the plain render's: the same rays per pass; the image is not
    plain = SR.shadowed_ref(orc, so, 32, 32, orc.canonical_viewport(32, 32), 5, 2, 1)
    assert [p["rays"] for p in plain.passes] == [p["rays"] for p in r.passes]
    assert not np.array_equal(plain.image, r.image) and (r.image <= plain.image).all() and (r.image[..., 3] == 0).all()
    # a pixel whose samples all miss shows the sky, lit or not
    sky = (plain.color.reshape(1024, 2, 4)[..., :3] == SR.FR.SKY).all(axis=(1, 2)).reshape(32, 32)
    assert sky.sum() > 700 and np.array_equal(r.image[sky], plain.image[sky])


def test_pass_0_is_the_direct_light_calls_first_candidate(canonical_pair, canonical_lit):
    """At j = 0 the shadow ray is candidate k = 0 of rtmi_render_light* on the same sample.  The restatement of that call with
    K = 1 tests the same hits plus the edge faces (the light buffer tests them, a path does not)."""
    import light_ref as LR
    orc = _orc()
    so, _ = canonical_pair
    vp12 = orc.canonical_viewport(32, 32)
    li = LR.light_ref(orc, so, 32, 32, vp12, 2, 1, 1, OR.LIGHT, 0.5)
    o4, d4, _, _ = SR.FR.tile_rays(orc, 32, 32, vp12, 2, 1)
    tri, _, face, _ = so.trace(o4, d4)
    edge = int(((tri != 0) & ((face & 2) != 0)).sum())
    p0 = canonical_lit.passes[0]
    assert edge > 0 and li.nhit == p0["tested"] + edge
    assert 0 <= li.nlive - p0["live"] <= edge and 0 <= li.nculled - p0["culled"] <= edge


def test_samples_and_tiles_select_the_same_paths(canonical_pair, canonical_lit):
    orc = _orc()
    so, _ = canonical_pair
    vp12 = orc.canonical_viewport(32, 32)
    s0 = SR.shadowed_ref(orc, so, 32, 32, vp12, 5, 2, 1, OR.LIGHT, 0.5, sample0=0, nsamples=1)
    s1 = SR.shadowed_ref(orc, so, 32, 32, vp12, 5, 2, 1, OR.LIGHT, 0.5, sample0=1, nsamples=1)
    both = canonical_lit.color.reshape(1024, 2, 4)
    assert np.array_equal(s0.color.view(np.uint32), both[:, 0].view(np.uint32))
    assert np.array_equal(s1.color.view(np.uint32), both[:, 1].view(np.uint32))
    assert s0.nlive + s1.nlive == canonical_lit.nlive
    tile = (1, 12, 3, 8)
    t = SR.shadowed_ref(orc, so, 32, 32, vp12, 5, 2, 1, OR.LIGHT, 0.5, tile=tile)
    assert np.array_equal(t.image.view(np.uint32), canonical_lit.image[SR.FR.tile_rows(tile)].view(np.uint32))


def test_a_wall_lit_from_the_cameras_side_has_no_shadowed_hit():
    """The wall covers the view and nothing stands between it and a point light behind the camera: every primary hit is
    tested, live and clear, and the image is the plain one.  At a depth of 1: half of a Matte wall's bounce rays start 0.001
    BEHIND it (lambertian_ray offsets the origin along the random vector) and meet its back face at once, which a light on the
    camera's side cannot reach -- deeper paths are checked below."""
    orc = _orc()
    so = SR.recipe_wall()(OracleApi(orc))
    vp12 = orc.canonical_viewport(32, 32)
    r = SR.shadowed_ref(orc, so, 32, 32, vp12, 1, 2, 1, SR.BEHIND_CAMERA, 0.0)
    assert r.passes == [dict(rays=2048, tested=2048, culled=0, live=2048, occluded=0, shadowed=0, refl_shadowed=0)]
    plain, _ = so.render(32, 32, vp12, 1, 2, seed=1)
    assert np.array_equal(r.image.view(np.uint32), plain.view(np.uint32))
    # mix_color(color, black, 0.5): half the wall's colour, exactly
    half = (orc.make_color(200, 200, 200) * F32(0.5)).astype(F32)
    assert (r.image[..., :3] == half).all()


def test_a_wall_lit_from_behind_has_every_hit_culled():
    orc = _orc()
    so = SR.recipe_wall()(OracleApi(orc))
    vp12 = orc.canonical_viewport(32, 32)
    r = SR.shadowed_ref(orc, so, 32, 32, vp12, 1, 2, 1, SR.BEHIND_WALL, 0.0)
    assert r.passes == [dict(rays=2048, tested=2048, culled=2048, live=0, occluded=0, shadowed=2048, refl_shadowed=0)]
    assert (r.image == 0).all() and r.nlive == 0
    # the same wall painted black, rendered plainly, is the same image
    black, _ = SR.recipe_wall(color=(0, 0, 0))(OracleApi(orc)).render(32, 32, vp12, 1, 2, seed=1)
    assert np.array_equal(r.image.view(np.uint32), black.view(np.uint32))


def test_deeper_paths_on_the_wall_alternate_between_its_faces():
    """Pass j >= 1 holds the bounce rays that started behind the face just hit: they meet the other face, whose side of the
    wall the other light is on.  So with either light the passes alternate between all clear and all culled."""
    orc = _orc()
    so = SR.recipe_wall()(OracleApi(orc))
    vp12 = orc.canonical_viewport(32, 32)
    for light, first in ((SR.BEHIND_CAMERA, 0), (SR.BEHIND_WALL, 1)):
        r = SR.shadowed_ref(orc, so, 32, 32, vp12, 5, 2, 1, light, 0.0)
        assert all(p["tested"] > 100 and p["occluded"] == 0 for p in r.passes)
        for j, p in enumerate(r.passes):
            assert (p["culled"], p["live"]) == ((0, p["tested"]) if j % 2 == first else (p["tested"], 0)), (light, j, p)


def test_the_corridor_fills_a_paths_whole_mask():
    """Two facing mirrors: paths survive to a depth of 32, and a box light that straddles one mirror shadows about half of
    the hits of every level, bit 31 included"""
    orc = _orc()
    so = SR.recipe_corridor()(OracleApi(orc))
    r = SR.shadowed_ref(orc, so, 16, 16, orc.canonical_viewport(16, 16), 32, 1, 1, SR.CORRIDOR_LIGHT, SR.CORRIDOR_LEN2)
    assert len(r.passes) == 32 and all(p["rays"] == 256 and p["tested"] == 256 for p in r.passes)
    assert all(0 < p["shadowed"] < 256 for p in r.passes) and r.passes[31]["refl_shadowed"] > 0
    assert sum(p["culled"] for p in r.passes) > 0 and sum(p["occluded"] for p in r.passes) > 0
