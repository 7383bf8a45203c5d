"""The preconditions of tests/test_capacity_edges.py, from the oracle alone (no GPU needed): the frames of capacity_cases.py hold
as many zero-component paths as the slow-path queue's cap, one more and many more, their reflections off the disc faces are
zero-component rays again, depth 32 traces more rays than depth 31, the corridor keeps every path alive for 32 levels, and the
palette scene has exactly 65 535 distinct surfaces whose high ids are seen at the first hit and below a path's top level.  So
a changed recipe cannot quietly turn a GPU test into one that checks nothing.  The surface limit of rtmi_scene_create is
checked here too: the check comes before the first HIP call."""
from types import SimpleNamespace

import numpy as np
import pytest

import capacity_cases as CC
from conftest import ROOT  # noqa: F401  (puts the repository on sys.path)

F32 = np.float32


def _orc():
    from oracle import orc
    return orc


# ---------------------------------------------------------------- A
def test_mirror_discs_is_401_triangles_with_exact_face_normals():
    so = CC.oracle_scene("discs")
    rec, kinds, _ = so.triangles()
    assert so.num_tris() == 401
    faces = kinds == 2
    assert faces.sum() == 200 and (rec[faces, 3:5] == 0).all()  # both sides of both discs; the rims are Matte
    assert {float(z) for z in rec[faces, 5]} == {-1.0, 1.0}


@pytest.mark.parametrize("name", list(CC.FRAMES))
def test_every_primary_ray_of_a_slow_frame_has_a_zero_component(name):
    orc = _orc()
    f = CC.FRAMES[name]
    o4, d4 = orc.primary_rays(f["w"], f["h"], np.asarray(CC.SLOW_VP12, F32), 1, seed=CC.SEED)
    assert f["w"] * f["h"] == f["paths"] == len(d4)
    assert (d4[:, 0] == 0).all() and int(CC.zero_component(d4).sum()) == f["paths"]
    assert (f["paths"] > CC.SLOW_CAP) == (name != "at_cap") and CC.FRAMES["cap_plus_one"]["paths"] == CC.SLOW_CAP + 1
    if "hits" in f:
        tri, _, _, _ = CC.oracle_scene("discs").trace(o4, d4)
        assert int((tri != 0).sum()) == f["hits"] > 0


def test_slow_viewport_is_test_progressives():
    import test_progressive
    assert CC.SLOW_VP12 == test_progressive.SLOW_VP12


def test_views_and_streams_frames_hold_the_same_rays():
    """160 x 64 (a view of the VIEWS case) and 160 x 256 (the two-stream case) are zero-component frames too; two samples
    per pixel (PASS and LIST) jitter within the plane x = 2"""
    orc = _orc()
    for w, h, spp in ((160, 64, 1), (160, 256, 1), (CC.OVER_W, CC.OVER_H, 2), (CC.OVER_W, CC.OVER_H, 3)):
        _, d4 = orc.primary_rays(w, h, np.asarray(CC.SLOW_VP12, F32), spp, seed=CC.SEED)
        assert len(d4) == w * h * spp and (d4[:, 0] == 0).all()


@pytest.mark.parametrize("name", ["cap_plus_one", "over"])
def test_rays_of_the_slow_frames_and_depth_32_beyond_depth_31(name):
    f = CC.FRAMES[name]
    so = CC.oracle_scene("discs")
    rays = {d: so.render(f["w"], f["h"], np.asarray(CC.SLOW_VP12, F32), d, 1, seed=CC.SEED, threads=8)[1]["rays"] for d in (5, 31, 32)}
    assert rays == f["rays"] and rays[32] > rays[31] > rays[5] > f["paths"]


def test_bounce_rays_off_the_disc_faces_are_zero_component_rays():
    """On `over`, at every level: a bounce ray that left a disc face has d.x == 0 exactly; the Matte rims scatter"""
    orc = _orc()
    so = CC.oracle_scene("discs")
    rec, kinds, _ = so.triangles()
    r, passes = CC.recorded_passes(orc, so, CC.OVER_W, CC.OVER_H, CC.SLOW_VP12, 5, 1, CC.SEED)
    assert r.rays == CC.FRAMES["over"]["rays"][5] and [len(p["tri"]) for p in passes] == [p["rays"] for p in r.passes]
    off_face = 0
    for j in range(1, len(passes)):
        go = CC.goes_on(so, passes[j - 1])
        src = passes[j - 1]["tri"][go]
        assert len(src) == len(passes[j]["d4"])
        face = (kinds[src] == 2) & (rec[src, 3] == 0) & (rec[src, 4] == 0)
        assert (passes[j]["d4"][face, 0] == 0).all(), j
        off_face += int(face.sum())
        if j == 1:
            assert face.sum() > 4096  # more zero-component reflections at the first bounce than the queue could still take
    assert off_face > 0
    # the refused primary rays (paths 16 384 and up go to the queue last in path order, whichever are refused some hit a disc)
    assert int(CC.goes_on(so, passes[0]).sum()) > 0


def test_axis_box_under_the_slow_view():
    """The second scene: every primary ray is a zero-component ray, some hit, and the oracle renders it"""
    orc = _orc()
    so = CC.oracle_scene("axis_box")
    o4, d4 = orc.primary_rays(CC.OVER_W, CC.OVER_H, np.asarray(CC.SLOW_VP12, F32), 1, seed=CC.SEED)
    tri, _, _, _ = so.trace(o4, d4)
    assert CC.zero_component(d4).all() and (tri != 0).sum() > 0 and so.num_tris() == 9


# ---------------------------------------------------------------- B
def test_corridor_paths_live_to_the_depth_limit():
    orc = _orc()
    so = CC.oracle_scene("corridor")
    c = CC.CORRIDOR
    vo = orc.canonical_viewport(c["w"], c["h"])
    npaths = c["w"] * c["h"] * c["spp"]
    _, cn = so.render(c["w"], c["h"], vo, c["maxdepth"], c["spp"], seed=CC.SEED, threads=4)
    assert c["maxdepth"] == CC.MAX_PASSES == 32 and cn["rays"] == 32 * npaths
    _, d4 = orc.primary_rays(c["w"], c["h"], vo, c["spp"], seed=CC.SEED)
    assert not CC.zero_component(d4).any()  # no slow path: the ordinary queues carry every level


# (maxdepth = 33: rtmi_render_rays' refusal is pinned by test_rays_cpu.py, the sample passes' by shadowed_ref.check_refusals,
# the views' by test_views_cpu.py; rtmi_render reads its scene first, so its refusal is in test_capacity_edges.py.)


# ---------------------------------------------------------------- C
@pytest.fixture(scope="module")
def palette():
    orc = _orc()
    so = CC.oracle_scene("palette")
    ids, distinct = CC.surface_ids(so)
    v = CC.PALETTE_VIEW
    r, passes = CC.recorded_passes(orc, so, v["w"], v["h"], CC.palette_viewport(orc), v["maxdepth"], v["spp"], CC.SEED)
    return SimpleNamespace(so=so, ids=ids, distinct=distinct, r=r, passes=passes)


def test_palette_has_exactly_65535_surfaces(palette):
    p = palette
    assert p.so.num_tris() == 1 + CC.PALETTE_WALL_TRIS + CC.PALETTE_EXTRA + 2 and CC.PALETTE_WALL_TRIS == 65522
    assert p.distinct == CC.MAX_SURFACES and p.ids[0] == 0 and p.ids.max() == 65534
    # triangle k of the wall and of the extras is scene triangle k + 1 and has surface id k + 1; the mirror has the top id
    nk = CC.PALETTE_WALL_TRIS + CC.PALETTE_EXTRA
    assert np.array_equal(p.ids[1:nk + 1], np.arange(1, nk + 1)) and (p.ids[nk + 1:] == 65534).all()


def test_palette_view_sees_high_ids_at_the_first_hit_and_below_the_top_level(palette):
    p = palette
    orc = _orc()
    v = CC.PALETTE_VIEW
    ref, cn = p.so.render(v["w"], v["h"], CC.palette_viewport(orc), v["maxdepth"], v["spp"], seed=CC.SEED, threads=8)
    assert np.array_equal(ref.view(np.uint32), p.r.image.view(np.uint32)) and cn["rays"] == p.r.rays
    first = p.ids[p.passes[0]["tri"][p.passes[0]["tri"] != 0]]
    seen = set(first.tolist())
    assert any(255 < i <= 32767 for i in seen) and any(i > 32767 for i in seen)
    assert dict(distinct=len(seen), high=sum(1 for i in seen if i > 32767), lowest=min(seen), top=max(seen)) == CC.PALETTE_SEEN
    # deeper levels (mstack[j], j >= 1): hits on high ids at passes 1 and 2, the mirror (the top id 65 534) at pass 1, and
    # paths the mirror returned to the wall's upper half at pass 2
    for j in (1, 2):
        tri = p.passes[j]["tri"]
        assert (p.ids[tri[tri != 0]] >= 32768).sum() > 100, j
    go1 = CC.goes_on(p.so, p.passes[1])
    from_mirror = p.ids[p.passes[1]["tri"][go1]] == 65534
    assert from_mirror.sum() > 50
    back = p.passes[2]["tri"][from_mirror]
    assert ((back != 0) & (p.ids[back] >= 32768) & (p.ids[back] < 65534)).sum() > 20


def _lib():
    from rust_raytrace_amd import _ffi
    return _ffi.lib()


def _create(tris):
    L = _lib()
    rc, h, msg = CC.create_one_leaf_scene(L, tris)
    if rc == CC.RTMI_OK:
        L.rtmi_scene_destroy(h)
    return rc, msg


def test_scene_create_takes_65535_surfaces_and_refuses_one_more(palette):
    rec, kinds, surf = palette.so.triangles()
    tris = CC.abi_triangles(rec, kinds, surf)
    rc, msg = _create(tris)
    assert rc in (CC.RTMI_OK, CC.RTMI_ERR_NO_DEVICE), (rc, msg)
    # one more distinct surface: a copy of the last triangle in a colour nothing else has
    more = np.concatenate([tris, tris[-1:]])
    more[-1, 21:24] = [0.5, 0.25, 0.125]
    rc, msg = _create(more)
    assert rc == CC.RTMI_ERR_UNSUPPORTED and b"distinct surfaces" in msg, (rc, msg)
    # ... and the same triangle again in a colour the scene has is accepted
    rc, msg = _create(np.concatenate([tris, tris[-1:]]))
    assert rc in (CC.RTMI_OK, CC.RTMI_ERR_NO_DEVICE), (rc, msg)


def test_fields_a_kind_does_not_carry_do_not_make_a_new_surface(palette):
    """At 65 535 surfaces: a Solid triangle with another alpha or scattering and a Matte one with another scattering are the
    surfaces they were; a Matte one with another alpha and a Reflective one with another scattering are new"""
    rec, kinds, surf = palette.so.triangles()
    tris = CC.abi_triangles(rec, kinds, surf)
    solid, matte, refl = (1 + int(np.argmax(kinds[1:] == k)) for k in (0, 1, 2))

    def with_copy(i, alpha=None, scattering=None):
        t = np.concatenate([tris, tris[i:i + 1]])
        if alpha is not None:
            t[-1, 24] = alpha
        if scattering is not None:
            t[-1, 25] = scattering
        return _create(t)

    for kw in (dict(i=solid, alpha=0.9), dict(i=solid, scattering=0.3), dict(i=solid, alpha=0.1, scattering=0.2), dict(i=matte, scattering=0.3)):
        rc, msg = with_copy(**kw)
        assert rc in (CC.RTMI_OK, CC.RTMI_ERR_NO_DEVICE), (kw, rc, msg)
    for kw in (dict(i=matte, alpha=0.9), dict(i=refl, scattering=0.3), dict(i=refl, alpha=0.9)):
        rc, msg = with_copy(**kw)
        assert rc == CC.RTMI_ERR_UNSUPPORTED and b"distinct surfaces" in msg, (kw, rc, msg)
