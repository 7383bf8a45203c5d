"""-m gpu: the device kernels against the float64 geometric referee (tests/geom_ref.py) directly -- no oracle between them.
Every closest-hit path (k_trace_oct, RTMI_OPT_GENERIC's k_trace, k_trace_linear, RTMI_OPT_BVH, RTMI_OPT_FAST, each also in its
counting instantiation), rtmi_occluded and rtmi_render_rays must return, on the rays the referee calls decided, the nearest
triangle the ray really crosses, its face, and the colour of the deterministic shading chain.  For RTMI_OPT_BVH and RTMI_OPT_FAST
this is the first criterion that is not their own rtmi_trace.  The scenes are built with the product alone and the referee reads
their corners, edge thicknesses and surfaces; the oracle's binding is used for one thing only, to MAKE camera rays (inputs).
Margins, caps and tolerances are those tests/test_geom_cpu.py measured on the CPU oracle; nothing here is tuned to a device."""
import functools
import os

import numpy as np
import pytest

from builder_cases import SOUP_ROOT, soup
from conftest import ProductApi, recipe_canonical
import geom_ref as G

pytestmark = pytest.mark.gpu
F32 = np.float32
# name -> (scene kind, option bits by name, the referee's view of the scene: "tree" keeps the root-box rule, "list" has none)
MODES = {"octree": ("tree", (), "tree"), "generic": ("tree", ("OPT_GENERIC",), "tree"), "list": ("list", (), "list"),
         "bvh": ("tree", ("OPT_BVH",), "list"), "fast": ("tree", ("OPT_FAST",), "tree")}


def _R():
    from rust_raytrace_amd import raytrace as R
    return R


def _options(R, names, counters):
    opts = R.OPT_COUNTERS if counters else 0
    for n in names:
        opts |= getattr(R, n)
    return opts


@functools.lru_cache(maxsize=None)
def soup_case(seed):
    R = _R()
    _, _, (maxdepth, minobjs), add = soup(seed)
    tree = add(ProductApi(R))
    tree.build_bounding_box(SOUP_ROOT[0], SOUP_ROOT[1], maxdepth, minobjs)
    lst = add(ProductApi(R))
    lst.build_trivial_bounding_box(SOUP_ROOT[0], SOUP_ROOT[1])
    g = G.geometry_from_records(tree.triangles()[0])
    o4, d4, fam = G.soup_rays(g, seed, SOUP_ROOT)
    h = G.closest_hit(g, None, o4, d4, SOUP_ROOT)
    ref = dict(tree=h, list=G.as_list(h))
    for kind in ref:                                  # the caps: conditions every comparison below stands on
        for f, name in enumerate(G.SOUP_FAMILIES):
            G.assert_caps(ref[kind], fam == f, G.SOUP_CAPS[name], f"soup {seed} {kind} {name}", misses_possible=G.SOUP_MISSES[name])
        G.assert_faces_occur(ref[kind], f"soup {seed} {kind}")
    return dict(tree=tree, list=lst, g=g, o4=o4, d4=d4, fam=fam, ref=ref, add=add, octree=(maxdepth, minobjs))


@functools.lru_cache(maxsize=None)
def canonical_case():
    from oracle import orc                            # camera rays only
    R = _R()
    tree = recipe_canonical()(ProductApi(R))
    lst = recipe_canonical(accel="trivial")(ProductApi(R))
    g = G.geometry_from_records(tree.triangles()[0])
    po, pd = orc.primary_rays(64, 64, orc.canonical_viewport(64, 64), 1)
    sets = {"primary": G.canonical_primary_subset(po, pd), "random": G.canonical_random_rays()}
    ref = {}
    for k, (o4, d4) in sets.items():
        h = G.closest_hit(g, None, o4, d4, G.CANONICAL_ROOT)
        ref[(k, "tree")], ref[(k, "list")] = h, G.as_list(h)
        for kind in ("tree", "list"):
            G.assert_caps(ref[(k, kind)], None, G.CANONICAL_CAP, f"canonical {k} {kind}")
    return dict(tree=tree, list=lst, g=g, sets=sets, ref=ref)


@functools.lru_cache(maxsize=None)
def mirror_case():
    from oracle import orc                            # camera rays only
    R = _R()
    sp = G.mirror_recipe()(ProductApi(R))
    scene = G.scene_from_records(*sp.triangles(), G.MIRROR_ROOT)
    o, d = [], []
    for c in G.mirror_cameras():
        vo = orc.create_viewport(c["w"], c["h"], c["size"], np.array(c["pos"], F32), orc.unit(list(c["aim"])), c["fov"], c["roll"])
        o4, d4 = orc.primary_rays(c["w"], c["h"], vo, 1)
        o.append(o4)
        d.append(d4)
    return dict(sp=sp, scene=scene, o4=np.concatenate(o), d4=np.concatenate(d))


def _trace_both_builds(case, mode, o4, d4, ref_of, what):
    R = _R()
    kind, names, view = MODES[mode]
    ref = ref_of(view)
    for counters in (False, True):                    # separate instantiations of every kernel
        tri, t, face, _ = R.HipRayCaster(options=_options(R, names, counters)).trace(case[kind], o4, d4)
        cmp = G.compare_hits(ref, tri, t, face, case["g"], o4, d4)
        print(f"{what} {mode}{' +counters' if counters else ''}: decided {int(ref.decided.sum())} of {len(tri)}, max plane residual {cmp['max_res']:.3g}")
        G.assert_hits(ref, tri, t, face, case["g"], o4, d4, f"{what}, {mode}{', counting build' if counters else ''}")


@pytest.fixture(scope="module", autouse=True)
def _release_scenes():
    """The cached scenes go when the module is done, not at interpreter shutdown"""
    yield
    for f in (soup_case, canonical_case, mirror_case):
        f.cache_clear()


# ---------------------------------------------------------------- closest hits
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("seed", G.SOUP_SEEDS)
def test_soup_closest_hits(seed, mode):
    case = soup_case(seed)
    _trace_both_builds(case, mode, case["o4"], case["d4"], lambda view: case["ref"][view], f"soup {seed}")


@pytest.mark.parametrize("mode", list(MODES))
def test_canonical_closest_hits(mode):
    case = canonical_case()
    for name, (o4, d4) in case["sets"].items():
        _trace_both_builds(case, mode, o4, d4, lambda view: case["ref"][(name, view)], f"canonical {name}")


@pytest.mark.parametrize("mode", list(MODES))
def test_mirror_set_closest_hits(mode):
    R = _R()
    case = mirror_case()
    if MODES[mode][0] == "list":
        sp = G.mirror_recipe("trivial")(ProductApi(R))
    else:
        sp = case["sp"]
    h = G.closest_hit(case["scene"].g, None, case["o4"], case["d4"], G.MIRROR_ROOT)
    G.assert_caps(h, None, 0.10, "mirror set")
    refs = dict(tree=h, list=G.as_list(h))
    one = dict(tree=sp, list=sp, g=case["scene"].g)
    _trace_both_builds(one, mode, case["o4"], case["d4"], lambda view: refs[view], "mirror set")


# ---------------------------------------------------------------- rtmi_occluded
@pytest.mark.parametrize("anyhit", ["1", "0"])
@pytest.mark.parametrize("seed", G.SOUP_SEEDS)
def test_soup_occluded(seed, anyhit):
    """The answer equals `referee t < tmax` for tmax = the referee's t (1 +- 1e-3) and +inf, through the any-hit kernels and
    through the closest-hit launch + k_occl_from_hits (RTMI_OCCLUDED_ANYHIT=0, read when a scene handle is created)"""
    R = _R()
    case = soup_case(seed)
    maxdepth, minobjs = case["octree"]
    o4, d4 = case["o4"], case["d4"]
    old = os.environ.get("RTMI_OCCLUDED_ANYHIT")
    os.environ["RTMI_OCCLUDED_ANYHIT"] = anyhit
    try:
        for kind in ("tree", "list"):
            sp = case["add"](ProductApi(R))           # a fresh scene: a fresh handle
            if kind == "tree":
                sp.build_bounding_box(SOUP_ROOT[0], SOUP_ROOT[1], maxdepth, minobjs)
            else:
                sp.build_trivial_bounding_box(SOUP_ROOT[0], SOUP_ROOT[1])
            ref = case["ref"][kind]
            hit = ref.tri != 0
            near = G.occlusion_rays(ref)
            for counters in (False, True):
                c = R.HipRayCaster(options=R.OPT_COUNTERS if counters else 0)
                for name, tmax, want, sel in (("t (1 + 1e-3)", (ref.t * (1 + 1e-3)).astype(F32), hit, near),
                                              ("t (1 - 1e-3)", (ref.t * (1 - 1e-3)).astype(F32), np.zeros_like(hit), near),
                                              ("+inf", None, hit, ref.decided)):
                    assert sel.sum() >= 1500 and (want & sel).sum() >= (200 if want.any() else 0)
                    got, st = c.occluded(sp, o4, d4, tmax)
                    bad = np.nonzero(sel & ((got != 0) != want))[0]
                    assert len(bad) == 0, f"soup {seed} {kind}, any-hit {anyhit}, counters {counters}, tmax {name}: {len(bad)} decided rays differ, first {bad[:5]}"
                    assert st["rays"] == len(got)
    finally:
        if old is None:
            del os.environ["RTMI_OCCLUDED_ANYHIT"]
        else:
            os.environ["RTMI_OCCLUDED_ANYHIT"] = old


# ---------------------------------------------------------------- rtmi_render_rays
@pytest.mark.parametrize("maxdepth", G.MIRROR_DEPTHS)
def test_mirror_set_render_rays(maxdepth):
    """Per-ray colours against mirror_colour on decided chains; the group guide buffers at G = 1 against the referee's first hit"""
    R = _R()
    case = mirror_case()
    scene, o4, d4 = case["scene"], case["o4"], case["d4"]
    col, dec, first = G.mirror_colour(scene, o4, d4, maxdepth)
    assert 1.0 - dec.mean() <= 0.10 and 1.0 - first.decided.mean() <= 0.10
    alb, nrm, ids = G.first_hit_guides(scene, first)
    fd = first.decided
    for counters in (False, True):
        caster = R.HipRayCaster(seed=3, options=R.OPT_COUNTERS if counters else 0)
        got, ctx = caster.walk_rays_explicit(case["sp"], o4, d4, maxdepth, group=1, color=True, albedo=True, normal=True, ids=True)
        err = np.abs(got["color"][:, :3].astype(np.float64) - col).max(axis=1)
        print(f"maxdepth {maxdepth}{' +counters' if counters else ''}: decided chains {int(dec.sum())} of {len(dec)}, max colour error {err[dec].max():.3g}")
        assert (err[dec] <= G.COL_TOL).all(), f"{int((err[dec] > G.COL_TOL).sum())} decided chains off by up to {err[dec].max():.3g} (tolerance {G.COL_TOL:.3g})"
        assert (got["color"][:, 3] == 0).all()
        # ids = tri | face << 30, normal lane 3 = t: the first hit itself
        tri, face = got["ids"] & np.uint32(0x3FFFFFFF), got["ids"] >> np.uint32(30)
        G.assert_hits(first, tri, got["normal"][:, 3], face, scene.g, o4, d4, f"guides at maxdepth {maxdepth}")
        assert np.array_equal(got["ids"][fd], ids[fd])
        aerr = np.abs(got["albedo"][fd].astype(np.float64) - alb[fd]).max()   # float32 colours: half an ulp below 1 = 2^-25
        assert aerr <= 2.0 ** -24, f"albedo (the first hit's surface colour, black on edges, the sky on a miss): off by {aerr:.3g}"
        nerr = np.abs(got["normal"][fd, :3].astype(np.float64) - nrm[fd, :3]).max()
        assert nerr <= G.NRM_TOL, f"normal: off the float64 face normal by {nerr:.3g} (tolerance {G.NRM_TOL:.3g})"
        assert (got["normal"][fd & (first.tri == 0)] == 0).all()
