"""The CPU oracle against the float64 geometric referee (tests/geom_ref.py): closest hits through the octree and the linear
list, the deterministic shading chain, leaf completeness of the octree builder, and a self-check that the referee can fail.
This is also where the referee's margins and tolerances are MEASURED: every test prints its figures (run with -s), and
DESIGN.md section 2 (vi) holds the table.  No GPU."""
import functools

import numpy as np
import pytest

from builder_cases import SOUP_ROOT, soup
from conftest import OracleApi, recipe_canonical
import geom_ref as G


def _orc():
    from oracle import orc
    return orc


# ---------------------------------------------------------------- shared cases (computed once)
@functools.lru_cache(maxsize=None)
def soup_case(seed):
    orc = _orc()
    _, ntri, (maxdepth, minobjs), add = soup(seed)
    tree = add(OracleApi(orc))
    tree.build_bounding_box(SOUP_ROOT[0], SOUP_ROOT[1], maxdepth, minobjs)
    lst = add(OracleApi(orc))
    lst.build_trivial_bounding_box(SOUP_ROOT[0], SOUP_ROOT[1])
    g = G.geometry_from_records(tree.triangles()[0])
    o4, d4, fam = G.soup_rays(g, seed, SOUP_ROOT)
    return dict(tree=tree, list=lst, g=g, o4=o4, d4=d4, fam=fam, octree=(maxdepth, minobjs),
                ref=dict(tree=(h := G.closest_hit(g, None, o4, d4, SOUP_ROOT)), list=G.as_list(h)))


@functools.lru_cache(maxsize=None)
def canonical_case():
    orc = _orc()
    tree = recipe_canonical()(OracleApi(orc))
    lst = recipe_canonical(accel="trivial")(OracleApi(orc))
    g = G.geometry_from_records(tree.triangles()[0])
    po, pd = orc.primary_rays(64, 64, orc.canonical_viewport(64, 64), 1)
    sets = {"primary": G.canonical_primary_subset(po, pd), "random": G.canonical_random_rays()}
    ref = {}
    for k, (o4, d4) in sets.items():
        ref[(k, "tree")] = G.closest_hit(g, None, o4, d4, G.CANONICAL_ROOT)
        ref[(k, "list")] = G.as_list(ref[(k, "tree")])
    return dict(tree=tree, list=lst, g=g, sets=sets, ref=ref)


def mirror_rays(orc):
    o, d = [], []
    for c in G.mirror_cameras():
        vo = orc.create_viewport(c["w"], c["h"], c["size"], np.array(c["pos"], np.float32), orc.unit(list(c["aim"])), c["fov"], c["roll"])
        o4, d4 = orc.primary_rays(c["w"], c["h"], vo, 1)
        o.append(o4)
        d.append(d4)
    return np.concatenate(o), np.concatenate(d)


def mirror_oracle_colours(orc, so, maxdepth):
    out = []
    for c in G.mirror_cameras():
        vo = orc.create_viewport(c["w"], c["h"], c["size"], np.array(c["pos"], np.float32), orc.unit(list(c["aim"])), c["fov"], c["roll"])
        img, _ = so.render(c["w"], c["h"], vo, maxdepth, 1, seed=1, threads=4)
        out.append(img.reshape(-1, 4))
    return np.concatenate(out)


@functools.lru_cache(maxsize=None)
def mirror_case():
    orc = _orc()
    so = G.mirror_recipe()(OracleApi(orc))
    scene = G.scene_from_records(*so.triangles(), G.MIRROR_ROOT)
    o4, d4 = mirror_rays(orc)
    return dict(so=so, scene=scene, o4=o4, d4=d4)


@pytest.fixture(scope="module", autouse=True)
def _release_scenes():
    """The cached scenes go when the module is done, not at interpreter shutdown"""
    yield
    for f in (soup_case, canonical_case, mirror_case):
        f.cache_clear()


def _row(what, c, extra=""):
    print(f"  {what:34s} rays {c['rays']:5d}  undecided {c['undecided']:7.3%}  decided hits {c['hits']:5d}  misses {c['misses']:5d}  {extra}")


# ---------------------------------------------------------------- hits
@pytest.mark.parametrize("seed", G.SOUP_SEEDS)
def test_soup_hits_octree_and_list(seed):
    case = soup_case(seed)
    g, o4, d4, fam = case["g"], case["o4"], case["d4"], case["fam"]
    assert o4.shape[0] == 2048
    print(f"\nsoup {seed}: {len(g.corners) - 1} triangles, octree {case['octree']}")
    for kind in ("tree", "list"):
        ref = case["ref"][kind]
        for f, name in enumerate(G.SOUP_FAMILIES):     # the caps come first: conditions, not measurements
            c = G.assert_caps(ref, fam == f, G.SOUP_CAPS[name], f"soup {seed} {kind} {name}", misses_possible=G.SOUP_MISSES[name])
            _row(f"{kind} {name}", c)
        faces = G.assert_faces_occur(ref, f"soup {seed} {kind}")
        tri, t, face, _ = case[kind].trace(o4, d4)
        hit = ref.decided & (ref.tri != 0)
        rel_t = np.abs(t[hit] - ref.t[hit]) / ref.t[hit]
        res = G.compare_hits(ref, tri, t, face, g, o4, d4)["max_res"]
        print(f"  {kind}: faces {faces.tolist()}, max plane residual {res:.3g}, max relative t error {rel_t.max():.3g}")
        G.assert_hits(ref, tri, t, face, g, o4, d4, f"soup {seed}, oracle {kind}")


def test_canonical_hits_octree_and_list():
    case = canonical_case()
    g = case["g"]
    print()
    for name, (o4, d4) in case["sets"].items():
        assert o4.shape[0] == 1024
        for kind in ("tree", "list"):
            ref = case["ref"][(name, kind)]
            c = G.assert_caps(ref, None, G.CANONICAL_CAP, f"canonical {name} {kind}")
            tri, t, face, _ = case[kind].trace(o4, d4)
            _row(f"canonical {name} {kind}", c, f"max plane residual {G.compare_hits(ref, tri, t, face, g, o4, d4)['max_res']:.3g}")
            G.assert_hits(ref, tri, t, face, g, o4, d4, f"canonical {name}, oracle {kind}")


# ---------------------------------------------------------------- the any-hit rule on decided rays (what tests/test_geom.py asks of rtmi_occluded)
@pytest.mark.parametrize("seed", G.SOUP_SEEDS)
def test_hit_times_decide_the_occlusion_limits(seed):
    """tests/test_geom.py sets tmax to the referee's t (1 +- 1e-3): the oracle's float32 t must fall on the referee's side of
    both limits on every decided hit whose error bound (Hits.terr) leaves room for it.  That is at least 90 % of the decided rays
    of every family but `near`: there t <= 0.3, and the float32 plane distance is only good to EPS_0 = 2e-5 in absolute terms."""
    case = soup_case(seed)
    for kind in ("tree", "list"):
        ref = case["ref"][kind]
        tri, t, _, _ = case[kind].trace(case["o4"], case["d4"])
        sel = G.occlusion_rays(ref)
        hit = sel & (ref.tri != 0)
        for f, name in enumerate(G.SOUP_FAMILIES[:4]):
            fam = case["fam"] == f
            assert (sel & fam).sum() >= 0.9 * (ref.decided & fam).sum(), f"{kind} {name}: the limits decide only {(sel & fam).sum()} rays"
        assert ((t[hit] < ref.t[hit] * (1 + 1e-3)) & (t[hit] > ref.t[hit] * (1 - 1e-3))).all()
        print(f"soup {seed} {kind}: {int(sel.sum())} of {int(ref.decided.sum())} decided rays usable, max relative t error "
              f"{(np.abs(t[hit] - ref.t[hit]) / ref.t[hit]).max():.3g}")


# ---------------------------------------------------------------- colours
def test_mirror_set_colours():
    orc = _orc()
    case = mirror_case()
    scene, o4, d4 = case["scene"], case["o4"], case["d4"]
    assert o4.shape[0] == 1024 and 25 <= len(scene.g.corners) - 1 <= 35
    print()
    worst = 0.0
    for depth in G.MIRROR_DEPTHS:
        col, dec, first = G.mirror_colour(scene, o4, d4, depth)
        share = 1.0 - dec.mean()
        assert share <= 0.10, f"maxdepth {depth}: {share:.2%} of the chains undecided"
        got = mirror_oracle_colours(orc, case["so"], depth)
        assert (got[:, 3] == 0).all()
        err = np.abs(got[:, :3].astype(np.float64) - col).max(axis=1)
        worst = max(worst, float(err[dec].max()))
        print(f"  mirror set maxdepth {depth}: rays {len(dec)}  undecided chains {share:7.3%}  max colour error {err[dec].max():.3g}")
        assert (err[dec] <= G.COL_TOL).all(), f"maxdepth {depth}: {int((err[dec] > G.COL_TOL).sum())} decided chains off by up to {err[dec].max():.3g}"
    # the set does what it is for: both mirrors from both sides, edge faces, the sky, and chains deeper than two
    _, _, first = G.mirror_colour(scene, o4, d4, 1)
    refl = np.nonzero(scene.kind == G.REFLECTIVE)[0]
    for alpha in (0.7, 0.3):
        ids = refl[np.isclose(scene.alpha[refl], alpha)]
        for face in (G.FRONT, G.BACK):
            assert (first.decided & np.isin(first.tri, ids) & (first.face == face)).sum() >= 10, (alpha, face)
    assert (first.decided & ((first.face & 2) != 0)).sum() >= 10 and (first.decided & (first.tri == 0)).sum() >= 10
    c2, d2, _ = G.mirror_colour(scene, o4, d4, 2)
    c6, d6, _ = G.mirror_colour(scene, o4, d4, 6)
    assert (np.abs(c2 - c6).max(axis=1)[d2 & d6] > 1e-3).sum() >= 10
    print(f"  largest colour error on decided chains {worst:.3g}, tolerance {G.COL_TOL:.3g}")


def test_mirror_set_first_hits():
    case = mirror_case()
    scene, o4, d4 = case["scene"], case["o4"], case["d4"]
    ref = G.closest_hit(scene.g, None, o4, d4, G.MIRROR_ROOT)
    c = G.assert_caps(ref, None, 0.10, "mirror set")
    tri, t, face, _ = case["so"].trace(o4, d4)
    cmp = G.assert_hits(ref, tri, t, face, scene.g, o4, d4, "mirror set, oracle")
    print()
    _row("mirror set first hits", c, f"max plane residual {cmp['max_res']:.3g}")
    # the guide normal of rtmi_render_rays is the record's float32 norm: how far it is from the float64 unit normal
    nerr = np.abs(case["so"].triangles()[0][1:, 3:6].astype(np.float64) - scene.g.nh[1:]).max()
    print(f"  mirror set: record norm against the float64 unit normal, max lane difference {nerr:.3g}, tolerance {G.NRM_TOL:.3g}")
    assert nerr <= G.NRM_TOL


# ---------------------------------------------------------------- builder
@pytest.mark.parametrize("seed", G.SOUP_SEEDS)
def test_octree_leaves_list_every_overlapping_triangle(seed):
    case = soup_case(seed)
    geo, topo, refs = case["tree"].tree_flatten()
    r = G.leaf_completeness(case["g"], geo, topo, refs)
    share = r["skipped"] / max(r["skipped"] + r["required"], 1)
    print(f"\nsoup {seed}: {r['leaves']} leaves, {r['required']} required references, {r['skipped']} within the margin ({share:.3%}), "
          f"{len(r['missing'])} missing")
    assert share <= 0.10 and r["required"] >= 200
    assert not r["missing"], f"holes in the octree: (box, triangle) {r['missing'][:8]}"


# ---------------------------------------------------------------- self-check: the referee can fail
def test_self_check_swapped_corners_are_reported():
    case = soup_case(1)
    g, o4, d4, ref = case["g"], case["o4"], case["d4"], case["ref"]["list"]
    tri, t, face, _ = case["list"].trace(o4, d4)
    hit = ref.decided & (ref.tri != 0)
    victim = int(np.bincount(ref.tri[hit]).argmax())
    corners = g.corners.copy()
    corners[victim, [1, 2]] = corners[victim, [2, 1]]
    g2 = G.Geometry(corners, g.th)
    cmp = G.compare_hits(G.closest_hit(g2, None, o4, d4, None), tri, t, face, g2, o4, d4)
    on_victim = hit & (ref.tri == victim)
    assert on_victim.sum() >= 3 and set(np.nonzero(on_victim)[0]) <= set(cmp["bad_face"])   # front and back change places
    assert not len(cmp["bad_id"])


def test_self_check_scaled_edge_thickness_is_reported():
    case = soup_case(1)
    g, o4, d4, ref = case["g"], case["o4"], case["d4"], case["ref"]["list"]
    tri, t, face, _ = case["list"].trace(o4, d4)
    edge_hit = ref.decided & (ref.tri != 0) & ((ref.face & 2) != 0)
    victim = int(np.bincount(ref.tri[edge_hit]).argmax())
    th = g.th.copy()
    th[victim] *= 1e-3
    g2 = G.Geometry(g.corners, th)
    ref2 = G.closest_hit(g2, None, o4, d4, None)
    cmp = G.compare_hits(ref2, tri, t, face, g2, o4, d4)
    lost = edge_hit & (ref.tri == victim) & ref2.decided
    assert lost.sum() >= 1 and set(np.nonzero(lost)[0]) <= set(cmp["bad_face"])


def test_self_check_dropped_leaf_reference_is_reported():
    case = soup_case(2)
    geo, topo, refs = case["tree"].tree_flatten()
    base = G.leaf_completeness(case["g"], geo, topo, refs)
    assert not base["missing"]
    done = False
    for b in np.nonzero(topo[:, 2] == 1)[0]:
        first, count = int(topo[b, 0]), int(topo[b, 1])
        pen = G.tri_box_penetration(case["g"].corners[refs[first:first + count]], geo[b, :3], float(geo[b, 3]))
        deep = np.nonzero(pen > 10 * G.BOX_MARGIN)[0]
        if len(deep):
            k = first + int(deep[0])
            victim = int(refs[k])
            topo2, refs2 = topo.copy(), np.delete(refs, k)
            topo2[b, 1] -= 1
            leaf = topo2[:, 2] == 1
            topo2[leaf & (topo2[:, 0] > first), 0] -= 1
            assert G.leaf_completeness(case["g"], geo, topo2, refs2)["missing"] == [(int(b), victim)]
            done = True
            break
    assert done


def test_self_check_negated_normal_is_reported():
    case = soup_case(3)
    g, o4, d4, ref = case["g"], case["o4"], case["d4"], case["ref"]["tree"]
    tri, t, face, _ = case["tree"].trace(o4, d4)
    assert not G.describe(G.compare_hits(ref, tri, t, face, g, o4, d4), ref, tri, face, "unperturbed")
    k = int(np.nonzero(ref.decided & (ref.tri != 0))[0][17])
    face2 = face.copy()
    face2[k] ^= 1                                       # the face normal of one hit, negated
    cmp = G.compare_hits(ref, tri, t, face2, g, o4, d4)
    assert cmp["bad_face"].tolist() == [k] and not len(cmp["bad_id"]) and not len(cmp["bad_pos"])
    # and a hit moved off its plane, or given to another triangle, is reported as such
    t2, tri2 = t.copy(), tri.copy()
    t2[k] *= np.float32(1.01)
    tri2[k] = 0
    assert G.compare_hits(ref, tri, t2, face, g, o4, d4)["bad_pos"].tolist() == [k]
    assert G.compare_hits(ref, tri2, t, face, g, o4, d4)["bad_id"].tolist() == [k]


def test_referee_reads_corners_thickness_and_surface_only():
    """geom_ref imports nothing but NumPy and the standard library: no oracle, no product, no other reference module"""
    import ast
    tree = ast.parse(open(G.__file__).read())
    names = {a.name for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names}
    froms = {n.module for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)}
    assert names <= {"collections", "functools", "numpy"} and not froms, (names, froms)
