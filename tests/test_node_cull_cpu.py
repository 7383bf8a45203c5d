"""Node cull of k_trace_oct (trace_oct.hpp, "Node cull"): one packed box per inner record of the octree form,
around every block box below it; a certified ray whose half-line misses it skips the subtree.  CPU only:
rtmi_debug_node_cull builds the records and evaluates the predicate on the host with the kernel's own __host__ __device__
functions.  Checked here: every node box contains the packed box of every block below it, no reference below a culled node
passes the f32 plane test, the cull removes a real share of a float64 model walk's SELECT steps, and hand-made trees agree
with brute force over the subtree's references."""
import ctypes as C

import numpy as np
import pytest

import test_block_cull_cpu as B
from test_block_cull_cpu import canonical, mkrays, mkrecs, unit  # noqa: F401  (canonical: a fixture)
from test_block_cull_packed_cpu import packed_box
from test_ray_cert_cpu import G, G_SMALL, ray_cull

f32 = np.float32
MISS, CUT = 1, 4
FN_WIDE = 0x10000


def node_cull(geo, topo, refs, recs, rays, g=G_SMALL):
    """A flattened tree (geo (nb, 4) f32, topo (nb, 4) u32, refs u32: the layout test_leaf_dedup.oct_form consumes), plane
    records (m, 8) f32 and rays (n, 8) f32 -> dict(records (nrec, 4) u32, cert (n,) bool, out (nrec, n) u8: MISS | CUT)."""
    from rust_raytrace_amd import _ffi
    L = _ffi.lib()
    vp = C.c_void_p
    L.rtmi_debug_node_cull.restype = C.c_int
    L.rtmi_debug_node_cull.argtypes = [vp, C.c_uint64, vp, C.c_uint64, C.c_uint64, vp, vp, C.c_uint64, C.c_uint32, vp, vp, vp, vp]
    boxes = np.ascontiguousarray(np.concatenate([np.ascontiguousarray(geo, f32).view(np.uint32), np.asarray(topo, np.uint32)], axis=1),
                                 np.uint32)
    refs = np.ascontiguousarray(refs, np.uint32)
    nrefs = len(refs)
    if nrefs == 0:
        refs = np.zeros(1, np.uint32)
    recs = np.ascontiguousarray(recs, f32)
    rays = np.ascontiguousarray(rays, f32)
    nrec = C.c_uint64(0)
    head = (boxes.ctypes.data, len(boxes), refs.ctypes.data, nrefs, len(recs), recs.ctypes.data, rays.ctypes.data, len(rays), g)
    rc = L.rtmi_debug_node_cull(*head, C.byref(nrec), None, None, None)
    assert rc == 0, L.rtmi_last_error()
    r = dict(records=np.zeros((nrec.value, 4), np.uint32), cert=np.zeros(len(rays), np.uint8),
             out=np.zeros((nrec.value, len(rays)), np.uint8))
    rc = L.rtmi_debug_node_cull(*head, C.byref(nrec), r["records"].ctypes.data, r["cert"].ctypes.data, r["out"].ctypes.data)
    assert rc == 0, L.rtmi_last_error()
    r["cert"] = r["cert"].astype(bool)
    return r


class Tree:
    """The tree as the walk sees it, decoded from the octree form: per inner box its record, per leaf box its first block
    and block count; parents; the packed box of every block."""

    def __init__(self, geo, topo, refs, recs):
        from test_leaf_dedup import oct_form
        self.geo, self.topo, self.refs = geo, np.asarray(topo, np.uint32), np.asarray(refs, np.uint32)
        fn, ob, wl, _ = oct_form(geo, topo, refs, len(recs))
        self.fn, self.ob = fn, ob
        nb = len(topo)
        self.inner = np.nonzero(self.topo[:, 2] == 0)[0]
        self.rec_of = np.full(nb, -1, np.int64)
        self.rec_of[self.inner] = np.arange(len(self.inner))
        self.parent = np.full(nb, -1, np.int64)
        self.first_block = np.full(nb, -1, np.int64)
        ends = np.nonzero((ob[:, 3] == 0) | ((ob[:, 3] >> 31) != 0))[0]
        for b in self.inner:
            rec = fn[self.rec_of[b]]
            w = int(rec[3])
            first, count = int(self.topo[b, 0]), int(self.topo[b, 1])
            self.parent[first:first + count] = b
            for c in range(first, first + count):
                if self.topo[c, 2]:
                    o = sum(1 << a for a in range(3) if geo[c, a] > geo[b, a])
                    if w & FN_WIDE:
                        self.first_block[c] = int(wl[int(rec[5]) * 8 + o])
                    else:
                        self.first_block[c] = int(rec[5]) + ((int(rec[6] if o < 4 else rec[7]) >> (8 * (o & 3))) & 0xFF)
        leaf = self.first_block >= 0
        self.nblocks = np.zeros(nb, np.int64)
        self.nblocks[leaf] = ends[np.searchsorted(ends, self.first_block[leaf])] + 1 - self.first_block[leaf]
        # packed block boxes and flags (rtmi_debug_ray_cull: the records k_trace_oct's LEAF step reads)
        pk = ray_cull(recs, ob, mkrays([0, 0, 0], [1, 2, 3]), 8)["packed"]
        self.blo, self.bhi = packed_box(pk)
        self.bnever = (pk[:, 3] & B.BC_NEVER) != 0

    def subtree_boxes(self):
        """per box (lo, hi, never): the union of the packed block boxes below it, bottom-up"""
        nb = len(self.topo)
        lo, hi = np.full((nb, 3), np.inf, f32), np.full((nb, 3), -np.inf, f32)
        never = np.zeros(nb, bool)
        for c in np.nonzero(self.first_block >= 0)[0]:
            s, k = self.first_block[c], self.nblocks[c]
            lo[c], hi[c], never[c] = self.blo[s:s + k].min(axis=0), self.bhi[s:s + k].max(axis=0), self.bnever[s:s + k].any()
        for b in self.inner[::-1]:
            f, n = int(self.topo[b, 0]), int(self.topo[b, 1])
            lo[b], hi[b], never[b] = lo[f:f + n].min(axis=0), hi[f:f + n].max(axis=0), never[f:f + n].any()
        return lo, hi, never

    def subtree_refs(self, b):
        if self.topo[b, 2]:
            return set(int(x) for x in self.refs[self.topo[b, 0]: self.topo[b, 0] + self.topo[b, 1]])
        out = set()
        for c in range(int(self.topo[b, 0]), int(self.topo[b, 0] + self.topo[b, 1])):
            out |= self.subtree_refs(c)
        return out


def check_records(tree, r):
    """Every node's unpacked box contains the unpacked box of every block of every leaf below it; a never-cull block below
    makes it [-inf, +inf]."""
    lo, hi, never = tree.subtree_boxes()
    nlo, nhi = packed_box(r["records"])
    ib = tree.inner
    assert len(ib) == len(nlo)
    ok = ~never[ib]
    assert (nlo[ok] <= lo[ib][ok]).all() and (nhi[ok] >= hi[ib][ok]).all(), "a node box does not contain a block box below it"
    assert np.isneginf(nlo[~ok]).all() and np.isposinf(nhi[~ok]).all(), "a never-cull block below, but a finite node box"
    assert not (r["out"][~ok] & (MISS | CUT)).any(), "a never-cull subtree missed or culled"
    return nlo, nhi


def check_brute(tree, recs, rays, r):
    """Brute force over each inner box's references: culled => none passes the f32 plane test; culled <=> missed & certified"""
    cut = (r["out"] & CUT) != 0
    assert (cut == (((r["out"] & MISS) != 0) & r["cert"][None, :])).all()
    pp = B.plane_pass(rays, recs)
    for b in tree.inner:
        ids = sorted(tree.subtree_refs(b))
        if ids:
            bad = cut[tree.rec_of[b]] & pp[ids].any(axis=0)
            assert not bad.any(), f"box {b}: culled for rays {np.nonzero(bad)[0][:8].tolist()} but a reference below passes"


# ---------------------------------------------------------------- the canonical tree
@pytest.fixture(scope="module")
def canon_nodes(canonical):
    so, raw, recs, (geo, topo, refs), ob, rays = canonical
    tree = Tree(geo, topo, refs, recs)
    return tree, node_cull(geo, topo, refs, recs, rays, G)


def test_canonical_boxes_contain_every_block_below(canonical, canon_nodes):
    tree, r = canon_nodes
    assert np.array_equal(tree.ob, canonical[4])
    nlo, nhi = check_records(tree, r)
    assert np.isfinite(nlo).all() and np.isfinite(nhi).all() and (nlo <= nhi).all()
    print(f"\ncanonical tree: {len(nlo)} node records ({len(nlo) * 16 / 1e6:.2f} MB)")


def test_canonical_culled_subtrees_hold_no_passing_reference(canonical, canon_nodes):
    """256 bounce-like rays: every reference that passes the f32 plane test for a ray lies in leaves none of whose
    ancestors is culled for that ray -- that is, no reference below a culled node passes."""
    so, raw, recs, (geo, topo, refs), ob, rays = canonical
    tree, r = canon_nodes
    assert r["cert"].mean() > 0.9
    cut = (r["out"] & CUT) != 0
    assert (cut == (((r["out"] & MISS) != 0) & r["cert"][None, :])).all()
    assert cut.any()
    pp = B.plane_pass(rays, recs)
    pp[0] = False
    leaves = np.nonzero(tree.topo[:, 2] == 1)[0]
    leaf_of_ref = np.repeat(leaves, tree.topo[leaves, 1].astype(np.int64))
    ref_ids = np.concatenate([tree.refs[tree.topo[c, 0]: tree.topo[c, 0] + tree.topo[c, 1]] for c in leaves])
    checked = 0
    for i in range(len(rays)):
        cur = np.unique(leaf_of_ref[pp[ref_ids, i]])  # the leaves that list a passing triangle
        while len(cur):
            cur = np.unique(tree.parent[cur])
            cur = cur[cur >= 0]
            bad = cut[tree.rec_of[cur], i]
            assert not bad.any(), f"ray {i}: a triangle passes the plane test below the culled boxes {cur[bad][:8].tolist()}"
            checked += len(cur)
    assert checked > 0


def _hits_f64(raw, rays):
    """(tri, t) of every geometric hit (t >= 0, inside the triangle) per ray, in float64 from the corners"""
    c = raw[:, 20:29].astype(np.float64).reshape(-1, 3, 3)
    e1, e2 = c[:, 1] - c[:, 0], c[:, 2] - c[:, 0]
    out = []
    with np.errstate(all="ignore"):
        for i in range(len(rays)):
            o, d = rays[i, 0:3].astype(np.float64), rays[i, 4:7].astype(np.float64)
            p = np.cross(d, e2)
            det = (e1 * p).sum(axis=1)
            s = o - c[:, 0]
            u = (s * p).sum(axis=1) / det
            q = np.cross(s, e1)
            v = (q * d).sum(axis=1) / det
            t = (q * e2).sum(axis=1) / det
            hit = (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= 0)
            hit[0] = False
            out.append({int(k): float(t[k]) for k in np.nonzero(hit)[0]})
    return out


def test_model_walk_loses_select_steps(canonical, canon_nodes):
    """The float64 model of the reference walk (children in ascending tmin over the whole line, the per-frame skip rule, no
    leaf memo), rerun with the PACKED node records over the 256 rays: SELECT steps and leaf visits with and without the
    cull.  A culled node costs the one step that tests it.  The cull must remove at least 15 % of the SELECT steps (half of
    the 33 % the float64 model with exact boxes gives): a vacuous test fails here."""
    so, raw, recs, (geo, topo, refs), ob, rays = canonical
    tree, r = canon_nodes
    cut = (r["out"] & CUT) != 0
    hits = _hits_f64(raw, rays)
    ctr, half = geo[:, 0:3].astype(np.float64), geo[:, 3].astype(np.float64)
    blo, bhi = ctr - half[:, None], ctr + half[:, None]
    topo = tree.topo
    tot = dict(sel=0, leaf=0, sel_in=0, leaf_in=0, culled=0)

    def walk(b, i, o, inv, inside):
        """-> best t in this box's subtree or None"""
        f, n = int(topo[b, 0]), int(topo[b, 1])
        if not inside and cut[tree.rec_of[b], i]:
            inside = True
            tot["culled"] += 1
        t1, t2 = (blo[f:f + n] - o) * inv, (bhi[f:f + n] - o) * inv
        tmin, tmax = np.minimum(t1, t2).max(axis=1), np.maximum(t1, t2).min(axis=1)
        best = None
        cand = [k for k in np.argsort(tmin, kind="stable") if tmin[k] < tmax[k]]
        steps = max(len(cand), 1)
        for j, k in enumerate(cand):
            if best is not None and not tmin[k] < best:
                steps = j + 1  # the step that finds no child to enter
                break
            c = f + int(k)
            if topo[c, 2]:
                tot["leaf"] += 1
                tot["leaf_in"] += inside
                ts = [hits[i][int(x)] for x in tree.refs[topo[c, 0]: topo[c, 0] + topo[c, 1]] if int(x) in hits[i]]
                res = min(ts) if ts else None
                assert not (inside and ts), f"ray {i}: a geometric hit below a culled box"
            else:
                res = walk(c, i, o, inv, inside)
            if res is not None and (best is None or res < best):
                best = res
        tot["sel"] += steps
        tot["sel_in"] += steps if inside else 0
        return best

    for i in range(len(rays)):
        walk(0, i, rays[i, 0:3].astype(np.float64), 1.0 / rays[i, 4:7].astype(np.float64), False)
    n = len(rays)
    sel_cull, leaf_cull = tot["sel"] - tot["sel_in"] + tot["culled"], tot["leaf"] - tot["leaf_in"]
    print(f"\nmodel walk, {n} rays, packed node records: SELECT steps per ray {tot['sel'] / n:.1f} -> {sel_cull / n:.1f} "
          f"({1 - sel_cull / tot['sel']:.3f} removed), leaf visits per ray {tot['leaf'] / n:.1f} -> {leaf_cull / n:.1f}, "
          f"culled nodes per ray {tot['culled'] / n:.2f}")
    assert sel_cull <= 0.85 * tot["sel"], f"the node cull removes only {1 - sel_cull / tot['sel']:.3f} of the SELECT steps"


# ---------------------------------------------------------------- trees built by hand
def hand_tree(lists_a, list_root=(), third_level=None):
    """Root (centre 0, half 1) with a leaf in octant 0 (list_root) and an inner box A in octant 7 (centre 0.5, half 0.5) whose
    leaves in octants 0 and 7 carry lists_a[0], lists_a[1]; third_level: lists of two more leaves below an inner box in
    octant 3 of A.  Box order: parents before children, children in octant order."""
    geo = [[0, 0, 0, 1], [-0.5, -0.5, -0.5, 0.5], [0.5, 0.5, 0.5, 0.5]]
    topo = [[1, 2, 0, 0], None, None]
    refs = []

    def leaf(lst, depth):
        row = [len(refs), len(lst), 1, depth]
        refs.extend(lst)
        return row

    topo[1] = leaf(list_root, 1)
    kids = [([0.25, 0.25, 0.25, 0.25], lists_a[0])]
    if third_level is not None:
        kids.append(([0.75, 0.75, 0.25, 0.25], None))
    kids.append(([0.75, 0.75, 0.75, 0.25], lists_a[1]))
    topo[2] = [3, len(kids), 0, 1]
    inner_at = None
    for g, lst in kids:
        geo.append(g)
        if lst is None:
            inner_at = len(topo)
            topo.append(None)
        else:
            topo.append(leaf(lst, 2))
    if third_level is not None:
        topo[inner_at] = [len(topo), 2, 0, 2]
        geo += [[0.625, 0.625, 0.125, 0.125], [0.875, 0.875, 0.375, 0.125]]
        topo += [leaf(third_level[0], 3), leaf(third_level[1], 3)]
    return np.array(geo, f32), np.array(topo, np.uint32), np.array(refs, np.uint32)


def scattered_rays(rng, n, centre, spread):
    return mkrays(np.asarray(centre) + rng.normal(size=(n, 3)) * spread, unit(rng.normal(size=(n, 3))))


def test_lists_that_reach_far_outside_their_boxes():
    """One inner node over two leaves whose lists name triangles far outside the leaves' (and the root's) boxes: the record
    bounds the REFERENCES, not the octree box, and the cull agrees with brute force."""
    rng = np.random.default_rng(21)
    c = np.concatenate([rng.uniform(0.1, 0.9, (6, 3)), rng.uniform(-30, 30, (6, 3))])
    recs = mkrecs(c, rng.uniform(0.02, 0.2, 12), rng.normal(size=(12, 3)))
    geo, topo, refs = hand_tree(([1, 2, 7, 8, 9], [3, 4, 5, 6, 10, 11, 12, 1, 2]), [2, 8])
    tree = Tree(geo, topo, refs, recs)
    rays = np.concatenate([scattered_rays(rng, 256, [0.5, 0.5, 0.5], 3.0), scattered_rays(rng, 256, [0, 0, 0], 40.0)])
    r = node_cull(geo, topo, refs, recs, rays)
    nlo, nhi = check_records(tree, r)
    check_brute(tree, recs, rays, r)
    # A's box reaches the far references: well beyond A's own cell [0, 1]^3
    assert (nlo[1] < -5).any() and (nhi[1] > 5).any()
    cut = (r["out"] & CUT) != 0
    assert cut[1].any() and not cut[1].all() and cut[0].any()


def test_three_levels_and_monotone_boxes():
    rng = np.random.default_rng(22)
    c = rng.uniform(-2, 2, (16, 3))
    recs = mkrecs(c, rng.uniform(0.02, 0.3, 16), rng.normal(size=(16, 3)))
    geo, topo, refs = hand_tree(([1, 2, 3], [4, 5, 6, 7]), [8, 9], ([10, 11, 12, 13, 14], [15, 16, 1]))
    tree = Tree(geo, topo, refs, recs)
    rays = scattered_rays(rng, 512, [0, 0, 0], 4.0)
    r = node_cull(geo, topo, refs, recs, rays)
    nlo, nhi = check_records(tree, r)
    check_brute(tree, recs, rays, r)
    assert len(nlo) == 3
    assert (nlo[0] <= nlo[1]).all() and (nlo[1] <= nlo[2]).all() and (nhi[0] >= nhi[1]).all() and (nhi[1] >= nhi[2]).all()
    assert ((r["out"] & CUT) != 0)[2].any()


def test_three_level_scene_of_the_gpu_test_culls_at_depth_1():
    """The hand-made scene of test_node_cull.py as the builder makes it: the depth-1 inner box lists a sliver that reaches
    far outside its cell, and bounce-like rays off the front triangle (towards the camera) cull that box while the root,
    whose box they start in, is kept."""
    from conftest import OracleApi
    from test_node_cull import recipe_three_levels
    so = recipe_three_levels()(OracleApi(B._orc()))
    raw, _, _ = so.triangles()
    recs = np.zeros((len(raw), 8), f32)
    recs[:, 0:3], recs[:, 3], recs[:, 4:7] = raw[:, 0:3], raw[:, 6], raw[:, 3:6]
    geo, topo, refs = so.tree_flatten()
    tree = Tree(geo, topo, refs, recs)
    d1 = [b for b in tree.inner if topo[b, 3] == 1]
    assert len(tree.inner) == 3 and len(d1) == 1 and max(topo[:, 3]) == 3
    sliver = len(raw) - 2
    assert sliver in tree.subtree_refs(d1[0]) and (raw[sliver, 20:29].reshape(3, 3) < geo[d1[0], 0:3] - geo[d1[0], 3]).any()
    rng = np.random.default_rng(27)
    n = 256
    w = rng.dirichlet([1, 1, 1], n)
    o = w @ raw[len(raw) - 1, 20:29].reshape(3, 3).astype(np.float64)
    d = unit(rng.normal(size=(n, 3)))
    d[:, 2] = -np.abs(d[:, 2])
    rays = mkrays(o, d)
    r = node_cull(geo, topo, refs, recs, rays)
    nlo, nhi = check_records(tree, r)
    check_brute(tree, recs, rays, r)
    k = tree.rec_of[d1[0]]
    assert (nlo[k] < geo[d1[0], 0:3] - 1.5 * geo[d1[0], 3]).any(), "the depth-1 box does not reach outside its cell"
    cut = (r["out"] & CUT) != 0
    assert cut[k].mean() > 0.5 and not cut[0].any()


def test_never_cull_record_below_makes_the_box_infinite():
    rng = np.random.default_rng(23)
    c = rng.uniform(0.1, 0.9, (8, 3))
    recs = mkrecs(c, [0.05] * 8, rng.normal(size=(8, 3)))
    recs[5, 3] = np.nan  # r2 of a reference of A's second leaf: its block is never-cull
    geo, topo, refs = hand_tree(([1, 2], [3, 4, 5, 6, 7]), [8], ([1], [2]))
    tree = Tree(geo, topo, refs, recs)
    assert tree.bnever.any()
    rays = scattered_rays(rng, 256, [0.5, 0.5, 0.5], 5.0)
    r = node_cull(geo, topo, refs, recs, rays)
    nlo, nhi = check_records(tree, r)
    # the root and A are infinite and never culled; the third-level box below A holds no such block and is still culled
    assert np.isinf(nlo[0]).all() and np.isinf(nlo[1]).all() and np.isfinite(nlo[2]).all()
    assert not (r["out"][0:2] & (MISS | CUT)).any()
    assert (r["out"][2] & CUT).any()
    check_brute(tree, recs, rays, r)


def test_subtree_without_a_real_reference():
    rng = np.random.default_rng(24)
    recs = mkrecs(rng.uniform(-0.9, -0.1, (3, 3)), [0.05] * 3, rng.normal(size=(3, 3)))
    geo, topo, refs = hand_tree(([], []), [1, 2, 3])
    tree = Tree(geo, topo, refs, recs)
    rays = scattered_rays(rng, 128, [0, 0, 0], 3.0)
    r = node_cull(geo, topo, refs, recs, rays)
    nlo, nhi = check_records(tree, r)
    assert (nlo[1] > nhi[1]).all(), "a subtree without a reference must keep the empty box"
    assert np.isfinite(nlo[0]).all() and (nlo[0] <= nhi[0]).all()
    check_brute(tree, recs, rays, r)


def test_origin_inside_the_subtree_box_is_never_culled():
    rng = np.random.default_rng(25)
    c = rng.uniform(-3, 3, (12, 3))
    recs = mkrecs(c, rng.uniform(0.05, 0.3, 12), rng.normal(size=(12, 3)))
    geo, topo, refs = hand_tree(([1, 2, 3, 4, 5], [6, 7, 8]), [9, 10], ([11], [12]))
    tree = Tree(geo, topo, refs, recs)
    r0 = node_cull(geo, topo, refs, recs, mkrays([0, 0, 0], [1, 2, 3]))
    nlo, nhi = packed_box(r0["records"])
    for k in range(3):
        o = rng.uniform(nlo[k], nhi[k], (64, 3)).astype(f32)
        o[0], o[1] = nlo[k], nhi[k]  # on the corners
        rays = mkrays(o, unit(rng.normal(size=(64, 3))))
        r = node_cull(geo, topo, refs, recs, rays)
        assert not (r["out"][k] & (MISS | CUT)).any(), f"record {k}: culled for an origin inside its box"
        check_brute(tree, recs, rays, r)


def test_grazing_node_box_face_edge_corner():
    """Rays through points within +-4 ulp of a face, an edge and a corner of the PACKED node box, towards it and away."""
    rng = np.random.default_rng(26)
    ncut = nkept = 0
    for it in range(30):
        c = rng.uniform(-3, 3, (9, 3))
        recs = mkrecs(c, rng.uniform(0.05, 0.5, 9), rng.normal(size=(9, 3)))
        geo, topo, refs = hand_tree(([1, 2, 3, 4, 5], [6, 7]), [8, 9])
        tree = Tree(geo, topo, refs, recs)
        nlo, nhi = packed_box(node_cull(geo, topo, refs, recs, mkrays([0, 0, 0], [1, 1, 1]))["records"])
        lo, hi = nlo[1].astype(np.float64), nhi[1].astype(np.float64)
        rays = []
        for naxes in (1, 2, 3):
            axes = rng.permutation(3)[:naxes]
            side = rng.integers(0, 2, 3)
            for k in (-4, -2, -1, 0, 1, 2, 4):
                p = rng.uniform(lo, hi).astype(f32)
                for a in axes:
                    p[a] = B._ulps(f32(hi[a] if side[a] else lo[a]), k if side[a] else -k)
                d = rng.normal(size=3)
                d[axes] *= 1e-3
                d = unit(d)
                s = rng.uniform(0.5, 5.0)
                o = (p.astype(np.float64) - s * d.astype(np.float64)).astype(f32)
                rays.append(np.concatenate([o, [0], d, [0]]))
                rays.append(np.concatenate([o, [0], -d, [0]]))
        rays = np.array(rays, f32)
        r = node_cull(geo, topo, refs, recs, rays)
        check_records(tree, r)
        check_brute(tree, recs, rays, r)
        ncut += int(((r["out"][1] & CUT) != 0).sum()); nkept += int(((r["out"][1] & CUT) == 0).sum())
    assert ncut > 0 and nkept > 0


def test_rays_the_certificate_refuses_are_never_culled():
    """Nonzero lane 3, zero / denormal / huge direction components, NaN and far origins, and a direction perpendicular to a
    normal of the scene: the box may be missed, the subtree is not culled."""
    recs = mkrecs([[5, 5, 5], [5.2, 5.1, 4.9], [6, 5, 5]], [0.1, 0.1, 0.1], [[0, 0, 1], [1, -1, 0], [1, 2, 3]])
    geo, topo, refs = hand_tree(([1], [2]), [3])
    good = mkrays([[0, 0, 0]], [unit([1, 2, -3])])
    r = node_cull(geo, topo, refs, recs, good)
    assert r["cert"].all() and (r["out"] & CUT).all()
    bad = []
    for col, val in ((3, 1e-3), (7, 1e-3), (3, np.nan), (7, -1.0), (0, np.nan), (5, np.nan), (0, 1e16), (1, -np.inf),
                     (4, 0.0), (5, -0.0), (6, 1e-42), (4, 1e-14), (4, np.inf), (4, 1e30)):
        x = good.copy()
        x[0, col] = f32(val)
        bad.append(x[0])
    for s in (1e-30, 1e-20, 1e-11, 1e11, 1e30):
        x = good.copy()
        x[0, 4:7] *= f32(s)
        bad.append(x[0])
    bad.append(mkrays([[0, 0, 9]], [unit([1, 1, 1e-3])])[0])  # perpendicular to the normal (1, -1, 0)
    r = node_cull(geo, topo, refs, recs, np.array(bad, f32))
    assert not r["cert"].any() and not (r["out"] & CUT).any()
    assert (r["out"][:, -1] & MISS).all()  # (the box IS missed: only the certificate keeps the subtree)
