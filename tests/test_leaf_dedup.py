"""Leaf lists stored once (rtmi_scene_create's exact-octree form) and the octree walk's one-entry leaf memo.

CPU: the layout the host builds, decoded with the walk's own rules, against the oracle's tree.
-m gpu: renders and traces that go through the memo stay bit-exact, counters included."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_bits_equal, build_pair, recipe_canonical, recipe_grid

RTMI_OK, RTMI_ERR_UNSUPPORTED = 0, 3
FN_WIDE = 0x10000


def _R():
    from rust_raytrace_amd import raytrace as R
    return R


def _orc():
    from oracle import orc
    return orc


def oct_form(geo, topo, refs, ntris):
    """rtmi_debug_oct_form: (fnodes (n, 8) u32, oblocks (m, 4) u32, wlinks u32, FN_WIDE boxes) for a flattened tree."""
    from rust_raytrace_amd import _ffi
    L = _ffi.lib()
    L.rtmi_debug_oct_form.restype = C.c_int
    L.rtmi_debug_oct_form.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    # rtmi_box_t = (orig[3], len2, first, count, is_leaf, depth): the flattened tree's geo | topo rows
    boxes = np.ascontiguousarray(np.concatenate([np.ascontiguousarray(geo, np.float32).view(np.uint32), topo], axis=1), np.uint32)
    refs = np.ascontiguousarray(refs, np.uint32)
    if refs.size == 0:
        refs = np.zeros(1, np.uint32)
    sizes = np.zeros(4, np.uint64)
    args = (boxes.ctypes.data, boxes.shape[0], refs.ctypes.data, len(refs), ntris)
    rc = L.rtmi_debug_oct_form(*args, None, None, None, sizes.ctypes.data)
    assert rc == RTMI_OK, L.rtmi_last_error()
    fn = np.zeros((int(sizes[0]), 4), np.uint32)
    ob = np.zeros((int(sizes[1]), 4), np.uint32)
    wl = np.zeros(max(int(sizes[2]), 1), np.uint32)
    rc = L.rtmi_debug_oct_form(*args, fn.ctypes.data, ob.ctypes.data, wl.ctypes.data, sizes.ctypes.data)
    assert rc == RTMI_OK, L.rtmi_last_error()
    return fn.reshape(-1, 8), ob, wl[: int(sizes[2])], int(sizes[3])


def decode_leaves(geo, topo, fn, ob, wl):
    """First block and decoded list of every leaf box, found the way oct_walk finds them: from the parent's record
    (FN_WIDE: wlinks; else base + byte offset of the octant), then blocks up to the terminator (a 0 index, or bit 31 of a
    full block's 4th index), 0s being padding.  Also checks the inner-child links and the centres."""
    gbits = np.ascontiguousarray(geo, np.float32).view(np.uint32)
    inner = np.nonzero(topo[:, 2] == 0)[0]
    rec_of = {int(b): r for r, b in enumerate(inner)}
    first_block, lists = {}, {}
    for b in inner:
        rec = fn[rec_of[int(b)]]
        assert list(rec[:3]) == list(gbits[b, :3]), f"box {b}: centre"
        w = int(rec[3])
        first, count = int(topo[b, 0]), int(topo[b, 1])
        leafmask = (w >> 8) & 0xFF
        for c in range(first, first + count):
            oct_ = sum(1 << a for a in range(3) if geo[c, a] > geo[b, a])
            assert (w >> oct_) & 1, f"box {b}: child {c} not in the present mask"
            below = (1 << oct_) - 1
            if topo[c, 2]:
                assert (leafmask >> oct_) & 1
                if w & FN_WIDE:
                    lb = int(wl[int(rec[5]) * 8 + oct_])
                else:
                    lb = int(rec[5]) + ((int(rec[6] if oct_ < 4 else rec[7]) >> (8 * (oct_ & 3))) & 0xFF)
                ids, k = [], lb
                while True:
                    blk = ob[k]
                    v = [int(blk[0]), int(blk[1]), int(blk[2]), int(blk[3]) & 0x7FFFFFFF]
                    nz = [x for x in v if x != 0]
                    assert v[: len(nz)] == nz, f"block {k}: a 0 before a triangle index"
                    ids += nz
                    if blk[3] == 0 or blk[3] >> 31:
                        break
                    k += 1
                first_block[c] = lb
                lists[c] = tuple(ids)
            else:
                assert not (leafmask >> oct_) & 1
                assert int(rec[4]) + bin((w & ~leafmask & 0xFF) & below).count("1") == rec_of[c], f"box {b}: inner link"
    return first_block, lists


def _check_layout(name, geo, topo, refs, ntris):
    fn, ob, wl, nwide = oct_form(geo, topo, refs, ntris)
    first_block, lists = decode_leaves(geo, topo, fn, ob, wl)
    leaves = np.nonzero(topo[:, 2] == 1)[0]
    assert len(first_block) == len(leaves)
    by_list = {}
    for c in leaves:
        want = tuple(int(x) for x in refs[topo[c, 0]: topo[c, 0] + topo[c, 1]])
        assert lists[c] == want, f"{name}: leaf {c} decodes to another list"
        by_list.setdefault(want, set()).add(first_block[c])
    # each distinct list is stored once: equal lists share a first block, different lists never do
    assert all(len(s) == 1 for s in by_list.values()), f"{name}: a list is stored twice"
    assert len({next(iter(s)) for s in by_list.values()}) == len(by_list), f"{name}: two lists share a first block"
    assert len(ob) == sum(max(1, -(-len(l) // 4)) for l in by_list), f"{name}: blocks nobody points at"
    nref_blocks = sum(max(1, -(-int(topo[c, 1]) // 4)) for c in leaves)
    print(f"\n{name}: {len(leaves)} leaves, {len(by_list)} distinct lists, {len(ob)} reference blocks "
          f"(one run per leaf: {nref_blocks}), {len(fn)} inner boxes, {nwide} FN_WIDE")
    return by_list, fn, ob


def test_canonical_leaf_lists_stored_once(canonical_pair):
    so, _ = canonical_pair
    geo, topo, refs = so.tree_flatten()
    by_list, _, _ = _check_layout("canonical (10, 19)", geo, topo, refs, so.num_tris())
    assert len(by_list) < (topo[:, 2] == 1).sum()  # the builder's lists repeat: there is something to share


def test_grid_leaf_lists_stored_once():
    so, _ = build_pair(recipe_grid())
    geo, topo, refs = so.tree_flatten()
    _check_layout("grid (config 5)", geo, topo, refs, so.num_tris())


def test_oct_form_rejects_non_octree():
    so, _ = build_pair(recipe_canonical(accel="trivial"))
    geo, topo, refs = so.tree_flatten()
    with pytest.raises(AssertionError, match="root box is a leaf"):
        oct_form(geo, topo, refs, so.num_tris())


# ---------------------------------------------------------------- -m gpu
def _debug_counters(sp):
    from rust_raytrace_amd import _ffi
    L = _ffi.lib()
    L.rth_debug_counters.argtypes = [C.c_void_p, C.c_void_p]
    out = (C.c_ulonglong * 16)()
    L.rth_debug_counters(sp.h, out)
    return list(out)


@pytest.mark.gpu
def test_memo_count_render_bit_exact(canonical_pair):
    """Counting build: image bits and all six work counters equal the oracle's (a memo hit adds the skipped list's plane
    and edge tests), and the memo was used."""
    so, sp = canonical_pair
    orc, R = _orc(), _R()
    w, h, spp, row0, nrows = 64, 64, 4, 16, 24
    vo = orc.canonical_viewport(w, h)
    vp = R.canonical_viewport(w, h, 5, spp)
    ref, cn = so.render(w, h, vo, 5, spp, seed=3, row0=row0, nrows=nrows, threads=8)
    img = np.zeros((nrows, w, 4), np.float32)
    ctx = R.HipRayCaster(seed=3, options=R.OPT_COUNTERS).walk_rows(vp, sp, row0, nrows, img)
    assert_bits_equal(ref, img, "image")
    for k in ("rays", "box_tests", "tri_tests", "full_tests", "nodes", "leaves"):
        assert ctx.stats[k] == cn[k], f"work counter {k}: device {ctx.stats[k]} vs oracle {cn[k]}"
    d = _debug_counters(sp)
    print(f"\nleaf visits {d[12]}, memo hits {d[13]}, plane tests skipped {d[14]}, edge tests skipped {d[15]}")
    assert d[13] > 0 and d[14] > 0 and d[12] > d[13]


@pytest.mark.gpu
def test_memo_independent_of_queue_order(canonical_pair):
    """The same rays traced in two queue orders (so lanes take different rays one after another): identical per-ray
    results, and the oracle's.  A memo carried from one ray to the next would show here."""
    so, sp = canonical_pair
    rng = np.random.default_rng(11)
    n = 30000
    o4 = np.zeros((n, 4), np.float32)
    d4 = np.zeros((n, 4), np.float32)
    o4[:, :3] = rng.uniform(-5, 5, (n, 3)) + np.array([0, 0, 5.5])
    d = rng.normal(size=(n, 3))
    d4[:, :3] = d / np.linalg.norm(d, axis=1, keepdims=True)
    perm = rng.permutation(n)
    R = _R()
    tri_a, t_a, face_a, _ = R.HipRayCaster().trace(sp, o4, d4)
    tri_b, t_b, face_b, _ = R.HipRayCaster().trace(sp, o4[perm], d4[perm])
    inv = np.empty(n, np.int64)
    inv[perm] = np.arange(n)
    assert np.array_equal(tri_a, tri_b[inv])
    assert_bits_equal(t_a, t_b[inv], "hit time")
    assert np.array_equal(face_a, face_b[inv])
    tri_o, t_o, face_o, _ = so.trace(o4, d4)
    assert np.array_equal(tri_o, tri_a)
    hit = tri_o != 0
    assert_bits_equal(t_o[hit], t_a[hit], "hit time vs oracle")
    assert np.array_equal(face_o[hit], face_a[hit])


@pytest.mark.gpu
def test_memo_parallel_rays_match_oracle(canonical_pair):
    """Rays in the plane of a triangle that sits in a list several leaves share (norm . dir exactly 0: t is NaN from an
    origin on the plane, +-inf elsewhere) -- the NaN results the memo stores and hands out -- against the oracle."""
    so, sp = canonical_pair
    geo, topo, refs = so.tree_flatten()
    by_list, _, _ = _check_layout("canonical (10, 19)", geo, topo, refs, so.num_tris())
    rec, _, _ = so.triangles()
    leaves = np.nonzero(topo[:, 2] == 1)[0]
    shared = {}
    for c in leaves:
        l = tuple(int(x) for x in refs[topo[c, 0]: topo[c, 0] + topo[c, 1]])
        shared[l] = shared.get(l, 0) + 1
    tris = sorted({t for l, k in shared.items() if k >= 3 and l for t in l})
    tris = np.array(tris[:: max(1, len(tris) // 48)][:48])
    assert len(tris) > 0
    c, nrm = rec[tris, 0:3], rec[tris, 3:6]
    o, dd = [], []
    for s in (1.0, -1.0):
        for off in (0.0, 0.03):
            d = np.zeros((len(tris), 4), np.float32)
            d[:, 0], d[:, 1] = s * nrm[:, 1], -s * nrm[:, 0]  # n.x * n.y + n.y * (-n.x) + n.z * 0 == 0 exactly
            oo = np.zeros((len(tris), 4), np.float32)
            oo[:, :3] = c + np.float32(off) * nrm
            o.append(oo)
            dd.append(d)
    o4, d4 = np.concatenate(o), np.concatenate(dd)
    tri_o, t_o, face_o, cn = so.trace(o4, d4)
    tri_g, t_g, face_g, st = _R().HipRayCaster(options=_R().OPT_COUNTERS).trace(sp, o4, d4)
    assert np.array_equal(tri_o, tri_g)
    hit = tri_o != 0
    assert_bits_equal(t_o[hit], t_g[hit], "hit time")
    assert np.array_equal(face_o[hit], face_g[hit])
    for k in ("rays", "box_tests", "tri_tests", "full_tests", "nodes", "leaves"):
        assert st[k] == cn[k], f"work counter {k}: device {st[k]} vs oracle {cn[k]}"
