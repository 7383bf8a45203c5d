"""Block cull of k_trace_oct (trace_oct.hpp, block_culls): whenever the predicate says "cull" for a reference block and a ray,
the exact plane test rejects every real reference of that block for that ray.  CPU only: rtmi_debug_block_cull builds the
cull records and evaluates the predicate on the host with the kernel's own __host__ __device__ functions; the exact test
is an f32 restatement of the plane part of Triangle::intersects and, for a sample, the oracle's own trace."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "tests", "golden", "teapot_tri.obj")
f32 = np.float32
BC_END, BC_NEVER = 1, 2
MISS, SIGN, CUT = 1, 2, 4


def _orc():
    from oracle import orc
    return orc


def block_cull(recs, blocks, rays):
    """recs (m, 8) f32 (incenter.xyz, r2, norm.xyz, 0), record 0 the sentinel; blocks (nb, 4) u32 in the form of oblocks;
    rays (n, 8) f32 (o.xyzw, d.xyzw) -> (cull records (nb, 8) u32, rayok (n,) bool, out (nb, n) u8: MISS | SIGN | CUT)."""
    from rust_raytrace_amd import _ffi
    L = _ffi.lib()
    L.rtmi_debug_block_cull.restype = C.c_int
    L.rtmi_debug_block_cull.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                        C.c_void_p, C.c_void_p, C.c_void_p]
    recs = np.ascontiguousarray(recs, f32)
    blocks = np.ascontiguousarray(blocks, np.uint32).reshape(-1, 4)
    rays = np.ascontiguousarray(rays, f32)
    records = np.zeros((len(blocks), 8), np.uint32)
    rayok = np.zeros(len(rays), np.uint8)
    out = np.zeros((len(blocks), len(rays)), np.uint8)
    rc = L.rtmi_debug_block_cull(recs.ctypes.data, len(recs), blocks.ctypes.data, len(blocks), rays.ctypes.data, len(rays),
                                 records.ctypes.data, rayok.ctypes.data, out.ctypes.data)
    assert rc == 0
    return records, rayok.astype(bool), out


def plane_pass(rays, recs):
    """The plane part of Triangle::intersects (raytrace.rs:400-439) in f32, in the operation order of the oracle and the
    kernels (lane 3 included): True where `t >= 0` (or NaN) and `len2(ip) <= r2` (or NaN), shape (m, n)."""
    o, d = rays[None, :, 0:4], rays[None, :, 4:8]
    c, r2, n = recs[:, None, 0:3], recs[:, None, 3], recs[:, None, 4:7]
    with np.errstate(all="ignore"):
        a = c - o[..., :3]
        num = ((((f32(0) + n[..., 0] * a[..., 0]) + n[..., 1] * a[..., 1]) + n[..., 2] * a[..., 2])
               + f32(0) * (f32(0) - o[..., 3]))
        den = ((((f32(0) + n[..., 0] * d[..., 0]) + n[..., 1] * d[..., 1]) + n[..., 2] * d[..., 2]) + f32(0) * d[..., 3])
        t = num / den
        p = d * t[..., None] + o
        ip = p[..., :3] - c
        pw = p[..., 3]
        l2 = ((ip[..., 0] * ip[..., 0] + ip[..., 1] * ip[..., 1]) + ip[..., 2] * ip[..., 2]) + pw * pw
        return ~(t < 0) & ~(l2 > r2)


def block_pass(rays, recs, blocks):
    """(nb, n): some real reference of the block passes the exact plane test for the ray"""
    blocks = np.asarray(blocks, np.uint32).reshape(-1, 4) & np.uint32(0x7FFFFFFF)
    pp = plane_pass(rays, recs)
    pp[0] = False  # index 0 is padding
    return pp[blocks[:, 0]] | pp[blocks[:, 1]] | pp[blocks[:, 2]] | pp[blocks[:, 3]]


def check(rays, recs, blocks):
    """0 violations; returns (records, rayok, out)"""
    records, rayok, out = block_cull(recs, blocks, rays)
    cut = (out & CUT) != 0
    assert not cut[:, ~rayok].any(), "a block culled for a ray that block_cull_ray() refuses"
    never = ((records[:, 7] >> 16) & BC_NEVER) != 0
    assert not cut[never].any(), "a never-cull block culled"
    assert (((out & (MISS | SIGN)) == (MISS | SIGN)) & rayok[None, :] & ~never[:, None] == cut).all()
    bad = cut & block_pass(rays, recs, blocks)
    assert not bad.any(), f"culled but a reference passed: (block, ray) {np.argwhere(bad)[:10].tolist()}"
    return records, rayok, out


def unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(f32)


def mkrays(o, d):
    o, d = np.atleast_2d(np.asarray(o, f32)), np.atleast_2d(np.asarray(d, f32))
    n = max(len(o), len(d))
    rays = np.zeros((n, 8), f32)
    rays[:, 0:3], rays[:, 4:7] = o, d
    return rays


def mkrecs(c, r, nrm):
    """records 1.. from incenters, radii and (unnormalised) normals; record 0 the sentinel"""
    c = np.atleast_2d(np.asarray(c, f32))
    recs = np.zeros((len(c) + 1, 8), f32)
    with np.errstate(over="ignore"):
        recs[1:, 0:3], recs[1:, 3], recs[1:, 4:7] = c, np.asarray(r, f32) * np.asarray(r, f32), unit(nrm)
    return recs


def one_per_block(m):
    b = np.zeros((m, 4), np.uint32)
    b[:, 0] = np.arange(1, m + 1)
    return b


def box_of(records):
    r = records.view(f32)
    return r[:, 0:3].astype(np.float64), np.stack([r[:, 3], r[:, 4], r[:, 5]], axis=1).astype(np.float64)


# ---------------------------------------------------------------- the canonical tree
@pytest.fixture(scope="module")
def canonical():
    from test_leaf_dedup import oct_form
    orc = _orc()
    so = orc.canonical_scene(OBJ)
    raw, _, _ = so.triangles()
    recs = np.zeros((len(raw), 8), f32)
    recs[:, 0:3], recs[:, 3], recs[:, 4:7] = raw[:, 0:3], raw[:, 6], raw[:, 3:6]
    geo, topo, refs = so.tree_flatten()
    _, ob, _, _ = oct_form(geo, topo, refs, so.num_tris())
    # bounce-like rays: origins on scene triangles, directions uniform over the hemisphere of the normal
    rng = np.random.default_rng(11)
    n = 256
    tri = rng.integers(1, len(raw), n)
    d = unit(rng.normal(size=(n, 3)))
    flip = (d.astype(np.float64) * raw[tri, 3:6]).sum(axis=1) < 0
    d[flip] = -d[flip]
    rays = mkrays(raw[tri, 0:3], d)
    return so, raw, recs, (geo, topo, refs), ob, rays


def test_canonical_blocks_sound_and_not_vacuous(canonical):
    """Every block of the canonical tree against 256 bounce-like rays: no culled block holds a passing reference, and of
    the (visited block, ray) pairs -- the blocks of the leaves whose box the ray's line crosses in front of its closest hit,
    which is what the walk scans -- at least 30 % are culled (measured: 64.0 %, the box missed for 80.1 %; 84.2 % of all
    (block, ray) pairs)."""
    so, raw, recs, (geo, topo, refs), ob, rays = canonical
    records, rayok, out = check(rays, recs, ob)
    assert rayok.all()
    cut = (out & CUT) != 0
    # leaf -> blocks of its list (each distinct list is stored once: find it by content)
    ends = (ob[:, 3] == 0) | ((ob[:, 3] >> 31) != 0)
    starts = np.concatenate([[0], np.nonzero(ends)[0][:-1] + 1])
    nblk = np.nonzero(ends)[0] + 1 - starts
    first_of = {}
    for s, k in zip(starts, nblk):
        ids = (ob[s:s + k] & np.uint32(0x7FFFFFFF)).ravel()
        first_of[ids[ids != 0].tobytes()] = (int(s), int(k))
    leaves = np.nonzero(topo[:, 2] == 1)[0]
    lf = np.array([first_of[np.ascontiguousarray(refs[topo[c, 0]: topo[c, 0] + topo[c, 1]], np.uint32).tobytes()] for c in leaves])
    # visited leaves: BoundingBox::collides on the whole line (the reference walks both half-lines), tmin < closest hit's t
    tri_hit, thit, _, _ = so.trace(rays[:, 0:4], rays[:, 4:8])
    tlim = np.where(tri_hit != 0, thit, np.inf).astype(np.float64)
    o, inv = rays[:, 0:3].astype(np.float64), 1.0 / rays[:, 4:7].astype(np.float64)
    ctr, half = geo[leaves, 0:3].astype(np.float64), geo[leaves, 3].astype(np.float64)
    blo, bhi = np.ascontiguousarray((ctr - half[:, None]).T), np.ascontiguousarray((ctr + half[:, None]).T)  # (3, leaves)
    o, inv = o[:, :, None], inv[:, :, None]
    csum = np.concatenate([np.zeros((1, cut.shape[1]), np.int32), np.cumsum(cut, axis=0, dtype=np.int32)])
    visited = culled = seen_aabb = 0
    miss = np.concatenate([np.zeros((1, cut.shape[1]), np.int32), np.cumsum((out & MISS) != 0, axis=0, dtype=np.int32)])
    for i in range(len(rays)):
        t1, t2 = (blo - o[i]) * inv[i], (bhi - o[i]) * inv[i]
        tmin, tmax = np.minimum(t1, t2).max(axis=0), np.maximum(t1, t2).min(axis=0)
        v = (tmin < tmax) & (tmin < tlim[i])
        visited += int(lf[v, 1].sum())
        culled += int((csum[lf[v, 0] + lf[v, 1], i] - csum[lf[v, 0], i]).sum())
        seen_aabb += int((miss[lf[v, 0] + lf[v, 1], i] - miss[lf[v, 0], i]).sum())
    print(f"\ncanonical tree: {len(ob)} blocks x {len(rays)} rays: {cut.mean():.3f} of all pairs culled; visited pairs "
          f"{visited} ({visited / len(rays):.1f} blocks per ray), box missed {seen_aabb / visited:.3f}, culled {culled / visited:.3f}")
    assert culled >= 0.30 * visited, f"only {culled} of {visited} visited (block, ray) pairs culled"


def test_oracle_rejects_culled(canonical):
    """For culled (block, ray) pairs whose triangles lie nearest to the ray, the oracle's own trace of a one-triangle scene
    misses."""
    orc = _orc()
    so, raw, recs, _, ob, rays = canonical
    rays = rays[:8]
    _, _, out = block_cull(recs, ob, rays)
    ids = ob & np.uint32(0x7FFFFFFF)
    checked = 0
    for i in range(len(rays)):
        c = recs[:, 0:3].astype(np.float64) - rays[i, 0:3]
        dist = np.linalg.norm(np.cross(c, rays[i, 4:7].astype(np.float64)), axis=1) - np.sqrt(recs[:, 3])
        dist[0] = np.inf
        bdist = np.where(ids != 0, dist[ids], np.inf).min(axis=1)
        pick = [int(b) for b in np.argsort(bdist) if out[b, i] & CUT][:6]
        for b in pick:
            for j in ids[b][ids[b] != 0]:
                one = orc.Scene(with_dummy=True)
                one.add_triangle(raw[j, 20:29], orc.Surface(orc.MATTE, orc.make_color(1, 2, 3), 0.2), float(raw[j, 19]))
                one.build_trivial_bounding_box([0.0, 0.0, 20.1], 20.0)
                tri, _, _, _ = one.trace(rays[i:i + 1, 0:4], rays[i:i + 1, 4:8])
                assert (tri == 0).all(), f"block {b} culled for ray {i} but the oracle hits triangle {j}"
                checked += 1
    assert checked > 0


# ---------------------------------------------------------------- adversarial cases
def _ulps(x, k):
    x = np.asarray(x, f32).copy()
    for _ in range(abs(k)):
        x = np.nextafter(x, f32(np.inf if k > 0 else -np.inf))
    return x


def test_grazing_box_face_and_corner():
    """Rays through points a few ulp inside and outside a face, an edge and a corner of the stored box."""
    rng = np.random.default_rng(5)
    ncut = nkept = 0
    for it in range(60):
        c = rng.uniform(-3, 3, 3)
        recs = mkrecs([c], rng.uniform(0.05, 0.5), rng.normal(size=3))
        blocks = one_per_block(1)
        records, _, _ = block_cull(recs, blocks, mkrays([0, 0, 0], [1, 1, 1]))
        lo, hi = box_of(records)
        lo, hi = lo[0], hi[0]
        rays = []
        for naxes in (1, 2, 3):  # face, edge, corner
            axes = rng.permutation(3)[:naxes]
            side = rng.integers(0, 2, 3)
            for k in (-4, -2, -1, 0, 1, 2, 4):
                p = rng.uniform(lo, hi).astype(f32)
                for a in axes:
                    p[a] = _ulps(f32(hi[a] if side[a] else lo[a]), k if side[a] else -k)
                # a direction that only touches the box at p: pointing along the touched faces
                d = rng.normal(size=3)
                d[axes] *= 1e-3
                d = unit(d)
                s = rng.uniform(0.5, 5.0)
                o = (p.astype(np.float64) - s * d.astype(np.float64)).astype(f32)
                rays.append(np.concatenate([o, [0], d, [0]]))
                rays.append(np.concatenate([o, [0], -d, [0]]))  # the box behind the origin
        _, _, out = check(np.array(rays, f32), recs, blocks)
        ncut += int(((out & CUT) != 0).sum()); nkept += int(((out & CUT) == 0).sum())
    assert ncut > 0 and nkept > 0


def test_grazing_spheres():
    """Rays tangent to the incenter sphere within a few ulp of the radius, with every normal: the cull must agree with the
    exact test wherever it speaks."""
    rng = np.random.default_rng(6)
    ncut = 0
    for it in range(100):
        c = rng.uniform(-3, 3, 3)
        r = rng.uniform(0.01, 1.0)
        recs = mkrecs([c] * 4, [r] * 4, rng.normal(size=(4, 3)))
        blocks = np.array([[1, 2, 3, 4 | 0x80000000]], np.uint32)
        rays = []
        for _ in range(40):
            d = unit(rng.normal(size=3)).astype(np.float64)
            perp = unit(np.cross(d, rng.normal(size=3))).astype(np.float64)
            dist = r * (1 + rng.choice([-1e-3, -1e-6, -1e-7, 0, 1e-7, 1e-6, 1e-5, 2e-5, 1e-4, 1e-3, 1e-1, 1.0]))
            o = c + perp * dist - d * rng.uniform(-2, 5)
            rays.append(np.concatenate([o, [0], d, [0]]))
        _, _, out = check(np.array(rays, f32), recs, blocks)
        ncut += int(((out & CUT) != 0).sum())
    assert ncut > 0


def test_origin_inside_box_is_never_culled():
    rng = np.random.default_rng(7)
    c = rng.uniform(-2, 2, (50, 3))
    recs = mkrecs(c, rng.uniform(0.05, 0.5, 50), rng.normal(size=(50, 3)))
    blocks = one_per_block(50)
    records, _, _ = block_cull(recs, blocks, mkrays([0, 0, 0], [1, 1, 1]))
    lo, hi = box_of(records)
    for b in range(50):
        o = rng.uniform(lo[b], hi[b], (20, 3))
        o[0], o[1] = lo[b], hi[b]  # on the corners
        _, rayok, out = check(mkrays(o, unit(rng.normal(size=(20, 3)))), recs, blocks[b:b + 1])
        assert rayok.all() and not (out & (CUT | MISS)).any()


def test_small_and_zero_den():
    """norm . dir of a few ulp and exactly 0: the sign certificate fails, nothing is culled although the box is missed."""
    rng = np.random.default_rng(8)
    for it in range(100):
        d = unit(rng.normal(size=3))
        nrm = unit(np.cross(d.astype(np.float64), rng.normal(size=3))).astype(np.float64)
        nrm = nrm + d * rng.choice([0.0, 1e-8, 1e-7, 1e-6, 1e-5])
        c = rng.uniform(-3, 3, 3)
        recs = mkrecs([c], 0.1, [nrm])
        o = c + unit(rng.normal(size=3)) * rng.uniform(1, 5)
        _, rayok, out = check(mkrays([o, o], [d, -d]), recs, one_per_block(1))
        assert rayok.all() and not (out & (CUT | SIGN)).any()
    # exactly 0: axis-aligned normal, direction in its plane
    recs = mkrecs([[5, 5, 5]], 0.1, [[0, 0, 1]])
    _, rayok, out = check(mkrays([[0, 0, 0]], [unit([1, 2, 0])]), recs, one_per_block(1))
    assert not rayok.any() and not (out & CUT).any()  # (a zero component: the ray does not qualify either)
    recs = mkrecs([[5, 5, 5]], 0.1, [[1, -1, 0]])
    _, rayok, out = check(mkrays([[0, 0, 9]], [unit([1, 1, 1e-3])]), recs, one_per_block(1))
    assert rayok.all() and (out & MISS).all() and not (out & (CUT | SIGN)).any()


def test_rays_that_do_not_qualify():
    """Nonzero lane 3, zero / denormal / huge / tiny direction components, NaN and far origins: never culled."""
    recs = mkrecs([[5, 5, 5]], 0.1, [[0, 0, 1]])
    blocks = one_per_block(1)
    good = mkrays([[0, 0, 0]], [unit([1, 2, -3])])
    _, rayok, out = check(good, recs, blocks)
    assert rayok.all() and (out & CUT).all()
    bad = []
    for col, val in ((3, 1e-3), (7, 1e-3), (3, np.nan), (7, -1.0), (0, np.nan), (5, np.nan), (0, 1e16), (1, -np.inf),
                     (4, 0.0), (5, -0.0), (6, 1e-42), (4, 1e-14), (4, np.inf), (4, 1e30)):
        r = good.copy()
        r[0, col] = f32(val)
        bad.append(r[0])
    for s in (1e-30, 1e-20, 1e-11, 1e11, 1e30):  # the whole direction scaled out of range
        r = good.copy()
        r[0, 4:7] *= f32(s)
        bad.append(r[0])
    _, rayok, out = check(np.array(bad, f32), recs, blocks)
    assert not rayok.any() and not (out & CUT).any()
    # scaled directions inside the range keep the cull and stay sound
    ok = np.concatenate([good * np.array([1, 1, 1, 1, s, s, s, 1], f32) for s in (1e-9, 1e-3, 1e3, 1e9)])
    _, rayok, out = check(ok, recs, blocks)
    assert rayok.all() and (out & CUT).all()


def test_coordinate_scales():
    """Scenes from 1e-30 to 1e30: sound everywhere, records outside [1e-15, 1e15] are flagged never-cull, and in the usual
    range the cull works."""
    rng = np.random.default_rng(9)
    for scale in (1e-30, 1e-20, 1e-12, 1e-6, 1e-3, 1.0, 1e3, 1e6, 1e12, 1e14, 1e16, 1e20, 1e30):
        c = (rng.normal(size=(200, 3)) * scale).astype(f32)
        recs = mkrecs(c, rng.uniform(0.001, 0.1, 200) * scale, rng.normal(size=(200, 3)))
        blocks = one_per_block(200)
        o = (rng.normal(size=(64, 3)) * scale).astype(f32)
        records, rayok, out = check(mkrays(o, unit(rng.normal(size=(64, 3)))), recs, blocks)
        never = ((records[:, 7] >> 16) & BC_NEVER) != 0
        if 1e-3 <= scale <= 1e6:
            assert rayok.all() and not never.any() and ((out & CUT) != 0).mean() > 0.5, scale
        if scale <= 1e-20 or scale >= 1e16:
            assert never.all() or not rayok.any(), scale
            assert not (out & CUT).any()


def test_nan_and_degenerate_records_are_never_cull():
    rng = np.random.default_rng(10)
    base = mkrecs(rng.uniform(4, 6, (4, 3)), [0.1] * 4, rng.normal(size=(4, 3)))
    rays = mkrays(rng.uniform(-1, 1, (32, 3)), unit(rng.normal(size=(32, 3))))
    blocks = np.array([[1, 2, 3, 4 | 0x80000000]], np.uint32)
    records, _, out = check(rays, base, blocks)
    assert not (records[0, 7] >> 16) & BC_NEVER and (out & CUT).any()
    for col, val in ((0, np.nan), (1, np.inf), (3, 0.0), (3, np.nan), (3, np.inf), (3, -1.0), (3, 1e-20), (3, 1e20),
                     (4, np.nan), (5, np.inf), (0, 1e20)):
        recs = base.copy()
        recs[2, col] = f32(val)
        records, _, out = check(rays, recs, blocks)
        assert (records[0, 7] >> 16) & BC_NEVER, (col, val)
        assert not (out & CUT).any()
    recs = base.copy()
    recs[3, 4:7] = 0.0  # a zero normal
    records, _, out = check(rays, recs, blocks)
    assert (records[0, 7] >> 16) & BC_NEVER and not (out & CUT).any()
    recs = base.copy()
    recs[1, 0:3] = 0.0  # an incenter at the origin: |c|_1 below the range
    records, _, out = check(rays, recs, blocks)
    assert (records[0, 7] >> 16) & BC_NEVER and not (out & CUT).any()


def test_blocks_with_padding_and_end_flags():
    """Partly filled blocks bound only their real references; the end flag follows the rule of oblocks."""
    rng = np.random.default_rng(12)
    c = rng.uniform(-3, 3, (8, 3))
    recs = mkrecs(c, rng.uniform(0.05, 0.3, 8), rng.normal(size=(8, 3)))
    blocks = np.array([[1, 2, 3, 4], [5, 6, 7, 8 | 0x80000000], [1, 2, 3, 0], [4, 5, 0, 0], [6, 0, 0, 0], [0, 0, 0, 0],
                       [1, 5, 2, 7]], np.uint32)
    rays = mkrays(rng.uniform(-4, 4, (256, 3)), unit(rng.normal(size=(256, 3))))
    records, rayok, out = check(rays, recs, blocks)
    assert rayok.all()
    assert [int((w >> 16) & BC_END) for w in records[:, 7]] == [0, 1, 1, 1, 1, 1, 0]
    assert not ((records[:, 7] >> 16) & BC_NEVER).any()
    lo, hi = box_of(records)
    # the box of [6, 0, 0, 0] is the sphere of record 6 alone, grown a little
    r6 = np.sqrt(recs[6, 3].astype(np.float64))
    assert (lo[4] < recs[6, 0:3] - r6).all() and (lo[4] > recs[6, 0:3] - 1.001 * r6 - 1e-3).all()
    assert (hi[4] > recs[6, 0:3] + r6).all() and (hi[4] < recs[6, 0:3] + 1.001 * r6 + 1e-3).all()
    assert (lo[5] > hi[5]).all()  # no real reference: the empty box
    # a padded block is culled at least where the full block with the same leading references is
    assert ((out[0] & CUT) <= (out[2] & CUT)).all()
    assert (out[4] & CUT).any()


def test_random_blocks_and_rays():
    rng = np.random.default_rng(13)
    for it in range(40):
        scale = 10.0 ** rng.uniform(-3, 3)
        m = 400
        c = rng.normal(size=(m, 3)) * scale
        recs = mkrecs(c, rng.uniform(0.001, 0.3, m) * scale, rng.normal(size=(m, 3)))
        # neighbours share a block, like the builder's lists
        order = np.argsort(c[:, 0]) + 1
        blocks = order.astype(np.uint32).reshape(-1, 4)
        o = np.concatenate([c[rng.integers(0, m, 96)], rng.normal(size=(32, 3)) * scale * 3])
        check(mkrays(o, unit(rng.normal(size=(128, 3)))), recs, blocks)
