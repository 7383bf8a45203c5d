"""The packed box-only cull records of k_trace_oct (trace_oct.hpp, packed_block_miss; DESIGN.md 4.1 "Sign certificate per
ray"): for a certified ray, a block whose packed box the half-line misses holds no reference that passes the exact plane
test.  CPU only (rtmi_debug_ray_cull); the exact test and the adversarial shapes are those of test_block_cull_cpu.py."""
import numpy as np
import pytest

import test_block_cull_cpu as B
from test_block_cull_cpu import canonical, mkrays, mkrecs, one_per_block, unit  # noqa: F401  (canonical: a fixture)
from test_ray_cert_cpu import G, G_SMALL, ray_cull

f32 = np.float32
MISS, CUT = 1, 4


def packed_box(packed):
    """(lo, hi) (nb, 3) f32 of packed records"""
    w = packed.astype(np.uint32)
    bits = np.stack([w[:, 0] << 16, w[:, 0] & 0xFFFF0000, w[:, 1] << 16, w[:, 1] & 0xFFFF0000, w[:, 2] << 16, w[:, 2] & 0xFFFF0000],
                    axis=1).astype(np.uint32)
    v = bits.view(f32)
    return v[:, 0:3], v[:, 3:6]


def check(rays, recs, blocks, g=G_SMALL):
    """0 violations, the packed box contains the f32 box, flags carried over; -> (result of ray_cull, 32-B records)"""
    r = ray_cull(recs, blocks, rays, g)
    records, rayok, out32 = B.block_cull(recs, blocks, rays)
    cut = (r["out"] & CUT) != 0
    assert not r["cert"][~rayok].any(), "a ray certified that block_cull_ray() refuses"
    assert not cut[:, ~r["cert"]].any(), "a block culled for a ray that is not certified"
    assert (cut == (((r["out"] & MISS) != 0) & r["cert"][None, :])).all()
    flags = records[:, 7] >> 16
    assert (r["packed"][:, 3] == flags).all()
    never = (flags & B.BC_NEVER) != 0
    assert not (r["out"][never] & (MISS | CUT)).any(), "a never-cull block missed or culled"
    lo32, hi32 = B.box_of(records)
    plo, phi = packed_box(r["packed"])
    ok = ~never
    assert (plo[ok] <= lo32[ok]).all() and (phi[ok] >= hi32[ok]).all(), "a packed box does not contain its f32 box"
    assert np.isneginf(plo[never]).all() and np.isposinf(phi[never]).all()
    # the f32 box's own miss implies the packed box's only the other way round: packed miss => f32 miss
    assert not (((r["out"] & MISS) != 0) & ((out32 & B.MISS) == 0) & rayok[None, :]).any(), "packed box missed, f32 box hit"
    bad = cut & B.block_pass(rays, recs, blocks)
    assert not bad.any(), f"culled but a reference passed: (block, ray) {np.argwhere(bad)[:10].tolist()}"
    return r, records


def test_canonical_blocks_sound_and_share(canonical):
    """Every block of the canonical tree against the 256 bounce-like rays: sound, and of the visited (block, ray) pairs (as
    test_block_cull_cpu counts them) at least 70 % are culled."""
    so, raw, recs, (geo, topo, refs), ob, rays = canonical
    r, _ = check(rays, recs, ob, G)
    cut = (r["out"] & CUT) != 0
    ends = (ob[:, 3] == 0) | ((ob[:, 3] >> 31) != 0)
    starts = np.concatenate([[0], np.nonzero(ends)[0][:-1] + 1])
    nblk = np.nonzero(ends)[0] + 1 - starts
    first_of = {}
    for s, k in zip(starts, nblk):
        ids = (ob[s:s + k] & np.uint32(0x7FFFFFFF)).ravel()
        first_of[ids[ids != 0].tobytes()] = (int(s), int(k))
    leaves = np.nonzero(topo[:, 2] == 1)[0]
    lf = np.array([first_of[np.ascontiguousarray(refs[topo[c, 0]: topo[c, 0] + topo[c, 1]], np.uint32).tobytes()] for c in leaves])
    tri_hit, thit, _, _ = so.trace(rays[:, 0:4], rays[:, 4:8])
    tlim = np.where(tri_hit != 0, thit, np.inf).astype(np.float64)
    o, inv = rays[:, 0:3].astype(np.float64), 1.0 / rays[:, 4:7].astype(np.float64)
    ctr, half = geo[leaves, 0:3].astype(np.float64), geo[leaves, 3].astype(np.float64)
    blo, bhi = np.ascontiguousarray((ctr - half[:, None]).T), np.ascontiguousarray((ctr + half[:, None]).T)
    o, inv = o[:, :, None], inv[:, :, None]
    csum = np.concatenate([np.zeros((1, cut.shape[1]), np.int32), np.cumsum(cut, axis=0, dtype=np.int32)])
    visited = culled = 0
    for i in range(len(rays)):
        t1, t2 = (blo - o[i]) * inv[i], (bhi - o[i]) * inv[i]
        tmin, tmax = np.minimum(t1, t2).max(axis=0), np.maximum(t1, t2).min(axis=0)
        v = (tmin < tmax) & (tmin < tlim[i])
        visited += int(lf[v, 1].sum())
        culled += int((csum[lf[v, 0] + lf[v, 1], i] - csum[lf[v, 0], i]).sum())
    print(f"\ncanonical tree, packed records: certified {r['cert'].mean():.4f}; visited pairs {visited}, culled {culled / visited:.3f}")
    assert culled >= 0.70 * visited, f"only {culled} of {visited} visited (block, ray) pairs culled"


def test_grazing_box_face_edge_corner():
    """Rays through points a few ulp inside and outside a face, an edge and a corner of the PACKED box."""
    rng = np.random.default_rng(31)
    ncut = nkept = 0
    for it in range(60):
        c = rng.uniform(-3, 3, 3)
        recs = mkrecs([c], rng.uniform(0.05, 0.5), rng.normal(size=3))
        blocks = one_per_block(1)
        lo, hi = packed_box(ray_cull(recs, blocks, mkrays([0, 0, 0], [1, 1, 1]))["packed"])
        lo, hi = lo[0].astype(np.float64), hi[0].astype(np.float64)
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
        r, _ = check(np.array(rays, f32), recs, blocks)
        ncut += int(((r["out"] & CUT) != 0).sum()); nkept += int(((r["out"] & CUT) == 0).sum())
    assert ncut > 0 and nkept > 0


def test_grazing_spheres():
    """Rays tangent to the incenter sphere within a few ulp of the radius, with every normal."""
    rng = np.random.default_rng(32)
    ncut = 0
    for it in range(100):
        c = rng.uniform(-3, 3, 3)
        rad = rng.uniform(0.01, 1.0)
        recs = mkrecs([c] * 4, [rad] * 4, rng.normal(size=(4, 3)))
        blocks = np.array([[1, 2, 3, 4 | 0x80000000]], np.uint32)
        rays = []
        for _ in range(40):
            d = unit(rng.normal(size=3)).astype(np.float64)
            perp = unit(np.cross(d, rng.normal(size=3))).astype(np.float64)
            dist = rad * (1 + rng.choice([-1e-3, -1e-6, -1e-7, 0, 1e-7, 1e-6, 1e-5, 2e-5, 1e-4, 1e-3, 1e-2, 1e-1, 1.0]))
            o = c + perp * dist - d * rng.uniform(-2, 5)
            rays.append(np.concatenate([o, [0], d, [0]]))
        r, _ = check(np.array(rays, f32), recs, blocks)
        ncut += int(((r["out"] & CUT) != 0).sum())
    assert ncut > 0


def test_origin_inside_box_is_never_culled():
    rng = np.random.default_rng(33)
    c = rng.uniform(-2, 2, (50, 3))
    recs = mkrecs(c, rng.uniform(0.05, 0.5, 50), rng.normal(size=(50, 3)))
    blocks = one_per_block(50)
    lo, hi = packed_box(ray_cull(recs, blocks, mkrays([0, 0, 0], [1, 1, 1]))["packed"])
    for b in range(50):
        o = rng.uniform(lo[b], hi[b], (20, 3))
        o[0], o[1] = lo[b], hi[b]
        r, _ = check(mkrays(o, unit(rng.normal(size=(20, 3)))), recs, blocks[b:b + 1])
        assert not (r["out"] & (CUT | MISS)).any()


def test_small_and_zero_den_refused_or_sound():
    """norm . dir of a few ulp and exactly 0 with the box missed: such a ray is refused, so nothing is culled for it."""
    rng = np.random.default_rng(34)
    for it in range(100):
        d = unit(rng.normal(size=3))
        nrm = unit(np.cross(d.astype(np.float64), rng.normal(size=3))).astype(np.float64)
        nrm = nrm + d * rng.choice([0.0, 1e-8, 1e-7, 3e-7])
        c = rng.uniform(-3, 3, 3)
        recs = mkrecs([c], 0.1, [nrm])
        o = c + unit(rng.normal(size=3)) * rng.uniform(1, 5)
        r, _ = check(mkrays([o, o], [d, -d]), recs, one_per_block(1))
        assert not r["cert"].any() and not (r["out"] & CUT).any()
    recs = mkrecs([[5, 5, 5]], 0.1, [[1, -1, 0]])
    r, _ = check(mkrays([[0, 0, 9]], [unit([1, 1, 1e-3])]), recs, one_per_block(1))
    assert (r["out"] & MISS).all() and not r["cert"].any() and not (r["out"] & CUT).any()


def test_coordinate_scales():
    """Scenes from 1e-30 to 1e30: sound everywhere, never-cull records have an infinite box, the usual range culls."""
    rng = np.random.default_rng(35)
    for scale in (1e-30, 1e-20, 1e-12, 1e-6, 1e-3, 1.0, 1e3, 1e6, 1e12, 1e14, 1e16, 1e20, 1e30):
        c = (rng.normal(size=(200, 3)) * scale).astype(f32)
        recs = mkrecs(c, rng.uniform(0.001, 0.1, 200) * scale, rng.normal(size=(200, 3)))
        o = (rng.normal(size=(64, 3)) * scale).astype(f32)
        r, records = check(mkrays(o, unit(rng.normal(size=(64, 3)))), recs, one_per_block(200))
        if 1e-3 <= scale <= 1e6:
            assert r["cert"].mean() > 0.9 and ((r["out"] & CUT) != 0).mean() > 0.5, scale
        if scale <= 1e-20 or scale >= 1e16:
            assert not (r["out"] & CUT).any()


def test_padding_end_flags_and_degenerate_records():
    rng = np.random.default_rng(36)
    c = rng.uniform(-3, 3, (8, 3))
    recs = mkrecs(c, rng.uniform(0.05, 0.3, 8), rng.normal(size=(8, 3)))
    blocks = np.array([[1, 2, 3, 4], [5, 6, 7, 8 | 0x80000000], [1, 2, 3, 0], [4, 5, 0, 0], [6, 0, 0, 0], [0, 0, 0, 0],
                       [1, 5, 2, 7]], np.uint32)
    rays = mkrays(rng.uniform(-4, 4, (256, 3)), unit(rng.normal(size=(256, 3))))
    r, _ = check(rays, recs, blocks)
    assert [int(w & B.BC_END) for w in r["packed"][:, 3]] == [0, 1, 1, 1, 1, 1, 0]
    lo, hi = packed_box(r["packed"])
    assert (lo[5] > hi[5]).all() and np.isfinite(lo[5]).all()  # no real reference: the empty box
    cert = r["cert"]
    assert cert.mean() > 0.9
    assert ((r["out"][0] & CUT) <= (r["out"][2] & CUT)).all() and (r["out"][4] & CUT).any()
    for col, val in ((0, np.nan), (1, np.inf), (3, 0.0), (3, np.nan), (3, 1e20), (4, np.nan), (5, np.inf), (0, 1e20)):
        q = recs.copy()
        q[2, col] = f32(val)
        r, records = check(rays, q, blocks)
        assert (records[0, 7] >> 16) & B.BC_NEVER and not (r["out"][0] & CUT).any(), (col, val)


def test_random_blocks_and_rays():
    rng = np.random.default_rng(37)
    for it in range(40):
        scale = 10.0 ** rng.uniform(-3, 3)
        m = 400
        c = rng.normal(size=(m, 3)) * scale
        recs = mkrecs(c, rng.uniform(0.001, 0.3, m) * scale, rng.normal(size=(m, 3)))
        order = np.argsort(c[:, 0]) + 1
        blocks = order.astype(np.uint32).reshape(-1, 4)
        o = np.concatenate([c[rng.integers(0, m, 96)], rng.normal(size=(32, 3)) * scale * 3])
        check(mkrays(o, unit(rng.normal(size=(128, 3)))), recs, blocks)
