"""Node cull of k_path_primary (trace_oct.hpp, the W_PRIMARY part of "Node cull"; DESIGN.md 4.1 "Node cull for primary rays").
CPU only: rtmi_debug_ray_cert_kappa and rtmi_debug_node_cull_kappa evaluate the certificate with the primary kernel's band
(CERT_KAPPA_PRIMARY, passed as kappa = 0) and the node predicate on the host with the kernel's own functions.  Checked here:
whole pixel packets hold the certificate, no reference below a culled node passes the f32 plane test for primary rays and
for their reflections off the mirror disks, rays whose den lies between the two bands are sound up to the ends of the
enforced ranges, and the cull removes a real share of a float64 model walk of primary rays."""
import ctypes as C

import numpy as np
import pytest

import test_block_cull_cpu as B
from test_block_cull_cpu import canonical, mkrays, mkrecs  # noqa: F401  (canonical: a fixture)
from test_node_cull_cpu import CUT, MISS, Tree, _hits_f64, hand_tree
from test_ray_cert_cpu import G, ray_cull

f32 = np.float32
KAPPA = f32(1e-6)           # CERT_KAPPA: the bounce passes
KAPPA_PRIMARY = f32(1e-9)   # CERT_KAPPA_PRIMARY


def _lib():
    from rust_raytrace_amd import _ffi
    return _ffi.lib()


def ray_cert(recs, rays, g, kappa):
    """(cert (n,) bool, ncand (n,) u32) of rtmi_debug_ray_cert_kappa; kappa = 0: the primary kernel's band"""
    L = _lib()
    vp = C.c_void_p
    L.rtmi_debug_ray_cert_kappa.restype = C.c_int
    L.rtmi_debug_ray_cert_kappa.argtypes = [vp, C.c_uint64, vp, C.c_uint64, C.c_uint32, C.c_float, vp, vp]
    recs, rays = np.ascontiguousarray(recs, f32), np.ascontiguousarray(rays, f32)
    cert, ncand = np.zeros(len(rays), np.uint8), np.zeros(len(rays), np.uint32)
    rc = L.rtmi_debug_ray_cert_kappa(recs.ctypes.data, len(recs), rays.ctypes.data, len(rays), g, float(kappa), cert.ctypes.data,
                                     ncand.ctypes.data)
    assert rc == 0, L.rtmi_last_error()
    return cert.astype(bool), ncand


def node_cull_kappa(geo, topo, refs, recs, rays, g, kappa=0.0):
    """test_node_cull_cpu.node_cull through the entry that takes the band"""
    L = _lib()
    vp = C.c_void_p
    L.rtmi_debug_node_cull_kappa.restype = C.c_int
    L.rtmi_debug_node_cull_kappa.argtypes = [vp, C.c_uint64, vp, C.c_uint64, C.c_uint64, vp, vp, C.c_uint64, C.c_uint32, vp, vp, vp, vp,
                                             C.c_float]
    boxes = np.ascontiguousarray(np.concatenate([np.ascontiguousarray(geo, f32).view(np.uint32), np.asarray(topo, np.uint32)], axis=1),
                                 np.uint32)
    refs = np.ascontiguousarray(refs, np.uint32)
    recs, rays = np.ascontiguousarray(recs, f32), np.ascontiguousarray(rays, f32)
    nrec = C.c_uint64(0)
    head = (boxes.ctypes.data, len(boxes), refs.ctypes.data, len(refs), len(recs), recs.ctypes.data, rays.ctypes.data, len(rays), g)
    rc = L.rtmi_debug_node_cull_kappa(*head, C.byref(nrec), None, None, None, float(kappa))
    assert rc == 0, L.rtmi_last_error()
    r = dict(records=np.zeros((nrec.value, 4), np.uint32), cert=np.zeros(len(rays), np.uint8),
             out=np.zeros((nrec.value, len(rays)), np.uint8))
    rc = L.rtmi_debug_node_cull_kappa(*head, C.byref(nrec), r["records"].ctypes.data, r["cert"].ctypes.data, r["out"].ctypes.data,
                                      float(kappa))
    assert rc == 0, L.rtmi_last_error()
    r["cert"] = r["cert"].astype(bool)
    return r


def canonical_primary(w, h, spp, seed=1):
    """rays (n, 8) of the canonical camera, path order: pixel-major, the samples of a pixel together"""
    orc = B._orc()
    o4, d4 = orc.primary_rays(w, h, orc.canonical_viewport(w, h), spp, seed=seed)
    return np.concatenate([o4, d4], axis=1).astype(f32)


# ---------------------------------------------------------------- (a) whole pixel packets hold the certificate
def test_pixel_packets_hold_the_certificate(canonical):
    """320 random pixels of the benchmark's 2048 x 2048 frame at 64 spp (8 pixels of each of 40 rows): a packet is the 64
    samples of a pixel, which share a wave.  With the primary band at least 0.95 of the packets are certified in all 64 lanes
    (measured: 0.995; with the bounce passes' band 0.56, which is what made a band of its own necessary).  The library's
    1e-6 certificate is what it was on these rays."""
    so, raw, recs, _, ob, _ = canonical
    orc = B._orc()
    w = h = 2048
    spp = 64
    rng = np.random.default_rng(5)
    sub = []
    for row in rng.choice(h, 40, replace=False):
        o4, d4 = orc.primary_rays(w, h, orc.canonical_viewport(w, h), spp, seed=1, row0=int(row), nrows=1)
        rays = np.concatenate([o4, d4], axis=1).astype(f32).reshape(w, spp, 8)
        # (the premise: the 64 rays of a group are the samples of one pixel)
        assert (np.ptp(rays[:, :, 4:7], axis=1) < 4.0 / w).all()
        sub.append(rays[rng.choice(w, 8, replace=False)])
    sub = np.concatenate(sub).reshape(-1, 8)
    cp, ncand = ray_cert(recs, sub, G, 0.0)
    cp9, _ = ray_cert(recs, sub, G, KAPPA_PRIMARY)
    c6, _ = ray_cert(recs, sub, G, KAPPA)
    assert np.array_equal(cp, cp9), "kappa = 0 is not CERT_KAPPA_PRIMARY"
    old = ray_cull(recs, ob, sub, G)["cert"].astype(bool)
    assert np.array_equal(old, c6), "the 1e-6 certificate of rtmi_debug_ray_cull changed"
    assert not (c6 & ~cp).any(), "a ray certified with the wide band but not with the narrow one"
    share_p, share_6 = cp.reshape(-1, spp).all(axis=1).mean(), c6.reshape(-1, spp).all(axis=1).mean()
    print(f"\npackets certified in all 64 lanes: {share_p:.3f} at 1e-9, {share_6:.3f} at 1e-6; rays refused {1 - cp.mean():.4f} / "
          f"{1 - c6.mean():.4f}; longest list {ncand.max()}")
    assert share_p >= 0.95
    assert share_6 < share_p, "the two bands certify the same packets: the condition above shows nothing"


# ---------------------------------------------------------------- (b) no reference below a culled node passes
def _mirror_reflections(so, raw, rays):
    """Reflections of the primary rays that hit a mirror disk first: the disks are the two planes that many triangles share
    a normal with.  Directions as color_ray makes them up to rounding (the check below holds for any ray)."""
    tri, t, _, _ = so.trace(rays[:, 0:4], rays[:, 4:8])
    nrm = raw[:, 3:6].astype(np.float64)
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-30)
    key = np.round(np.abs(nrm), 4)
    _, inv, cnt = np.unique(key, axis=0, return_inverse=True, return_counts=True)
    disk = cnt[inv.reshape(-1)] >= 32
    disk[0] = False
    sel = np.nonzero(disk[tri] & (tri != 0))[0]
    o = rays[sel, 0:3].astype(np.float64) + rays[sel, 4:7].astype(np.float64) * t[sel, None].astype(np.float64)
    d = rays[sel, 4:7].astype(np.float64)
    n = nrm[tri[sel]]
    r = d - 2.0 * (d * n).sum(axis=1, keepdims=True) * n
    return mkrays(o + 1e-3 * r, B.unit(r))


@pytest.fixture(scope="module")
def primary_nodes(canonical):
    so, raw, recs, (geo, topo, refs), ob, _ = canonical
    frame = canonical_primary(64, 64, 1)
    rng = np.random.default_rng(9)
    prim = frame[rng.choice(len(frame), 160, replace=False)]
    refl = _mirror_reflections(so, raw, frame)
    assert len(refl) >= 32, "no mirror disk in view of the canonical camera"
    refl = refl[rng.choice(len(refl), min(len(refl), 96), replace=False)]
    rays = np.concatenate([prim, refl])
    tree = Tree(geo, topo, refs, recs)
    return tree, rays, len(prim), node_cull_kappa(geo, topo, refs, recs, rays, G)


def test_culled_subtrees_hold_no_passing_reference(canonical, primary_nodes):
    """160 canonical primary rays and up to 96 reflections off the mirror disks against all node records: every reference that
    passes the f32 plane test for a ray lies in leaves none of whose ancestors is culled for that ray."""
    so, raw, recs, _, ob, _ = canonical
    tree, rays, nprim, r = primary_nodes
    assert len(r["records"]) == len(tree.inner) == 35140
    cut = (r["out"] & CUT) != 0
    assert (cut == (((r["out"] & MISS) != 0) & r["cert"][None, :])).all()
    assert cut[:, :nprim].any() and cut[:, nprim:].any()
    assert r["cert"].mean() > 0.95
    pp = B.plane_pass(rays, recs)
    pp[0] = False
    leaves = np.nonzero(tree.topo[:, 2] == 1)[0]
    leaf_of_ref = np.repeat(leaves, tree.topo[leaves, 1].astype(np.int64))
    ref_ids = np.concatenate([tree.refs[tree.topo[c, 0]: tree.topo[c, 0] + tree.topo[c, 1]] for c in leaves])
    checked = 0
    for i in range(len(rays)):
        cur = np.unique(leaf_of_ref[pp[ref_ids, i]])
        while len(cur):
            cur = np.unique(tree.parent[cur])
            cur = cur[cur >= 0]
            bad = cut[tree.rec_of[cur], i]
            assert not bad.any(), f"ray {i}: a triangle passes the plane test below the culled boxes {cur[bad][:8].tolist()}"
            checked += len(cur)
    assert checked > 0


# ---------------------------------------------------------------- (c) den between the two bands
def _den32(n, d):
    """`plane`'s den in f32, in the kernel's operation order"""
    n, d = np.asarray(n, f32), np.asarray(d, f32)
    return (((f32(0) + n[..., 0] * d[..., 0]) + n[..., 1] * d[..., 1]) + n[..., 2] * d[..., 2]) + f32(0) * f32(0)


def _thr32(n, d, kappa):
    """the certificate's threshold n.w * (kappa * |d|_1) in f32, as ray_sign_certified computes it"""
    n, d = np.abs(np.asarray(n, f32)), np.abs(np.asarray(d, f32))
    return ((n[..., 0] + n[..., 1]) + n[..., 2]) * (f32(kappa) * ((d[..., 0] + d[..., 1]) + d[..., 2]))


def _band_directions(rng, n, count, dscale):
    """`count` directions of length ~dscale, every component nonzero, whose f32 den against normal n is at most the wide
    threshold: a quarter at or below the narrow threshold (refused; den == 0 among them), a quarter the nearest above it that
    f32 offers -- 1e-9 |n|_1 |d|_1 is far below the rounding of the three products, so den moves in steps of an ulp of the
    partial sums and "a few ulp above the threshold" are its smallest nonzero values -- and the rest anywhere in the band."""
    n64 = n.astype(np.float64)
    u = np.cross(n64, rng.normal(size=(60000, 3)))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    eps = rng.choice([-1.0, 1.0], len(u)) * 10.0 ** rng.uniform(-9.5, -6.5, len(u))
    d = ((u + eps[:, None] * n64) * dscale).astype(f32)
    d = d[(d != 0).all(axis=1) & np.isfinite(d).all(axis=1)]
    den, thr9, thr6 = np.abs(_den32(n, d)), _thr32(n, d, KAPPA_PRIMARY), _thr32(n, d, KAPPA)
    below = np.nonzero(den <= thr9)[0]
    band = np.nonzero((den > thr9) & (den <= thr6))[0]
    q = count // 4
    assert len(below) >= q and (den[below] == 0).any() and len(band) >= count
    near = band[np.argsort(den[band] / thr9[band], kind="stable")[:q]]
    rest = rng.choice(np.setdiff1d(band, near), count - 2 * q, replace=False)
    zero = below[den[below] == 0][:1]
    return d[np.concatenate([zero, rng.choice(below, q - 1, replace=False), near, rest])]


@pytest.mark.parametrize("cscale,oscale,dscale", [(1.0, 1.0, 1.0), (1e15 / 8, 1.0, 1.0), (1.0, 1e15 / 8, 1.0), (1e15 / 8, 1e15 / 8, 1e-10 * 2),
                                                   (1.0, 1.0, 1e10 / 2), (1e15 / 8, 1e15 / 8, 1e10 / 2), (1e-3, 1e15 / 8, 1e-10 * 2)])
def test_den_between_the_bands(cscale, oscale, dscale):
    """A hand-made tree whose references all share ONE normal, rays whose den against it lies between 1e-9 and 1e-6 of
    |n|_1 |d|_1 (some a few ulp above the narrow threshold, some just below), with incenters, origins and directions scaled to
    the ends of the ranges block_cull_ray and the records enforce.  The certificate is exactly `|den| > n.w (kappa |d|_1)` in
    f32; a culled node's references all fail the f32 plane test with a finite t, and nothing in that evaluation is NaN."""
    rng = np.random.default_rng(int(np.log10(cscale * 10) * 7 + np.log10(oscale * 10) * 3 + np.log10(dscale * 1e11)))
    nrm = B.unit(rng.normal(size=3))
    nrm[nrm == 0] = f32(0.25)
    cen = (rng.uniform(0.55, 0.95, (12, 3)) * cscale).astype(f32)
    recs = mkrecs(cen, rng.uniform(0.02, 0.08, 12) * cscale, np.tile(nrm, (12, 1)))
    recs[1:, 4:7] = nrm  # one normal, bit for bit
    geo, topo, refs = hand_tree(([1, 2, 3, 4, 5], [6, 7, 8, 9]), [10, 11, 12])
    dirs = _band_directions(rng, nrm, 96, dscale)
    org = (rng.normal(size=(len(dirs), 3)) * oscale).astype(f32)
    rays = mkrays(org, dirs)
    den, thr9, thr6 = np.abs(_den32(nrm, dirs)), _thr32(nrm, dirs, KAPPA_PRIMARY), _thr32(nrm, dirs, KAPPA)
    assert (den <= thr6).all(), "a constructed ray is outside the wide band"
    assert (den > thr9).sum() >= 48 and (den <= thr9).sum() >= 16 and (den == 0).any()
    print(f"\nden / threshold(1e-9) of the rays nearest above it: {np.sort((den / thr9)[den > thr9])[:4]}")
    cp, ncand = ray_cert(recs, rays, 64, 0.0)
    c6, _ = ray_cert(recs, rays, 64, KAPPA)
    assert (ncand == 1).all(), "the normal is not listed for a direction nearly perpendicular to it"
    assert np.array_equal(cp, den > thr9), "the certificate is not |den| > n.w (kappa |d|_1)"
    assert not c6.any()
    r = node_cull_kappa(geo, topo, refs, recs, rays, 64)
    assert np.array_equal(r["cert"], cp)
    cut = (r["out"] & CUT) != 0
    assert (cut == (((r["out"] & MISS) != 0) & cp[None, :])).all()
    # the plane test of every reference for every certified ray, in f32 with every intermediate value kept
    with np.errstate(all="ignore"):
        o, d = rays[None, :, 0:4], rays[None, :, 4:8]
        c, r2, n = recs[1:, None, 0:3], recs[1:, None, 3], recs[1:, None, 4:7]
        a = c - o[..., :3]
        num = (((f32(0) + n[..., 0] * a[..., 0]) + n[..., 1] * a[..., 1]) + n[..., 2] * a[..., 2]) + f32(0) * (f32(0) - o[..., 3])
        dn = (((f32(0) + n[..., 0] * d[..., 0]) + n[..., 1] * d[..., 1]) + n[..., 2] * d[..., 2]) + f32(0) * d[..., 3]
        t = num / dn
        p = d * t[..., None] + o
        ip = p[..., :3] - c
        pw = p[..., 3]
        l2 = ((ip[..., 0] * ip[..., 0] + ip[..., 1] * ip[..., 1]) + ip[..., 2] * ip[..., 2]) + pw * pw
        passes = ~(t < 0) & ~(l2 > r2)
    for v in (a, num, dn, t, p, ip, pw, l2):
        assert not np.isnan(v[..., cp] if v.ndim == 2 else v[:, cp]).any(), "NaN in the plane test of a certified ray"
    assert np.isfinite(t[:, cp]).all() and (pw[:, cp] == 0).all()
    tree = Tree(geo, topo, refs, recs)
    for b in tree.inner:
        ids = np.array(sorted(tree.subtree_refs(b))) - 1
        bad = cut[tree.rec_of[b]] & passes[ids].any(axis=0)
        assert not bad.any(), f"box {b}: culled for rays {np.nonzero(bad)[0][:8].tolist()} but a reference below passes"
    if cscale == oscale == dscale == 1.0:
        assert cut.any(), "nothing culled at unit scale: the case shows nothing"


def test_zero_and_subnormal_den_are_refused():
    """den exactly 0 (the three products cancel exactly) at three direction scales, and a subnormal den at the small ends of
    the ranges (|n| = 1.4e-15, max |d_k| = 1e-10, the smallest component 2^-39 of it): block_cull_ray accepts the rays, the
    normal is listed, and both bands refuse them."""
    recs = np.zeros((2, 8), f32)
    recs[1] = [0.7, 0.7, 0.7, 0.0025, 0.5, 0.25, 0.25, 0]
    dirs = np.array([[s, -s, -s] for s in (1.0, 2e-10, 5e9)], f32)
    assert (_den32(recs[1, 4:7], dirs) == 0).all()
    sub = np.zeros((2, 8), f32)
    sub[1] = [0.7, 0.7, 0.7, 0.0025, 1e-15, 1e-15, 1e-17, 0]
    tiny = np.array([[1e-10, -1e-10, 1e-10 * 2.0 ** -39]], f32)
    den = abs(_den32(sub[1, 4:7], tiny)[0])
    assert 0 < den < np.finfo(f32).tiny, den
    for kappa in (0.0, KAPPA):
        cert, ncand = ray_cert(recs, mkrays(np.zeros((3, 3)), dirs), 64, kappa)
        assert (ncand == 1).all() and not cert.any()
        cert, ncand = ray_cert(sub, mkrays([0, 0, 0], tiny), 64, kappa)
        assert (ncand == 1).all() and not cert.any()


# ---------------------------------------------------------------- (d) the model walk
def test_model_walk_of_primary_rays(canonical, primary_nodes):
    """test_node_cull_cpu's float64 model of the reference walk over the 160 primary rays, with the packed node records and
    the primary band: the cull removes at least 15 % of the SELECT steps and 25 % of the leaf visits (measured: 28-32 % and
    48-54 %), and no geometric hit lies below a culled box."""
    so, raw, recs, (geo, topo, refs), ob, _ = canonical
    tree, rays, nprim, r = primary_nodes
    rays = rays[:nprim]
    assert nprim >= 128
    cut = (r["out"][:, :nprim] & CUT) != 0
    hits = _hits_f64(raw, rays)
    ctr, half = geo[:, 0:3].astype(np.float64), geo[:, 3].astype(np.float64)
    blo, bhi = ctr - half[:, None], ctr + half[:, None]
    topo = tree.topo
    tot = dict(sel=0, leaf=0, sel_in=0, leaf_in=0, culled=0)

    def walk(b, i, o, inv, inside):
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
                steps = j + 1
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

    for i in range(nprim):
        walk(0, i, rays[i, 0:3].astype(np.float64), 1.0 / rays[i, 4:7].astype(np.float64), False)
    sel_cull, leaf_cull = tot["sel"] - tot["sel_in"] + tot["culled"], tot["leaf"] - tot["leaf_in"]
    print(f"\nmodel walk, {nprim} primary rays: SELECT steps per ray {tot['sel'] / nprim:.1f} -> {sel_cull / nprim:.1f} "
          f"({1 - sel_cull / tot['sel']:.3f} removed), leaf visits per ray {tot['leaf'] / nprim:.1f} -> {leaf_cull / nprim:.1f} "
          f"({1 - leaf_cull / max(tot['leaf'], 1):.3f} removed), culled nodes per ray {tot['culled'] / nprim:.2f}")
    assert sel_cull <= 0.85 * tot["sel"], f"the node cull removes only {1 - sel_cull / tot['sel']:.3f} of the SELECT steps"
    assert leaf_cull <= 0.75 * tot["leaf"], f"the node cull removes only {1 - leaf_cull / tot['leaf']:.3f} of the leaf visits"
