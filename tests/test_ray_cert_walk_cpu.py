"""The list walk of the per-ray sign certificate (trace_oct.hpp, ray_sign_certified / cert_walk; DESIGN.md 4.1 "Sign
certificate per ray", the list walk).  CPU only.  The walk reads CERT_BATCH entries of a list per iteration; its result is an
AND of independent comparisons, so it must be the bit the entry-at-a-time loop returns.  rtmi_debug_ray_cert_kappa runs the
batched walk on the host, rtmi_debug_ray_cert_ref the loop as it was (ray_sign_certified_ref), and a NumPy restatement reads
the table that rtmi_debug_ray_cull returns: the three must agree on canonical rays (short, empty and over-long lists, both
bands), on hand-made lists of 1 .. 9 normals with a zero den at every list position, on a table with 32-bit indices, and on
the last list of a table, where a batch must not run past the index area."""
import ctypes as C

import numpy as np
import pytest

import test_block_cull_cpu as B
from test_block_cull_cpu import canonical, mkrays, unit  # noqa: F401  (canonical: a fixture)
from test_primary_node_cull_cpu import ray_cert
from test_ray_cert_cpu import CAP, den_f32, table_parts

f32 = np.float32
KAPPAS = (1e-6, 1e-9)  # CERT_KAPPA (bounce passes), CERT_KAPPA_PRIMARY (primary kernels)
NO_CELL = 0xFFFFFFFF


def ray_cert_ref(recs, rays, g, kappa):
    """(cert (n,) bool, ncand (n,) u32) of rtmi_debug_ray_cert_ref: the list walked an entry at a time"""
    from rust_raytrace_amd import _ffi
    L = _ffi.lib()
    vp = C.c_void_p
    L.rtmi_debug_ray_cert_ref.restype = C.c_int
    L.rtmi_debug_ray_cert_ref.argtypes = [vp, C.c_uint64, vp, C.c_uint64, C.c_uint32, C.c_float, vp, vp]
    recs, rays = np.ascontiguousarray(recs, f32), np.ascontiguousarray(rays, f32)
    cert, ncand = np.zeros(len(rays), np.uint8), np.zeros(len(rays), np.uint32)
    rc = L.rtmi_debug_ray_cert_ref(recs.ctypes.data, len(recs), rays.ctypes.data, len(rays), g, float(kappa), cert.ctypes.data,
                                   ncand.ctypes.data)
    assert rc == 0, L.rtmi_last_error()
    return cert.astype(bool), ncand


def table_and_cells(recs, rays, g, cap_words):
    """(table words, cell (n,) u32, cert (n,) bool at 1e-6) of rtmi_debug_ray_cull, with room for cap_words table words
    (0: the table is not wanted)"""
    from rust_raytrace_amd import _ffi
    L = _ffi.lib()
    vp = C.c_void_p
    L.rtmi_debug_ray_cull.restype = C.c_int
    L.rtmi_debug_ray_cull.argtypes = [vp, C.c_uint64, vp, C.c_uint64, vp, C.c_uint64, C.c_uint32, vp, vp, vp, vp, vp, vp, C.c_uint64, vp]
    recs, rays = np.ascontiguousarray(recs, f32), np.ascontiguousarray(rays, f32)
    cert, cell = np.zeros(len(rays), np.uint8), np.zeros(len(rays), np.uint32)
    tab, words = np.zeros(max(cap_words, 1), np.uint32), C.c_uint64(0)
    rc = L.rtmi_debug_ray_cull(recs.ctypes.data, len(recs), None, 0, rays.ctypes.data, len(rays), g, None, cert.ctypes.data, None,
                               cell.ctypes.data, None, tab.ctypes.data if cap_words else None, cap_words, C.byref(words))
    assert rc == 0 and (cap_words == 0 or words.value <= cap_words), (rc, words.value)
    return tab[:words.value if cap_words else 0], cell, cert.astype(bool)


def cert_numpy(table, cell, rays, kappa):
    """The certificate restated from the table: for a ray block_cull_ray accepts (cell != NO_CELL), the list of its cell is at
    most CAP long and every listed normal has |den| > kappa |n|_1 |d|_1, all in f32 in the kernel's operation order
    -> (cert (n,) bool, ncand (n,))"""
    g, off, idx, nrm = table_parts(table)
    d = rays[:, 4:8]
    kd1 = f32(kappa) * ((np.abs(d[:, 0]) + np.abs(d[:, 1])) + np.abs(d[:, 2]))
    cert, ncand = np.zeros(len(rays), bool), np.zeros(len(rays), np.uint32)
    for i in np.nonzero(cell != NO_CELL)[0]:
        b, e = int(off[cell[i]]), int(off[cell[i] + 1])
        ncand[i] = e - b
        if e - b > CAP:
            continue
        n = nrm[idx[b:e]]
        den = den_f32(d[i:i + 1], n[:, 0:3])[:, 0]
        cert[i] = bool((np.abs(den) > n[:, 3] * kd1[i]).all())
    return cert, ncand


def assert_walks_agree(recs, rays, g, kappa, what):
    """new walk == referee, cert and ncand -> (cert, ncand)"""
    c, nc = ray_cert(recs, rays, g, kappa)
    cr, ncr = ray_cert_ref(recs, rays, g, kappa)
    assert np.array_equal(nc, ncr), f"{what}: list lengths differ"
    bad = np.nonzero(c != cr)[0]
    assert len(bad) == 0, f"{what}: the batched walk and the entry-at-a-time loop disagree for rays {bad[:8].tolist()} (lists {nc[bad[:8]].tolist()})"
    return c, nc


# ---------------------------------------------------------------- canonical records
@pytest.fixture(scope="module")
def canon_rays(canonical):
    """name -> 4096 rays: bounce-like (origins on scene triangles, directions over the hemisphere of the normal, the recipe
    of test_block_cull_cpu.canonical) and primary-like (the canonical camera, 64 x 64 at 1 spp)"""
    _, raw, _, _, _, _ = canonical
    rng = np.random.default_rng(31)
    n = 4096
    tri = rng.integers(1, len(raw), n)
    d = unit(rng.normal(size=(n, 3)))
    flip = (d.astype(np.float64) * raw[tri, 3:6]).sum(axis=1) < 0
    d[flip] = -d[flip]
    orc = B._orc()
    o4, d4 = orc.primary_rays(64, 64, orc.canonical_viewport(64, 64), 1, seed=1)
    return {"bounce": mkrays(raw[tri, 0:3], d), "primary": np.concatenate([o4, d4], axis=1).astype(f32)}


@pytest.fixture(scope="module")
def canon_tables(canonical, canon_rays):
    """g -> (table, name -> cell, name -> the 1e-6 certificate of rtmi_debug_ray_cull), built once"""
    recs = canonical[2]
    out = {}
    for g in (1024, 128):
        cells, certs = {}, {}
        for name, rays in canon_rays.items():
            t, cells[name], certs[name] = table_and_cells(recs, rays, g, 3 * g * g * 12 + (1 << 20))
        out[g] = (t, cells, certs)
    return out


@pytest.mark.parametrize("g", [1024, 128])
@pytest.mark.parametrize("kind", ["bounce", "primary"])
def test_canonical_walks_agree(canonical, canon_rays, canon_tables, g, kind):
    """The batched walk, the entry-at-a-time loop and the NumPy restatement give the same certificate and list length for
    4096 rays, at both bands.  G = 1024: short and empty lists; G = 128: lists on both sides of CERT_CAP."""
    recs, rays = canonical[2], canon_rays[kind]
    table, cells, certs = canon_tables[g]
    for kappa in KAPPAS:
        c, nc = assert_walks_agree(recs, rays, g, kappa, f"{kind} G {g} kappa {kappa}")
        cn, ncn = cert_numpy(table, cells[kind], rays, kappa)
        assert np.array_equal(nc, ncn) and np.array_equal(c, cn), f"{kind} G {g} kappa {kappa}: the NumPy restatement disagrees"
        print(f"\n{kind} G {g} kappa {kappa}: certified {c.mean():.4f}, list length mean {nc.mean():.1f} min {nc.min()} max {nc.max()}, "
              f"longer than the cap {(nc > CAP).sum()}")
        if kappa == KAPPAS[0]:
            assert np.array_equal(c, certs[kind]), "rtmi_debug_ray_cull's certificate is not the 1e-6 one"
    assert c.any() and not c.all(), "every ray certified, or none: the comparison shows nothing"
    if g == 128:
        assert (nc > CAP).any() and ((nc > 0) & (nc <= CAP)).any(), "no lists on both sides of the cap"
        assert not c[nc > CAP].any()
    else:
        # (lists that are no multiple of the batch, lists shorter than one batch)
        assert (nc % 4 != 0).any() and ((nc > 0) & (nc < 4)).any() and (nc > 4).any()


def test_pinned_1e6_certificate_unchanged(canonical, canon_rays, canon_tables):
    """rtmi_debug_ray_cull (the entry the existing tests pin) and the referee loop agree at 1e-6: the pinned result of
    tests/test_primary_node_cull_cpu.py holds for the new walk."""
    recs = canonical[2]
    for kind, rays in canon_rays.items():
        cr, _ = ray_cert_ref(recs, rays, 1024, 1e-6)
        assert np.array_equal(cr, canon_tables[1024][2][kind])


# ---------------------------------------------------------------- hand-made lists
G_HAND = 8


def hand_scene(n):
    """n distinct (unnormalised) normals and n + 1 directions of ONE cell of a G = 8 table (face x, a and b in (0, 1/4)): the
    great circle of normal j passes through direction j, where its f32 den is exactly 0 -- every operand is a small multiple
    of 1/128, so the products and sums are exact.  Direction n is refused by none.  -> (recs, rays)"""
    recs = np.zeros((n + 1, 8), f32)
    dirs = []
    for j in range(n):
        a, b = (3 + 2 * j) / 128.0, (5 + 3 * j) / 128.0
        p, q = 1 + j % 3, 1 + j // 3
        recs[j + 1, 0:4] = [0.1 * j, -0.2, 0.3, 0.01]
        recs[j + 1, 4:7] = [-(p * a + q * b), p, q]
        dirs.append([1.0, a, b])
    # a direction of the cell that is in nobody's band: the candidate with the largest smallest |den| / (|n|_1 |d|_1)
    cand = np.array([[1.0, (1 + 2 * i) / 256.0 + 1 / 1024.0, (1 + 2 * k) / 256.0 + 1 / 2048.0] for i in range(30) for k in range(30)], f32)
    den = np.abs(den_f32(np.concatenate([cand, np.zeros((len(cand), 1), f32)], axis=1), recs[1:, 4:7]))
    rel = (den / np.abs(recs[1:, 4:7]).sum(axis=1)[:, None] / np.abs(cand).sum(axis=1)[None]).min(axis=0)
    best = int(np.argmax(rel))
    assert rel[best] > 1e-4
    dirs.append(cand[best])
    return recs, mkrays(np.zeros(3), np.array(dirs, f32))


@pytest.mark.parametrize("n", [1, 3, 4, 5, 8, 9])
def test_hand_made_lists(n):
    """One cell lists all n normals.  The ray with den == 0 for the normal at list position j is refused, for every j (the
    entries of a batch's every slot, and of the part-filled last batch), the ray that no normal refuses is certified; walk,
    referee and restatement agree."""
    recs, rays = hand_scene(n)
    assert len(np.unique(recs[1:, 4:7], axis=0)) == n
    den = den_f32(rays[:, 4:8], recs[1:, 4:7])  # (normal, ray)
    assert (den[np.arange(n), np.arange(n)] == 0).all(), "the construction no longer reaches den == 0"
    table, cell, _ = table_and_cells(recs, rays, G_HAND, 1 << 16)
    assert (cell == cell[0]).all(), "the rays are not in one cell"
    for kappa in KAPPAS:
        c, nc = assert_walks_agree(recs, rays, G_HAND, kappa, f"hand {n}")
        assert (nc == n).all(), f"the cell does not list all {n} normals: {nc.tolist()}"
        assert not c[:n].any(), f"a ray with a zero den was certified: positions {np.nonzero(c[:n])[0].tolist()} of {n}"
        assert c[n], "the ray that no normal refuses was refused"
        cn, ncn = cert_numpy(table, cell, rays, kappa)
        assert np.array_equal(c, cn) and np.array_equal(nc, ncn)


# ---------------------------------------------------------------- 32-bit indices
@pytest.fixture(scope="module")
def wide_scene():
    """66 049 distinct normals within 4e-4 rad of +z (their lists are the cells along the equator z = 0) and, behind them, 40
    generic ones: indices 66 049 .. 66 088, beyond 16 bits.  Rays: 2048 directions with |d_z| largest, away from the equator,
    half of them nearly perpendicular to a generic normal -- their lists hold generic normals only."""
    rng = np.random.default_rng(41)
    i, j = np.meshgrid(np.arange(257), np.arange(257), indexing="ij")
    near_z = np.stack([i.ravel() * 1e-6, j.ravel() * 1e-6, np.ones(i.size)], axis=1)
    gen = unit(rng.normal(size=(40, 3))).astype(np.float64)
    gen = gen[np.abs(gen[:, 2]) < 0.9]
    nrm = np.concatenate([near_z, gen]).astype(f32)
    recs = np.zeros((len(nrm) + 1, 8), f32)
    recs[1:, 0:3], recs[1:, 3], recs[1:, 4:7] = rng.uniform(-1, 1, (len(nrm), 3)), 0.01, nrm
    d = rng.uniform(-0.9, 0.9, (2048, 3))
    d[:, 2] = rng.choice([-1.0, 1.0], len(d))
    k = rng.integers(0, len(gen), len(d) // 2)
    # move the first half onto the great circle of generic normal k (solve d_z n_z = -(d_x n_x + d_y n_y) for d_x or d_y)
    for r, g in enumerate(gen[k]):
        a = 0 if abs(g[0]) > abs(g[1]) else 1
        d[r, a] = -(d[r, 1 - a] * g[1 - a] + d[r, 2] * g[2]) / g[a]
    d = d[(np.abs(d[:, 0:2]) < 0.95).all(axis=1)]
    return recs, mkrays(rng.uniform(-1, 1, (len(d), 3)), d.astype(f32)), len(near_z)


def test_wide_indices(wide_scene):
    """More than 65 536 normals: the table has 32-bit indices.  The lists the rays read hold indices beyond 16 bits; walk,
    referee and restatement agree, and the comparison is not vacuous."""
    recs, rays, first_generic = wide_scene
    table, cell, c6 = table_and_cells(recs, rays, G_HAND, 1 << 23)
    g, off, idx, nrm = table_parts(table)
    assert int(table[3]) == 1 and len(nrm) > 65536, "the table has 16-bit indices"
    for kappa in KAPPAS:
        c, nc = assert_walks_agree(recs, rays, G_HAND, kappa, "wide")
        cn, ncn = cert_numpy(table, cell, rays, kappa)
        assert np.array_equal(c, cn) and np.array_equal(nc, ncn), "wide: the NumPy restatement disagrees"
    read = np.concatenate([idx[off[c_]:off[c_ + 1]] for c_ in np.unique(cell[nc <= CAP])])
    print(f"\nwide: {len(nrm)} normals, lists read {nc.min()} .. {nc.max()} long, indices {read.min()} .. {read.max()}, certified {c.mean():.3f}")
    assert (nc <= CAP).all() and (nc > 0).any() and read.min() >= first_generic > 65535
    assert c.any() and not c.all()


# ---------------------------------------------------------------- the last list of the table
def last_list_rays(table, n=64, seed=51):
    """rays whose cell is the one whose list ends where the index area ends (the last non-empty list) -> (directions, cell)"""
    g, off, _, _ = table_parts(table)
    c = int(np.nonzero(np.diff(off.astype(np.int64)) > 0)[0][-1])
    assert off[c + 1] == off[-1]
    face, i, j = c // (g * g), (c // g) % g, c % g
    rng = np.random.default_rng(seed)
    a = -1.0 + 2.0 * (i + rng.uniform(0.1, 0.9, n)) / g
    b = -1.0 + 2.0 * (j + rng.uniform(0.1, 0.9, n)) / g
    d = np.zeros((n, 3))
    d[:, face], d[:, (face + 1) % 3], d[:, (face + 2) % 3] = 1.0, a, b
    return (d * rng.uniform(0.5, 2.0, (n, 1))).astype(f32), c


@pytest.mark.parametrize("g", [1024, 128, 8])
def test_last_list_of_the_table(canonical, canon_tables, g):
    """A batch that starts inside the last list would run past the index area: no slot beyond the list's end may be read
    as an index (behind the index area lie padding and the normals: a word of those taken for an index would address a normal
    far outside the table).  Canonical table at G = 1024 (1 entry) and 128 (23 entries: five batches and a part-filled one),
    and the hand-made table of 5 normals at G = 8.  tools/cert_walk_host_check.cpp runs such rays in a stand-alone program
    for a build with -fsanitize=address,undefined."""
    if g == 8:
        recs, _ = hand_scene(5)
        table, _, _ = table_and_cells(recs, mkrays(np.zeros(3), [[1, 2, 3]]), g, 1 << 16)
    else:
        recs, table = canonical[2], canon_tables[g][0]
    d, c = last_list_rays(table)
    rays = mkrays(np.zeros(3), d)
    _, cell, _ = table_and_cells(recs, rays, g, len(table))
    assert (cell == c).all(), "the rays miss the last list's cell"
    _, off, _, _ = table_parts(table)
    for kappa in KAPPAS:
        cert, nc = assert_walks_agree(recs, rays, g, kappa, f"last list G {g}")
        assert (nc == off[c + 1] - off[c]).all()
        cn, _ = cert_numpy(table, cell, rays, kappa)
        assert np.array_equal(cert, cn)
    print(f"\nlast list G {g}: cell {c}, {nc[0]} entries, certified {cert.mean():.2f}")
