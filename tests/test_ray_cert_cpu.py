"""Per-ray sign certificate of k_trace_oct's block cull (trace_oct.hpp, ray_sign_certified; DESIGN.md 4.1 "Sign certificate
per ray").  CPU only: rtmi_debug_ray_cull builds the direction table and the packed records and evaluates the certificate on
the host with the kernel's own __host__ __device__ functions.  Checked here: the table lists every normal that can be
near-perpendicular to a direction of a cell (float64), a certified ray has a nonzero f32 `den` and a finite `t` for every
triangle of the scene, and adversarial directions are refused or sound."""
import ctypes as C

import numpy as np
import pytest

from test_block_cull_cpu import canonical, mkrays, mkrecs, one_per_block, unit  # noqa: F401  (canonical: a fixture)

f32 = np.float32
TAU, KAPPA, CAP = 1e-4, 1e-6, 64  # CERT_TAU, CERT_KAPPA, CERT_CAP of trace_oct.hpp
G = 1024                          # the default of rtmi_scene_create (the canonical scene's table)
G_SMALL = 256                     # for the many small synthetic scenes


def ray_cull(recs, blocks, rays, g=G_SMALL, table=False):
    """-> dict(packed (nb, 4) u32, cert (n,) bool, ncand (n,) u32, cell (n,) u32, out (nb, n) u8 [, table u32 words])"""
    from rust_raytrace_amd import _ffi
    L = _ffi.lib()
    vp = C.c_void_p
    L.rtmi_debug_ray_cull.restype = C.c_int
    L.rtmi_debug_ray_cull.argtypes = [vp, C.c_uint64, vp, C.c_uint64, vp, C.c_uint64, C.c_uint32, vp, vp, vp, vp, vp, vp,
                                      C.c_uint64, vp]
    recs = np.ascontiguousarray(recs, f32)
    blocks = np.ascontiguousarray(blocks, np.uint32).reshape(-1, 4)
    rays = np.ascontiguousarray(rays, f32)
    r = dict(packed=np.zeros((len(blocks), 4), np.uint32), cert=np.zeros(len(rays), np.uint8), ncand=np.zeros(len(rays), np.uint32),
             cell=np.zeros(len(rays), np.uint32), out=np.zeros((len(blocks), len(rays)), np.uint8))
    words = C.c_uint64(0)
    cap = 3 * g * g * 12 + (1 << 20) if table else 0
    tab = np.zeros(max(cap, 1), np.uint32)
    rc = L.rtmi_debug_ray_cull(recs.ctypes.data, len(recs), blocks.ctypes.data, len(blocks), rays.ctypes.data, len(rays), g,
                               r["packed"].ctypes.data, r["cert"].ctypes.data, r["ncand"].ctypes.data, r["cell"].ctypes.data,
                               r["out"].ctypes.data, tab.ctypes.data if table else None, cap, C.byref(words))
    assert rc == 0
    r["cert"] = r["cert"].astype(bool)
    if table:
        assert words.value <= cap, "table larger than the test's buffer"
        r["table"] = tab[:words.value]
    return r


def table_parts(t):
    """(G, offsets (3 G G + 1,), indices, normals (k, 4) f32: n.xyz, |n|_1)"""
    g, i0, n0, wide = int(t[0]), int(t[1]), int(t[2]), int(t[3])
    off = t[4:4 + 3 * g * g + 1]
    idx = t[i0:n0] if wide else t[i0:n0].view(np.uint16)
    return g, off, idx[:off[-1]], t[n0:].view(f32).reshape(-1, 4)


def den_f32(d, n):
    """`den` of the LEAF step's plane test in the kernel's operation order: d (k, 4) f32, n (m, 3) f32 -> (m, k)"""
    d, n = d[None], n[:, None]
    with np.errstate(all="ignore"):
        return (((f32(0) + n[..., 0] * d[..., 0]) + n[..., 1] * d[..., 1]) + n[..., 2] * d[..., 2]) + f32(0) * d[..., 3]


def t_f32(rays, recs):
    """(den, t) of the plane test, (m, n)"""
    o, c, n = rays[None, :, 0:4], recs[:, None, 0:3], recs[:, None, 4:7]
    with np.errstate(all="ignore"):
        a = c - o[..., :3]
        num = ((((f32(0) + n[..., 0] * a[..., 0]) + n[..., 1] * a[..., 1]) + n[..., 2] * a[..., 2]) + f32(0) * (f32(0) - o[..., 3]))
        den = den_f32(rays[:, 4:8], recs[:, 4:7])
        return den, num / den


def assert_certified_sound(rays, recs, cert):
    """every certified ray: den != 0 and t finite for every real record"""
    den, t = t_f32(rays[cert], recs[1:])
    assert (den != 0).all() and np.isfinite(den).all(), "a certified ray has a zero den"
    assert np.isfinite(t).all(), "a certified ray has a non-finite t"


def assert_table_sound(t, d):
    """directions d (k, 3) f32, all accepted by block_cull_ray: every normal NOT listed for d's cell has |u . d| > tau |d|_1"""
    g, off, idx, nrm = table_parts(t)
    rays = mkrays(np.zeros(3), d)
    cell = ray_cull(np.zeros((1, 8), f32), np.zeros((0, 4), np.uint32), rays, g)["cell"]
    assert (cell < 3 * g * g).all()
    u = nrm[:, 0:3].astype(np.float64)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    dd = d.astype(np.float64)
    dots = np.abs(u @ dd.T)                      # (normals, k)
    thr = TAU * np.abs(dd).sum(axis=1)[None, :]
    listed = np.zeros(dots.shape, bool)
    for k, c in enumerate(cell):
        listed[idx[off[c]:off[c + 1]], k] = True
    bad = ~listed & (dots <= thr)
    assert not bad.any(), f"unlisted but near-perpendicular: (normal, direction) {np.argwhere(bad)[:5].tolist()}"
    return listed


def border_directions(g, rng, n=400):
    """directions on cell borders, cube edges and corners of the folded cube map, a few ulp to either side"""
    out = []
    for _ in range(n):
        face = rng.integers(0, 3)
        a = -1.0 + 2.0 * rng.integers(0, g + 1) / g
        b = rng.choice([-1.0 + 2.0 * rng.integers(0, g + 1) / g, rng.uniform(-1, 1), -1.0, 1.0])
        v = np.zeros(3)
        v[face], v[(face + 1) % 3], v[(face + 2) % 3] = rng.choice([-1.0, 1.0]), a, b
        v = (v * 10.0 ** rng.uniform(-2, 2)).astype(f32)
        for k in (-2, -1, 0, 1, 2):
            w = v.copy()
            j = rng.integers(0, 3)
            for _ in range(abs(k)):
                w[j] = np.nextafter(w[j], f32(np.inf if k > 0 else -np.inf))
            out.append(w)
    d = np.array(out, f32)
    return d[(np.abs(d) > 1e-6).all(axis=1)]  # (a zero or denormal component: block_cull_ray refuses the ray)


SYN = mkrecs([[0, 0, 5], [1, 2, 3], [-2, 1, 4]], [0.5, 0.3, 0.2], [[0, 0, 1], [1, -1, 0], [0.3, -0.7, 0.2]])


@pytest.fixture(scope="module")
def canon_table(canonical):
    so, raw, recs, _, ob, rays = canonical
    return ray_cull(recs, ob[:1], rays, G, table=True)


def test_table_sound_canonical(canonical, canon_table):
    """Random and border directions against the canonical scene's table; list lengths reported."""
    rng = np.random.default_rng(21)
    t = canon_table["table"]
    g, off, idx, nrm = table_parts(t)
    d = np.concatenate([unit(rng.normal(size=(600, 3))), border_directions(g, rng)])
    assert_table_sound(t, d)
    ln = np.diff(off.astype(np.int64))
    print(f"\ncanonical table: G {g}, {len(nrm)} distinct normals, {off[-1]} entries, {ln.mean():.1f} per cell (longest {ln.max()}), "
          f"{t.nbytes / 1e6:.1f} MB")
    assert len(nrm) < len(canonical[2])  # deduplicated


def test_table_sound_synthetic():
    rng = np.random.default_rng(22)
    for g in (8, 64, 256):
        t = ray_cull(SYN, one_per_block(3), mkrays([0, 0, 0], [1, 1, 1]), g, table=True)["table"]
        _, off, idx, nrm = table_parts(t)
        assert len(nrm) == 3
        d = np.concatenate([unit(rng.normal(size=(300, 3))), border_directions(g, rng, 200)])
        listed = assert_table_sound(t, d)
        assert not listed.all()


def test_certified_rays_sound_and_share(canonical, canon_table):
    """The fixture's 256 bounce-like rays: >= 95 % certified, and every certified one has a nonzero den and a finite t for
    every triangle of the scene."""
    _, _, recs, _, _, rays = canonical
    cert, ncand = canon_table["cert"], canon_table["ncand"]
    print(f"\ncertified {cert.mean():.4f} of {len(rays)} rays; candidates per ray {ncand.mean():.1f} (max {ncand.max()})")
    assert cert.mean() >= 0.95
    assert_certified_sound(rays, recs, cert)


def _ulps(x, k):
    x = f32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, f32(np.inf if k > 0 else -np.inf))
    return x


def test_adversarial_directions(canonical):
    """d perpendicular to a scene normal in f32 (computed den == 0) and 1, 2, 4 ulp off; scaled 1e-9 .. 1e9."""
    _, _, recs, _, ob, _ = canonical
    rng = np.random.default_rng(23)
    ds = []
    for j in rng.integers(1, len(recs), 150):
        n = recs[j, 4:7].astype(np.float64)
        d = unit(np.cross(n, rng.normal(size=3)))
        # solve the smallest-weight component so that the f32 den is as near 0 as it gets
        k = int(np.argmax(np.abs(n)))
        rest = sum(float(n[a]) * float(d[a]) for a in range(3) if a != k)
        d[k] = f32(-rest / n[k])
        # the neighbour of that within 16 ulp whose f32 den is smallest in magnitude (often exactly 0)
        cand = np.repeat(d[None], 33, axis=0)
        for i, ul in enumerate(range(-16, 17)):
            cand[i, k] = _ulps(d[k], ul)
        dn = np.abs(den_f32(np.concatenate([cand, np.zeros((33, 1), f32)], axis=1), recs[j:j + 1, 4:7])[0])
        d = cand[int(np.argmin(dn))]
        for ul in (0, 1, -1, 2, -2, 4, -4):
            w = d.copy()
            w[k] = _ulps(w[k], ul)
            for s in (1.0, 1e-9, 1e-3, 1e3, 1e9):
                ds.append(w * f32(s))
    d = np.array(ds, f32)
    d = d[(d != 0).all(axis=1)]
    rays = mkrays(recs[rng.integers(1, len(recs), len(d)), 0:3], d)
    r = ray_cull(recs, ob[:1], rays, G)
    den = den_f32(rays[:, 4:8], recs[1:, 4:7])
    zero = (den == 0).any(axis=0)
    print(f"\n{len(d)} adversarial directions: {zero.sum()} with an exactly-zero den, {(~r['cert']).sum()} refused")
    assert zero.sum() > 0, "the construction no longer reaches den == 0"
    assert not r["cert"][zero].any(), "a ray with a zero den was certified"
    # each direction is within 4 ulp of one whose den is a rounding residue: far below kappa |n|_1 |d|_1
    assert (~r["cert"]).mean() > 0.9
    assert_certified_sound(rays, recs, r["cert"])
    # an exactly-zero den with no zero component: n = (1, -1, 0) / sqrt(2), d = (p, p, q)
    dz = np.array([[1, 1, 1e-3], [0.5, 0.5, -0.7], [3e-9, 3e-9, 1e-9], [2e8, 2e8, 1e9]], f32)
    rz = mkrays([[0, 0, 9]], dz)
    assert (den_f32(rz[:, 4:8], SYN[1:, 4:7]) == 0).any(axis=0).all()
    assert not ray_cull(SYN, one_per_block(3), rz)["cert"].any()


def test_axis_aligned_normals_and_refused_rays():
    """Axis-aligned normals with d in their plane (a zero component: block_cull_ray refuses) or a few ulp off it; rays that
    block_cull_ray refuses are never certified."""
    blocks = one_per_block(3)
    o = [0.1, 0.2, 0.3]
    d = [unit([1, 2, 0]), [1, 2, 1e-12], [1, 2, 1e-7], [1, 2, 1e-4], unit([1, 2, -3])]
    # |d_z| = 1e-12 is below 2^-40 max |d_k|: refused by block_cull_ray; 1e-7 |d|: den = 1e-7, below kappa |n|_1 |d|_1
    r = ray_cull(SYN, blocks, mkrays(o, np.array(d, f32)))
    assert r["cert"].tolist() == [False, False, False, True, True]
    bad = []
    good = mkrays([o], [unit([1, 2, -3])])
    for col, val in ((3, 1e-3), (7, 1e-3), (3, np.nan), (7, -1.0), (0, np.nan), (5, np.nan), (0, 1e16), (1, -np.inf), (4, 0.0),
                     (5, -0.0), (6, 1e-42), (4, 1e-14), (4, np.inf), (4, 1e30)):
        q = good.copy()
        q[0, col] = f32(val)
        bad.append(q[0])
    for s in (1e-30, 1e-20, 1e-11, 1e11, 1e30):
        q = good.copy()
        q[0, 4:7] *= f32(s)
        bad.append(q[0])
    r = ray_cull(SYN, blocks, np.array(bad, f32))
    assert not r["cert"].any() and not (r["out"] & 4).any() and (r["ncand"] == 0).all()
    ok = np.concatenate([good * np.array([1, 1, 1, 1, s, s, s, 1], f32) for s in (1e-9, 1e-3, 1e3, 1e9)])
    r = ray_cull(SYN, blocks, ok)
    assert r["cert"].all()
    assert_certified_sound(ok, SYN, r["cert"])


def test_long_list_refuses():
    """More normals near-perpendicular to one direction than the cap: the ray is refused, others are not."""
    rng = np.random.default_rng(24)
    d0 = unit([0.3, -0.5, 0.8]).astype(np.float64)
    nrm = np.cross(d0, rng.normal(size=(CAP + 40, 3))) + d0 * rng.uniform(2e-4, 1e-3, (CAP + 40, 1))
    recs = mkrecs(rng.uniform(-1, 1, (len(nrm), 3)), [0.1] * len(nrm), nrm)
    r = ray_cull(recs, one_per_block(4), mkrays([[0, 0, 0]] * 2, [d0, unit([1, 1, 1])]))
    assert r["ncand"][0] > CAP and not r["cert"][0]
    assert r["cert"][1]
