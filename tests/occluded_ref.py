"""The definition of the any-hit occlusion query (rtmi_occluded*, include/rtmi.h) in NumPy, from the oracle as it is:

    occluded[i] = (tri != 0) & (t < tmax[i])        compared in float32

where (tri, t) is the oracle's closest hit of ray i (Scene.trace, plus Scene.trace_spheres and the replacement rule where the
scene has analytic spheres).  NaN needs no special case: `t < tmax` is False when either side is NaN.  Also the ray sets and
the tmax families that tests/test_occluded_cpu.py and tests/test_occluded.py share."""
import numpy as np

F32 = np.float32
INF = F32(np.inf)

# The light of the shadow-segment set on the canonical scene (camera at (2, 0, 0) looking down +z, teapot around (0, 0.5, 5),
# mirror disks at (4, 4, 7) and (4, -3, 5)): above and to the left of the camera, in front of the teapot.  Checked in
# tests/test_occluded_cpu.py: between 5 % and 95 % of the segments are occluded.
LIGHT = (-3.0, 6.0, 1.0)


def closest_hits(so, o4, d4, spheres=False):
    """(tri, t) as rtmi_trace defines them: the tree's hit, replaced by a sphere's iff that is strictly closer (hit index =
    ntris + sphere index)."""
    tri, t, _, cn = so.trace(o4, d4)
    if spheres:
        idx_s, t_s, _ = so.trace_spheres(o4, d4)
        take = (idx_s != 0) & ((tri == 0) | (t_s < t))
        tri = np.where(take, so.num_tris() + idx_s - 1, tri).astype(np.uint32)
        t = np.where(take, t_s, t).astype(F32)
    return tri, t, cn


def from_hits(tri, t, tmax):
    """The rule itself; tmax None = +inf for every ray"""
    t = np.asarray(t, F32)
    lim = np.full(t.shape, INF, F32) if tmax is None else np.asarray(tmax, F32)
    with np.errstate(invalid="ignore"):
        return ((np.asarray(tri) != 0) & (t < lim)).astype(np.uint8)


def expected(so, o4, d4, tmax, spheres=False):
    tri, t, _ = closest_hits(so, o4, d4, spheres)
    return from_hits(tri, t, tmax)


def tmax_families(t, seed=0):
    """name -> tmax (None = the NULL pointer) for rays whose closest-hit times are t (0 for a miss): the limits the issue
    lists, and a per-ray random mix of all of them so that neighbouring lanes leave the walk at different steps."""
    t = np.asarray(t, F32)
    n = t.shape[0]
    fam = {
        "null": None,
        "inf": np.full(n, INF, F32),
        "t": t.copy(),
        "nextafter": np.nextafter(t, INF),
        "half": t / F32(2),
        "zero": np.zeros(n, F32),
        "nan": np.full(n, np.nan, F32),
        "minus_one": np.full(n, -1.0, F32),
    }
    rng = np.random.default_rng(seed)
    names = [k for k in fam if k != "null"]
    pick = rng.integers(0, len(names), n)
    fam["mix"] = np.choose(pick, [fam[k] for k in names]).astype(F32)
    return fam


def shadow_segments(so, o4, d4, light=LIGHT):
    """Shadow segments from the first hits of the rays (o4, d4) to `light`: for every ray that hits with a finite t, origin =
    hit point moved 1e-3 along the hit normal (the triangle's norm, turned to the side the ray came from), direction = unit
    vector to the light, tmax = distance to the light.  All arithmetic in float32, in the order written here.
    -> (orig4, dir4, tmax)"""
    tri, t, face, _ = so.trace(o4, d4)
    rec, _, _ = so.triangles()
    keep = (tri != 0) & np.isfinite(t)
    tri, t, face = tri[keep], t[keep].astype(F32), face[keep]
    o, d = o4[keep, :3].astype(F32), d4[keep, :3].astype(F32)
    nrm = rec[tri, 3:6].astype(F32) * np.where(face & 1, F32(-1), F32(1)).astype(F32)[:, None]
    p = o + d * t[:, None]
    org = p + nrm * F32(1e-3)
    v = np.asarray(light, F32)[None, :] - org
    dist = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]).astype(F32)
    n = org.shape[0]
    so4, sd4 = np.zeros((n, 4), F32), np.zeros((n, 4), F32)
    so4[:, :3] = org
    sd4[:, :3] = v / dist[:, None]
    return so4, sd4, dist


def random_rays_canonical(n=20000, seed=7):
    """The rays of tests/test_gpu_parity.py::test_trace_random_rays_canonical (same generator, same seed)"""
    rng = np.random.default_rng(seed)
    o4 = np.zeros((n, 4), F32)
    d4 = np.zeros((n, 4), F32)
    o4[:, :3] = rng.uniform(-6, 6, (n, 3)) + np.array([0, 0, 6])
    d = rng.normal(size=(n, 3))
    d4[:, :3] = d / np.linalg.norm(d, axis=1, keepdims=True)
    return o4, d4, rng


def edge_case_rays():
    """The rays of tests/test_gpu_parity.py::test_trace_edge_case_rays on the axis-box scene: zero direction components,
    origins on planes, NaN, inf and a zero direction"""
    rays = []
    for ox in (-1.0, -0.5, 0.0, 0.25, 1.0):
        for oy in (-1.0, 0.0, 0.25, 0.5):
            for dvec in ((0, 0, 1), (0, 0, -1), (1, 0, 0), (0, 1, 0), (0, -1, 0), (-1, 0, 0), (0.6, 0, 0.8), (0, 0.6, 0.8),
                         (-0.0, 0.0, 1.0), (1e-30, 0, 1), (0.57735026, 0.57735026, 0.57735026)):
                rays.append(((ox, oy, 3.5, 0.0), (*dvec, 0.0)))
                rays.append(((ox, oy, 5.0, 0.0), (*dvec, 0.0)))
                rays.append(((-1.0, oy, 4.0, 0.0), (*dvec, 0.0)))
    rays += [((0, 0, 0, 0), (np.nan, 0, 1, 0)), ((np.nan, 0, 0, 0), (0, 0, 1, 0)), ((0, 0, 0, np.nan), (0, 0, 1, 0)),
             ((0, 0, 0, 0), (0, 0, 1, np.nan)), ((np.inf, 0, 0, 0), (0, 0, 1, 0)), ((0, 0, 0, 0), (0, 0, 0, 0))]
    return np.array([r[0] for r in rays], F32), np.array([r[1] for r in rays], F32)


def soup_recipe(seed):
    """The scene of tests/test_gpu_parity.py::test_random_triangle_soups for `seed` (same generator, same draws) ->
    (recipe(api), (w, h, viewport arguments))"""
    rng = np.random.default_rng(1000 + seed)
    ntri = int(rng.integers(40, 400))
    centre = rng.uniform(-3, 3, (ntri, 3)) + np.array([0, 0, 8.0])
    pts = (centre[:, None, :] + rng.normal(scale=rng.uniform(0.2, 1.2), size=(ntri, 3, 3))).astype(F32)
    kinds = rng.integers(0, 3, ntri)
    cols = rng.integers(0, 256, (ntri, 3))
    alphas = rng.uniform(0.05, 0.95, ntri)
    scat = rng.uniform(0.0, 0.3, ntri)
    edges = rng.choice([0.0, 0.05, 0.3, -1.0], ntri)
    maxdepth, minobjs = int(rng.integers(2, 9)), int(rng.integers(2, 24))

    def recipe(api):
        s = api.scene()
        for i in range(ntri):
            c = tuple(int(x) for x in cols[i])
            surf = (api.solid(c), api.matte(c, float(alphas[i])), api.reflective(float(scat[i]), c, float(alphas[i])))[kinds[i]]
            try:
                api.add_triangle(s, pts[i], surf, float(edges[i]))
            except RuntimeError:
                pass  # degenerate triangle: rejected identically by both implementations
        s.populate_triangle_numbers()
        s.build_bounding_box([0.0, 0.0, 8.0], 8.0, maxdepth, minobjs)
        return s
    pos = rng.uniform(-1, 1, 3).astype(F32)
    aim = [float(rng.uniform(-0.3, 0.3)), float(rng.uniform(-0.3, 0.3)), 1.0]
    return recipe, (40, 28, pos, aim)
