"""A float64 statistical referee for everything that draws: Lambert sampling, fuzzy reflection, the pixel jitter, the AO
hemisphere rays and the keying of the random blocks per pixel, sample and bounce.  Plain NumPy with NumPy's own generator; it
imports nothing of oracle/ and none of the other *_ref.py.  It simulates the reference's DEFINITIONS, read from the reference's
source (cited by line below), and asks one question of a renderer's own outputs: do its draws have the distribution the
definition says, independently across pixels, samples and bounces?  The scene is the measuring instrument.

The definitions (raytrace_lib/src/raytrace.rs):
  * random_vec (:188-192): r = unit(U - 0.5), U uniform in the unit cube.  NOT isotropic: the cube's corners weigh more.
  * lambertian_ray (:292-297): origin p + 0.001 r, direction n + r (make_ray stores its unit), n the normal of the face that was
    hit, negated on the back face.  The offset is along r, not n: when r.n < 0 the origin lies behind the surface, the ray
    re-hits its own triangle on the back face, and the next bounce leaves with the negated normal.
  * reflect_ray (:278-290): reflect = d + 2 |d.n| n, direction unit(reflect + fuzz r), origin p + 0.001 direction.
  * color_ray / project_ray (:1199-1295): depth 0 is black, a miss is the sky, Solid returns its colour, Matte and Reflective
    return mix_color(colour, next, alpha) = colour (1 - alpha) + next alpha (:299-301): with alpha = 1 exactly the next colour.
  * pixel_ray (:1374-1394): the ray's origin is the viewport point orig + vu/width (col + u) + vv/height (row + v) (walk_ray_set
    calls it with (row, col), :1416), (u, v) = (0.5, 0.5) at one sample per pixel and two uniform draws otherwise.
  * the AO buffer (include/rtmi.h, rtmi_render_ao): K rays per primary sample from p + n bias along unit(n + r), a ray counts
    as occluded when it hits anything at t < radius.

The probe: a 3 x 3 floor quad (two triangles, no edge band, alpha 1) centred at C = (0, 0, 5) inside a closed dome, an
icosahedron subdivided once (80 Solid triangles, each its own colour), radius 8 about C, turned by a fixed rotation.  The camera
sits at the origin and looks down +z through a 0.01 x 0.01 viewport with a field of view of one degree: every primary ray lands
within 0.05 of C.  round(colour * 255) then says, per sample and exactly, which dome face a path ended on; black means it ran
out of depth on the floor, the sky that a ray left a watertight dome."""
import statistics

import numpy as np

F32 = np.float32
C = np.array([0.0, 0.0, 5.0])
DOME_RADIUS, FLOOR_EDGE = 8.0, 3.0
ROOT = ([0.137, -0.211, 5.093], 9.3)          # the floor lies in no split plane of this box
OCTREE = (4, 8)                               # depth, minobjs
NORMALS = {"facing": (0.0, 0.0, -1.0), "diagonal": (1.0, 1.0, -1.0), "tilted": (0.3, 0.52, -0.8)}
SEEDS = (1, 2, 3)
W = H = 256
P_FALSE = 1e-6                                # false-alarm probability of every statistical assertion
MIN_EXPECTED = 20                             # bins expected to hold fewer samples than this are pooled into one
REF_FACTOR = 16                               # the referee draws 16 chains per observed one
NFACES = 80
BLACK, SKY, UNDECODED = 80, 81, 82            # bin numbers after the dome's faces
SKY_RGB = (128, 180, 255)                     # raytrace.rs:1264
FLOOR_RGB = (200, 200, 200)                   # never seen: alpha is 1
VIEW = dict(size=(0.01, 0.01), pos=(0.0, 0.0, 0.0), aim=(0.0, 0.0, 1.0), fov=1.0, roll=0.0)


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


# ---------------------------------------------------------------- the probe's geometry
def _rotation():
    ax = _unit([0.43, -0.71, 0.56])
    ang = 1.234
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)


def dome_triangles():
    """(80, 3, 3) float32: an icosahedron subdivided once, vertices pushed out to DOME_RADIUS about C, turned by _rotation()"""
    g = (1 + 5 ** 0.5) / 2
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1),
         (-g, 0, -1), (-g, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    verts = [_unit(x) for x in v]
    mid = {}

    def midpoint(a, b):
        key = (min(a, b), max(a, b))
        if key not in mid:
            verts.append(_unit(verts[a] + verts[b]))
            mid[key] = len(verts) - 1
        return mid[key]

    faces = []
    for a, b, c in f:
        ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
        faces += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
    p = (np.array(verts) * DOME_RADIUS) @ _rotation().T + C
    p32 = p.astype(F32)                                     # one float32 value per shared vertex: watertight by construction
    return p32[np.array(faces)]


FLOOR_TURN = -1.45


def _frame(normal):
    """(n, u, v), right-handed with u x v = n, the in-plane axes turned by FLOOR_TURN.  The turn matters for the floor that
    faces the camera: a triangle parallel to an axis plane fails every face test of the reference's builder (the axis-plane
    quirks of DESIGN.md), so a leaf lists it only if it holds one of its corners or its centre.  With this turn the corner the two
    floor triangles share lies in the leaf of ROOT that holds C, so both are listed there (tests/test_draw_cpu.py checks it)."""
    n = _unit(normal)
    e = np.eye(3)[np.abs(n).argmin()]
    u0 = _unit(np.cross(n, e))
    v0 = np.cross(n, u0)
    u = np.cos(FLOOR_TURN) * u0 + np.sin(FLOOR_TURN) * v0
    return n, u, np.cross(n, u)


def floor_triangles(normal, flip=False):
    """(2, 3, 3) float32: the floor quad with face normal unit(normal) (flip: the opposite winding, so -unit(normal))"""
    n, u, v = _frame(normal)
    a = FLOOR_EDGE / 2
    p00, p10, p11, p01 = C - a * u - a * v, C + a * u - a * v, C + a * u + a * v, C - a * u + a * v
    t = np.array([(p00, p10, p11), (p00, p11, p01)])
    if flip:
        t = t[:, ::-1]
    return t.astype(F32)


def occluder_triangles(normal):
    """(2, 3, 3) float32: a quad standing on the floor one unit from C (along the floor's u axis), 8 wide and 4 high on the
    side unit(normal) points to: with an AO radius of 3 part of it is beyond the radius"""
    n, u, v = _frame(normal)
    b = C + 1.0 * u
    q00, q10, q11, q01 = b - 4 * v, b + 4 * v, b + 4 * v + 4 * n, b - 4 * v + 4 * n
    return np.array([(q00, q10, q11), (q00, q11, q01)]).astype(F32)


def dome_rgb(k):
    return (k + 1, 254 - k, 7)


def recipe(normal="tilted", floor=("matte",), accel="octree", dome=True, occluder=False, flip=False, extra=()):
    """recipe(api) for conftest.OracleApi / ProductApi.  floor: ("matte",) or ("reflective", scattering), alpha 1 either way;
    extra: further (corners (3, 3), rgb) Solid triangles."""
    def r(api):
        s = api.scene()
        surf = api.matte(FLOOR_RGB, 1.0) if floor[0] == "matte" else api.reflective(float(floor[1]), FLOOR_RGB, 1.0)
        for t in floor_triangles(NORMALS[normal], flip):
            api.add_triangle(s, t, surf, 0.0)
        if dome:
            for k, t in enumerate(dome_triangles()):
                api.add_triangle(s, t, api.solid(dome_rgb(k)), 0.0)
        if occluder:
            for t in occluder_triangles(NORMALS[normal]):
                api.add_triangle(s, t, api.solid((9, 9, 9)), 0.0)
        for t, rgb in extra:
            api.add_triangle(s, np.asarray(t, F32), api.solid(rgb), 0.0)
        s.populate_triangle_numbers()
        if accel == "octree":
            s.build_bounding_box(ROOT[0], ROOT[1], *OCTREE)
        else:
            s.build_trivial_bounding_box(ROOT[0], ROOT[1])
        return s
    return r


def decode(rgba):
    """Per-sample colours (..., >= 3) -> bins: the dome face 0..79, BLACK, SKY or UNDECODED.  A colour decodes only when
    colour * 255 is an integer triple to 1e-3 (float32 colours are exact to 255 * 2^-24 = 1.5e-5)."""
    c = np.asarray(rgba, np.float64)[..., :3] * 255.0
    q = np.rint(c)
    exact = (np.abs(c - q) < 1e-3).all(axis=-1)
    q = q.astype(np.int64)
    r, g, b = q[..., 0], q[..., 1], q[..., 2]
    out = np.full(q.shape[:-1], UNDECODED, np.int64)
    face = exact & (b == 7) & (r >= 1) & (r <= NFACES) & (g == 255 - r)
    out[face] = r[face] - 1
    out[exact & (r == 0) & (g == 0) & (b == 0)] = BLACK
    out[exact & (r == SKY_RGB[0]) & (g == SKY_RGB[1]) & (b == SKY_RGB[2])] = SKY
    return out


class Probe:
    """The float64 view of a probe scene: floor (2, 3, 3), the dome as 80 outward planes (valid because the dome is convex and
    every chain stays inside it: convex() checks the first), optional occluder triangles."""

    def __init__(self, normal="tilted", flip=False, dome=True, occluder=False, extra=()):
        self.frame = _frame(NORMALS[normal])
        self.extra = np.array([np.asarray(t, F32) for t, _ in extra], np.float64).reshape(-1, 3, 3)
        self.floor = floor_triangles(NORMALS[normal], flip).astype(np.float64)
        a, b, c = self.floor[0]
        self.n = _unit(np.cross(b - a, c - a))               # the face normal of the floor as built
        self.dome = dome_triangles().astype(np.float64) if dome else None
        if dome:
            d = self.dome
            nk = _unit(np.cross(d[:, 1] - d[:, 0], d[:, 2] - d[:, 0]))
            nk *= np.sign(np.einsum("kj,kj->k", nk, d[:, 0] - C))[:, None]
            self.nk, self.hk = nk, np.einsum("kj,kj->k", nk, d[:, 0])
        self.occ = occluder_triangles(NORMALS[normal]).astype(np.float64) if occluder else None

    def convex(self):
        """the largest n_k . (vertex - plane k) over all dome vertices and faces, in units of the radius: <= 0 up to rounding"""
        v = self.dome.reshape(-1, 3)
        return float((v @ self.nk.T - self.hk[None, :]).max() / DOME_RADIUS)

    @staticmethod
    def tri_hits(tris, o, d):
        """Nearest t > 0 at which rays (o, d) cross any of tris (m, 3, 3), inf for none (Moeller-Trumbore in float64)"""
        best = np.full(len(o), np.inf)
        for a, b, c in tris:
            e1, e2 = b - a, c - a
            pv = np.cross(d, e2)
            det = pv @ e1
            with np.errstate(all="ignore"):
                inv = 1.0 / det
                tv = o - a
                u = np.einsum("kj,kj->k", tv, pv) * inv
                qv = np.cross(tv, e1)
                v = np.einsum("kj,kj->k", qv, d) * inv
                t = (qv @ e2) * inv
            ok = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0)
            best = np.where(ok & (t < best), t, best)
        return best

    def blockers(self):
        """everything a secondary ray of the AO and light buffers can hit in a scene without the dome"""
        return np.concatenate([self.floor] + ([self.occ] if self.occ is not None else []) + ([self.extra] if len(self.extra) else []))

    def floor_hit(self, o, d):
        return self.tri_hits(self.floor, o, d)

    def dome_exit(self, o, d):
        """(t, face) where a ray from inside the convex dome leaves it"""
        den = d @ self.nk.T
        num = self.hk[None, :] - o @ self.nk.T
        with np.errstate(all="ignore"):
            t = np.where(den > 0, num / den, np.inf)
        k = t.argmin(axis=1)
        return t[np.arange(len(o)), k], k

    def primary_hits(self, o4, d4):
        """Where the primary rays (the renderer's own, as inputs) meet the floor, in float64 -> (p, unit d); all must hit"""
        o = np.asarray(o4, np.float64).reshape(len(o4), -1)[:, :3]
        d = _unit(np.asarray(d4, np.float64).reshape(len(d4), -1)[:, :3])
        t = self.floor_hit(o, d)
        assert np.isfinite(t).all(), "a primary ray of the probe misses the floor"
        p = o + t[:, None] * d
        assert np.abs(p - C).max() <= 0.15, "primary hits must land near C (0.05 across the view, more along a tilted floor)"
        return p, d


# ---------------------------------------------------------------- samplers: the right one and the wrong ones
def random_vec(rng, idx, j, total):
    """raytrace.rs:188-192"""
    return _unit(rng.random((len(idx), 3)) - 0.5)


def wrong_sphere(rng, idx, j, total):
    return _unit(rng.normal(size=(len(idx), 3)))


def wrong_unnormalised(rng, idx, j, total):
    return rng.random((len(idx), 3)) - 0.5


def wrong_reused_word(rng, idx, j, total):
    u = rng.random((len(idx), 3))
    u[:, 2] = u[:, 1]
    return _unit(u - 0.5)


def wrong_uncentred(rng, idx, j, total):
    return _unit(rng.random((len(idx), 3)) + 1e-300)


class WrongSameDrawEveryBounce:
    """bounce 2, 3, ... reuse the vector of bounce 1 (one random block used for every bounce)"""

    def __init__(self):
        self.first = None

    def __call__(self, rng, idx, j, total):
        if j == 1:
            self.first = np.zeros((total, 3))
            self.first[idx] = random_vec(rng, idx, j, total)
        return self.first[idx]


# ---------------------------------------------------------------- the chain simulators
def chains(probe, p, d, floor, maxdepth, rng, sampler=random_vec, flip_hemisphere=False, chunk=1 << 16):
    """Follow project_ray from primary hits p (M, 3) reached along unit d (M, 3) on a floor ("matte",) / ("reflective", fuzz)
    of alpha 1, against the floor and the dome, for up to `maxdepth` rays per chain (the primary is ray 1).
    -> (end (M,): the number of the ray that reached the dome, maxdepth + 1 if none did; face (M,): the dome face, -1 if none).
    outcome(end, face, D) and rays(end, D) read off the result for any D <= maxdepth: the draws do not depend on D."""
    M = len(p)
    end = np.full(M, maxdepth + 1, np.int64)
    face = np.full(M, -1, np.int64)
    sampler_state = sampler
    for s0 in range(0, M, chunk):
        sl = slice(s0, min(s0 + chunk, M))
        pp, dd = p[sl].copy(), d[sl].copy()
        m = len(pp)
        if isinstance(sampler, type):
            sampler_state = sampler()
        alive = np.arange(m)
        for j in range(1, maxdepth):                                      # hit j is on the floor: spawn ray j + 1
            if len(alive) == 0:
                break
            pa, da = pp[alive], dd[alive]
            nf = probe.n[None, :] * -np.sign(da @ probe.n)[:, None]       # the face normal, negated on the back face
            if flip_hemisphere:
                nf = -nf
            r = sampler_state(rng, alive, j, m)
            if floor[0] == "matte":
                o2, d2 = pa + 0.001 * r, _unit(nf + r)
            else:
                refl = da + 2 * np.abs(np.einsum("kj,kj->k", da, nf))[:, None] * nf
                d2 = _unit(refl + float(floor[1]) * r)
                o2 = pa + 0.001 * d2
            tf = probe.floor_hit(o2, d2)
            td, fk = probe.dome_exit(o2, d2)
            again = tf < td
            done = alive[~again]
            end[s0 + done] = j + 1
            face[s0 + done] = fk[~again]
            pp[alive[again]] = o2[again] + tf[again, None] * d2[again]
            dd[alive[again]] = d2[again]
            alive = alive[again]
    return end, face


def outcome(end, face, D):
    """the bin of every chain at maxdepth D: its dome face, or BLACK when the chain ran out of depth on the floor"""
    return np.where(end <= D, face, BLACK)


def rays(end, D):
    """rays traced per chain at maxdepth D (the `rays` counter, raytrace.rs:1278)"""
    return np.minimum(end, D)


def referee_points(p, d, factor=REF_FACTOR):
    """REF_FACTOR copies of every observed primary hit: the referee's chains start where the renderer's do"""
    return np.repeat(p, factor, axis=0), np.repeat(d, factor, axis=0)


def ao_visible(probe, p, nf, K, radius, bias, rng, sampler=random_vec, shared=False):
    """rtmi_render_ao's rule at points p (m, 3) with face normals nf (m, 3): K rays each from p + nf bias along unit(nf + r),
    visible unless something (floor or occluder) is hit at t < radius -> visible counts (m,).  shared: one r for all K (wrong)."""
    tris = probe.blockers()
    vis = np.zeros(len(p), np.int64)
    idx = np.arange(len(p))
    r = None
    for k in range(K):
        if r is None or not shared:
            r = sampler(rng, idx, 1, len(p))
        t = Probe.tri_hits(tris, p + bias * nf, _unit(nf + r))
        vis += ~(t < radius)
    return vis


# ---------------------------------------------------------------- statistics
def z_quantile(p):
    """the standard normal's upper quantile: P(Z > z) = p"""
    return statistics.NormalDist().inv_cdf(1.0 - p)


Z_TWO_SIDED = z_quantile(P_FALSE / 2)


def chi2_threshold(df, p=P_FALSE):
    """The chi-square quantile with upper tail probability p by Wilson and Hilferty's cube-root normal approximation:
    df (1 - 2 / (9 df) + z sqrt(2 / (9 df)))^3.  In the far upper tail it errs to the large side (a few per cent at df >= 5,
    15 % at df = 1: tests/test_draw_cpu.py holds it against scipy where scipy imports): no false alarm comes from it."""
    df = float(df)
    if df <= 0:
        return 0.0
    a = 2.0 / (9.0 * df)
    return df * max(1.0 - a + z_quantile(p) * a ** 0.5, 0.0) ** 3


def two_sample_chi2(obs, ref, min_expected=MIN_EXPECTED):
    """Two-sample chi-square of observed bin counts (N in all) against the referee's (M in all): bins whose expected count at N
    (ref N / M) is below min_expected are pooled into one bin, whatever that bin then expects; sum (sqrt(M/N) o - sqrt(N/M) r)^2
    / (o + r) over the bins, which accounts for the referee's own noise.  -> dict(chi2, df, bins (unpooled), pooled (observed,
    expected at N) or None, threshold, ok)"""
    obs, ref = np.asarray(obs, np.float64), np.asarray(ref, np.float64)
    N, M = obs.sum(), ref.sum()
    keep = ref * (N / M) >= min_expected
    o, r = list(obs[keep]), list(ref[keep])
    pooled = None
    if (~keep).any() and (obs[~keep].sum() + ref[~keep].sum()) > 0:
        o.append(obs[~keep].sum())
        r.append(ref[~keep].sum())
        pooled = (int(o[-1]), float(r[-1] * N / M))
    o, r = np.array(o), np.array(r)
    chi2 = float((((M / N) ** 0.5 * o - (N / M) ** 0.5 * r) ** 2 / (o + r)).sum())
    df = len(o) - 1
    thr = chi2_threshold(df)
    return dict(chi2=chi2, df=df, bins=int(keep.sum()), pooled=pooled, threshold=thr, ok=chi2 <= thr)


def contingency_chi2(a, b, na, nb):
    """Pearson's chi-square of independence of two class labels a, b (same length, values < na, < nb); empty rows and columns
    are left out.  -> dict(chi2, df, threshold, ok, min_expected)"""
    t = np.zeros((na, nb))
    np.add.at(t, (np.asarray(a), np.asarray(b)), 1)
    t = t[t.sum(axis=1) > 0][:, t.sum(axis=0) > 0]
    e = np.outer(t.sum(axis=1), t.sum(axis=0)) / t.sum()
    chi2 = float(((t - e) ** 2 / e).sum())
    df = (t.shape[0] - 1) * (t.shape[1] - 1)
    thr = chi2_threshold(df)
    return dict(chi2=chi2, df=df, threshold=thr, ok=chi2 <= thr, min_expected=float(e.min()))


def coarse_classes(ref_counts, nclasses=5):
    """Map the bins to classes: BLACK is class 0, the dome bins are dealt to `nclasses` classes of roughly equal expected mass
    (largest first, each to the lightest class so far).  -> (class of bin (len(ref_counts),), number of classes)"""
    ref = np.asarray(ref_counts, np.float64)
    cls = np.zeros(len(ref), np.int64)
    load = np.zeros(nclasses)
    for k in np.argsort(-ref[:NFACES]):
        c = int(load.argmin())
        cls[k] = 1 + c
        load[c] += ref[k]
    cls[BLACK] = 0
    cls[SKY:] = 0
    return cls, nclasses + 1


def z_test(obs_mean, n_obs, ref_mean, ref_var, n_ref):
    """z of an observed mean of n_obs values against the referee's mean of n_ref, the variance per value from the referee
    (no variance at all: the means must be equal)"""
    diff = obs_mean - ref_mean
    if ref_var == 0:
        z = 0.0 if diff == 0 else float("inf")
    else:
        z = diff / (ref_var * (1.0 / n_obs + 1.0 / n_ref)) ** 0.5
    return dict(z=float(z), threshold=Z_TWO_SIDED, ok=abs(z) <= Z_TWO_SIDED)


def binomial_dispersion(counts, n, p_hat, m_ref, min_var=5.0):
    """sum (c_i - n p_i)^2 / (n p_i (1 - p_i) (1 + n / m_ref)) over the cells with n p_i (1 - p_i) >= min_var, p_i estimated
    by the referee from m_ref trials per cell (the last factor is that estimate's own noise), against chi-square(cells) on
    both sides: too large when trials of a cell share a draw, too small when they are not random at all.
    -> dict(chi2, df, lo, hi, ok)"""
    c, p = np.asarray(counts, np.float64), np.asarray(p_hat, np.float64)
    var = n * p * (1 - p)
    use = var >= min_var
    chi2 = float((((c - n * p) ** 2)[use] / (var[use] * (1 + n / m_ref))).sum())
    df = int(use.sum())
    lo, hi = chi2_threshold(df, 1 - P_FALSE / 2), chi2_threshold(df, P_FALSE / 2)
    return dict(chi2=chi2, df=df, lo=lo, hi=hi, ok=df > 0 and lo <= chi2 <= hi)


# ---------------------------------------------------------------- the pixel jitter
def pixel_offsets(o4, vp12, w, h, spp):
    """Solve pixel_ray for the jitter: origin - vp.orig = vu/w (col + u) + vv/h (row + v), least squares in float64 from the
    viewport's twelve floats (orig, cam, vu, vv).  Rays in orc.primary_rays' order ([row][col][sample]).
    -> (u, v (rows * w * spp,), residual: the largest distance of an origin from the viewport plane's solution,
    margin: the error of (u, v) the float32 format allows)"""
    vp = np.asarray(vp12, np.float64)
    o = np.asarray(o4, np.float64).reshape(len(o4), -1)[:, :3]
    A = np.stack([vp[6:9] / w, vp[9:12] / h], axis=1)                     # (3, 2)
    sol, *_ = np.linalg.lstsq(A, (o - vp[0:3]).T, rcond=None)
    resid = float(np.abs(A @ sol - (o - vp[0:3]).T).max())
    n = len(o) // spp
    col = np.repeat(np.arange(n) % w, spp)
    row = np.repeat(np.arange(n) // w, spp)
    u, v = sol[0] - col, sol[1] - row
    # float32: col + u is rounded to half an ulp of max(w, h); the products and the two sums each to half an ulp of the
    # largest coordinate, which moves (u, v) by that over the pixel's size
    step = min(np.linalg.norm(A[:, 0]), np.linalg.norm(A[:, 1]))
    big = max(np.abs(o).max(), np.abs(vp[0:3]).max(), 1e-30)
    margin = 0.5 * np.spacing(F32(max(w, h))) + 4 * 0.5 * float(np.spacing(F32(big))) / step
    return u, v, resid, float(margin)


def jitter_report(u, v, w, h, spp, margin):
    """Everything the jitter must satisfy, from the recovered offsets in [row][col][sample] order -> dict of results:
    outside (offsets outside [0, 1) by more than the margin), grid (chi-square of uniformity on an 8 x 8 grid, df 63), corr (z of
    the u-v correlation: r sqrt(n) is standard normal for independent draws), twins (pairs of (pixel, sample) with the same
    offsets: all pairs within a pixel, and every sample pair of a pixel with its right and lower neighbour; "the same" = both
    within twice the margin, which two independent draws meet with probability (4 margin)^2 per pair), samples / pixels
    (contingency of the 4 x 4 cell of sample s against sample s + 1 of the pixel, and of a pixel against its right neighbour's
    same sample), all_pairs (the count of near-equal pairs over the whole frame against its Poisson limit)."""
    n = len(u)
    U, V = u.reshape(h, w, spp), v.reshape(h, w, spp)
    out = dict(outside=int(((u < -margin) | (u >= 1 + margin) | (v < -margin) | (v >= 1 + margin)).sum()))
    uc, vc = np.clip(u, 0, 1 - 1e-12), np.clip(v, 0, 1 - 1e-12)
    cells = np.bincount((uc * 8).astype(int) * 8 + (vc * 8).astype(int), minlength=64)
    chi2 = float(((cells - n / 64) ** 2 / (n / 64)).sum())
    out["grid"] = dict(chi2=chi2, df=63, threshold=chi2_threshold(63), ok=chi2 <= chi2_threshold(63))
    z = float(np.corrcoef(u, v)[0, 1] * n ** 0.5) if n > 2 and u.std() > 0 and v.std() > 0 else float("inf")
    out["corr"] = dict(z=z, threshold=Z_TWO_SIDED, ok=abs(z) <= Z_TWO_SIDED)
    twins = 0
    tol = 2 * margin

    def same(a_u, a_v, b_u, b_v):
        return int(((np.abs(a_u - b_u) <= tol) & (np.abs(a_v - b_v) <= tol)).sum())

    for s in range(spp):
        for t in range(spp):
            if s < t:
                twins += same(U[:, :, s], V[:, :, s], U[:, :, t], V[:, :, t])
            twins += same(U[:, :-1, s], V[:, :-1, s], U[:, 1:, t], V[:, 1:, t])
            twins += same(U[:-1, :, s], V[:-1, :, s], U[1:, :, t], V[1:, :, t])
    out["twins"] = twins
    # every pair of the frame, near or far (a key that wraps or strides repeats a distant pixel's draws): pairs with both offsets
    # within tol.  Independent draws give a Poisson count with mean n (n - 1) / 2 (2 tol - tol^2)^2; the count must stay below
    # that mean + z sqrt(mean) + 1 at the one-sided 1e-6 quantile (a repeated key adds whole pixels' worth of pairs)
    order = np.argsort(u, kind="stable")
    us, vs = u[order], v[order]
    pairs, k = 0, 1
    while k < n:
        close = us[k:] - us[:-k] <= tol
        if not close.any():
            break
        pairs += int((close & (np.abs(vs[k:] - vs[:-k]) <= tol)).sum())
        k += 1
    mean = n * (n - 1) / 2 * (2 * tol - tol * tol) ** 2
    limit = mean + z_quantile(P_FALSE) * mean ** 0.5 + 1
    out["all_pairs"] = dict(count=pairs, mean=float(mean), limit=float(limit), ok=pairs <= limit)
    cell = ((uc * 4).astype(int) * 4 + (vc * 4).astype(int)).reshape(h, w, spp)
    if spp > 1:
        out["samples"] = contingency_chi2(cell[:, :, :-1].reshape(-1), cell[:, :, 1:].reshape(-1), 16, 16)
    out["pixels"] = contingency_chi2(cell[:, :-1, :].reshape(-1), cell[:, 1:, :].reshape(-1), 16, 16)
    return out


JITTER_TESTS = ("grid", "corr", "samples", "pixels", "all_pairs")


def centre_origins(vp12, w, h):
    """pixel_ray's origin at one sample per pixel in its own float32 arithmetic (raytrace.rs:1379-1391 with 0.5f): (h * w, 3)"""
    vp = np.asarray(vp12, F32)
    col, row = np.tile(np.arange(w), h).astype(F32), np.repeat(np.arange(h), w).astype(F32)
    a = (vp[0:3][None] + ((vp[6:9] * (F32(1) / F32(w)))[None] * (col + F32(0.5))[:, None]).astype(F32)).astype(F32)
    return (a + ((vp[9:12] * (F32(1) / F32(h)))[None] * (row + F32(0.5))[:, None]).astype(F32)).astype(F32)


def jitter_ok(rep):
    return rep["outside"] == 0 and rep["twins"] == 0 and all(rep[k]["ok"] for k in JITTER_TESTS if k in rep)


def pixel_points(p_grid, rng, m):
    """m uniformly jittered points in every pixel's footprint on the floor, from the (h, w, 3) hits of the centre rays: the
    footprint is the centre +- half a step to the neighbours (the floor is a plane and the view one degree wide: affine to
    1e-4 of a step) -> (h * w, m, 3)"""
    h, w, _ = p_grid.shape
    du = (p_grid[:, -1] - p_grid[:, 0]).mean(axis=0) / (w - 1)
    dv = (p_grid[-1] - p_grid[0]).mean(axis=0) / (h - 1)
    a, b = rng.random((h * w, m, 1)) - 0.5, rng.random((h * w, m, 1)) - 0.5
    return p_grid.reshape(h * w, 1, 3) + a * du + b * dv


def ao_expectation(probe, p_grid, d, K_per_pixel, radius, bias, rng, sampler=random_vec, shared_k=0):
    """The visible share p_i of every pixel under rtmi_render_ao's rule, from REF_FACTOR * K_per_pixel referee rays per pixel
    at jittered points of its footprint -> (p_hat (h * w,), m_ref).  shared_k > 0: the rays come in groups of shared_k that
    share one random vector (the wrong sampler of the self-check) and the result is visible COUNTS of K_per_pixel rays."""
    h, w, _ = p_grid.shape
    nf = probe.n * -np.sign(float(d[0] @ probe.n))
    if shared_k:
        groups = K_per_pixel // shared_k
        pts = pixel_points(p_grid, rng, groups).reshape(-1, 3)
        vis = ao_visible(probe, pts, np.broadcast_to(nf, pts.shape), shared_k, radius, bias, rng, sampler, shared=True)
        return vis.reshape(h * w, groups).sum(axis=1), K_per_pixel
    m = REF_FACTOR * K_per_pixel
    pts = pixel_points(p_grid, rng, m).reshape(-1, 3)
    vis = ao_visible(probe, pts, np.broadcast_to(nf, pts.shape), 1, radius, bias, rng, sampler)
    return vis.reshape(h * w, m).mean(axis=1), m


def ao_report(counts, n, p_hat, m_ref):
    """counts: visible rays per pixel of n each.  total: z of the frame total against sum n p_i (variance sum n p (1 - p), plus
    the referee's own share n / m_ref of it); dispersion: binomial_dispersion."""
    c, p = np.asarray(counts, np.float64), np.asarray(p_hat, np.float64)
    var = (n * p * (1 - p)).sum() * (1 + n / m_ref)
    z = float((c.sum() - n * p.sum()) / var ** 0.5) if var > 0 else (0.0 if c.sum() == n * p.sum() else float("inf"))
    return dict(total=dict(z=z, threshold=Z_TWO_SIDED, ok=abs(z) <= Z_TWO_SIDED, share=float(c.sum() / (n * len(c))),
                           expected=float(p.mean())), dispersion=binomial_dispersion(c, n, p, m_ref))


def ao_counts(ao_img, n):
    """the integer visible counts behind an AO (or shadow) plane: value = count * (1 / n) in float32, exact to rounding"""
    c = np.asarray(ao_img, np.float64).reshape(-1) * n
    assert np.abs(c - np.rint(c)).max() < 1e-3, "a plane value is no multiple of 1 / (samples * rays)"
    return np.rint(c).astype(np.int64)


# ---------------------------------------------------------------- the direct light (include/rtmi.h, rtmi_render_light)
def light_samples(probe, pts, nf, K, orig, len2, bias, rng, unbounded=False):
    """rtmi_render_light's rule at points pts (m, 3) with unit face normal nf (3,): K samples adj = orig + U len2 (U uniform in
    the unit cube), dir = unit(adj - point), c = nf . dir, culled unless c > 0, the shadow ray from point + nf bias (u_3 + 1)
    visible unless something is hit at t < |adj - point| (unbounded: at any t).
    -> (live (m, K) bool, visible (m, K) bool, c (m, K), adj (m, K, 3))"""
    m = len(pts)
    tris = probe.blockers()
    live, vis, cc = np.zeros((m, K), bool), np.zeros((m, K), bool), np.zeros((m, K))
    adj_all = np.zeros((m, K, 3))
    for k in range(K):
        u = rng.random((m, 4))
        adj = np.asarray(orig, np.float64)[None, :] + u[:, :3] * len2
        v = adj - pts
        r = np.linalg.norm(v, axis=1)
        with np.errstate(all="ignore"):
            dirs = v / r[:, None]
        c = dirs @ nf
        o = pts + nf[None, :] * (bias * (u[:, 3:4] + 1.0))
        t = Probe.tri_hits(tris, o, np.where(np.isfinite(dirs), dirs, 0.0))
        lv = c > 0
        live[:, k], cc[:, k], adj_all[:, k] = lv, c, adj
        vis[:, k] = lv & ~(t < (np.inf if unbounded else r))
    return live, vis, cc, adj_all


def light_expectation(probe, p_grid, d, n, orig, len2, bias, rng, unbounded=False):
    """Per pixel, from m_ref = REF_FACTOR * n referee samples at jittered points of its footprint: the visible share, the live
    share, the mean and variance of the irradiance term (c where visible, else 0) -> dict of (h * w,) arrays and m_ref"""
    h, w, _ = p_grid.shape
    nf = probe.n * -np.sign(float(d[0] @ probe.n))
    m = REF_FACTOR * n
    pts = pixel_points(p_grid, rng, m).reshape(-1, 3)
    live, vis, c, _ = light_samples(probe, pts, nf, 1, orig, len2, bias, rng, unbounded)
    e = np.where(vis, c, 0.0).reshape(h * w, m)
    return dict(visible=vis.reshape(h * w, m).mean(axis=1), live=live.reshape(h * w, m).mean(axis=1), irr_mean=e.mean(axis=1),
                irr_var=e.var(axis=1), m_ref=m)


def share_z(total, n_each, p_hat, m_ref):
    """z of a count total over cells of n_each Bernoulli trials against the referee's shares p_hat (m_ref trials per cell)"""
    p = np.asarray(p_hat, np.float64)
    var = (n_each * p * (1 - p)).sum() * (1 + n_each / m_ref)
    exp = n_each * p.sum()
    z = float((total - exp) / var ** 0.5) if var > 0 else (0.0 if total == exp else float("inf"))
    return dict(z=z, threshold=Z_TWO_SIDED, ok=abs(z) <= Z_TWO_SIDED, observed=float(total), expected=float(exp))


def mean_z(values, n_each, mean_hat, var_hat, m_ref):
    """z of the frame mean of per-pixel means (each over n_each terms) against the referee's per-pixel mean and variance"""
    mu, var = np.asarray(mean_hat, np.float64), np.asarray(var_hat, np.float64)
    v = (var / n_each + var / m_ref).sum()
    diff = float(np.asarray(values, np.float64).sum() - mu.sum())
    z = diff / v ** 0.5 if v > 0 else (0.0 if diff == 0 else float("inf"))
    return dict(z=float(z), threshold=Z_TWO_SIDED, ok=abs(z) <= Z_TWO_SIDED, observed=float(np.mean(values)), expected=float(mu.mean()))
