"""Deterministic adversarial inputs for the octree builder's overlap test (box_contains_polygon, raytrace.rs:753-779) and
for make_triangle (raytrace.rs:340-383).  A plain module (not a conftest), NumPy only, fixed seeds; shared by
test_builder_cases_cpu.py (oracle <-> host mirror) and test_gpu_builder.py (oracle <-> k_box_contains / k_make_triangles).

pair_family(name) -> dict(boxes (nb,4) f32 [centre, half edge], box_kind (nb,) 0 builder / 1 round, tris (n,3,3) f32,
pair_box (n,), tag (n,) str): pair i tests triangle i against box pair_box[i].  realise(name) passes the corners through
the oracle's add_triangle (rejected ones are dropped) and returns the oracle scene, its records and its answers."""
import functools
import itertools

import numpy as np

F = np.float32
FAMILIES = ("A", "B", "C", "D", "E", "F")
_SEED = {"A": 11, "B": 12, "C": 13, "D": 14, "E": 15, "F": 16}


# ---------------------------------------------------------------- f32 arithmetic in the oracle's operation order
def _v4(p):
    p = np.asarray(p, F)
    return np.concatenate([p, np.zeros(p.shape[:-1] + (1,), F)], -1)


def _rsum(p):  # ordered reduce_sum seeded with +0 (rt_oracle.cpp reduce_sum)
    return (((F(0) + p[..., 0]) + p[..., 1]) + p[..., 2]) + p[..., 3]


def _dot(a, b):
    return _rsum(a * b)


def _unit(a):
    return a * (F(1) / np.sqrt(_dot(a, a)))[..., None]


def median_solve_f32(pts):
    """The centroid computation of make_triangle restated in f32 NumPy, in the oracle's operation order (rt_oracle.cpp
    ray_intersect_helper / ray_intersect / make_triangle): pts (n,3,3) -> dict(det (n,3): the determinant of coordinate pairs
    (0,1), (0,2), (1,2); pair (n,): the pair used, 3 = none; dist2 (n,): |p2 - p1|^2; ok (n,); incenter (n,3))."""
    pts = np.asarray(pts, F).reshape(-1, 3, 3)
    with np.errstate(all="ignore"):
        a, b, c = _v4(pts[:, 0]), _v4(pts[:, 1]), _v4(pts[:, 2])
        ab, ac, bc = b - a, c - a, c - b
        sd = _unit(ac + ab)
        rd = _unit(bc + ab * F(-1))
        n = len(pts)
        det = np.zeros((n, 3), F)
        t1 = np.zeros(n, F)
        t2 = np.zeros(n, F)
        pair = np.full(n, 3)
        for q, (i, j) in reversed(list(enumerate(((0, 1), (0, 2), (1, 2))))):
            d = rd[:, i] * sd[:, j] - rd[:, j] * sd[:, i]
            dx = b[:, i] - a[:, i]
            dy = b[:, j] - a[:, j]
            good = ~(np.abs(d) < F(0.0001))
            t1 = np.where(good, (dy * rd[:, i] - dx * rd[:, j]) / d, t1)
            t2 = np.where(good, (dy * sd[:, i] - dx * sd[:, j]) / d, t2)
            pair = np.where(good, q, pair)
            det[:, q] = d
        p1 = sd * t1[:, None] + a
        p2 = rd * t2[:, None] + b
        e = p2 - p1
        dist2 = _dot(e, e)
        ok = (pair < 3) & (dist2 < F(0.01))
    return dict(det=det, pair=pair, dist2=dist2, ok=ok, incenter=p1[:, :3])


def face_first_pass_tmin(box, axis, norm, incenter):
    """tmin of the first slab pass of face_contains_triangle (raytrace.rs:645-685) in f32 NumPy, the oracle's operation
    order: box (4,), axis 0..5 = +x -x +y -y +z -z, norm / incenter (n,3) from the oracle's records -> (n,) f32."""
    with np.errstate(all="ignore"):
        p = _v4(np.asarray(box[:3], F))
        L = F(box[3])
        n1 = np.zeros(4, F)
        n1[axis >> 1] = F(-1) if axis & 1 else F(1)
        n2, inc = _v4(norm), _v4(incenter)
        h1 = _dot(n1, p + n1 * L)
        h2 = _dot(n2, inc)
        nn = _dot(n1[None, :], n2)
        c1 = (h1 - h2 * nn) / (F(1) - nn * nn)
        c2 = (h2 - h1 * nn) / (F(1) - nn * nn)
        orig = n1[None, :] * c1[:, None] + n2 * c2[:, None]
        n1b = np.broadcast_to(n1, n2.shape)
        s1, s2 = n1b[:, [1, 2, 0, 3]], n1b[:, [2, 0, 1, 3]]
        o1, o2 = n2[:, [1, 2, 0, 3]], n2[:, [2, 0, 1, 3]]
        du = _unit(s1 * o2 - s2 * o1)
        inv = F(1) / du
        tmin = np.full(len(n2), np.finfo(F).max, F)
        for k in range(3):
            if k == axis >> 1:
                continue
            t1 = (p[k] - L - orig[:, k]) * inv[:, k]
            t2 = (p[k] + L - orig[:, k]) * inv[:, k]
            tmin = np.fmin(tmin, np.fmin(t1, t2))
    return tmin


def points_inside(box, pts):
    """box_contains_point with the same strict `<` on f32 |p - c| (raytrace.rs:636-643): pts (..., 3) -> (...)."""
    d = np.abs(np.asarray(pts, F) - np.asarray(box[:3], F))
    return (d < F(box[3])).all(-1)


# ---------------------------------------------------------------- boxes
def builder_boxes(rng, per_depth=2):
    """Boxes as the builder makes them: root (0, 0, 20.1), L = 20, descended by c +- L/2 in f32 (raytrace.rs:820-833)."""
    out = []
    for depth in range(11):
        for _ in range(per_depth):
            c, L = np.array([0.0, 0.0, 20.1], F), F(20.0)
            for _ in range(depth):
                L = F(L / F(2))
                sg = (rng.integers(0, 2, 3) * 2 - 1).astype(F)
                c = (c + sg * L).astype(F)
            out.append(np.array([c[0], c[1], c[2], L], F))
    return out


def round_boxes():
    """Power-of-two half edges; centres at 0 and offset by about 1e3 so that p - c cancels."""
    out = []
    for L in (2.0 ** -10, 1.0, 2.0 ** 10):
        out.append(np.array([0.0, 0.0, 0.0, L], F))
        out.append(np.array([1000.25, -999.5, 1001.125, L], F))
    return out


def _basis(rng):
    n = rng.normal(size=3)
    n /= np.linalg.norm(n)
    e1 = np.cross(n, [1.0, 0.0, 0.0] if abs(n[0]) < 0.9 else [0.0, 1.0, 0.0])
    e1 /= np.linalg.norm(e1)
    return e1, np.cross(n, e1), n


def _steps(x, away_sign):
    """x (f32), one f32 step towards -away_sign, one step towards +away_sign."""
    x = F(x)
    return x, np.nextafter(x, F(-away_sign * np.inf)), np.nextafter(x, F(away_sign * np.inf))


def _boundary_coord(ck, L, s):
    """An f32 p with |p - ck| == L exactly in f32 on side s (the nearest to ck + s*L if none is exact)."""
    p0 = F(F(ck) + F(s) * F(L))
    cand = [p0]
    lo = hi = p0
    for _ in range(3):
        lo, hi = np.nextafter(lo, F(-np.inf)), np.nextafter(hi, F(np.inf))
        cand += [lo, hi]
    for p in cand:
        if np.abs(F(p - F(ck))) == F(L):
            return p
    return p0


# ---------------------------------------------------------------- pair families (one box -> triangles + tags)
def _fam_A(rng, box):
    c, L = box[:3].astype(np.float64), float(box[3])
    tris, tags = [], []
    for ratio in (1 / 64, 1 / 4, 1.0, 4.0, 64.0):
        for _ in range(36):
            centre = c + rng.uniform(-1.2, 1.2, 3) * L * (1.0 + ratio)
            tris.append(centre + rng.normal(scale=ratio * L, size=(3, 3)))
            tags.append(f"ratio{ratio:g}")
    return tris, tags


def _fam_B(rng, box):
    c, L = box[:3], box[3]
    tris, tags = [], []
    j = rng.uniform(-0.05, 0.05, 4)
    foot = {"inside": [(-0.5 + j[0], -0.5), (0.4, -0.5), (-0.5 + j[0], 0.3 + j[1])],       # right angle, legs along the axes
            "overlap": [(0.5, 0.5 + j[2]), (2.0, 0.5 + j[2]), (0.5, 2.5)],
            "straddle": [(-1.7, -0.3 + j[3]), (1.9, -0.6), (0.2, 1.8)],                   # crosses the square, no corner in it
            "skew": [(-0.83 + j[0], -0.41), (1.37, 0.29 + j[1]), (0.11 + j[2], 1.63)],      # no right angle: the unit normal
            "disjoint": [(1.5, 1.5), (3.0, 1.5), (1.5, 2.5 + j[1])]}                     # computed for it may miss +-1 by an ulp
    for k in range(3):
        u, v = (k + 1) % 3, (k + 2) % 3
        for s in (1, -1):
            face = F(c[k] + F(s) * L)
            on, inn, out = _steps(face, s)
            planes = {"interior": F(c[k] + F(s * 0.375) * L), "on": on, "in": inn, "out": out, "far": F(c[k] + F(s * 3.0) * L)}
            for pname, w in planes.items():
                for fname, f in foot.items():
                    for winding in (0, 1):
                        t = np.zeros((3, 3), F)
                        for i, (a, b) in enumerate(f if winding == 0 else f[::-1]):
                            t[i, k] = w
                            t[i, u] = F(c[u] + F(a) * L)
                            t[i, v] = F(c[v] + F(b) * L)
                        tris.append(t)
                        tags.append(f"{pname}/{fname}")
    return tris, tags


def _fam_C(rng, box):
    c, L = box[:3].astype(np.float64), float(box[3])
    tris, tags = [], []

    def big(point, e1, e2, R, shift):
        th = np.array([0.0, 2.1, 4.2]) + rng.uniform(-0.3, 0.3, 3) + rng.uniform(0, 6.28)
        sh = shift * np.array([np.cos(th[0] + 1.0), np.sin(th[0] + 1.0)])
        return np.array([point + e1 * (R * np.cos(a) + sh[0]) + e2 * (R * np.sin(a) + sh[1]) for a in th])

    for _ in range(40):                                              # pierces the middle of the box
        e1, e2, _n = _basis(rng)
        R = L * rng.choice([24.0, 64.0, 200.0])
        tris.append(big(c + rng.uniform(-0.3, 0.3, 3) * L, e1, e2, R, 0.25 * R))
        tags.append("pierce")
    for sg in itertools.product((-1.0, 1.0), repeat=3):              # grazes past a box corner, either side
        q = c + np.array(sg) * L
        for side in (-1.0, 1.0):
            for _ in range(4):
                m = np.array(sg) * rng.uniform(0.35, 1.0, 3)
                m /= np.linalg.norm(m)
                e1 = np.cross(m, [1.0, 0.0, 0.0])
                e1 /= np.linalg.norm(e1)
                e2 = np.cross(m, e1)
                R = L * rng.choice([24.0, 64.0])
                tris.append(big(q + m * side * L * 2.0 ** -10, e1, e2, R, 0.2 * R))
                tags.append("graze_out" if side > 0 else "graze_in")
    for k in range(3):                                               # parallel to a face at distance L/2
        e1, e2 = np.eye(3)[(k + 1) % 3], np.eye(3)[(k + 2) % 3]
        for s in (-1.0, 1.0):
            for where, d in (("par_in", 0.5), ("par_out", 1.5)):
                for _ in range(3):
                    pt = c + rng.uniform(-0.2, 0.2, 3) * L
                    pt[k] = c[k] + s * d * L
                    R = L * rng.choice([24.0, 64.0])
                    tris.append(big(pt, e1, e2, R, 0.25 * R))
                    tags.append(where)
    return tris, tags


def _fam_D(rng, box):
    c, L = box[:3], box[3]
    c64, L64 = c.astype(np.float64), float(L)
    tris, tags = [], []
    subsets = [s for r in (1, 2, 3) for s in itertools.combinations(range(3), r)]
    for S in subsets:
        for place in ("on", "in", "out"):
            for rep in range(4):
                sg = rng.integers(0, 2, 3) * 2 - 1
                p = (c64 + rng.uniform(-0.7, 0.7, 3) * L64).astype(F)
                for k in S:
                    on, inn, out = _steps(_boundary_coord(c[k], L, sg[k]), sg[k])
                    p[k] = {"on": on, "in": inn, "out": out}[place]
                # a corner on the boundary, the other two further out
                t = np.zeros((3, 3), F)
                t[0] = p
                for i in (1, 2):
                    o = rng.uniform(-1.0, 1.0, 3) * L64
                    for k in S:
                        o[k] = sg[k] * rng.uniform(1.0, 3.0) * L64
                    t[i] = (p.astype(np.float64) + o).astype(F)
                tris.append(np.roll(t, rep % 3, axis=0))
                tags.append(f"corner{len(S)}/{place}")
                # the centroid ("incenter") on the boundary, every corner at 4 L or more from it: all outside the box
                e1, e2, _n = _basis(rng)
                R = rng.uniform(4.0, 6.0) * L64
                th = rng.uniform(0, 6.28)
                d1 = R * (np.cos(th) * e1 + np.sin(th) * e2)
                d2 = R * (np.cos(th + 2.0) * e1 + np.sin(th + 2.0) * e2)
                t = (p.astype(np.float64) + np.array([d1, d2, -(d1 + d2)])).astype(F)
                for _ in range(8):                                   # walk the f32 centroid onto the target coordinate
                    q = median_solve_f32(t[None])["incenter"][0]
                    if not np.isfinite(q).all() or all(q[k] == p[k] for k in S):
                        break
                    for k in S:
                        t[:, k] = t[:, k] + F(p[k] - q[k])
                tris.append(t)
                tags.append(f"incenter{len(S)}/{place}")
    return tris, tags


def _fam_E(rng, box):
    c, L = box[:3], box[3]
    c64, L64 = c.astype(np.float64), float(L)
    tris, tags = [], []
    for k in range(3):
        u, v = (k + 1) % 3, (k + 2) % 3
        for s in (1, -1):
            face = F(c[k] + F(s) * L)
            # one edge exactly in the face plane; the third corner beyond the face, or through the box to the far side
            for spanu, third in itertools.product(((-0.6, 0.5), (-2.0, 2.5)), (1.5, -2.5)):
                t = np.zeros((3, 3), F)
                vv = rng.uniform(-0.8, 0.8)
                for i, a in enumerate(spanu):
                    t[i, k], t[i, u], t[i, v] = face, F(c64[u] + a * L64), F(c64[v] + vv * L64)
                t[2] = (c64 + rng.uniform(-0.5, 0.5, 3) * L64).astype(F)
                t[2, k] = F(c64[k] + s * (1.0 + third if third > 0 else third) * L64)
                tris.append(t)
                tags.append("edge_in_face")
    for k in range(3):                                                # the box's 12 edges: direction k, at (su, sv)
        u, v = (k + 1) % 3, (k + 2) % 3
        for su, sv in itertools.product((1, -1), repeat=2):
            eu, ev = F(c[u] + F(su) * L), F(c[v] + F(sv) * L)
            for span in ((-0.5, 0.7), (-2.0, 2.0)):                   # a triangle edge along the box edge
                t = np.zeros((3, 3), F)
                for i, a in enumerate(span):
                    t[i, k], t[i, u], t[i, v] = F(c64[k] + a * L64), eu, ev
                t[2, k] = F(c64[k] + rng.uniform(-0.5, 0.5) * L64)
                t[2, u] = F(c64[u] + su * rng.uniform(1.5, 3.0) * L64)
                t[2, v] = F(c64[v] + sv * rng.uniform(1.5, 3.0) * L64)
                tris.append(t)
                tags.append("edge_on_box_edge")
            for phi in (0.25 * np.pi, 0.75 * np.pi, rng.uniform(0.05, 3.1)):   # the triangle's plane contains the box edge
                w = np.zeros(3)
                w[u], w[v] = su * np.cos(phi), -sv * np.sin(phi)       # phi in (0, pi/2): tangent outside; beyond: cuts in
                ek = np.eye(3)[k]
                base = np.zeros(3)
                base[k], base[u], base[v] = c64[k], float(eu), float(ev)
                t = np.array([base + ek * (-3.0 * L64) + w * (-2.5 * L64), base + ek * (3.5 * L64) + w * (-2.0 * L64),
                              base + ek * (0.3 * L64) + w * (4.0 * L64)])
                tris.append(t.astype(F))
                tags.append("plane_has_box_edge")
    # the face/plane intersection line starts on a slab plane (first-pass tmin == 0) and heads into the face's square
    for k in range(3):
        for s in (1, -1):
            P = float(F(c[k] + F(s) * L))
            for u, v in (((k + 1) % 3, (k + 2) % 3), ((k + 2) % 3, (k + 1) % 3)):
                for su, sv, sd in itertools.product((1, -1), repeat=3):
                    u0 = float(F(c[u] + F(su) * L))
                    v0 = c64[v] + sv * rng.uniform(1.3, 2.5) * L64
                    foot = np.zeros(3)
                    foot[k], foot[u], foot[v] = P, u0, v0
                    d = np.zeros(3)
                    d[u], d[v] = -v0 * sd, u0 * sd
                    if np.linalg.norm(d) == 0 or not (d[u] * (c64[u] - u0) > 0 and d[v] * (c64[v] - v0) > 0):
                        continue
                    d /= np.linalg.norm(d)
                    m = foot.copy()
                    m[k] = 0.0
                    m /= np.linalg.norm(m)
                    for phi in (0.5 * np.pi, rng.uniform(1.1, 2.0)):
                        n2 = np.cos(phi) * np.eye(3)[k] + np.sin(phi) * m
                        # foot lies in span(face normal, n2) and is orthogonal to d: it is the line's point nearest the
                        # origin, which is where face_contains_triangle starts the line
                        w = np.cross(n2, d)
                        t = np.array([foot + d * (0.5 * L64) + w * (3.0 * L64), foot + d * (3.0 * L64) - w * (3.5 * L64),
                                      foot - d * (1.0 * L64) - w * (3.0 * L64)])
                        tris.append(t.astype(F))
                        tags.append("tmin0")
    return tris, tags


def _needle(rng, centre, length, aspect):
    e1, e2, _n = _basis(rng)
    h = length / aspect
    x = rng.choice([0.0, 0.5, 1.0]) * length + rng.uniform(-0.5, 0.5) * h     # needle (apex over an end) or sliver
    return centre + np.array([-0.5 * length * e1, 0.5 * length * e1, (x - 0.5 * length) * e1 + h * e2])


def aspect_ratio(tris):
    """Longest edge over the height on it, of f32 corners (n,3,3), in f64."""
    c = np.asarray(tris, F).astype(np.float64)
    e = np.linalg.norm(c - np.roll(c, 1, axis=1), axis=2)
    area = np.linalg.norm(np.cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0]), axis=1) / 2
    with np.errstate(all="ignore"):
        return e.max(1) ** 2 / (2 * area)


def _fam_F(rng, box):
    c, L = box[:3].astype(np.float64), float(box[3])
    tris, tags = [], []
    for _ in range(150):
        aspect = 10.0 ** rng.uniform(3.0, 5.0)
        t = _needle(rng, c + rng.uniform(-1.5, 1.5, 3) * L, rng.uniform(0.5, 4.0) * L, aspect).astype(F)
        if aspect_ratio(t[None])[0] >= 1e3:                  # still a needle after rounding to f32 (not so where ulp(c) > height)
            tris.append(t)
            tags.append("needle")
    return tris, tags


_GEN = {"A": _fam_A, "B": _fam_B, "C": _fam_C, "D": _fam_D, "E": _fam_E, "F": _fam_F}


@functools.lru_cache(maxsize=None)
def pair_family(name):
    rng = np.random.default_rng(_SEED[name])
    bb = builder_boxes(rng)
    boxes = bb + round_boxes()
    kind = np.array([0] * len(bb) + [1] * (len(boxes) - len(bb)))
    tris, pair_box, tags = [], [], []
    for b, box in enumerate(boxes):
        with np.errstate(all="ignore"):
            t, g = _GEN[name](rng, box)
        tris += [np.asarray(x, np.float64).astype(F) for x in t]
        pair_box += [b] * len(t)
        tags += g
    return dict(name=name, boxes=np.array(boxes, F), box_kind=kind, tris=np.array(tris, F).reshape(-1, 3, 3),
                pair_box=np.array(pair_box), tag=np.array(tags))


class Realised:
    """A family after the oracle's add_triangle: scene (oracle, triangle 0 = the dummy), rec (n+1, 29) its records,
    tri (m,) scene index of pair j, box (m,) box index, tag (m,), answer (m,) the oracle's box_contains_polygon."""


@functools.lru_cache(maxsize=None)
def realise(name):
    from oracle import orc
    fam = pair_family(name)
    s = orc.Scene(with_dummy=True)
    surf = orc.Surface(orc.SOLID, orc.make_color(10, 20, 30))
    keep = np.zeros(len(fam["tris"]), bool)
    with np.errstate(all="ignore"):
        finite = np.isfinite(fam["tris"]).all((1, 2))
    for i, t in enumerate(fam["tris"]):
        if not finite[i]:
            continue
        try:
            s.add_triangle(t, surf, 0.0)
            keep[i] = True
        except RuntimeError:
            pass
    r = Realised()
    r.name, r.fam, r.scene, r.accepted = name, fam, s, keep
    r.rec = s.triangles()[0]
    r.tri = np.arange(1, int(keep.sum()) + 1)
    r.box = fam["pair_box"][keep]
    r.tag = fam["tag"][keep]
    r.boxes, r.box_kind = fam["boxes"], fam["box_kind"]
    r.answer = np.array([s.box_contains_polygon(r.boxes[b, :3], float(r.boxes[b, 3]), int(t)) for b, t in zip(r.box, r.tri)], bool)
    return r


def tris15(rec):
    """The 15-float records of rtmi_builder_create from the oracle's 29-float records (incenter, norm, corners)."""
    return np.ascontiguousarray(np.concatenate([rec[:, 0:6], rec[:, 20:29]], 1), F)


def split_plane_scene():
    """Corners for a scene of families B and D placed around the builder's own split planes: the boxes are the root
    (0, 0, 20.1; 20) and its descendants, so face planes of one box are split planes of its parent."""
    rng = np.random.default_rng(21)
    tris = []
    for box in builder_boxes(rng, per_depth=1)[:5]:
        for gen in (_fam_B, _fam_D):
            t, tags = gen(rng, box)
            tris += [np.asarray(x, F) for x, g in zip(t, tags) if not g.startswith(("far", "interior/disjoint"))][::7]
    return np.array(tris, F).reshape(-1, 3, 3)


# ---------------------------------------------------------------- random soup scenes (test_random_triangle_soups)
def soup(seed):
    """The scene of test_random_triangle_soups: returns (rng, ntri, (maxdepth, minobjs), add) where add(api) makes the scene
    with either API (conftest OracleApi / ProductApi) without a tree, and rng is left where the camera draws continue."""
    rng = np.random.default_rng(1000 + seed)
    ntri = int(rng.integers(40, 400))
    centre = rng.uniform(-3, 3, (ntri, 3)) + np.array([0, 0, 8.0])
    pts = (centre[:, None, :] + rng.normal(scale=rng.uniform(0.2, 1.2), size=(ntri, 3, 3))).astype(np.float32)
    kinds = rng.integers(0, 3, ntri)
    cols = rng.integers(0, 256, (ntri, 3))
    alphas = rng.uniform(0.05, 0.95, ntri)
    scat = rng.uniform(0.0, 0.3, ntri)
    edges = rng.choice([0.0, 0.05, 0.3, -1.0], ntri)
    maxdepth, minobjs = int(rng.integers(2, 9)), int(rng.integers(2, 24))

    def add(api):
        s = api.scene()
        for i in range(ntri):
            c = tuple(int(x) for x in cols[i])
            surf = (api.solid(c), api.matte(c, float(alphas[i])), api.reflective(float(scat[i]), c, float(alphas[i])))[kinds[i]]
            try:
                api.add_triangle(s, pts[i], surf, float(edges[i]))
            except RuntimeError:
                pass  # degenerate triangle: rejected identically by both implementations
        s.populate_triangle_numbers()
        return s
    return rng, ntri, (maxdepth, minobjs), add


SOUP_ROOT = ([0.0, 0.0, 8.0], 8.0)


# ---------------------------------------------------------------- corner sets for make_triangle
@functools.lru_cache(maxsize=None)
def corner_sets():
    """name -> (n,3,3) f32 corners, unfiltered (rejected triangles included)."""
    rng = np.random.default_rng(31)
    out = {}
    soup_pts = []
    for scale in (1e-3, 1.0, 1e3):
        centre = rng.uniform(-3, 3, (400, 1, 3)) * scale
        soup_pts.append(centre + rng.normal(scale=scale * rng.uniform(0.2, 1.5, (400, 1, 1)), size=(400, 3, 3)))
    mixed = rng.uniform(-3, 3, (300, 1, 3)) * 1e3 + rng.normal(size=(300, 3, 3)) * 10.0 ** rng.uniform(-3, 0, (300, 1, 1))
    out["soup"] = np.concatenate(soup_pts + [mixed]).astype(F)
    ax = []
    for k in range(3):                                       # right angle at corner 0, legs along the two in-plane axes
        u, v = (k + 1) % 3, (k + 2) % 3
        for _ in range(120):
            t = np.zeros((3, 3))
            p = rng.uniform(-4, 4, 3) * 10.0 ** rng.integers(-1, 3)
            lu, lv = rng.uniform(0.1, 3.0, 2) * rng.choice([-1.0, 1.0], 2) * 10.0 ** rng.integers(-2, 2)
            t[:] = p
            t[1, u] += lu
            t[2, v] += lv
            ax.append(np.roll(t, rng.integers(0, 3), axis=0))
    out["axis"] = np.array(ax).astype(F)
    nd = []
    for _ in range(1200):                                    # the median determinant is about 3 h / length
        length = 10.0 ** rng.uniform(-1, 1)
        nd.append(_needle(rng, rng.uniform(-2, 2, 3), length, 3.0 / (1e-4 * 10.0 ** rng.uniform(-0.7, 0.7))))
    out["needle_det"] = np.array(nd).astype(F)
    nr = []
    for _ in range(24000):                                   # ill-conditioned medians far from the origin: |p2 - p1| ~ 0.1
        length = 10.0 ** rng.uniform(2, 3.5)
        centre = rng.normal(size=3) * 10.0 ** rng.uniform(4, 6.5)
        nr.append(_needle(rng, centre, length, 3.0 / (1e-4 * 10.0 ** rng.uniform(0.05, 1.0))))
    nr = np.array(nr).astype(F)
    m = median_solve_f32(nr)
    with np.errstate(all="ignore"):
        near = (m["pair"] < 3) & (m["dist2"] > F(0.0005)) & (m["dist2"] < F(0.2))
    out["near_reject"] = nr[near][:800]
    z = np.zeros((3, 3))
    p = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 1.0], [0.0, 1.0, 1.0]])
    out["degenerate"] = np.array([z, [p[0], p[0], p[1]], [p[0], p[1], p[1]], [p[0], p[1], p[0]], [p[0], p[0], p[0]],
                                  [p[0], p[1], 2 * p[1] - p[0]], [[1, 2, 3], [2, 4, 6], [4, 8, 12]], p,
                                  [[-1, -1, -1], [0, 0, 0], [1, 1, 1]], p + 5.0], np.float64).astype(F)
    return out


def all_corners():
    cs = corner_sets()
    names = sorted(cs)
    return np.concatenate([cs[n] for n in names]), np.concatenate([[n] * len(cs[n]) for n in names])


@functools.lru_cache(maxsize=None)
def oracle_make_triangles(edge=0.0):
    """Every corner set through the oracle's add_triangle: (accepted mask over all_corners(), records (n_acc, 29))."""
    from oracle import orc
    pts, _ = all_corners()
    s = orc.Scene(with_dummy=False)
    surf = orc.Surface(orc.SOLID, orc.make_color(10, 20, 30))
    acc = np.zeros(len(pts), bool)
    for i, t in enumerate(pts):
        try:
            s.add_triangle(t, surf, edge)
            acc[i] = True
        except RuntimeError:
            pass
    return acc, s.triangles()[0]
