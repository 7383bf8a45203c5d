"""A float64 geometric referee for closest hits, faces, the edge band, leaf completeness and the deterministic (mirror) shading
chain.  Plain NumPy, written from textbook geometry: it imports nothing of oracle/ and reads nothing of a triangle record but
the nine corner floats, the edge thickness and the surface.  It answers "is this the nearest triangle the ray really crosses?"
for the rays where float32 and float64 cannot disagree (the DECIDED rays) and says which rays those are; every comparison
leaves the others out, and every test caps their share first.  DESIGN.md section 2 (vi) records what this pins and what not.

What the reference does that a naive referee gets wrong (each named here because the comparison depends on it):
  * its "incenter" is the centroid (bac_bisect = ac + ab is a median, raytrace.rs:340-357), and each edge has its own
    side_len = the centroid's distance to that edge: the edge band of edge i is `distance to edge i < thickness * h_i`,
    h_i = 2 area / (3 |edge i|);
  * triangle 0 (the dummy) has corners like any other; a ray whose nearest crossing is triangle 0 is left undecided;
  * at grazing incidence the float32 hit point slides along the plane by (position error) / |n.d|, so every margin
    below is divided by |n.d| (unit normal, unit direction);
  * the t >= 0 test is made on a float32 quotient: a plane the origin lies on (within EPS_0) can go either way;
  * an octree holds only what its root box holds: a nearest crossing outside the root box (or within the margin of one of
    its faces) is undecided for a tree and decided for a list (root_box=None);
  * a ray exactly parallel to some triangle's plane (n.d == 0) is undecided: the reference's lane-3 NaN rule accepts such
    "hits" (exactness rules).

A plain helper module of tests/test_geom_cpu.py (oracle against referee) and tests/test_geom.py (device against referee)."""
import collections
import functools

import numpy as np

F32 = np.float32
# include/rtmi.h, rtmi_trace: "face (0 front, 1 back, 2 edge front, 3 edge back)"
FRONT, BACK, EDGE_FRONT, EDGE_BACK = 0, 1, 2, 3
SKY = np.array([128.0, 180.0, 255.0]) / 255.0          # raytrace.rs:1264
SOLID, MATTE, REFLECTIVE = 0, 1, 2

# ---------------------------------------------------------------- decision margins
# None of these comes from a device's output.  They are sized from the float32 format and the coordinate range of the test
# inputs (|coordinate| <= 41: the canonical root box reaches z = 40.1; the soups and the mirror set stay below 16), and
# tests/test_geom_cpu.py measures on the CPU oracle that they are wide enough (its table is in DESIGN.md section 2 (vi)).
#   EPS_P  in-plane slide of a float32 hit point at normal incidence: ulp(16) = 1.9e-6, about five roundings -> 1e-5
#   EPS_M  the same relative to a triangle's size (sqrt(area)); the issue's figure
#   EPS_T  relative error of a float32 hit time apart from the plane-distance term below (measured: 3.8e-5 at most)
#   EPS_0  absolute error of the float32 plane distance n.(c - o): ulp(41) * 5 = 2e-5; bounce origins sit 1e-3 off a surface
#   TINY   floor of |n.d| in the divisions
EPS_M, EPS_P, EPS_T, EPS_0, TINY = 1e-4, 1e-5, 1e-4, 2e-5, 1e-9
BOX_MARGIN = 1e-4    # leaf completeness: an overlap deeper than this must be listed, one within +-this is skipped (and counted)

# Tolerances of the comparisons, each = 4 x the largest oracle-versus-referee value measured on decided rays by
# tests/test_geom_cpu.py on 2026-10-19 (the hardware kernels are bit-equal to the oracle; the factor guards input changes):
#   plane residual |n.(o + t d - a)| / max(1, |o|, |p|) (unit n, infinity norms): measured 1.15e-05 x 4
#   (soup 1, a sliver whose float32 normal is that far off its corners' plane; 1.55e-07 on the canonical scene)
POS_TOL = 4.6e-5
#   colour, largest absolute difference on decided chains of the mirror set (maxdepth 0, 1, 2, 6): measured 7.1e-08 x 4
COL_TOL = 2.9e-7
#   guide normal: the record's float32 norm (unit(sides[0] x sides[1]), several roundings deep) against the float64 unit normal on
#   the mirror set, largest lane difference: measured 2.15e-06 x 4
NRM_TOL = 8.6e-6

Hits = collections.namedtuple("Hits", "tri t face decided why terr")
# why: bit 0 grazed margin, 1 runner-up, 2 edge band, 3 origin on a plane, 4 triangle 0, 5 root box, 6 parallel plane
WHY = ("margin", "runner-up", "edge band", "t ~ 0", "triangle 0", "root box", "parallel")


class Geometry:
    """Per-triangle float64 quantities from corners (n, 3, 3) and edge thicknesses (n,); entry 0 is the dummy."""

    def __init__(self, corners, edge_thickness):
        c = np.asarray(corners, np.float64).reshape(-1, 3, 3)
        self.corners = c
        self.th = np.asarray(edge_thickness, np.float64).reshape(-1)
        assert self.th.shape[0] == c.shape[0]
        a, b, cc = c[:, 0], c[:, 1], c[:, 2]
        # n = (b - a) x (c - a).  The reference's norm is unit(sides[0] x sides[1]) with sides[i] the unit vector from the
        # centroid to edge i (perpendicular to it, pointing out): sides[i] = e_i x n / (|e_i| |n|), i.e. both are the edge
        # directions turned by -90 degrees about n, a turn that keeps cross products, so sides[0] x sides[1] =
        # (e_0 x e_1) / (|e_0| |e_1|) = n / (|e_0| |e_1|): a positive multiple of n.  Back face <=> d.n > 0 with this n.
        self.n = np.cross(b - a, cc - a)
        self.n_len = np.linalg.norm(self.n, axis=1)                     # 2 area
        with np.errstate(all="ignore"):
            self.nh = self.n / self.n_len[:, None]
        self.area = self.n_len / 2
        e = np.roll(c, -1, axis=1) - c                                  # e[:, i] = corner i+1 - corner i
        self.e_len = np.linalg.norm(e, axis=2)
        with np.errstate(all="ignore"):
            # in-plane unit normal of edge i pointing INTO the triangle: n x e_i / (|n| |e_i|)
            self.m = np.cross(self.n[:, None, :], e) / (self.n_len[:, None] * self.e_len)[..., None]
            self.h = self.n_len[:, None] / (3 * self.e_len)             # the centroid's distance to edge i
        self.mp = np.einsum("nkj,nkj->nk", self.m, c)                   # m_i . corner i
        self.an = np.einsum("nj,nj->n", self.n, a)
        self.size_tol = np.maximum(EPS_M * np.sqrt(self.area), EPS_P)   # margin at normal incidence
        self.centroid = c.mean(axis=1)

    def edge_distances(self, p, tri):
        """Signed in-plane distances (positive inside) of points p (k, 3) to the three edge lines of triangles tri (k,)."""
        return np.einsum("kij,kj->ki", self.m[tri], p) - self.mp[tri]


def closest_hit(corners, edge_thickness, orig, dir, root_box=None, slack=1.0):
    """The nearest triangle each ray really crosses, brute force in float64.  corners (n, 3, 3) or a Geometry; orig / dir (R, 3)
    or (R, 4) (lane 3 ignored), dir as the kernels get it (t is in units of |dir|); root_box = (centre (3,), half edge) for a
    tree, None for a list; slack scales every margin (mirror_colour raises it bounce by bounce).
    -> Hits(tri (0 = miss), t, face, decided, why (bits, see WHY), terr (the bound on the float32 error of t that was used))."""
    g = corners if isinstance(corners, Geometry) else Geometry(corners, edge_thickness)
    o_all = np.asarray(orig, np.float64).reshape(len(orig), -1)[:, :3]
    d_all = np.asarray(dir, np.float64).reshape(len(dir), -1)[:, :3]
    R, N = o_all.shape[0], g.n.shape[0]
    tri = np.zeros(R, np.uint32)
    tt = np.zeros(R)
    face = np.zeros(R, np.uint32)
    why = np.zeros(R, np.uint32)
    terr_out = np.zeros(R)
    step = max(1, 300000 // N)
    rows = np.arange(step)
    for s in range(0, R, step):
        o, d = o_all[s:s + step], d_all[s:s + step]
        C = o.shape[0]
        r = rows[:C]
        with np.errstate(all="ignore"):
            dl = np.linalg.norm(d, axis=1)
            nd = d @ g.n.T                                              # (C, N)
            cosi = np.maximum(np.abs(nd) / (g.n_len[None, :] * dl[:, None]), TINY)
            num = g.an[None, :] - o @ g.n.T
            t = num / nd
            fin = np.isfinite(t)
            p = o[:, None, :] + np.where(fin, t, 0.0)[..., None] * d[:, None, :]
            dist = np.einsum("cnj,nkj->cnk", p, g.m) - g.mp[None]       # (C, N, 3)
            margin = dist.min(axis=2)
            tol = slack * g.size_tol[None, :] / cosi
            terr = slack * (EPS_T * np.abs(t) + EPS_0 / (cosi * dl[:, None]))
            hit = fin & (t >= 0) & (margin > 0)
            th = np.where(hit, t, np.inf)
            w = th.argmin(axis=1)
            best = th[r, w]
            have = np.isfinite(best)
            lim = np.where(have, best + terr[r, w], np.inf)[:, None]
            near = fin & (t >= -terr) & (t - terr <= lim)
            y = np.zeros(C, np.uint32)
            y |= (near & (np.abs(margin) <= tol)).any(axis=1).astype(np.uint32) << 0
            other = hit & (t - terr <= lim)
            other[r, w] = False
            y |= (have & other.any(axis=1)).astype(np.uint32) << 1
            dw, thw, hw, tolw = dist[r, w], g.th[w], g.h[w], tol[r, w]
            band = np.abs(dw - thw[:, None] * hw) <= tolw[:, None]
            y |= (have & (thw > 0) & band.any(axis=1)).astype(np.uint32) << 2
            onplane = fin & (np.abs(num) / g.n_len[None, :] <= slack * EPS_0) & (margin > -tol)
            y |= onplane.any(axis=1).astype(np.uint32) << 3
            y |= (have & (w == 0)).astype(np.uint32) << 4
            pw = p[r, w]
            if root_box is not None:
                c0, L = np.asarray(root_box[0], np.float64), float(root_box[1])
                inside = L - np.abs(pw - c0[None, :]).max(axis=1)
                y |= (have & (inside <= tolw + slack * EPS_0)).astype(np.uint32) << 5
            y |= (~fin).any(axis=1).astype(np.uint32) << 6
            edge = (dw < thw[:, None] * hw).any(axis=1)
            back = nd[r, w] > 0
        tri[s:s + C] = np.where(have, w, 0)
        tt[s:s + C] = np.where(have, best, 0.0)
        face[s:s + C] = np.where(have, back.astype(np.uint32) | (edge.astype(np.uint32) << 1), 0)
        why[s:s + C] = y
        terr_out[s:s + C] = np.where(have, terr[r, w], 0.0)
    return Hits(tri, tt, face, why == 0, why, terr_out)


# ---------------------------------------------------------------- the deterministic shading chain
class MirrorScene:
    """What mirror_colour reads: corners (n, 3, 3), edge (n,), kind (n,) SOLID / REFLECTIVE, colour (n, 3), alpha (n,),
    scattering (n,) (must be 0 for REFLECTIVE), root_box or None."""

    def __init__(self, corners, edge, kind, colour, alpha, scattering, root_box):
        self.g = Geometry(corners, edge)
        self.kind = np.asarray(kind).reshape(-1)
        self.colour = np.asarray(colour, np.float64).reshape(-1, 3)
        self.alpha = np.asarray(alpha, np.float64).reshape(-1)
        self.root_box = root_box
        k = self.kind[1:]
        assert np.isin(k, (SOLID, REFLECTIVE)).all() and (np.asarray(scattering).reshape(-1)[1:][k == REFLECTIVE] == 0).all(), \
            "mirror_colour: Solid and Reflective { scattering: 0 } surfaces only (no random draw may change the result)"


def scene_from_records(rec, kinds, surf, root_box):
    """A MirrorScene from what Scene.triangles() returns (either API): only the corners (rec[:, 20:29]), the edge thickness
    (rec[:, 19]) and the surface are read."""
    rec = np.asarray(rec)
    return MirrorScene(rec[:, 20:29].reshape(-1, 3, 3), rec[:, 19], kinds, surf[:, 0:3], surf[:, 3], surf[:, 4], root_box)


def geometry_from_records(rec):
    rec = np.asarray(rec)
    return Geometry(rec[:, 20:29].reshape(-1, 3, 3), rec[:, 19])


def mirror_colour(scene, orig, dir, maxdepth):
    """The reference's project_ray (raytrace.rs:1256-1295, color_ray :1199-1254) where it is deterministic: depth 0 is black, a
    miss is the sky, an edge face is black Solid, Solid returns its colour, Reflective returns mix_color(colour, next, alpha)
    = colour (1 - alpha) + next alpha with the next ray leaving the hit point p along r = unit(d + 2 |d.n| n_face) from
    p + 0.001 r (reflect_ray, raytrace.rs:278-301, with scattering 0).  -> (colour (R, 3), decided (R,), first: Hits).
    A colour is decided iff every hit of its chain is; the margins of bounce k are scaled by 1 + k, because the float32 chain
    carries the rounding of every earlier bounce."""
    g = scene.g
    o = np.asarray(orig, np.float64).reshape(len(orig), -1)[:, :3].copy()
    d = np.asarray(dir, np.float64).reshape(len(dir), -1)[:, :3].copy()
    R = o.shape[0]
    colour = np.zeros((R, 3))
    weight = np.ones(R)
    decided = np.ones(R, bool)
    alive = np.ones(R, bool)
    first = None
    for k in range(int(maxdepth)):
        idx = np.nonzero(alive)[0]
        if len(idx) == 0:
            break
        hk = closest_hit(g, None, o[idx], d[idx], scene.root_box, slack=1.0 + k)
        if first is None:
            first = hk
        decided[idx] &= hk.decided
        miss = hk.tri == 0
        edge = (hk.face & 2) != 0
        refl = ~miss & ~edge & (scene.kind[hk.tri] == REFLECTIVE)
        stop_col = np.where(miss[:, None], SKY, np.where(edge[:, None], 0.0, scene.colour[hk.tri]))
        a = np.where(refl, scene.alpha[hk.tri], 0.0)
        colour[idx] += (weight[idx] * (1 - a))[:, None] * stop_col
        weight[idx] *= a
        alive[idx] = refl
        j = idx[refl]
        nf = g.nh[hk.tri[refl]] * np.where(hk.face[refl] & 1, -1.0, 1.0)[:, None]
        p = o[j] + hk.t[refl, None] * d[j]
        r = d[j] + 2 * np.abs(np.einsum("kj,kj->k", d[j], nf))[:, None] * nf
        r /= np.linalg.norm(r, axis=1)[:, None]
        o[j], d[j] = p + 0.001 * r, r
    if first is None:
        first = closest_hit(g, None, o, d, scene.root_box)
    # whatever is still alive ran out of depth: its next colour is black, so nothing is added
    return colour, decided, first


# ---------------------------------------------------------------- comparisons (they RETURN what they found; tests assert)
def plane_residual(g, tri, t, orig, dir):
    """|n.(o + t d - a)| / max(1, |o|_inf, |p|_inf) with the unit normal of triangle tri, per ray."""
    o = np.asarray(orig, np.float64).reshape(len(orig), -1)[:, :3]
    d = np.asarray(dir, np.float64).reshape(len(dir), -1)[:, :3]
    p = o + np.asarray(t, np.float64)[:, None] * d
    res = np.abs(np.einsum("kj,kj->k", g.nh[tri], p - g.corners[tri, 0]))
    return res / np.maximum(1.0, np.maximum(np.abs(o).max(axis=1), np.abs(p).max(axis=1)))


def compare_hits(ref, tri, t, face, g, orig, dir, pos_tol=POS_TOL):
    """(tri, t, face) of some implementation against the referee's Hits on the decided rays -> dict(bad_id, bad_face, bad_pos:
    ray indices; max_res: the largest plane residual among decided hits with the right id)."""
    tri, face = np.asarray(tri, np.uint32), np.asarray(face, np.uint32)
    dec = ref.decided
    bad_id = np.nonzero(dec & (tri != ref.tri))[0]
    same = dec & (ref.tri != 0) & (tri == ref.tri)
    bad_face = np.nonzero(same & (face != ref.face))[0]
    res = np.zeros(len(tri))
    k = np.nonzero(same)[0]
    res[k] = plane_residual(g, tri[k], np.asarray(t)[k], np.asarray(orig)[k], np.asarray(dir)[k])
    with np.errstate(invalid="ignore"):
        bad_pos = np.nonzero(same & ~(res <= pos_tol))[0]
    return dict(bad_id=bad_id, bad_face=bad_face, bad_pos=bad_pos, max_res=float(res.max(initial=0.0)))


def describe(cmp, ref, tri, face, what):
    out = []
    for k in ("bad_id", "bad_face", "bad_pos"):
        b = cmp[k]
        if len(b):
            out.append(f"{what}: {len(b)} decided rays with {k}, first {b[:5]}: got tri {np.asarray(tri)[b[:5]]} face "
                       f"{np.asarray(face)[b[:5]]}, referee tri {ref.tri[b[:5]]} face {ref.face[b[:5]]}")
    return "; ".join(out)


def assert_hits(ref, tri, t, face, g, orig, dir, what):
    cmp = compare_hits(ref, tri, t, face, g, orig, dir)
    msg = describe(cmp, ref, tri, face, what)
    assert not msg, msg + f" (max plane residual {cmp['max_res']:.3g}, tolerance {POS_TOL:.3g})"
    return cmp


def occlusion_rays(ref, rel=1e-3):
    """The decided rays on which tmax = t (1 +- rel) decides the any-hit answer: misses, and hits whose float32 time cannot
    cross either limit (error bound terr below a quarter of the window; the near-origin grazing rays fall out here, their
    relative t error reaches 1e-2 while their hit POINT is exact to a plane residual of 1e-6)."""
    return ref.decided & ((ref.tri == 0) | (ref.terr <= 0.25 * rel * ref.t))


def family_counts(ref, sel=None):
    """rays, undecided share, decided hits and misses of (a subset of) a ray set"""
    sel = np.ones(len(ref.tri), bool) if sel is None else sel
    n = int(sel.sum())
    dec = ref.decided & sel
    return dict(rays=n, undecided=1.0 - dec.sum() / max(n, 1), hits=int((dec & (ref.tri != 0)).sum()), misses=int((dec & (ref.tri == 0)).sum()))


def assert_caps(ref, sel, cap, what, misses_possible=True, min_hits=200, min_misses=20):
    """The issue's caps: conditions a ray family must meet BEFORE anything is compared on it."""
    c = family_counts(ref, sel)
    assert c["undecided"] <= cap, f"{what}: {c['undecided']:.2%} of {c['rays']} rays undecided, cap {cap:.0%}"
    assert c["hits"] >= min_hits, f"{what}: only {c['hits']} decided hits"
    if misses_possible:
        assert c["misses"] >= min_misses, f"{what}: only {c['misses']} decided misses"
    return c


def assert_faces_occur(ref, what, least=20):
    hit = ref.decided & (ref.tri != 0)
    cnt = np.bincount(ref.face[hit], minlength=4)
    assert (cnt >= least).all(), f"{what}: decided hits per face {cnt.tolist()}, every face must occur {least} times"
    return cnt


# ---------------------------------------------------------------- leaf completeness (float64 separating-axis test)
def tri_box_penetration(corners, centre, half):
    """How deep triangles (n, 3, 3) reach into a box (centre (3,) or one per triangle (n, 3), half edge scalar or (n,)): the
    smallest overlap of the projections over the 13 separating axes of a triangle and a box (3 box normals, the triangle's
    normal, 9 edge x axis products); negative = the gap of a separated pair.  For convex polytopes this minimum is the
    distance to move them apart."""
    centre = np.asarray(centre, np.float64)
    v = np.asarray(corners, np.float64) - (centre[None, None, :] if centre.ndim == 1 else centre[:, None, :])
    n = v.shape[0]
    e = np.roll(v, -1, axis=1) - v
    axes = [np.broadcast_to(np.eye(3)[k], (n, 3)) for k in range(3)]
    axes.append(np.cross(e[:, 0], e[:, 1]))
    for i in range(3):
        for k in range(3):
            axes.append(np.cross(e[:, i], np.broadcast_to(np.eye(3)[k], (n, 3))))
    pen = np.full(n, np.inf)
    scale = np.abs(e).max(axis=(1, 2))
    for ax in axes:
        ln = np.linalg.norm(ax, axis=1)
        ok = ln > 1e-12 * np.maximum(scale, 1e-300)
        with np.errstate(all="ignore"):
            u = ax / ln[:, None]
        proj = np.einsum("nkj,nj->nk", v, u)
        rb = half * np.abs(u).sum(axis=1)
        ov = np.minimum(proj.max(axis=1) + rb, rb - proj.min(axis=1))
        pen = np.where(ok, np.minimum(pen, ov), pen)
    return pen


def leaf_completeness(g, geo, topo, refs, margin=BOX_MARGIN):
    """Every leaf of a flattened tree (geo (nb, 4) centre + half edge, topo (nb, 4) first / count / is_leaf / depth, refs) must
    list every triangle 1..n-1 that reaches more than `margin` into its box.  -> dict(missing: list of (box, triangle),
    required: pairs that must be listed, skipped: pairs within +-margin (not judged), leaves).
    A triangle lying exactly in a split plane of the octree touches every box on either side with a penetration of 0, inside
    the +-margin: such pairs are skipped, so this check does not see that the reference's builder lists that triangle in NO
    leaf (tests/test_draw_cpu.py::test_floor_in_a_split_plane_is_listed_in_no_leaf states that behaviour)."""
    geo, topo, refs = np.asarray(geo, np.float64), np.asarray(topo), np.asarray(refs, np.int64)
    boxes = np.nonzero(topo[:, 2] == 1)[0]
    leaves, ntri = len(boxes), len(g.corners)
    lo, hi = g.corners[1:].min(axis=1), g.corners[1:].max(axis=1)
    pb, pt = [], []
    for s0 in range(0, leaves, 4096):                # the box axes first: most (leaf, triangle) pairs are apart on one of them
        b = boxes[s0:s0 + 4096]
        c, L = geo[b, None, :3], geo[b, None, 3:4]
        ov = np.minimum(hi[None] - (c - L), (c + L) - lo[None]).min(axis=2)
        i, j = np.nonzero(ov >= -margin)
        pb.append(b[i])
        pt.append(j + 1)
    pb, pt = np.concatenate(pb), np.concatenate(pt)
    pen = tri_box_penetration(g.corners[pt], geo[pb, :3], geo[pb, 3])
    listed = set()
    for b in boxes:
        first, count = int(topo[b, 0]), int(topo[b, 1])
        listed.update((int(b) << 32) | refs[first:first + count])
    must = pen > margin
    required, skipped = int(must.sum()), int((np.abs(pen) <= margin).sum())
    missing = [(int(b), int(t)) for b, t in zip(pb[must], pt[must]) if ((int(b) << 32) | int(t)) not in listed]
    return dict(missing=missing, required=required, skipped=skipped, leaves=leaves)


# ---------------------------------------------------------------- ray sets
SOUP_SEEDS = (1, 2, 3, 4)
SOUP_FAMILIES = ("interior", "edge", "vertex", "band", "near")
SOUP_COUNTS = dict(interior=256, edge=512, vertex=512, band=384, near=384)          # 2 048 rays per soup
SOUP_CAPS = dict(interior=0.02, edge=0.10, vertex=0.10, band=0.10, near=0.10)
SOUP_MISSES = dict(interior=False, edge=True, vertex=True, band=False, near=False)  # can a ray of the family miss everything?
MISS_QUOTA = 40                                                                      # (the others are aimed at an inside point)
DISPLACE = 4.0                                                                       # x the decision margin, both sides


def _rays4(o, d):
    o4, d4 = np.zeros((len(o), 4), F32), np.zeros((len(d), 4), F32)
    o4[:, :3], d4[:, :3] = o, d
    return o4, d4


def _aim(o32, target):
    v = target - o32.astype(np.float64)
    return (v / np.linalg.norm(v)).astype(F32)


def soup_rays(g, seed, root_box):
    """2 048 rays for a soup's Geometry in five families (SOUP_FAMILIES, SOUP_COUNTS) -> (o4, d4, family index (R,)).
    interior: aimed at a uniformly random point of a random triangle.  edge / vertex / band: aimed at a point of an edge, at a
    vertex or at the edge-band boundary, displaced IN THE PLANE by +-DISPLACE x the decision margin of that ray, so the ray is
    adversarial and yet decided by construction (unless another triangle interferes: that is what the cap absorbs).  near:
    origins 0.02 .. 0.3 in front of an interior target, inside the tree, a quarter of them grazing (|n.d| in 1e-3 .. 1e-2).
    Origins are random float32 triples inside the root box: none lies on a box plane (the axis-plane quirks stay with the
    oracle-parity tests)."""
    rng = np.random.default_rng(77000 + seed)
    c0, L = np.asarray(root_box[0], np.float64), float(root_box[1])
    ntri = len(g.corners)
    out_o, out_d, out_f = [], [], []

    def origin():
        return (c0 + rng.uniform(-0.9, 0.9, 3) * L).astype(F32)

    def margin_for(j, o32, q):
        v = q - o32.astype(np.float64)
        return g.size_tol[j] / max(abs(float(g.nh[j] @ v)) / np.linalg.norm(v), TINY), np.linalg.norm(v)

    for f, fam in enumerate(SOUP_FAMILIES):
        got = tries = misses = 0
        while got < SOUP_COUNTS[fam]:
            tries += 1
            assert tries < 400 * SOUP_COUNTS[fam], f"soup {seed}: cannot draw the {fam} family"
            j = int(rng.integers(1, ntri))
            c = g.corners[j]
            side = 1.0 if got % 2 == 0 else -1.0                      # +: towards the inside, -: the other side
            if fam in ("interior", "near"):
                wgt = rng.dirichlet((1.0, 1.0, 1.0))
                q = wgt @ c
                if fam == "near":
                    graze = got % 4 == 3
                    u = rng.normal(size=3)
                    if graze:
                        u -= (u @ g.nh[j]) * g.nh[j]
                        u /= np.linalg.norm(u)
                        u = u + rng.choice((-1.0, 1.0)) * rng.uniform(1e-3, 1e-2) * g.nh[j]
                    u /= np.linalg.norm(u)
                    o32 = (q - rng.uniform(0.02, 0.3) * u).astype(F32)
                    if (np.abs(o32 - c0) >= 0.99 * L).any():
                        continue
                else:
                    o32 = origin()
                if fam == "interior" and np.linalg.norm(q - o32) < 0.5:
                    continue
                d32 = _aim(o32, q)
            else:
                o32 = origin()
                k = int(rng.integers(0, 3))
                if fam == "edge":
                    q0 = c[k] + rng.uniform(0.15, 0.85) * (c[(k + 1) % 3] - c[k])
                elif fam == "vertex":
                    q0 = c[k]
                else:
                    if not g.th[j] > 0:
                        continue
                    q0 = c[k] + rng.uniform(0.35, 0.65) * (c[(k + 1) % 3] - c[k]) + g.th[j] * g.h[j, k] * g.m[j, k]
                tol, dist = margin_for(j, o32, q0)
                if dist < 0.5 or tol > 2e-3 * np.sqrt(g.area[j]):         # no grazing views here: the near family has them
                    continue
                if fam == "vertex":
                    u = g.centroid[j] - c[k]
                    u /= np.linalg.norm(u)
                    gk = min(g.m[j, k] @ u, g.m[j, (k + 2) % 3] @ u)      # the two edges that meet in corner k
                    q = q0 + side * (DISPLACE * tol / gk) * u
                else:
                    q = q0 + side * DISPLACE * tol * g.m[j, k]
                dd = g.edge_distances(q[None], np.array([j]))[0]
                want_in = side > 0 or fam == "band"
                if (dd.min() > 0) != want_in or np.abs(dd).min() < 0.99 * DISPLACE * tol:
                    continue
                if g.th[j] > 0 and np.abs(dd - g.th[j] * g.h[j]).min() < 0.99 * DISPLACE * tol:
                    continue
                d32 = _aim(o32, q)
                if side < 0 and fam != "band" and misses < MISS_QUOTA:    # a dense soup stops nearly every line: draw until
                    one = closest_hit(g, None, o32[None], d32[None])      # the family has its decided misses
                    if one.tri[0] != 0 or not one.decided[0]:
                        continue
                    misses += 1
            out_o.append(o32)
            out_d.append(d32)
            out_f.append(f)
            got += 1
    o4, d4 = _rays4(np.array(out_o), np.array(out_d))
    return o4, d4, np.array(out_f)


def canonical_random_rays(n=1024, seed=7, isotropic=384):
    """Random rays in the canonical scene.  Origins and the first `isotropic` directions are the draws of
    tests/test_gpu_parity.py::test_trace_random_rays_canonical (same generator, same seed); of 1 024 such rays only 77 hit
    anything, fewer than the 200 decided hits a family needs, so the other directions are aimed at uniformly random points of
    the ball of radius 3 about the teapot (0, 0.5, 5)."""
    rng = np.random.default_rng(seed)
    o4 = np.zeros((n, 4), F32)
    d4 = np.zeros((n, 4), F32)
    o4[:, :3] = rng.uniform(-6, 6, (n, 3)) + np.array([0, 0, 6])
    d = rng.normal(size=(n, 3))
    v = rng.normal(size=(n, 3))
    target = np.array([0.0, 0.5, 5.0]) + 3.0 * v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(0, 1, (n, 1)) ** (1 / 3)
    d[isotropic:] = (target - o4[:, :3])[isotropic:]
    d4[:, :3] = d / np.linalg.norm(d, axis=1, keepdims=True)
    return o4, d4


def canonical_primary_subset(o4, d4):
    """Every fourth of the 64 x 64 primary rays, from ray 1 on (from ray 0 on only 198 of the 1 024 hit anything)"""
    return np.ascontiguousarray(o4[1::4]), np.ascontiguousarray(d4[1::4])


def as_list(h):
    """The Hits of a tree's rays for the same triangles as a list: the root box no longer makes a ray undecided"""
    why = h.why & ~np.uint32(1 << 5)
    return h._replace(decided=why == 0, why=why)


CANONICAL_ROOT = ([0.0, 0.0, 20.1], 20.0)      # conftest.recipe_canonical, octree
CANONICAL_CAP = 0.02


# ---------------------------------------------------------------- the mirror set
MIRROR_ROOT = ([0.15, -0.25, 8.35], 8.0)
MIRROR_OCTREE = (3, 4)
MIRROR_DEPTHS = (0, 1, 2, 6)
# Four 16 x 16 views (spp 1: centred rays), positions in the room's own frame (mirror_triangles).  The reference's
# create_viewport (raytrace.rs:1343-1370) places the viewport's corner with an offset that is not turned with the camera, so only
# a camera that looks down +z looks where it is told: two views do (from the open side, at both mirrors' fronts), and two are
# told -z with tan(fov / 2) = 1 / 2, which makes them look along (0, -1, -1): down from above the back wall, at the mirrors' backs.
MIRROR_VIEWS = (dict(pos=(0.3, 0.1, -2.9), aim=(0.0, 0.0, 1.0), fov=90.0),
                dict(pos=(-0.4, -0.5, -1.6), aim=(0.0, 0.0, 1.0), fov=75.0),
                dict(pos=(-2.4, 2.6, 2.9), aim=(0.0, 0.0, -1.0), fov=53.130102),
                dict(pos=(2.4, 2.6, 2.9), aim=(0.0, 0.0, -1.0), fov=53.130102))
MIRROR_VIEW_SIZE = (16, 16)


def _mirror_frame():
    ax = np.array([0.31, -0.52, 0.8])
    ax /= np.linalg.norm(ax)
    ang = 0.15
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K), np.array([0.21, -0.13, 8.4])


def mirror_cameras():
    """The four views in world coordinates: dicts of w, h, size, pos (f32), aim, fov, roll for create_viewport (the aims are
    world axes: the room's frame is turned against the world by 0.15 rad only)"""
    rot, centre = _mirror_frame()
    w, h = MIRROR_VIEW_SIZE
    return [dict(w=w, h=h, size=(1.0, 1.0), pos=(rot @ np.array(v["pos"]) + centre).astype(F32), aim=list(v["aim"]), fov=v["fov"],
                 roll=0.0) for v in MIRROR_VIEWS]


@functools.lru_cache(maxsize=None)
def mirror_triangles():
    """The hand-made mirror set: (points (n, 3, 3) f32, surfaces: list of ('solid', rgb) / ('reflective', rgb, alpha), edge
    thickness (n,)).  An open room of five Solid walls (ten triangles, ten colours), two facing Reflective quads (scattering 0,
    alpha 0.7 and 0.3) standing free in it so that rays reach their fronts and their backs, one thick-edged Solid triangle and
    a few free Solid quads; everything turned by a generic rotation so that no plane is axis-aligned."""
    rot, centre = _mirror_frame()
    tris, surfs, edges = [], [], []

    def quad(p0, du, dv, s0, s1, edge=0.0):
        p0, du, dv = (np.asarray(x, np.float64) for x in (p0, du, dv))
        for pts, s in (((p0, p0 + du, p0 + du + dv), s0), ((p0, p0 + du + dv, p0 + dv), s1)):
            tris.append(np.array(pts))
            surfs.append(s)
            edges.append(edge)

    def sol(r, gc, b):
        return ("solid", (r, gc, b))

    a = 3.2
    quad((-a, -a, a), (2 * a, 0, 0), (0, 2 * a, 0), sol(200, 40, 40), sol(220, 90, 60))          # back wall z = +a
    quad((-a, -a, -a), (2 * a, 0, 0), (0, 0, 2 * a), sol(40, 200, 40), sol(90, 220, 60))         # floor y = -a
    quad((-a, a, -a), (0, 0, 2 * a), (2 * a, 0, 0), sol(40, 40, 200), sol(60, 90, 220))          # ceiling y = +a
    quad((-a, -a, -a), (0, 0, 2 * a), (0, 2 * a, 0), sol(200, 200, 40), sol(220, 160, 60))       # left wall x = -a
    quad((a, -a, -a), (0, 2 * a, 0), (0, 0, 2 * a), sol(200, 40, 200), sol(160, 60, 220))        # right wall x = +a
    m1, m2 = ("reflective", (230, 230, 230), 0.7), ("reflective", (210, 230, 250), 0.3)
    quad((-2.3, -1.5, 0.1), (0.3, 2.9, -0.8), (1.6, 0.1, 2.2), m1, m1)                            # mirror 1, front to +x -z
    quad((2.2, -1.6, 0.2), (-1.5, 0.1, 2.1), (-0.3, 3.0, -0.9), m2, m2)                           # mirror 2, front to -x -z
    tris.append(np.array([(-0.9, -2.4, 1.2), (1.1, -2.2, 1.5), (0.2, -0.6, 2.2)]))               # the thick-edged triangle
    surfs.append(sol(250, 250, 250))
    edges.append(0.3)
    quad((-0.6, 1.1, 0.3), (1.3, 0.2, 0.1), (0.1, 0.9, 0.7), sol(20, 160, 160), sol(160, 20, 160), 0.05)
    quad((-2.6, -2.9, -1.8), (1.0, 0.1, 0.3), (0.0, 0.9, 0.4), sol(120, 70, 20), sol(20, 70, 120))
    quad((1.2, 1.6, -2.0), (1.1, 0.0, 0.5), (-0.2, 0.8, 0.1), sol(90, 90, 90), sol(170, 170, 170), -1.0)
    quad((-0.7, -0.6, 2.4), (1.4, 0.1, 0.0), (0.0, 1.4, 0.2), sol(255, 128, 0), sol(0, 128, 255), 0.3)
    quad((0.3, -3.0, -2.8), (1.5, 0.0, 0.2), (0.1, 0.3, 1.4), sol(60, 0, 30), sol(0, 60, 30), 0.3)
    pts = np.array(tris) @ rot.T + centre
    return pts.astype(F32), surfs, np.array(edges)


def mirror_recipe(accel="octree"):
    """recipe(api) for conftest.OracleApi / ProductApi"""
    def r(api):
        pts, surfs, edges = mirror_triangles()
        s = api.scene()
        for p, sf, e in zip(pts, surfs, edges):
            surf = api.solid(sf[1]) if sf[0] == "solid" else api.reflective(0.0, sf[1], sf[2])
            api.add_triangle(s, p, surf, float(e))
        s.populate_triangle_numbers()
        if accel == "octree":
            s.build_bounding_box(MIRROR_ROOT[0], MIRROR_ROOT[1], *MIRROR_OCTREE)
        else:
            s.build_trivial_bounding_box(MIRROR_ROOT[0], MIRROR_ROOT[1])
        return s
    return r


def first_hit_guides(scene, first):
    """The group guide buffers of rtmi_render_rays at G = 1 from the referee's first hits (include/rtmi.h): albedo = the
    surface's colour (black on an edge face, the sky on a miss; lane 3 = coverage), normal = the unit normal, flipped on the
    back (0 on a miss; lane 3 = t), ids = tri | face << 30 (0 on a miss)."""
    miss = first.tri == 0
    edge = (first.face & 2) != 0
    alb = np.zeros((len(miss), 4))
    alb[:, :3] = np.where(miss[:, None], SKY, np.where(edge[:, None], 0.0, scene.colour[first.tri]))
    alb[:, 3] = np.where(miss, 0.0, 1.0)
    nrm = np.zeros((len(miss), 4))
    nrm[:, :3] = np.where(miss[:, None], 0.0, scene.g.nh[first.tri] * np.where(first.face & 1, -1.0, 1.0)[:, None])
    nrm[:, 3] = first.t
    ids = np.where(miss, 0, first.tri | (first.face << np.uint32(30))).astype(np.uint32)
    return alb, nrm, ids
