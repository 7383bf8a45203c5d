"""Scenes and rays of the vertex-normal tests (tests/test_smooth_cpu.py, tests/test_smooth.py), built by one recipe with both APIs.

The patch: three pairs of tilted triangles that share an edge (A, B, C) + (B, D, C), one pair Matte, one Reflective, one
Dielectric, with hand-set, strongly tilted corner normals (25 to 70 degrees off the geometric one; the shared corners B and C carry
one normal in both triangles); then a smooth Matte triangle with a FLAT one (nine zeros) beside it on a shared edge; then a Matte
triangle whose corner normals point to the wrong side of it.  No plane of the scene is parallel to an axis and no ray below has
a zero direction component.  patch_rays aims at the three corners (a hair inside), the edge midpoints, the centroid and points a
hair outside every edge of every triangle, from far in front, from far behind (back-face hits) and at grazing angles from eight
sides in front and behind, where a tilted normal faces away from the incoming ray and where a ray refracted about it leaves the
glass on the side it came from."""
import numpy as np

import glass_cases as GC
from rays_ref import vunit

F32 = np.float32
A, B, C, D = (-1.0, -0.6, 4.0), (1.0, -0.5, 4.3), (0.1, 0.9, 3.8), (1.3, 1.0, 4.6)
PAIR_DX = (-3.1, 0.0, 3.2)
E, F, G, H = (-2.0, 2.2, 4.1), (-0.2, 2.4, 4.4), (-1.1, 3.6, 3.9), (0.4, 3.7, 4.5)   # (E, F, G) smooth, (F, H, G) flat
P, Q, R_ = (1.6, 2.3, 4.2), (3.3, 2.5, 4.5), (2.4, 3.8, 4.0)                          # normals on the wrong side
IOR = 1.5
# per corner position of a pair: what is added to the pair's geometric normal before normalising
TILT = {A: (0.9, 0.5, 0.0), B: (-1.2, 0.3, 0.0), C: (0.2, -1.5, 0.0), D: (-0.8, -0.9, 0.0)}


def _shift(p, dx):
    return (p[0] + dx, p[1], p[2])


def triangles():
    """[(three corners, surface name)] in scene order (triangle 1, 2, ...)"""
    out = []
    for dx, surf in zip(PAIR_DX, ("matte", "reflective", "glass")):
        out.append(((_shift(A, dx), _shift(B, dx), _shift(C, dx)), surf))
        out.append(((_shift(B, dx), _shift(D, dx), _shift(C, dx)), surf))
    out.append(((E, F, G), "matte"))
    out.append(((F, H, G), "matte"))
    out.append(((P, Q, R_), "matte"))
    return out


def recipe_patch(accel="octree"):
    def r(api):
        s = api.scene()
        surf = dict(matte=api.matte((200, 120, 60), 0.5), reflective=api.reflective(0.05, (220, 220, 230), 0.6),
                    glass=GC.dielectric(api, IOR, (240, 250, 255), 0.9))
        for pts, name in triangles():
            api.add_triangle(s, np.array(pts, F32), surf[name], 0.0)
        # a Solid wall behind and a Matte floor, so that bounce rays find something
        GC._quad(api, s, [-8, -6, 9.3], [8, -6.2, 9.1], [8.1, 7, 9.4], [-8, 7.1, 9.2], api.solid((40, 90, 200)))
        GC._quad(api, s, [-8, -2.1, 0.5], [8, -2.3, 0.4], [8, -2.2, 9.5], [-8, -2.0, 9.6], api.matte((120, 160, 120), 0.4))
        s.populate_triangle_numbers()
        if accel == "octree":
            s.build_bounding_box([0.0, 0.0, 5.0], 10.0, 3, 2)
        else:
            s.build_trivial_bounding_box([0.0, 0.0, 0.0], 20.0)
        return s
    return r


NTRI_PATCH = 9  # the triangles that take part; the wall and the floor after them are flat


def patch_normals(recs):
    """The hand-set corner normals of the patch, (ntris, 3, 3) float32, from the records (Scene.triangles()[0]) of either API:
    rec[3:6] the geometric normal, rec[20:29] the corners"""
    recs = np.asarray(recs, F32)
    out = np.zeros((len(recs), 3, 3), F32)
    tris = triangles()
    for i, (pts, _) in enumerate(tris, start=1):
        ng = recs[i, 3:6].astype(np.float64)
        if i <= 6:
            dx = PAIR_DX[(i - 1) // 2]
            ng = recs[1 + 2 * ((i - 1) // 2), 3:6].astype(np.float64)  # the pair's first triangle: one normal per shared corner
            for k, p in enumerate(pts):
                v = ng + np.array(TILT[_nearest(p, dx)])
                out[i, k] = (v / np.linalg.norm(v)).astype(F32)
        elif i == 7:
            for k, t in enumerate(((0.7, 0.2, 0.0), (-0.6, 0.5, 0.0), (0.1, -0.9, 0.0))):
                v = ng + np.array(t)
                out[i, k] = (v / np.linalg.norm(v)).astype(F32)
        elif i == 8:
            pass  # flat
        else:
            for k, t in enumerate(((0.3, 0.1, 0.0), (-0.2, 0.2, 0.0), (0.1, -0.3, 0.0))):
                v = -ng + np.array(t)
                out[i, k] = (v / np.linalg.norm(v)).astype(F32)
    return out


def _nearest(p, dx):
    q = np.array([p[0] - dx, p[1], p[2]])
    return min(TILT, key=lambda k: np.abs(np.array(k) - q).sum())


def patch_rays():
    """(o4, d4) float32: see the module's docstring.  Origins carry small offsets that keep every direction component off zero."""
    o, d = [], []
    dirs8 = [(np.cos(a), np.sin(a)) for a in np.linspace(0.2, 2 * np.pi + 0.2, 8, endpoint=False)]
    for pts, _ in triangles()[:NTRI_PATCH]:
        p = np.array(pts, np.float64)
        cen = p.mean(axis=0)
        n = np.cross(p[1] - p[0], p[2] - p[0])
        n /= np.linalg.norm(n)
        t1 = (p[1] - p[0]) / np.linalg.norm(p[1] - p[0])
        t2 = np.cross(n, t1)
        targets = [cen]
        for k in range(3):
            targets.append(p[k] + 2e-3 * (cen - p[k]))                   # a corner, a hair inside
            mid = 0.5 * (p[k] + p[(k + 1) % 3])
            targets.append(mid + 1e-3 * (cen - mid))                     # an edge midpoint, a hair inside
            targets.append(mid - 1e-4 * (cen - mid))                     # the edge band: a hair outside
            targets.append(0.5 * (mid + cen))
        for tg in targets:
            for s in (1.0, -1.0):                                          # from far in front and from far behind
                og = tg + s * 3.7 * n + 0.013 * t1 + 0.007 * t2
                o.append(og)
                d.append(tg - og)
            for (ca, sa) in dirs8:                                         # grazing, from eight sides, in front and behind
                for s in (0.21, -0.33):
                    og = tg + 2.9 * (ca * t1 + sa * t2) + s * n
                    o.append(og)
                    d.append(tg - og)
    o4, d4 = np.zeros((len(o), 4), F32), np.zeros((len(o), 4), F32)
    o4[:, :3], d4[:, :3] = np.array(o), np.array(d)
    d4 = vunit(d4)
    assert (d4[:, :3] != 0).all()
    return o4, d4


def uv_sphere(nlat, nlon, radius=1.0, center=(0.0, 0.0, 0.0)):
    """A closed UV sphere from a shared vertex array: (corners (n, 3, 3) float32, wound outwards)"""
    verts = [(0.0, 0.0, 1.0)]
    for i in range(1, nlat):
        th = np.pi * i / nlat
        for j in range(nlon):
            ph = 2 * np.pi * j / nlon
            verts.append((np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)))
    verts.append((0.0, 0.0, -1.0))
    v = (np.array(verts) * radius + np.array(center)).astype(F32)   # ONE array: shared corners are bit-identical
    ring = lambda i, j: 1 + (i - 1) * nlon + j % nlon
    idx = []
    for j in range(nlon):
        idx.append((0, ring(1, j), ring(1, j + 1)))
        idx.append((len(v) - 1, ring(nlat - 1, j + 1), ring(nlat - 1, j)))
    for i in range(1, nlat - 1):
        for j in range(nlon):
            idx.append((ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)))
            idx.append((ring(i, j), ring(i + 1, j + 1), ring(i, j + 1)))
    return v[np.array(idx)]
