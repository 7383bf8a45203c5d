"""Scenes, textures and rays of the texture tests (tests/test_tex_cpu.py, tests/test_tex.py), built by one recipe with both APIs.

The patch is tests/smooth_cases.py's -- three pairs of tilted triangles, Matte, Reflective and Dielectric, a smooth Matte triangle
with a flat one beside it, a Matte triangle whose normals point to the wrong side, all with smooth_cases' hand-set normals when a
test wants them -- and after its nine triangles a textured SOLID triangle (10) and a sliver (11) that make_triangle accepts and
whose den = d00 * d11 - d01 * d01 is exactly 0.f in float32, so that it is stored without a texture although it is given one.  Then
the Solid wall and the Matte floor, which stay untextured.  Textures: 1 x 1, 1 x 4, 5 x 3 and 8 x 8 (width x height), seeded
random floats in [0, 2].  The corner uvs run from below 0 to above 1 on every textured triangle, so that over the rays hits
with u or v < 0 and > 1 and texel indices -1 and W - 1 (H - 1) all occur; triangles 2 and 8 are untextured beside textured ones.
rays(): smooth_cases.patch_rays() and the same pattern aimed at the Solid triangle.  (The closest-hit test finds no ray that hits
the sliver, 2^-9 high at its widest: what is held of it is the stored table.)"""
import numpy as np

import glass_cases as GC
import smooth_cases as SC
from rays_ref import vunit

F32 = np.float32
S1, S2, S3 = (-4.4, 2.3, 4.3), (-2.6, 2.5, 4.0), (-3.5, 3.7, 4.4)            # the textured Solid triangle
# the sliver: e1 = (8, 0, 0), e2 = (16, 2^-9, 0): d00 = 64, d01 = 128, d11 = 256 + 2^-18 -> 256.f, den = 64 * 256 - 128 * 128 = 0.f
V1, V2, V3 = (-8.0, -1.5, 6.0), (0.0, -1.5, 6.0), (8.0, -1.5 + 2.0 ** -9, 6.0)
NTRI_TEX = 11                                                                # triangles 1 .. 11; the wall and the floor follow
SOLID_TRI, SLIVER_TRI = 10, 11
TEX_OF_TRI = (0, 3, 0, 4, 2, 3, 1, 4, 0, 2, 3, 4)                            # entry 0 the sentinel's; 2 and 8 untextured
SIZES = ((1, 1), (1, 4), (5, 3), (8, 8))                                     # (width, height) of textures 1 .. 4
UV0 = np.array([(-0.3, -0.2), (1.4, 0.1), (0.2, 1.3)])


def images(ones=False):
    """The four textures, (h, w, 3) float32 each: seeded random floats in [0, 2], or all ones"""
    rng = np.random.default_rng(7)
    out = [(rng.random((h, w, 3)) * 2.0).astype(F32) for w, h in SIZES]
    return [np.ones_like(a) for a in out] if ones else out


def recipe_patch(accel="octree"):
    def r(api):
        s = api.scene()
        surf = dict(matte=api.matte((200, 120, 60), 0.5), reflective=api.reflective(0.05, (220, 220, 230), 0.6),
                    glass=GC.dielectric(api, SC.IOR, (240, 250, 255), 0.9))
        for pts, name in SC.triangles():
            api.add_triangle(s, np.array(pts, F32), surf[name], 0.0)
        api.add_triangle(s, np.array([S1, S2, S3], F32), api.solid((250, 200, 90)), 0.0)
        api.add_triangle(s, np.array([V1, V2, V3], F32), api.solid((90, 250, 120)), 0.0)
        # smooth_cases' Solid wall behind and Matte floor, so that bounce rays find something
        GC._quad(api, s, [-8, -6, 9.3], [8, -6.2, 9.1], [8.1, 7, 9.4], [-8, 7.1, 9.2], api.solid((40, 90, 200)))
        GC._quad(api, s, [-8, -2.1, 0.5], [8, -2.3, 0.4], [8, -2.2, 9.5], [-8, -2.0, 9.6], api.matte((120, 160, 120), 0.4))
        s.populate_triangle_numbers()
        if accel == "octree":
            s.build_bounding_box([0.0, 0.0, 5.0], 10.0, 3, 2)
        else:
            s.build_trivial_bounding_box([0.0, 0.0, 0.0], 20.0)
        return s
    return r


def patch_uvs(ntris):
    """(uvs (ntris, 3, 2) float32, tex_of_tri (ntris,) uint32) of the patch: every triangle 1 .. 11 gets uvs (a shifted copy of
    UV0), the textured ones a texture number; the wall and the floor zeros"""
    uvs, tot = np.zeros((ntris, 3, 2), F32), np.zeros(ntris, np.uint32)
    for i in range(1, NTRI_TEX + 1):
        uvs[i] = (UV0 + 0.07 * i * np.array([1.0, -1.0])).astype(F32)
        tot[i] = TEX_OF_TRI[i]
    return uvs, tot


def rays():
    """(o4, d4) float32: smooth_cases.patch_rays(), its pattern (centre, corners, edge midpoints, the edge band; from far in front,
    from behind, grazing from eight sides) at the Solid triangle"""
    o4, d4 = SC.patch_rays()
    o, d = [], []
    p = np.array([S1, S2, S3], np.float64)
    cen = p.mean(axis=0)
    n = np.cross(p[1] - p[0], p[2] - p[0])
    n /= np.linalg.norm(n)
    t1 = (p[1] - p[0]) / np.linalg.norm(p[1] - p[0])
    t2 = np.cross(n, t1)
    targets = [cen]
    for k in range(3):
        mid = 0.5 * (p[k] + p[(k + 1) % 3])
        targets += [p[k] + 2e-3 * (cen - p[k]), mid + 1e-3 * (cen - mid), mid - 1e-4 * (cen - mid), 0.5 * (mid + cen)]
    for tg in targets:
        for s in (1.0, -1.0):
            og = tg + s * 3.7 * n + 0.013 * t1 + 0.007 * t2
            o.append(og)
            d.append(tg - og)
        for a in np.linspace(0.2, 2 * np.pi + 0.2, 8, endpoint=False):
            for s in (0.21, -0.33):
                og = tg + 2.9 * (np.cos(a) * t1 + np.sin(a) * t2) + s * n
                o.append(og)
                d.append(tg - og)
    eo, ed = np.zeros((len(o), 4), F32), np.zeros((len(o), 4), F32)
    eo[:, :3], ed[:, :3] = np.array(o), np.array(d)
    ed = vunit(ed)
    assert (ed[:, :3] != 0).all()
    return np.concatenate([o4, eo]), np.concatenate([d4, ed])
