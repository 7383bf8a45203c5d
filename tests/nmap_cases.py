"""Scenes, maps and rays of the normal-map tests (tests/test_nmap_cpu.py, tests/test_nmap.py).

The patch is tests/tex_cases.py's, with its four textures and its uvs.  Four map images are appended as textures 5 to 8, sizes
1 x 1, 1 x 4, 5 x 3 and 8 x 8 (width x height): seeded "tame" maps, x and y in [0.25, 0.75], z in [0.75, 1], so that the decoded
vector has length >= 0.5 and leans at most moderately.  images(wild=True) replaces texture 8 by a "wild" 8 x 8 map of arbitrary floats
in [-1, 2] whose upper-left 4 x 4 texels are exactly (0.5, 0.5, 0.5) -- a lookup inside that block is exactly (0.5, 0.5, 0.5) and
decodes to the zero vector, NaN after vunit -- and whose other texels lean any way, z < 0.5 (below the surface) among them.

NMAP_OF_TRI (entry 0 the sentinel's): the three pairs carry maps on Matte (1, 2), Reflective (3, 4) and Dielectric (5) triangles;
1, 3, 4, 5 are mapped and textured, 2 and 8 mapped and untextured, 7 textured and unmapped; the flat triangle (8), the triangle with
wrong-side normals (9) and the Solid triangle (10, which only the guide sees) are mapped.  Triangle 6 is given a map and collinear
uvs (0, 0), (0.5, 0.5), (1, 1): det is exactly 0.f and it is stored as map 0.  The sliver (11) is given a map and stored as map 0
because its den is 0.f.  The wall and the floor have none.  rays(): tex_cases.rays()."""
import numpy as np

import tex_cases as TC

F32 = np.float32
MAP_SIZES = ((1, 1), (1, 4), (5, 3), (8, 8))                     # (width, height) of textures 5 .. 8
NMAP_OF_TRI = (0, 8, 7, 6, 5, 7, 5, 0, 8, 6, 5, 7)               # entry 0 the sentinel's
COLLINEAR_TRI = 6
TEX_OF_TRI = TC.TEX_OF_TRI
recipe_patch = TC.recipe_patch
rays = TC.rays


def tame_maps():
    """The four tame maps, (h, w, 3) float32 each"""
    rng = np.random.default_rng(17)
    out = []
    for w, h in MAP_SIZES:
        m = np.zeros((h, w, 3))
        m[..., :2] = 0.25 + 0.5 * rng.random((h, w, 2))
        m[..., 2] = 0.75 + 0.25 * rng.random((h, w))
        out.append(m.astype(F32))
    return out


def wild_map():
    """The wild 8 x 8 map"""
    rng = np.random.default_rng(23)
    m = (rng.random((8, 8, 3)) * 3.0 - 1.0).astype(F32)
    m[:4, :4] = F32(0.5)
    assert (m[..., 2] < 0.5).sum() >= 8
    return m


def images(wild=False):
    """The scene's eight images: tex_cases' four textures, then the four maps"""
    maps = tame_maps()
    if wild:
        maps[3] = wild_map()
    return TC.images() + maps


def patch_uvs(ntris):
    """tex_cases.patch_uvs with triangle 6's uvs collinear: (uvs (ntris, 3, 2) float32, tex_of_tri (ntris,) uint32)"""
    uvs, tot = TC.patch_uvs(ntris)
    uvs[COLLINEAR_TRI] = np.array([(0.0, 0.0), (0.5, 0.5), (1.0, 1.0)], F32)
    return uvs, tot


def patch_nmaps(ntris):
    """nmap_of_tri (ntris,) uint32 of the patch"""
    nm = np.zeros(ntris, np.uint32)
    nm[:len(NMAP_OF_TRI)] = NMAP_OF_TRI
    return nm


def heights(w=8, h=8, seed=29):
    """Seeded heights for normal_map_from_height"""
    return np.random.default_rng(seed).random((h, w)).astype(F32)
