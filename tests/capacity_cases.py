"""Inputs that reach the fixed capacities of the wavefront pipeline: the slow-path queue's RTMI_SLOW_CAP entries per stream and
batch, RTMI_MAX_PASSES = 32 levels, and the 65 535 surfaces a path's uint16_t surface stack can name.  A plain module (not a
conftest), shared by test_capacity_edges_cpu.py (which asserts every precondition below from the oracle alone) and
test_capacity_edges.py (the product on the GPU against the oracle).  Every figure in here is the oracle's."""
import ctypes as C
import functools

import numpy as np

# test_progressive.SLOW_VP12, copied so that this module imports no test module: a raw viewport (orig, cam, vu, vv) whose
# orig - cam, vu and vv have x = 0, so every primary ray has d.x == 0 exactly
SLOW_VP12 = [2.0, 0.6, 1.0, 2.0, 0.0, 0.0, 0.0, -1.2, 0.0, 0.0, 0.0, 0.5]

F32 = np.float32
SLOW_CAP = 16384       # RTMI_SLOW_CAP (rtmi_device.hip)
MAX_PASSES = 32        # RTMI_MAX_PASSES
MAX_SURFACES = 65535   # rtmi_scene_create refuses more distinct surfaces
SEED = 3
COUNTERS = ("rays", "box_tests", "tri_tests", "full_tests", "nodes", "leaves")
RTMI_OK, RTMI_ERR_INVALID, RTMI_ERR_NO_DEVICE, RTMI_ERR_UNSUPPORTED = 0, 1, 2, 3


# ---------------------------------------------------------------- A: the slow-path queue
def recipe_mirror_discs():
    """Two Reflective discs without scattering facing each other, normals exactly (0, 0, -1) and (0, 0, 1), Matte rims: 401
    triangles with the sentinel.  reflect_ray off a face whose normal has x = 0 keeps a direction's x = 0 exactly (dir_p =
    norm * |d.n|, reflect = dir_p + (dir + dir_p), the scattering term is rand * 0, then unit), so under SLOW_VP12 the bounce
    rays off the disc faces are zero-component rays like the primary rays."""
    def r(api):
        s = api.scene()
        side = api.matte((40, 40, 40), 0.2)
        api.add_disk(s, [2.0, 0.7, 2.5], api.unit([0.0, 0.0, -1.0]), 2.0, 0.05, 50, api.reflective(0.0, (230, 230, 230), 0.7), side, -1.0)
        api.add_disk(s, [2.0, 0.7, 0.5], api.unit([0.0, 0.0, 1.0]), 2.0, 0.05, 50, api.reflective(0.0, (120, 200, 90), 0.6), side, -1.0)
        s.populate_triangle_numbers()
        s.build_bounding_box([2.0, 0.5, 1.5], 4.0, 5, 8)
        return s
    return r


# SLOW_VP12 frames at 1 spp, seed 3, on recipe_mirror_discs: paths, primary rays that hit, "Rays" at depth 5 / 31 / 32
FRAMES = {
    "at_cap": dict(w=128, h=128, paths=SLOW_CAP),
    "cap_plus_one": dict(w=113, h=145, paths=SLOW_CAP + 1, hits=5366, rays={5: 26016, 31: 45268, 32: 45672}),
    "over": dict(w=160, h=128, paths=20480, hits=6524, rays={5: 31778, 31: 51133, 32: 51456}),
}
OVER_W, OVER_H = 160, 128


def zero_component(d4):
    return (np.asarray(d4, F32).reshape(-1, 4)[:, :3] == 0).any(axis=1)


def recorded_passes(orc, so, w, h, vp12, maxdepth, spp, seed):
    """shadowed_ref without a light (the plain path trace, pinned to Scene.render by test_shadowed_cpu.py) with every pass's
    rays and closest hits kept: returns (its namespace, [dict(o4, d4, tri, face)] per pass that traced rays)."""
    import shadowed_ref as SR
    rec = []

    def trace(o4, d4):
        tri, t, face, _ = so.trace(o4, d4)
        rec.append(dict(o4=o4.copy(), d4=d4.copy(), tri=np.asarray(tri, np.uint32).copy(), face=np.asarray(face, np.uint32).copy()))
        return tri, t, face
    r = SR.shadowed_ref(orc, so, w, h, np.asarray(vp12, F32), maxdepth, spp, seed, trace=trace)
    return r, rec


def goes_on(so, p):
    """The hits of a recorded pass whose path goes on (color_ray: a surface hit, not an edge face, not Solid): their bounce rays
    are the next pass's rays, in this order."""
    _, kinds, _ = so.triangles()
    return (p["tri"] != 0) & ((p["face"] & 2) == 0) & (kinds[p["tri"]] != 0)


# ---------------------------------------------------------------- B: depth 32 without the slow path
CORRIDOR = dict(w=16, h=16, spp=2, maxdepth=MAX_PASSES)


# ---------------------------------------------------------------- C: 65 535 surfaces
PALETTE_N = 181                       # quads per side of the wall: 2 * 181 * 181 = 65 522 triangles
PALETTE_VIEW = dict(w=64, h=64, spp=2, maxdepth=3, size=(1.0, 1.0), pos=[0.0, 0.0, 0.0], dir=[0.0, 0.0, 1.0], fov=36.0, roll=0.0)
PALETTE_ROOT = ([0.1, 0.05, 4.03], 4.5, 7, 19)
# the second mirror (Reflective, no scattering), behind the camera: the wall's Reflective triangles send the camera's rays back
# past the camera onto it, and it returns them to the wall's upper half
PALETTE_MIRROR_C, PALETTE_MIRROR_HALF = (1.6, -0.9, -0.1), 1.0
PALETTE_MIRROR_SLOPE = (0.27, -0.22)  # z = cz + sx (x - cx) + sy (y - cy)


def _palette_z(x, y):
    return 6.0 + 0.13 * x - 0.07 * y


def palette_surface(api, k):
    """Triangle k's own surface: kind k % 3, colour (k & 255, k >> 8, 77)."""
    c = (k & 255, (k >> 8) & 255, 77)
    return (api.solid(c), api.matte(c, 0.4), api.reflective(0.0, c, 0.5))[k % 3]


def recipe_palette(extra=None, tree=True):
    """A wall of 181 x 181 quads on the plane z = 6 + 0.13 x - 0.07 y over [-2, 2]^2, triangle k (row-major from y = -2 up, so
    the upper half holds the high k) with palette_surface(k); then `extra` small triangles on the same plane left of the view
    (k goes on counting) and the mirror's two.  With extra = PALETTE_EXTRA the scene has exactly 65 535 distinct surfaces:
    the sentinel's (id 0), 65 522 + extra palette surfaces (triangle k has id k + 1) and the mirror's (id 65 534)."""
    extra = PALETTE_EXTRA if extra is None else extra

    def r(api):
        s = api.scene()
        n = PALETTE_N
        g = np.linspace(-2.0, 2.0, n + 1)
        p = lambda x, y: [x, y, _palette_z(x, y)]
        k = 0
        for iy in range(n):
            for ix in range(n):
                a, b, c, d = p(g[ix], g[iy]), p(g[ix + 1], g[iy]), p(g[ix + 1], g[iy + 1]), p(g[ix], g[iy + 1])
                api.add_triangle(s, np.array([a, b, c], F32), palette_surface(api, k), 0.0)
                api.add_triangle(s, np.array([a, c, d], F32), palette_surface(api, k + 1), 0.0)
                k += 2
        for e in range(extra):
            x, y = -3.0, -2.0 + 0.25 * e
            api.add_triangle(s, np.array([p(x, y), p(x + 0.1, y), p(x, y + 0.1)], F32), palette_surface(api, k), 0.0)
            k += 1
        (cx, cy, cz), hh, (sx, sy) = PALETTE_MIRROR_C, PALETTE_MIRROR_HALF, PALETTE_MIRROR_SLOPE
        q = lambda x, y: [x, y, cz + sx * (x - cx) + sy * (y - cy)]
        a, b, c, d = q(cx - hh, cy - hh), q(cx + hh, cy - hh), q(cx + hh, cy + hh), q(cx - hh, cy + hh)
        m = api.reflective(0.0, (250, 250, 250), 0.9)
        api.add_triangle(s, np.array([a, b, c], F32), m, 0.0)
        api.add_triangle(s, np.array([a, c, d], F32), m, 0.0)
        s.populate_triangle_numbers()
        if tree:
            s.build_bounding_box(*PALETTE_ROOT)
        return s
    return r


PALETTE_WALL_TRIS = 2 * PALETTE_N * PALETTE_N
# the surface ids PALETTE_VIEW sees at the first hit (seed 3, both samples): how many, how many above 32 767, the lowest, the highest
PALETTE_SEEN = dict(distinct=5359, high=2756, lowest=8, top=65513)
# 65 535 = the sentinel's surface + the wall's + the extra triangles' + the mirror's
PALETTE_EXTRA = MAX_SURFACES - 1 - PALETTE_WALL_TRIS - 1


def surface_ids(so):
    """rtmi_scene_create's matmap restated: the surface id of every triangle of an oracle scene (the sentinel included), in
    order of first appearance, where fields a kind does not carry (Solid alpha, Solid / Matte scattering) do not distinguish
    surfaces.  Returns (ids (n,) int64, number of distinct surfaces)."""
    _, kinds, surf = so.triangles()
    key = np.zeros((len(kinds), 6), np.uint32)
    key[:, 0] = kinds
    key[:, 1:4] = surf[:, 0:3].astype(F32).view(np.uint32)
    key[:, 4] = np.where(kinds == 0, F32(0), surf[:, 3]).astype(F32).view(np.uint32)
    key[:, 5] = np.where(kinds == 2, surf[:, 4], F32(0)).astype(F32).view(np.uint32)
    _, first, inv = np.unique(key, axis=0, return_index=True, return_inverse=True)
    rank = np.empty(len(first), np.int64)
    rank[np.argsort(first)] = np.arange(len(first))
    return rank[inv.reshape(-1)], len(first)


def palette_viewport(orc):
    v = PALETTE_VIEW
    return orc.create_viewport(v["w"], v["h"], v["size"], v["pos"], orc.unit(v["dir"]), v["fov"], v["roll"])


# ---------------------------------------------------------------- the raw ABI's arrays, without a Python loop per triangle
class Box(C.Structure):
    _fields_ = [("orig", C.c_float * 3), ("len2", C.c_float), ("first", C.c_uint32), ("count", C.c_uint32), ("is_leaf", C.c_uint32),
                ("depth", C.c_uint32)]


def abi_triangles(rec, kinds, surf):
    """rtmi_triangle_t[] (26 words each, as test_gpu_abi_raw.Tri lays them out) from Scene.triangles()'s arrays."""
    n = len(rec)
    a = np.zeros((n, 26), F32)
    a[:, 0:20] = rec[:, 0:20]                      # incenter, norm, bounding_r2, sides, side_lens, edge_thickness
    a[:, 20] = np.asarray(kinds, np.uint32).view(F32)
    a[:, 21:26] = surf[:, 0:5]                     # colour, alpha, scattering
    return np.ascontiguousarray(a)


def create_one_leaf_scene(L, tris):
    """rtmi_scene_create on a tree of one leaf that lists every triangle but the sentinel -> (rc, handle, last error)."""
    n = len(tris)
    root = (Box * 1)()
    root[0].orig[:] = [0.0, 0.0, 0.0]
    root[0].len2 = 64.0
    root[0].first, root[0].count, root[0].is_leaf, root[0].depth = 0, n - 1, 1, 0
    refs = np.arange(1, n, dtype=np.uint32)
    h = C.c_void_p()
    L.rtmi_scene_create.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p]
    L.rtmi_scene_destroy.argtypes = [C.c_void_p]
    L.rtmi_last_error.restype = C.c_char_p
    rc = L.rtmi_scene_create(tris.ctypes.data_as(C.c_void_p), n, root, 1, refs.ctypes.data_as(C.c_void_p), len(refs), 0, C.byref(h))
    return rc, h, L.rtmi_last_error()


@functools.lru_cache(maxsize=None)
def oracle_scene(name):
    """The oracle's build of a scene of these tests, built once per process."""
    from oracle import orc
    from conftest import OracleApi, recipe_axis_box
    import shadowed_ref as SR
    recipes = {"discs": recipe_mirror_discs, "axis_box": recipe_axis_box, "corridor": SR.recipe_corridor, "palette": recipe_palette}
    return recipes[name]()(OracleApi(orc))
