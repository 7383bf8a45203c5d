"""Python view of the host-side mirror of rust_raytrace's `raytrace` module.

Names follow raytrace_lib/src/raytrace.rs: make_color, create_transform,
create_viewport, Scene (tris + boxes), make_disk / make_sphere / parse_obj
(as Scene.extend_* helpers, since triangles live in the C++ Scene),
build_bounding_box, build_trivial_bounding_box, and the RayCaster plug-in
`HipRayCaster` whose walk_rays() runs the MI355X kernels through the C ABI.
"""
import ctypes as C
import time
from types import SimpleNamespace

import numpy as np

from . import _ffi

SOLID, MATTE, REFLECTIVE, DIELECTRIC = 0, 1, 2, 3
OPT_COUNTERS, OPT_GENERIC, OPT_FAST, OPT_BVH = 1, 2, 4, 8


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _chk(rc):
    if rc != 0:
        raise RuntimeError(_ffi.lib().rth_last_error().decode())


def make_color(r, g, b):
    """raytrace.rs:176-180"""
    out = np.zeros(3, np.float32)
    _ffi.lib().rth_make_color(r, g, b, _p(out))
    return out


def unit(v):
    out = np.zeros(3, np.float32)
    _ffi.lib().rth_unit(_p(_f(v)), _p(out))
    return out


def to_radians(deg):
    return float(_ffi.lib().rth_to_radians(deg))


def create_transform(direction, d_roll):
    """raytrace.rs:1320-1341 -> 9 floats (three basis rows)."""
    out = np.zeros(9, np.float32)
    _ffi.lib().rth_create_transform(_p(_f(direction)), d_roll, _p(out))
    return out


class SurfaceKind:
    """raytrace.rs:303-308, and Dielectric (include/rtmi.h, RTMI_DIELECTRIC), whose `scattering` is the index of refraction"""

    def __init__(self, kind, color, alpha=0.0, scattering=0.0):
        self.kind, self.color, self.alpha, self.scattering = kind, _f(color), float(alpha), float(scattering)

    @staticmethod
    def Solid(color):
        return SurfaceKind(SOLID, color)

    @staticmethod
    def Matte(color, alpha):
        return SurfaceKind(MATTE, color, alpha)

    @staticmethod
    def Reflective(scattering, color, alpha):
        return SurfaceKind(REFLECTIVE, color, alpha, scattering)

    @staticmethod
    def Dielectric(ior, color, alpha=1.0):
        return SurfaceKind(DIELECTRIC, color, alpha, ior)

    def args(self):
        return (self.kind, _p(self.color), self.alpha, self.scattering)


class Viewport:
    """raytrace.rs:1305-1318"""

    def __init__(self, width, height, vp12, maxdepth, samples_per_pixel):
        self.width, self.height = int(width), int(height)
        self.vp12 = _f(vp12)
        self.maxdepth, self.samples_per_pixel = int(maxdepth), int(samples_per_pixel)


def create_viewport(px, size, pos, direction, fov, c_roll, maxdepth, samples):
    """raytrace.rs:1343-1370"""
    out = np.zeros(12, np.float32)
    _ffi.lib().rth_create_viewport(px[0], px[1], size[0], size[1], _p(_f(pos)), _p(_f(direction)), fov, c_roll, _p(out))
    return Viewport(px[0], px[1], out, maxdepth, samples)


class Scene:
    """raytrace.rs:1297-1303: tris + boxes (held by the C++ mirror)."""

    def __init__(self, with_dummy=True):
        self.h = C.c_void_p(_ffi.lib().rth_scene_new(1 if with_dummy else 0))
        self._debug_en = False
        self._debug = None

    # --- Scene.debug_en / debug_ctx (raytrace.rs:1297-1303)
    @property
    def debug_en(self):
        """With debug_en set, HipRayCaster.walk_rays also records sample 0's primary ray of every pixel (the reference's
        debug_ctx); debug_records() returns them.  Octree scenes only: walk_rays raises before rendering otherwise."""
        return self._debug_en

    @debug_en.setter
    def debug_en(self, on):
        _chk(_ffi.lib().rth_scene_set_debug(self.h, 1 if on else 0))
        self._debug_en = bool(on)

    def debug_records(self):
        """The RayRecords of the last walk_rays with debug_en set (None before one)."""
        return self._debug

    def __del__(self):
        if getattr(self, "h", None) and _ffi is not None:  # module globals are None while the interpreter shuts down
            _ffi.lib().rth_scene_free(self.h)
            self.h = None

    # --- Scene.tris
    def num_tris(self):
        return int(_ffi.lib().rth_num_tris(self.h))

    def push_triangle(self, points, surface, edge_thickness):
        """obj_data.push(make_triangle(points, surface, edge_thickness))"""
        _chk(_ffi.lib().rth_add_triangle(self.h, _p(_f(points).reshape(9)), *surface.args(), edge_thickness))

    def extend_make_triangles_gpu(self, points, surface, edge_thickness, device=0):
        """obj_data.extend(points.map(make_triangle)) computed by the GPU kernel (rtmi_make_triangles); points: (n, 3, 3)."""
        pts = _f(points).reshape(-1, 9)
        _chk(_ffi.lib().rth_add_triangles_gpu(self.h, _p(pts), pts.shape[0], *surface.args(), edge_thickness, device))

    def extend_parse_obj(self, path, offset, scale, transform, surface, edge_thickness, robust=False, normals=None, crease_cos=0.5,
                         uvs=None, texture=1):
        """obj_data.extend(obj_parser::parse_obj(...)) — obj_parser.rs:47-73.  robust=True is an opt-in loader extension
        (fan-triangulated polygons, negative indices, degenerate triangles skipped); the default is the reference's loader.
        normals (an extension, include/rtmi.h "VERTEX NORMALS OF A SCENE"): None leaves the mesh flat; "file" reads the `vn` lines
        and the third field of every a/b/c or a//c face corner (each normal through the transform and unit(); a corner without a
        normal index is an error); "smooth" generates them from the mesh's shared corner positions (smooth_normals).
        uvs (an extension, include/rtmi.h "TEXTURES OF A SCENE"): None leaves the mesh untextured; "file" reads the `vt` lines and
        the second field of every a/b or a/b/c face corner (a corner without one is an error); "box" projects them (project_uvs
        with lo = (0, 0, 0), scale = 1).  The new triangles get texture number `texture`.  "file" cannot be combined with normals."""
        if normals not in (None, "file", "smooth"):
            raise ValueError(f"extend_parse_obj: normals must be None, 'file' or 'smooth', not {normals!r}")
        if uvs not in (None, "file", "box"):
            raise ValueError(f"extend_parse_obj: uvs must be None, 'file' or 'box', not {uvs!r}")
        if uvs == "file":
            if normals is not None:
                raise ValueError("extend_parse_obj: uvs='file' cannot be combined with normals")
            _chk(_ffi.lib().rth_add_obj_uvs(self.h, path.encode(), _p(_f(offset)), scale, _p(_f(transform)), *surface.args(),
                                            edge_thickness, 1 if robust else 0, int(texture)))
            return
        first = self.num_tris()
        if normals is None:
            _chk(_ffi.lib().rth_add_obj_mode(self.h, path.encode(), _p(_f(offset)), scale, _p(_f(transform)), *surface.args(),
                                             edge_thickness, 1 if robust else 0))
        else:
            _chk(_ffi.lib().rth_add_obj_normals(self.h, path.encode(), _p(_f(offset)), scale, _p(_f(transform)), *surface.args(),
                                                edge_thickness, 1 if robust else 0, 1 if normals == "file" else 2, float(crease_cos)))
        if uvs == "box" and self.num_tris() > first:
            self.project_uvs(first=first, count=self.num_tris() - first, texture=texture)

    def extend_make_disk(self, orig, norm, r, d, num_tris, surface, side_surface, edge_thickness):
        """obj_data.extend(make_disk(...)) — raytrace.rs:531-592"""
        _chk(_ffi.lib().rth_add_disk(self.h, _p(_f(orig)), _p(_f(norm)), r, d, num_tris, *surface.args(),
                                     *side_surface.args(), edge_thickness))

    def extend_make_sphere(self, orig, r, lat_lon, surface, edge_thickness):
        """obj_data.extend(make_sphere(...)) — raytrace.rs:464-529"""
        _chk(_ffi.lib().rth_add_sphere(self.h, _p(_f(orig)), r, lat_lon[0], lat_lon[1], *surface.args(), edge_thickness))

    def push_analytic_sphere(self, center, radius, surface):
        """Analytic sphere primitive: a build-defined extension (the reference only tessellates, raytrace.rs:464-529);
        a flat list tested against every ray after the box tree.  Semantics: include/rtmi.h (rtmi_sphere_t)."""
        _chk(_ffi.lib().rth_add_analytic_sphere(self.h, _p(_f(center)), radius, *surface.args()))

    def populate_triangle_numbers(self):
        _ffi.lib().rth_populate_triangle_numbers(self.h)

    # --- the environment: a build-defined extension (include/rtmi.h, "THE ENVIRONMENT OF A SCENE")
    def set_environment(self, rgb, frame=None):
        """Light the scene by an HDR map: a path that leaves the scene starts its fold at the map's colour in the direction of
        its last ray instead of the reference's sky constant.  rgb: (n, n, 3) f32 texels over the octahedral map of the
        directions, row j, column i, any float (values above 1 are the point); frame: 3 x 3, its rows take a world direction to
        map space (default: the identity).  Kept with the scene; HipRayCaster applies it on every device it uploads to."""
        t = _f(rgb)
        if t.ndim != 3 or t.shape[0] != t.shape[1] or t.shape[2] != 3 or t.shape[0] < 1:
            raise ValueError(f"environment: rgb must be (n, n, 3) with n >= 1, not {t.shape}")
        fr = None if frame is None else _f(frame).reshape(9)
        _chk(_ffi.lib().rth_scene_set_environment(self.h, _p(t), t.shape[0], None if fr is None else _p(fr)))

    def set_sky(self, n, **sky):
        """A generated environment (rtmi_scene_set_sky): an n x n table the device fills with a gradient sky and a sun disc.
        Keywords are rtmi_sky_t's fields (up, sun_dir, sun_cos, zenith, horizon, ground, sun_color); the rest keep their defaults."""
        k = _ffi.Sky()
        _ffi.lib().rtmi_sky_defaults(C.byref(k))
        for name, val in sky.items():
            if name not in dict(_ffi.Sky._fields_):
                raise TypeError(f"set_sky: unknown field {name!r}")
            if name == "sun_cos":
                k.sun_cos = float(val)
            else:
                setattr(k, name, (C.c_float * 3)(*[float(x) for x in val]))
        _chk(_ffi.lib().rth_scene_set_sky(self.h, int(n), C.byref(k)))

    def clear_environment(self):
        """Back to the reference's sky constant: the scene is exactly the scene it was before it had an environment."""
        _chk(_ffi.lib().rth_scene_set_environment(self.h, None, 0, None))

    # --- vertex normals: a build-defined extension (include/rtmi.h, "VERTEX NORMALS OF A SCENE")
    def smooth_normals(self, first=1, count=None, crease_cos=0.5):
        """Generate vertex normals for triangles [first, first + count) (default: all), for example one mesh, from the corner
        positions they share among themselves (rtmi_smooth_normals): area-weighted face normals, averaged across the edges whose
        faces' normals have a cosine of at least crease_cos.  Triangles outside the range keep what they had (flat if nothing)."""
        _chk(_ffi.lib().rth_scene_smooth_normals(self.h, int(first), 2 ** 64 - 1 if count is None else int(count), float(crease_cos)))

    def set_vertex_normals(self, normals, first=1):
        """Corner normals of triangles first, first + 1, ...: (n, 3, 3) f32, corner k of triangle i at [i, k].  A triangle whose
        nine floats are zero is flat.  Kept with the scene; HipRayCaster applies them on every device it uploads to."""
        t = _f(normals)
        if t.ndim != 3 or t.shape[1:] != (3, 3):
            raise ValueError(f"vertex normals must be (n, 3, 3), not {t.shape}")
        _chk(_ffi.lib().rth_scene_set_normals(self.h, _p(t), int(first), t.shape[0]))

    def vertex_normals(self):
        """The scene's vertex normals, (ntris, 3, 3) f32 with entry 0 the sentinel's (zeros), or None when it has none"""
        n = C.c_uint64(0)
        _chk(_ffi.lib().rth_scene_normals_size(self.h, C.byref(n)))
        if n.value == 0:
            return None
        out = np.zeros((n.value, 3, 3), np.float32)
        _chk(_ffi.lib().rth_scene_get_normals(self.h, _p(out), out.size))
        return out

    def clear_vertex_normals(self):
        """Back to flat shading: the scene is exactly the scene it was before it had vertex normals."""
        _chk(_ffi.lib().rth_scene_set_normals(self.h, None, 0, 0))

    # --- textures: a build-defined extension (include/rtmi.h, "TEXTURES OF A SCENE")
    def set_textures(self, images, uvs, tex_of_tri, first=1, flip_v=False):
        """The scene's images, and uvs and texture numbers of triangles first, first + 1, ...: images a list of (h, w, 3) f32
        arrays, row 0 at v = 0 (flip_v=True: the arrays are stored top row first, as image files are); uvs (n, 3, 2) f32, corner k
        of triangle i at [i, k]; tex_of_tri (n,) with 0 = no texture, or 1..len(images).  uvs=None sets the images alone and keeps
        the uvs the scene has.  Kept with the scene; HipRayCaster applies them on every device it uploads to."""
        imgs = []
        for k, im in enumerate(images):
            a = _f(im)
            if a.ndim != 3 or a.shape[2] != 3:
                raise ValueError(f"texture {k + 1} must be (h, w, 3), not {a.shape}")
            imgs.append(np.ascontiguousarray(a[::-1]) if flip_v else a)
        arr = (_ffi.Texture * max(len(imgs), 1))()
        for k, a in enumerate(imgs):
            arr[k] = _ffi.Texture(a.ctypes.data, a.shape[1], a.shape[0], 0)
        if uvs is not None:
            t, tt = _f(uvs), np.ascontiguousarray(tex_of_tri, dtype=np.uint32)
            if t.ndim != 3 or t.shape[1:] != (3, 2) or tt.shape != (t.shape[0],):
                raise ValueError(f"uvs must be (n, 3, 2) and tex_of_tri (n,), not {t.shape} and {tt.shape}")
            if imgs and tt.size and int(tt.max()) > len(imgs):
                raise RuntimeError(f"textures: tex_of_tri of triangle {int(first) + int(np.argmax(tt > len(imgs)))} is above ntex")
        if not imgs:
            raise ValueError("set_textures: no images (clear_textures() removes them)")
        _chk(_ffi.lib().rth_scene_set_textures(self.h, arr, len(imgs)))
        if uvs is not None:
            _chk(_ffi.lib().rth_scene_set_uvs(self.h, _p(t), _p(tt), int(first), t.shape[0]))

    def project_uvs(self, first=1, count=None, lo=(0, 0, 0), scale=1.0, texture=1):
        """Box-projected uvs (rtmi_project_uvs) for triangles [first, first + count) (default: all), for example one mesh, which get
        texture number `texture`: per triangle the two coordinates other than the face normal's largest, (p - lo) * scale."""
        _chk(_ffi.lib().rth_scene_project_uvs(self.h, int(first), 2 ** 64 - 1 if count is None else int(count), _p(_f(lo).reshape(3)),
                                              float(scale), int(texture)))

    def textures(self):
        """The scene's textures: (images, uvs (ntris, 3, 2) f32, tex_of_tri (ntris,) u32) with entry 0 the sentinel's, or None when it
        has neither images nor uvs"""
        ntex, n = C.c_uint32(0), C.c_uint64(0)
        _chk(_ffi.lib().rth_scene_textures_size(self.h, C.byref(ntex), C.byref(n)))
        if n.value == 0:
            return None
        uv, tt = np.zeros((n.value, 3, 2), np.float32), np.zeros(n.value, np.uint32)
        _chk(_ffi.lib().rth_scene_get_uvs(self.h, _p(uv), _p(tt), n.value))
        images = []
        for k in range(1, ntex.value + 1):
            w, h = C.c_uint32(0), C.c_uint32(0)
            _chk(_ffi.lib().rth_scene_get_texture(self.h, k, None, 0, C.byref(w), C.byref(h)))
            im = np.zeros((h.value, w.value, 3), np.float32)
            _chk(_ffi.lib().rth_scene_get_texture(self.h, k, _p(im), im.size, C.byref(w), C.byref(h)))
            images.append(im)
        return images, uv, tt

    def clear_textures(self):
        """Back to one colour per material: the scene is exactly the scene it was before it had textures.  Its normal maps, which
        are images of the textures, go too."""
        _chk(_ffi.lib().rth_scene_set_textures(self.h, None, 0))

    # --- normal maps: a build-defined extension (include/rtmi.h, "NORMAL MAPS OF A SCENE")
    def set_normal_maps(self, nmap_of_tri, first=1, strength=1.0):
        """Normal maps of triangles first, first + 1, ...: nmap_of_tri (n,) with 0 = no map, or the number 1..len(images) of the
        texture image (set_textures) whose rgb encodes the tangent-space normal as 2 * rgb - 1; strength scales x and y of every
        map.  Independent of tex_of_tri.  Kept with the scene; set_textures and clear_textures remove the maps."""
        nm = np.ascontiguousarray(nmap_of_tri, dtype=np.uint32).reshape(-1)
        if nm.size == 0:
            raise ValueError("set_normal_maps: no entries (clear_normal_maps() removes the maps)")
        _chk(_ffi.lib().rth_scene_set_normal_maps(self.h, _p(nm), int(first), nm.size, float(strength), 0))

    def normal_maps(self):
        """The scene's normal maps: (nmap_of_tri (ntris,) u32 with entry 0 the sentinel's, strength), or None when it has none"""
        n = C.c_uint64(0)
        _chk(_ffi.lib().rth_scene_normal_maps_size(self.h, C.byref(n)))
        if n.value == 0:
            return None
        nm, st = np.zeros(n.value, np.uint32), C.c_float(0)
        _chk(_ffi.lib().rth_scene_get_normal_maps(self.h, _p(nm), C.byref(st), n.value))
        return nm, float(st.value)

    def normal_map_frames(self):
        """What a device stores per triangle for the scene's maps (rtmi_normal_map_frames): (T (ntris, 3) f32, hand (ntris,) f32 of
        +-1, nmap (ntris,) u32 -- 0 where the triangle has no map or no tangent frame), entry 0 the sentinel's."""
        n = self.num_tris()
        fr = np.zeros((n, 4), np.float32)
        _chk(_ffi.lib().rth_scene_normal_map_frames(self.h, _p(fr), n))
        bits = np.ascontiguousarray(fr[:, 3]).view(np.uint32)
        return np.ascontiguousarray(fr[:, :3]), np.where(bits >> 31 != 0, np.float32(-1.0), np.float32(1.0)), bits & np.uint32(0x7FFFFFFF)

    def clear_normal_maps(self):
        """No normal maps: the scene is exactly the scene it was before it had them."""
        _chk(_ffi.lib().rth_scene_set_normal_maps(self.h, None, 0, 0, 1.0, 0))

    # --- emitters: a build-defined extension (include/rtmi.h, "EMISSIVE TRIANGLES")
    def set_emitters(self, mask_or_indices, first=1):
        """Mark Solid triangles as lamps for HipRayCaster.walk_rays_emissive*: a boolean (or uint8) mask for triangles first, first + 1,
        ..., or an integer array of triangle numbers (first is then ignored; every other triangle keeps its mark).  A lamp's radiance
        is its surface colour, which may exceed 1.  No other call changes: the scene renders everywhere else exactly as before.  Kept
        with the scene like its vertex normals (triangles appended later are no lamps); HipRayCaster applies the marks on every
        device it uploads to, where a marked triangle that is not Solid is an error."""
        a = np.asarray(mask_or_indices)
        if a.ndim != 1 or a.size == 0:
            raise ValueError("set_emitters: a non-empty 1-d mask or index array (clear_emitters() removes the marks)")
        if a.dtype == np.bool_ or a.dtype == np.uint8:
            m = np.ascontiguousarray(a != 0, dtype=np.uint8)
            _chk(_ffi.lib().rth_scene_set_emitters(self.h, _p(m), int(first), m.size))
            return
        if not np.issubdtype(a.dtype, np.integer):
            raise ValueError(f"set_emitters: a boolean mask or integer triangle numbers, not {a.dtype}")
        n = self.num_tris()
        if a.min() < 1 or a.max() >= n:
            raise ValueError("set_emitters: triangle numbers must be 1 to the number of triangles - 1")
        m = self.emitters()
        m = np.zeros(n, np.uint8) if m is None else m.astype(np.uint8)
        m[a] = 1
        _chk(_ffi.lib().rth_scene_set_emitters(self.h, _p(np.ascontiguousarray(m[1:])), 1, n - 1))

    def emitters(self):
        """The scene's lamp marks, (ntris,) bool with entry 0 the sentinel's (False), or None when no triangle is marked"""
        m = np.zeros(self.num_tris(), np.uint8)
        _chk(_ffi.lib().rth_scene_get_emitters(self.h, _p(m), m.size))
        return m.astype(bool) if m.any() else None

    def clear_emitters(self):
        """No lamps: walk_rays_emissive* refuses the scene again; every other call is as it always was."""
        _chk(_ffi.lib().rth_scene_set_emitters(self.h, None, 0, 0))

    # --- Scene.boxes
    def build_bounding_box(self, orig, len2, maxdepth, minobjs, threads=0, gpu_device=None):
        """raytrace.rs:790-845.  gpu_device: evaluate the box/triangle overlap tests of every level on that GPU
        (rtmi_builder_*, k_box_contains) instead of on `threads` host threads; the tree is bit-equal either way."""
        if gpu_device is not None:
            _chk(_ffi.lib().rth_build_bounding_box_gpu(self.h, _p(_f(orig)), len2, maxdepth, minobjs, int(gpu_device)))
        else:
            _chk(_ffi.lib().rth_build_bounding_box(self.h, _p(_f(orig)), len2, maxdepth, minobjs, threads))

    def build_trivial_bounding_box(self, orig, len2):
        """raytrace.rs:847-856"""
        _chk(_ffi.lib().rth_build_trivial_bounding_box(self.h, _p(_f(orig)), len2))

    def box_contains_polygon(self, orig, len2, tri):
        return bool(_ffi.lib().rth_box_contains_polygon(self.h, _p(_f(orig)), len2, tri))

    def face_contains_triangle(self, p, norm, len2, tri):
        return bool(_ffi.lib().rth_face_contains_triangle(self.h, _p(_f(p)), _p(_f(norm)), len2, tri))

    # --- inspection
    def triangles(self):
        n = self.num_tris()
        rec = np.zeros((n, 29), np.float32)
        kinds = np.zeros(n, np.int32)
        surf = np.zeros((n, 5), np.float32)
        _ffi.lib().rth_get_triangles(self.h, _p(rec), _p(kinds), _p(surf))
        return rec, kinds, surf

    def tree(self):
        nb, nr = C.c_uint64(0), C.c_uint64(0)
        _ffi.lib().rth_tree_sizes(self.h, C.byref(nb), C.byref(nr))
        geo = np.zeros((nb.value, 4), np.float32)
        topo = np.zeros((nb.value, 4), np.uint32)
        refs = np.zeros(max(nr.value, 1), np.uint32)
        _ffi.lib().rth_tree_get(self.h, _p(geo), _p(topo), _p(refs))
        return geo, topo, refs[: nr.value]

    def tree_stats(self):
        _, topo, refs = self.tree()
        leaf = topo[:, 2] == 1
        return dict(inner=int((~leaf).sum()), leaves=int(leaf.sum()), refs=int(len(refs)),
                    maxdepth=int(topo[:, 3].max()) if len(topo) else 0)


# rtmi_ray_record_t (include/rtmi.h) as a numpy record; the natural offsets of these fields are the C layout (72 B)
REC_DTYPE = np.dtype([("orig", "<f4", (4,)), ("dir", "<f4", (4,)), ("tri", "<u4"), ("t", "<f4"), ("face", "<u4"), ("nleaves", "<u4"),
                      ("leaf_first", "<u8"), ("box_tests", "<u4"), ("tri_tests", "<u4"), ("full_tests", "<u4"), ("nodes", "<u4")])
assert REC_DTYPE.itemsize == C.sizeof(_ffi.RayRecord)


def format_f32(x):
    """A float32 as Rust's `{}` prints an f32: the shortest digits that round-trip, never an exponent (1.0 -> "1",
    1e-10 -> "0.0000000001", -0.0 -> "-0", NaN -> "NaN", infinities -> "inf" / "-inf")."""
    x = np.float32(x)
    if np.isnan(x):
        return "NaN"
    if np.isinf(x):
        return "inf" if x > 0 else "-inf"
    return np.format_float_positional(x, unique=True, trim="-")


class RayRecords:
    """Per-ray records of the octree walk (rtmi_trace_records / rtmi_primary_records): numpy arrays orig, dir ((n, 4)
    f32), tri, t, face, nleaves, leaf_first, leaf_ids, counters (dict of per-ray arrays: box_tests, tri_tests, full_tests,
    nodes, leaves) and, for primary records, pixel ((n, 2): row, col).  Leaf ids index Scene.tree()'s boxes."""

    def __init__(self, recs, leaf_ids, pixel=None, stats=None):
        recs = np.asarray(recs, REC_DTYPE)
        self.orig, self.dir = recs["orig"].copy(), recs["dir"].copy()
        self.tri, self.t, self.face = recs["tri"].copy(), recs["t"].copy(), recs["face"].copy()
        self.nleaves, self.leaf_first = recs["nleaves"].copy(), recs["leaf_first"].copy()
        self.leaf_ids = np.asarray(leaf_ids, np.uint32).copy()
        self.counters = {k: recs[k].copy() for k in ("box_tests", "tri_tests", "full_tests", "nodes")}
        self.counters["leaves"] = self.nleaves.copy()
        self.pixel = None if pixel is None else np.asarray(pixel, np.uint32).reshape(-1, 2)
        self.stats = stats

    def __len__(self):
        return len(self.tri)

    def leaves(self, i):
        """The leaves ray i entered, in visiting order (a leaf entered twice is listed twice)."""
        a = int(self.leaf_first[i])
        return self.leaf_ids[a:a + int(self.nleaves[i])]

    @staticmethod
    def _lists(scene):
        _, topo, refs = scene.tree()
        return topo, refs

    def check_tris(self, i, scene, _tree=None):
        """The reference's check_tris of ray i: the sorted, de-duplicated union of its leaves' triangle lists."""
        topo, refs = _tree if _tree is not None else self._lists(scene)
        parts = [refs[topo[b, 0]:topo[b, 0] + topo[b, 1]] for b in self.leaves(i)]
        return np.unique(np.concatenate(parts)) if parts else np.zeros(0, np.uint32)

    def write_csv(self, f, scene):
        """The reference's debug CSV (main.rs writes it as debug_*.csv): one line per pixel in (row, col) order,
        `row;col;ox,oy,oz;dx,dy,dz;tri;t;i1,i2,...` after the header.  An empty check_tris is an empty field (the
        reference panics there).  f: a path or a text file object."""
        if self.pixel is None:
            raise ValueError("write_csv needs primary records (a pixel per record)")
        if isinstance(f, str):
            with open(f, "w") as fh:
                return self.write_csv(fh, scene)
        tree = self._lists(scene)
        f.write("Pixel_x;Pixel_y;ray_p;ray_v;tri_hit;hit_t;check_tris\n")
        for i in np.lexsort((self.pixel[:, 1], self.pixel[:, 0])):
            p = ",".join(format_f32(x) for x in self.orig[i, :3])
            d = ",".join(format_f32(x) for x in self.dir[i, :3])
            ct = ",".join(str(int(x)) for x in self.check_tris(i, scene, tree))
            f.write(f"{int(self.pixel[i, 0])};{int(self.pixel[i, 1])};{p};{d};{int(self.tri[i])};{format_f32(self.t[i])};{ct}\n")


class ProgressCtx:
    """What progress.rs:157-184 reports."""

    def __init__(self, total_rays, seconds, stats):
        self.total_rays, self.seconds, self.stats = total_rays, seconds, stats

    def stats_line(self):
        m = self.total_rays / 1e6
        return f"Processed {m:.3f} million rays in {self.seconds:.3f} seconds. {m / max(self.seconds, 1e-12):.3f} million rays/s"


class HipRayCaster:
    """impl RayCaster (raytrace.rs:1128-1165) on MI355X.

    walk_rays(v, s, data, threads, show_progress) fills `data` ((H, W, 4) f32,
    the reference's `&mut [Color]`) and returns a ProgressCtx.  `threads` is
    accepted and ignored, as the reference's CudaRayCaster does.
    """

    def __init__(self, seed=1, device=0, options=0, tuning=None, devices=None):
        """tuning: dict of rtmi_tuning_t fields (batch_paths, streams, subtile_min_paths, oct_waves_per_cu,
        refill_min0, refill_min, xcd_aware); fields not given keep the library default.  Never changes a pixel.
        devices: list of device indices for the in-library multi-GPU fan-out (rtmi_render_frame_multi); entry 0 is the
        root, an entry may repeat a device.  With more than one entry walk_rays() stripes the frame over them."""
        self.seed, self.device, self.options = int(seed), int(device), int(options)
        self.tuning = dict(tuning) if tuning else None
        self.devices = [int(d) for d in devices] if devices else None
        if self.devices:
            self.device = self.devices[0]
        self._scene = None

    def _config(self, s):
        self._scene = s  # denoise() / denoise_device() without a scene use the last one this caster worked on
        _chk(_ffi.lib().rth_caster_config(s.h, self.seed, self.device, self.options))
        devs = self.devices or [self.device]
        arr = (C.c_int32 * len(devs))(*devs)
        _chk(_ffi.lib().rth_caster_set_devices(s.h, arr, len(devs)))
        if self.tuning is None:
            if getattr(s, "_tuned", False):
                _chk(_ffi.lib().rth_caster_set_tuning(s.h, None))
                s._tuned = False
        else:
            t = _ffi.Tuning()
            for k, v in self.tuning.items():
                setattr(t, k, int(v) + 1 if k == "xcd_aware" else int(v))
            _chk(_ffi.lib().rth_caster_set_tuning(s.h, C.byref(t)))
            s._tuned = True

    def walk_rays(self, v, s, data, threads=1, show_progress=False, progress=None, bands=16):
        """progress: callable(thread, row, pixels, stats) -- what DefaultRayCaster sends over its channel per finished row
        (raytrace.rs:1411, :1429-1435).  With a callback (or show_progress=True, which prints one line per band like the
        reference's TUI redraw) the frame is rendered in `bands` row bands, one render call and one tuple each; same image, a
        few per cent slower than in one piece (a band's launches do not overlap the next band's).
        With s.debug_en (and maxdepth > 0) the same image is rendered and s.debug_records() receives the primary records of
        sample 0 of every pixel, taken first: an unsupported scene raises before anything is rendered."""
        if s.debug_en and v.maxdepth > 0:
            rec = self.primary_records(v, s, 0, v.height, 0)
            ctx = self._walk_rays(v, s, data, show_progress, progress, bands)
            s._debug = rec
            return ctx
        return self._walk_rays(v, s, data, show_progress, progress, bands)

    def _walk_rays(self, v, s, data, show_progress, progress, bands):
        if self.devices and len(self.devices) > 1:
            return self.walk_frame_multi(v, s, data)
        if progress is None and not show_progress:
            return self.walk_rows(v, s, 0, v.height, data)
        flat = data.reshape(v.height, v.width * 4)
        total, secs, summed = 0, 0.0, None
        bands = max(1, min(int(bands), v.height))
        for b in range(bands):
            r0, r1 = v.height * b // bands, v.height * (b + 1) // bands
            if r1 == r0:
                continue
            ctx = self.walk_rows(v, s, r0, r1 - r0, flat[r0:r1])
            total += ctx.total_rays
            secs += ctx.seconds
            if summed is None:
                summed = dict(ctx.stats)
            else:
                for k in ("rays", "box_tests", "tri_tests", "full_tests", "nodes", "leaves", "kernel_ms", "trace_ms", "trace_launches",
                          "primary_ms", "bounce_ms", "slow_paths"):
                    summed[k] += ctx.stats[k]
            if progress is not None:
                progress(0, r1 - 1, (r1 - r0) * v.width, {"Rays": ctx.total_rays})
            if show_progress:
                print(f"rows {r0}..{r1 - 1} done: {ctx.stats_line()}", flush=True)
        return ProgressCtx(total, secs, summed)

    def walk_frame_multi(self, v, s, data=None, rgb8=False, stripe_rows=0, out_device_ptr=None, rccl=False):
        """One frame striped over self.devices inside the library.  data: (H, W, 4) f32, or (H, W, 3) u8 with rgb8=True
        (each band is quantised on its device before it crosses to the root).  rccl=True: the bands cross with one ncclGather
        (RTMI_FRAME_RCCL; every entry of self.devices must then be a different device).  Returns ProgressCtx; .per_device
        holds the stats of every device."""
        want = (np.uint8, 3) if rgb8 else (np.float32, 4)
        if data is not None and (data.dtype != want[0] or not data.flags.c_contiguous or data.size != v.height * v.width * want[1]):
            raise ValueError("data must be C-contiguous (H, W, 4) float32, or (H, W, 3) uint8 with rgb8")
        self._config(s)
        n = len(self.devices or [self.device])
        st = _ffi.Stats()
        per = (_ffi.Stats * n)()
        wall = C.c_double(0)
        _chk(_ffi.lib().rth_caster_walk_frame_multi(s.h, v.width, v.height, _p(v.vp12), v.maxdepth, v.samples_per_pixel, stripe_rows,
                                                    (1 if rgb8 else 0) | (2 if rccl else 0), _p(data) if data is not None else None,
                                                    C.c_void_p(out_device_ptr or 0), C.byref(st), per, n, C.byref(wall)))
        ctx = ProgressCtx(st.rays, wall.value, st.as_dict())
        ctx.per_device = [p.as_dict() for p in per]
        return ctx

    def walk_rows(self, v, s, row0, nrows, data):
        """Rows [row0, row0+nrows) only — the unit of multi-GPU image tiling."""
        if data.dtype != np.float32 or not data.flags.c_contiguous or data.size != nrows * v.width * 4:
            raise ValueError("data must be a C-contiguous float32 array of nrows*width*4 elements")
        self._config(s)
        st = _ffi.Stats()
        wall = C.c_double(0)
        _chk(_ffi.lib().rth_caster_walk_rows(s.h, v.width, v.height, _p(v.vp12), v.maxdepth, v.samples_per_pixel, row0,
                                             nrows, _p(data), C.byref(st), C.byref(wall)))
        return ProgressCtx(st.rays, wall.value, st.as_dict())

    def walk_rows_device(self, v, s, row0, nrows, out_ptr, stream_ptr=None):
        """Same, writing nrows*width float4 of device memory at `out_ptr` on HIP stream `stream_ptr`."""
        self._config(s)
        st = _ffi.Stats()
        wall = C.c_double(0)
        _chk(_ffi.lib().rth_caster_walk_rows_device(s.h, v.width, v.height, _p(v.vp12), v.maxdepth, v.samples_per_pixel,
                                                    row0, nrows, C.c_void_p(out_ptr), C.c_void_p(stream_ptr or 0),
                                                    C.byref(st), C.byref(wall)))
        return ProgressCtx(st.rays, wall.value, st.as_dict())

    def walk_tile_device(self, v, s, tile, out_ptr, stream_ptr=None):
        """Striped row set: tile = (row0, nrows, stripe_rows, stripe_step) — rtmi_tile_t."""
        self._config(s)
        st = _ffi.Stats()
        wall = C.c_double(0)
        t = _ffi.Tile(*[int(x) for x in tile])
        _chk(_ffi.lib().rth_caster_walk_tile_device(s.h, v.width, v.height, _p(v.vp12), v.maxdepth, v.samples_per_pixel,
                                                    C.byref(t), C.c_void_p(out_ptr), C.c_void_p(stream_ptr or 0),
                                                    C.byref(st), C.byref(wall)))
        return ProgressCtx(st.rays, wall.value, st.as_dict())

    def walk_samples(self, v, s, row0, nrows, sample0, nsamples, accum, out=None):
        """Progressive pass on host arrays (rtmi_render_samples): samples [sample0, sample0+nsamples) of the frame's
        v.samples_per_pixel for rows [row0, row0+nrows).  accum (nrows*width*4 f32) holds the running per-pixel sums: read
        when sample0 > 0, always rewritten.  out (optional, same shape) receives the preview accum * (1/(sample0+nsamples)).
        Passes over [0, spp) in sample order end in the bits of walk_rows."""
        for name, a in (("accum", accum), ("out", out)):
            if a is not None and (a.dtype != np.float32 or not a.flags.c_contiguous or a.size != nrows * v.width * 4):
                raise ValueError(f"{name} must be a C-contiguous float32 array of nrows*width*4 elements")
        self._config(s)
        st = _ffi.Stats()
        wall = C.c_double(0)
        _chk(_ffi.lib().rth_caster_walk_samples(s.h, v.width, v.height, _p(v.vp12), v.maxdepth, v.samples_per_pixel, row0, nrows,
                                                sample0, nsamples, _p(accum), _p(out) if out is not None else None,
                                                C.byref(st), C.byref(wall)))
        return ProgressCtx(st.rays, wall.value, st.as_dict())

    def walk_samples_device(self, v, s, tile, sample0, nsamples, accum_ptr, out_ptr, stream_ptr=None):
        """The same on device memory (rtmi_render_samples_device) for a striped row set tile = (row0, nrows, stripe_rows,
        stripe_step), enqueued on HIP stream `stream_ptr`; out_ptr may be None/0 (no preview).  No host copies."""
        self._config(s)
        st = _ffi.Stats()
        wall = C.c_double(0)
        t = _ffi.Tile(*[int(x) for x in tile])
        _chk(_ffi.lib().rth_caster_walk_samples_device(s.h, v.width, v.height, _p(v.vp12), v.maxdepth, v.samples_per_pixel,
                                                       C.byref(t), sample0, nsamples, C.c_void_p(accum_ptr),
                                                       C.c_void_p(out_ptr or 0), C.c_void_p(stream_ptr or 0),
                                                       C.byref(st), C.byref(wall)))
        return ProgressCtx(st.rays, wall.value, st.as_dict())

    def walk_rays_progressive(self, v, s, data, pass_samples=8, on_pass=None):
        """walk_rays in passes of `pass_samples` samples per pixel (the last pass may be shorter).  After each pass `data`
        ((H, W, 4) f32) holds the preview of the samples done and on_pass(samples_done, ctx) is called with the running
        ProgressCtx; if it returns False the loop stops there.  Returns a ProgressCtx with the total rays, summed stats and
        `samples_done`.  When every pass runs, `data` ends bit-identical to walk_rays.  The preview after k samples equals a
        render at samples_per_pixel = k when k >= 2 (a first pass of one sample of a larger frame is jittered).  Each pass
        copies the running sums to and from the device (2 x 16 B per pixel); walk_samples_device avoids that."""
        if data.dtype != np.float32 or not data.flags.c_contiguous or data.size != v.height * v.width * 4:
            raise ValueError("data must be a C-contiguous float32 array of height*width*4 elements")
        spp, step = int(v.samples_per_pixel), int(pass_samples)
        if step < 1:
            raise ValueError("pass_samples must be >= 1")
        accum = np.zeros_like(data)
        ctx = ProgressCtx(0, 0.0, None)
        ctx.samples_done = 0
        for k0 in range(0, spp, step):
            n = min(step, spp - k0)
            p = self.walk_samples(v, s, 0, v.height, k0, n, accum, data)
            ctx.total_rays += p.total_rays
            ctx.seconds += p.seconds
            if ctx.stats is None:
                ctx.stats = dict(p.stats)
            else:
                for k in ("rays", "box_tests", "tri_tests", "full_tests", "nodes", "leaves", "kernel_ms", "trace_ms", "trace_launches",
                          "primary_ms", "bounce_ms", "slow_paths"):
                    ctx.stats[k] += p.stats[k]
            ctx.samples_done = k0 + n
            if on_pass is not None and on_pass(ctx.samples_done, ctx) is False:
                break
        return ctx

    # Default stop tolerances of walk_rays_adaptive: the standard error of a pixel's mean must fall below
    # half an 8-bit step of the PNG output (write_png's `(c * 255.) as u8`) plus 1 % of its brightest channel.
    ADAPTIVE_REL_TOL = 0.01
    ADAPTIVE_ABS_TOL = 0.5 / 255.0

    @staticmethod
    def _adaptive(v, min_samples, pass_samples, rel_tol, abs_tol):
        spp, m, p = int(v.samples_per_pixel), int(min_samples), int(pass_samples)
        if spp < 2:
            raise ValueError("adaptive sampling needs samples_per_pixel >= 2")
        if not 2 <= m <= spp:
            raise ValueError("min_samples must be in [2, samples_per_pixel]")
        if p < 1:
            raise ValueError("pass_samples must be >= 1")
        return _ffi.Adaptive(m, p, float(rel_tol), float(abs_tol))

    @staticmethod
    def _adaptive_ctx(st, wall, ad):
        ctx = ProgressCtx(st.rays, wall.value, st.as_dict())
        ctx.passes, ctx.unconverged, ctx.samples = ad.passes, ad.unconverged, ad.samples
        return ctx

    def walk_rays_adaptive(self, v, s, data, min_samples=8, pass_samples=8, rel_tol=None, abs_tol=None, counts=None):
        """Adaptive sampling (rtmi_render_adaptive): v.samples_per_pixel is the most samples a pixel gets.  Every pixel gets
        samples [0, min_samples), then passes of pass_samples more until its stop rule holds (include/rtmi.h) or it reaches
        samples_per_pixel.  data ((H, W, 4) f32) receives every pixel at its own count, bit-identical to walk_rays at
        samples_per_pixel = that count.  counts (optional, (H, W) uint32) receives the count map; it is also returned as
        ctx.counts, with ctx.passes, ctx.samples (the sum of counts) and ctx.unconverged (pixels that reached
        samples_per_pixel without stopping).  abs_tol = NaN runs every pixel to samples_per_pixel (in passes), +inf stops
        every pixel at min_samples.  Defaults: ADAPTIVE_REL_TOL, ADAPTIVE_ABS_TOL."""
        if data.dtype != np.float32 or not data.flags.c_contiguous or data.size != v.height * v.width * 4:
            raise ValueError("data must be a C-contiguous float32 array of height*width*4 elements")
        if counts is None:
            counts = np.zeros((v.height, v.width), np.uint32)
        elif counts.dtype != np.uint32 or not counts.flags.c_contiguous or counts.size != v.height * v.width:
            raise ValueError("counts must be a C-contiguous uint32 array of height*width elements")
        ad = self._adaptive(v, min_samples, pass_samples, self.ADAPTIVE_REL_TOL if rel_tol is None else rel_tol,
                            self.ADAPTIVE_ABS_TOL if abs_tol is None else abs_tol)
        self._config(s)
        st = _ffi.Stats()
        wall = C.c_double(0)
        _chk(_ffi.lib().rth_caster_walk_adaptive(s.h, v.width, v.height, _p(v.vp12), v.maxdepth, v.samples_per_pixel, 0, v.height,
                                                 C.byref(ad), _p(data), _p(counts), C.byref(st), C.byref(wall)))
        ctx = self._adaptive_ctx(st, wall, ad)
        ctx.counts = counts
        return ctx

    def walk_adaptive_device(self, v, s, tile, accum_ptr, sumsq_ptr, counts_ptr, out_ptr=None, stream_ptr=None, min_samples=8,
                             pass_samples=8, rel_tol=None, abs_tol=None):
        """The same on device memory (rtmi_render_adaptive_device) for a striped row set tile = (row0, nrows, stripe_rows,
        stripe_step), enqueued on HIP stream `stream_ptr`: accum / sumsq (one float4 per pixel of the tile), counts (one
        uint32 per pixel) and out (optional) stay on the device.  Returns ctx with passes, unconverged and samples."""
        ad = self._adaptive(v, min_samples, pass_samples, self.ADAPTIVE_REL_TOL if rel_tol is None else rel_tol,
                            self.ADAPTIVE_ABS_TOL if abs_tol is None else abs_tol)
        self._config(s)
        st = _ffi.Stats()
        wall = C.c_double(0)
        t = _ffi.Tile(*[int(x) for x in tile])
        _chk(_ffi.lib().rth_caster_walk_adaptive_device(s.h, v.width, v.height, _p(v.vp12), v.maxdepth, v.samples_per_pixel,
                                                        C.byref(t), C.byref(ad), C.c_void_p(accum_ptr), C.c_void_p(sumsq_ptr),
                                                        C.c_void_p(counts_ptr), C.c_void_p(out_ptr or 0),
                                                        C.c_void_p(stream_ptr or 0), C.byref(st), C.byref(wall)))
        return self._adaptive_ctx(st, wall, ad)

    def _views(self, views, seeds):
        """(count, view 0, vp12s, seeds) of a batch of views: vp12s is (count, 12) float32, seeds (count,) uint64.  Raises
        ValueError on an empty or mismatched batch."""
        views = list(views)
        if not views:
            raise ValueError("views must hold at least one Viewport")
        v0 = views[0]
        for k, v in enumerate(views):
            if (v.width, v.height, v.maxdepth, v.samples_per_pixel) != (v0.width, v0.height, v0.maxdepth, v0.samples_per_pixel):
                raise ValueError(f"view {k}: width, height, maxdepth and samples_per_pixel must equal view 0's")
        seeds = [self.seed] * len(views) if seeds is None else [int(x) for x in seeds]
        if len(seeds) != len(views):
            raise ValueError("seeds must hold one seed per view")
        vp12s = np.ascontiguousarray(np.stack([np.asarray(v.vp12, np.float32).reshape(12) for v in views]))
        return len(views), v0, vp12s, np.asarray(seeds, np.uint64)

    def walk_rays_views(self, views, s, data=None, seeds=None):
        """A batch of views of one scene in one call (rtmi_render_views): views[k] (a Viewport) with seeds[k] (default
        self.seed for every view) renders data[k] ((K, H, W, 4) float32; allocated when None, returned as ctx.data), the
        bits walk_rays of that view and seed would give.  The views share width, height, maxdepth and samples_per_pixel.
        Returns a ProgressCtx over the whole batch.  Records of views are out of scope: s.debug_en raises."""
        n, v0, vp12s, sd = self._views(views, seeds)
        if s.debug_en:
            raise ValueError("per-ray records (Scene.debug_en) are not available for batches of views")
        if data is None:
            data = np.zeros((n, v0.height, v0.width, 4), np.float32)
        elif data.dtype != np.float32 or not data.flags.c_contiguous or data.shape != (n, v0.height, v0.width, 4):
            raise ValueError("data must be a C-contiguous float32 array of shape (K, H, W, 4)")
        self._config(s)
        st = _ffi.Stats()
        wall = C.c_double(0)
        _chk(_ffi.lib().rth_caster_walk_views(s.h, n, v0.width, v0.height, _p(vp12s), v0.maxdepth, v0.samples_per_pixel, _p(sd),
                                              _p(data), C.byref(st), C.byref(wall)))
        ctx = ProgressCtx(st.rays, wall.value, st.as_dict())
        ctx.data = data
        return ctx

    def walk_views_device(self, views, s, tile, out_ptr, stream_ptr=None, seeds=None):
        """The same on device memory (rtmi_render_views_device): the rows tile = (row0, nrows, stripe_rows, stripe_step) of
        the stacked image (K * H rows, row k * H + r = row r of view k) into nrows * width float4 at out_ptr, enqueued on
        HIP stream stream_ptr."""
        n, v0, vp12s, sd = self._views(views, seeds)
        self._config(s)
        st = _ffi.Stats()
        wall = C.c_double(0)
        t = _ffi.Tile(*[int(x) for x in tile])
        _chk(_ffi.lib().rth_caster_walk_views_device(s.h, n, v0.width, v0.height, _p(vp12s), v0.maxdepth, v0.samples_per_pixel,
                                                     _p(sd), C.byref(t), C.c_void_p(out_ptr), C.c_void_p(stream_ptr or 0),
                                                     C.byref(st), C.byref(wall)))
        return ProgressCtx(st.rays, wall.value, st.as_dict())

    @staticmethod
    def _feature_samples(v, sample0, nsamples):
        spp, k0 = int(v.samples_per_pixel), int(sample0)
        n = spp - k0 if nsamples is None else int(nsamples)
        if n < 1:
            raise ValueError("nsamples must be >= 1")
        if k0 < 0 or k0 + n > spp:
            raise ValueError("samples [sample0, sample0 + nsamples) must lie inside the frame's samples_per_pixel")
        return k0, n

    def walk_rays_features(self, v, s, sample0=0, nsamples=None, albedo=None, normal=None, ids=None):
        """First-hit feature buffers of the whole frame (rtmi_render_features): the means over samples [sample0, sample0 +
        nsamples) (default: all from sample0) of the PRIMARY rays' (albedo.rgb, coverage) -> albedo and (normal.xyz, depth)
        -> normal, both (H, W, 4) float32, and ids (H, W) uint32 = tri | face << 30 of every pixel's sample `sample0` (0 = a
        miss).  The rays are walk_rays' own (same seed, same jitter); v.maxdepth is not used.  The mean normal is not
        renormalised; the mean depth of the samples that hit is normal[..., 3] / albedo[..., 3] where coverage is non-zero.
        Each buffer: None allocates it, False leaves it out (not all three), an array is filled in place.
        Returns (albedo, normal, ids, ctx), None for a buffer left out."""
        k0, n = self._feature_samples(v, sample0, nsamples)
        bufs = []
        for name, a, shape, dt in (("albedo", albedo, (v.height, v.width, 4), np.float32), ("normal", normal, (v.height, v.width, 4), np.float32),
                                   ("ids", ids, (v.height, v.width), np.uint32)):
            if a is None:
                a = np.zeros(shape, dt)
            elif a is False:
                a = None
            elif not isinstance(a, np.ndarray) or a.dtype != dt or not a.flags.c_contiguous or a.shape != shape:
                raise ValueError(f"{name} must be a C-contiguous {np.dtype(dt).name} array of shape {shape}")
            bufs.append(a)
        if all(a is None for a in bufs):
            raise ValueError("at least one of albedo, normal and ids must be produced")
        self._config(s)
        st = _ffi.Stats()
        wall = C.c_double(0)
        _chk(_ffi.lib().rth_caster_walk_features(s.h, v.width, v.height, _p(v.vp12), v.maxdepth, v.samples_per_pixel, 0, v.height, k0, n,
                                                 *[_p(a) if a is not None else None for a in bufs], C.byref(st), C.byref(wall)))
        return bufs[0], bufs[1], bufs[2], ProgressCtx(st.rays, wall.value, st.as_dict())

    def walk_features_device(self, v, s, tile, albedo_ptr, normal_ptr, ids_ptr, sample0=0, nsamples=None, stream_ptr=None):
        """The same on device memory (rtmi_render_features_device) for a striped row set tile = (row0, nrows, stripe_rows,
        stripe_step), enqueued on HIP stream `stream_ptr`: albedo / normal are nrows*width float4, ids nrows*width uint32; a
        pointer of None/0 leaves that buffer out (not all three).  No host copies."""
        k0, n = self._feature_samples(v, sample0, nsamples)
        ptrs = [int(p or 0) for p in (albedo_ptr, normal_ptr, ids_ptr)]
        if not any(ptrs):
            raise ValueError("at least one of albedo_ptr, normal_ptr and ids_ptr must be given")
        if len({p for p in ptrs if p}) != sum(1 for p in ptrs if p):
            raise ValueError("albedo_ptr, normal_ptr and ids_ptr must be different buffers")
        self._config(s)
        st = _ffi.Stats()
        wall = C.c_double(0)
        t = _ffi.Tile(*[int(x) for x in tile])
        _chk(_ffi.lib().rth_caster_walk_features_device(s.h, v.width, v.height, _p(v.vp12), v.maxdepth, v.samples_per_pixel,
                                                        C.byref(t), k0, n, C.c_void_p(ptrs[0]), C.c_void_p(ptrs[1]), C.c_void_p(ptrs[2]),
                                                        C.c_void_p(stream_ptr or 0), C.byref(st), C.byref(wall)))
        return ProgressCtx(st.rays, wall.value, st.as_dict())

    CAMERA_MODELS = {"pinhole": _ffi.CAMERA_PINHOLE, "thin_lens": _ffi.CAMERA_THIN_LENS, "ortho": _ffi.CAMERA_ORTHO}

    @staticmethod
    def camera_params(v, model="pinhole", aperture=0.0, focus_distance=None):
        """rtmi_camera_t for viewport v (include/rtmi.h defines the models).  model: "pinhole" (the reference's camera),
        "thin_lens" or "ortho".  aperture: the radius of the lens in world units.  focus_distance: the distance from the eye,
        along the camera's axis, of the plane that is in focus, in world units (None: the image plane itself); it becomes
        rtmi_camera_t.focus = focus_distance / |c - cam| with c the centre of the image plane, computed in float64 and rounded
        once.  Both are ignored by the pinhole and the orthographic camera."""
        if model not in HipRayCaster.CAMERA_MODELS:
            raise ValueError(f"model must be one of {sorted(HipRayCaster.CAMERA_MODELS)}")
        cam = _ffi.Camera()
        _ffi.lib().rtmi_camera_defaults(C.byref(cam))
        cam.model = HipRayCaster.CAMERA_MODELS[model]
        if model == "thin_lens":
            cam.lens_radius = float(aperture)
            if focus_distance is not None:
                vp = np.asarray(v.vp12, np.float64)
                c = vp[0:3] + 0.5 * vp[6:9] + 0.5 * vp[9:12]
                cam.focus = float(focus_distance) / float(np.sqrt(((c - vp[3:6]) ** 2).sum()))
        return cam

    @staticmethod
    def _camera_guides(guides, shape4, shape1):
        """(albedo, normal, ids) as given to a camera call -> arrays or None: None / False leaves a buffer out, True allocates it."""
        out = []
        for name, a, shape, dt in (("albedo", guides[0], shape4, np.float32), ("normal", guides[1], shape4, np.float32),
                                   ("ids", guides[2], shape1, np.uint32)):
            if a is None or a is False:
                a = None
            elif a is True:
                a = np.zeros(shape, dt)
            elif not isinstance(a, np.ndarray) or a.dtype != dt or not a.flags.c_contiguous or a.size != int(np.prod(shape)):
                raise ValueError(f"{name} must be a C-contiguous {np.dtype(dt).name} array of {int(np.prod(shape))} elements")
            out.append(a)
        return out

    def walk_samples_camera(self, v, s, row0, nrows, camera, sample0, nsamples, accum, out=None, albedo=None, normal=None, ids=None):
        """walk_samples through a built-in camera model (rtmi_render_camera): samples [sample0, sample0 + nsamples) of rows
        [row0, row0 + nrows) with the rays of `camera` (camera_params).  accum / out as in walk_samples.  albedo, normal
        (nrows*width*4 f32) and ids (nrows*width u32): the feature buffers of THIS call's samples, traced with the same rays;
        None leaves one out, True allocates it.  Returns ctx; ctx.albedo / .normal / .ids are the guide arrays (or None)."""
        for name, a in (("accum", accum), ("out", out)):
            if a is not None and (a.dtype != np.float32 or not a.flags.c_contiguous or a.size != nrows * v.width * 4):
                raise ValueError(f"{name} must be a C-contiguous float32 array of nrows*width*4 elements")
        g = self._camera_guides((albedo, normal, ids), (nrows, v.width, 4), (nrows, v.width))
        go = _ffi.CameraOut(*[_p(a) if a is not None else None for a in g])
        self._config(s)
        st = _ffi.Stats()
        wall = C.c_double(0)
        _chk(_ffi.lib().rth_caster_walk_camera(s.h, v.width, v.height, _p(v.vp12), v.maxdepth, v.samples_per_pixel, row0, nrows,
                                               C.byref(camera), sample0, nsamples, _p(accum), _p(out) if out is not None else None,
                                               C.byref(go) if any(a is not None for a in g) else None, C.byref(st), C.byref(wall)))
        ctx = ProgressCtx(st.rays, wall.value, st.as_dict())
        ctx.albedo, ctx.normal, ctx.ids = g
        return ctx

    def walk_rays_camera(self, v, s, data, camera, pass_samples=None, albedo=None, normal=None, ids=None):
        """walk_rays through a built-in camera model: the whole frame, all v.samples_per_pixel samples, in passes of
        `pass_samples` samples (None: one pass) like walk_rays_progressive; `data` ((H, W, 4) f32) ends as the image, the same
        bits whatever the passes.  albedo / normal / ids (None: left out, True: allocated, or an array to fill): the feature
        buffers of the FIRST pass's samples (all samples with one pass).  Returns a ProgressCtx with the total rays, summed
        stats, samples_done, accum and the guide arrays as .albedo / .normal / .ids."""
        if data.dtype != np.float32 or not data.flags.c_contiguous or data.size != v.height * v.width * 4:
            raise ValueError("data must be a C-contiguous float32 array of height*width*4 elements")
        spp = int(v.samples_per_pixel)
        step = spp if pass_samples is None else int(pass_samples)
        if step < 1:
            raise ValueError("pass_samples must be >= 1")
        g = self._camera_guides((albedo, normal, ids), (v.height, v.width, 4), (v.height, v.width))
        accum = np.zeros_like(data)
        ctx = ProgressCtx(0, 0.0, None)
        ctx.samples_done, ctx.accum = 0, accum
        ctx.albedo, ctx.normal, ctx.ids = g
        for k0 in range(0, spp, step):
            n = min(step, spp - k0)
            p = self.walk_samples_camera(v, s, 0, v.height, camera, k0, n, accum, data, *(g if k0 == 0 else (None, None, None)))
            ctx.total_rays += p.total_rays
            ctx.seconds += p.seconds
            if ctx.stats is None:
                ctx.stats = dict(p.stats)
            else:
                for k in ("rays", "box_tests", "tri_tests", "full_tests", "nodes", "leaves", "kernel_ms", "trace_ms", "trace_launches",
                          "primary_ms", "bounce_ms", "slow_paths"):
                    ctx.stats[k] += p.stats[k]
            ctx.samples_done = k0 + n
        return ctx

    def walk_rays_camera_device(self, v, s, camera, accum, out=None, tile=None, sample0=0, nsamples=None, albedo=None, normal=None,
                                ids=None, stream=None):
        """The same on device memory (rtmi_render_camera_device) for a striped row set tile = (row0, nrows, stripe_rows,
        stripe_step) (default: the whole frame): samples [sample0, sample0 + nsamples) (default: all from sample0).  accum, out,
        albedo, normal (nrows * width float4) and ids (nrows * width uint32) are torch tensors on the scene's device or raw
        device pointers (ints); out and the guides may be None.  The work is enqueued on `stream` (a torch stream, a raw HIP
        stream pointer or None).  No host copies.  Returns ctx."""
        k0, n = self._feature_samples(v, sample0, nsamples)
        t = _ffi.Tile(*[int(x) for x in (tile if tile is not None else (0, v.height, v.height, 0))])
        npix = int(t.nrows) * int(v.width)
        ptrs = []
        for name, x, want, dt in (("accum", accum, npix * 4, "torch.float32"), ("out", out, npix * 4, "torch.float32"),
                                  ("albedo", albedo, npix * 4, "torch.float32"), ("normal", normal, npix * 4, "torch.float32"),
                                  ("ids", ids, npix, "torch.int32")):
            if x is None:
                if name == "accum":
                    raise ValueError("accum is needed")
                ptrs.append(0)
            elif hasattr(x, "data_ptr"):
                dts = (dt, "torch.uint32") if name == "ids" else (dt,)
                if not x.is_cuda or str(x.dtype) not in dts or not x.is_contiguous() or x.numel() != want:
                    raise ValueError(f"{name} must be a contiguous {dt} tensor of {want} elements on the device")
                ptrs.append(int(x.data_ptr()))
            elif isinstance(x, int):
                ptrs.append(x)
            else:
                raise ValueError(f"{name} must be a tensor on the device or a device pointer")
        go = _ffi.CameraOut(*[C.c_void_p(p) if p else None for p in ptrs[2:]])
        self._config(s)
        st = _ffi.Stats()
        wall = C.c_double(0)
        _chk(_ffi.lib().rth_caster_walk_camera_device(s.h, v.width, v.height, _p(v.vp12), v.maxdepth, v.samples_per_pixel, C.byref(t),
                                                      C.byref(camera), k0, n, C.c_void_p(ptrs[0]), C.c_void_p(ptrs[1]),
                                                      C.byref(go) if any(ptrs[2:]) else None,
                                                      C.c_void_p(getattr(stream, "cuda_stream", stream) or 0), C.byref(st), C.byref(wall)))
        return ProgressCtx(st.rays, wall.value, st.as_dict())

    @staticmethod
    def ao_params(rays=None, radius=None, bias=None):
        """rtmi_ao_t from the library's defaults (rtmi_ao_defaults: 4 rays, radius +inf, bias 0.001) with the given fields
        replaced.  Raises ValueError for what the library would refuse."""
        a = _ffi.Ao()
        _ffi.lib().rtmi_ao_defaults(C.byref(a))
        if rays is not None:
            if not 1 <= int(rays) <= 256:
                raise ValueError("rays must be in [1, 256]")
            a.rays = int(rays)
        if radius is not None:
            if not float(radius) >= 0.0:
                raise ValueError("radius must be >= 0 (inf: unlimited) and not NaN")
            a.radius = float(radius)
        if bias is not None:
            if not np.isfinite(float(bias)):
                raise ValueError("bias must be finite")
            a.bias = float(bias)
        return a

    def _ao_args(self, v, sample0, nsamples, rays, radius, bias):
        k0, n = self._feature_samples(v, sample0, nsamples)
        a = self.ao_params(rays, radius, bias)
        if n * a.rays >= 1 << 24:
            raise ValueError("nsamples * rays must stay below 2^24")
        return k0, n, a

    def walk_rays_ao(self, v, s, rays=None, radius=None, bias=None, sample0=0, nsamples=None, out=None):
        """Ambient occlusion of the whole frame (rtmi_render_ao; include/rtmi.h defines it): (H, W) float32, per pixel the
        share of `rays` hemisphere rays per primary sample of [sample0, sample0 + nsamples) (default: all from sample0) that
        are not occluded within `radius`; 1.0 where every sample missed.  The primary rays are walk_rays' own (same seed,
        same jitter); v.maxdepth is not used.  None for rays / radius / bias takes the library's default (4, inf, 0.001).
        out: None allocates it, an array is filled in place.  Returns (ao, ctx)."""
        k0, n, a = self._ao_args(v, sample0, nsamples, rays, radius, bias)
        shape = (v.height, v.width)
        if out is None:
            out = np.zeros(shape, np.float32)
        elif not isinstance(out, np.ndarray) or out.dtype != np.float32 or not out.flags.c_contiguous or out.shape != shape:
            raise ValueError(f"out must be a C-contiguous float32 array of shape {shape}")
        self._config(s)
        st = _ffi.Stats()
        wall = C.c_double(0)
        _chk(_ffi.lib().rth_caster_walk_ao(s.h, v.width, v.height, _p(v.vp12), v.maxdepth, v.samples_per_pixel, 0, v.height, k0, n,
                                           C.byref(a), _p(out), C.byref(st), C.byref(wall)))
        return out, ProgressCtx(st.rays, wall.value, st.as_dict())

    def walk_rays_ao_device(self, v, s, out, tile=None, rays=None, radius=None, bias=None, sample0=0, nsamples=None, stream=None):
        """The same into a torch tensor on the scene's device (rtmi_render_ao_device) for a striped row set tile = (row0,
        nrows, stripe_rows, stripe_step) (default: the whole frame): `out` is a contiguous float32 tensor of nrows * width
        elements, written by work enqueued on `stream` (a torch stream, a raw HIP stream pointer or None).  Returns ctx."""
        k0, n, a = self._ao_args(v, sample0, nsamples, rays, radius, bias)
        t = _ffi.Tile(*[int(x) for x in (tile if tile is not None else (0, v.height, v.height, 0))])
        want = int(t.nrows) * int(v.width)
        if not hasattr(out, "data_ptr") or not out.is_cuda or str(out.dtype) != "torch.float32" or not out.is_contiguous() or out.numel() != want:
            raise ValueError(f"out must be a contiguous float32 tensor of {want} elements on the device")
        self._config(s)
        st = _ffi.Stats()
        wall = C.c_double(0)
        _chk(_ffi.lib().rth_caster_walk_ao_device(s.h, v.width, v.height, _p(v.vp12), v.maxdepth, v.samples_per_pixel, C.byref(t), k0, n,
                                                  C.byref(a), C.c_void_p(out.data_ptr()), C.c_void_p(getattr(stream, "cuda_stream", stream) or 0),
                                                  C.byref(st), C.byref(wall)))
        return ProgressCtx(st.rays, wall.value, st.as_dict())

    LIGHT_UNBOUNDED = 1

    @staticmethod
    def light_params(orig=None, len2=None, rays=None, unbounded=False, bias=None):
        """rtmi_light_t from the library's defaults (rtmi_light_defaults: orig (0, 0, 0), len2 0, 4 rays, bounded, bias 0.005)
        with the given fields replaced.  Raises ValueError for what the library would refuse."""
        a = _ffi.Light()
        _ffi.lib().rtmi_light_defaults(C.byref(a))
        if orig is not None:
            o = [float(x) for x in orig]
            if len(o) != 3 or not all(np.isfinite(x) for x in o):
                raise ValueError("orig must be three finite numbers")
            a.orig[0], a.orig[1], a.orig[2] = o
        if len2 is not None:
            if not float(len2) >= 0.0 or not np.isfinite(float(len2)):
                raise ValueError("len2 must be >= 0, finite and not NaN")
            a.len2 = float(len2)
        if rays is not None:
            if not 1 <= int(rays) <= 256:
                raise ValueError("rays must be in [1, 256]")
            a.rays = int(rays)
        if unbounded:
            a.flags = HipRayCaster.LIGHT_UNBOUNDED
        if bias is not None:
            if not np.isfinite(float(bias)):
                raise ValueError("bias must be finite")
            a.bias = float(bias)
        return a

    def _light_args(self, v, sample0, nsamples, orig, len2, rays, unbounded, bias):
        k0, n = self._feature_samples(v, sample0, nsamples)
        a = self.light_params(orig, len2, rays, unbounded, bias)
        if n * a.rays >= 1 << 24:
            raise ValueError("nsamples * rays must stay below 2^24")
        return k0, n, a

    def walk_rays_light(self, v, s, orig=None, len2=None, rays=None, unbounded=False, bias=None, sample0=0, nsamples=None,
                        shadow=True, irradiance=True):
        """Direct light of the whole frame from one box light (rtmi_render_light; include/rtmi.h defines it): two (H, W)
        float32 planes.  shadow: per pixel the share of `rays` samples of the light (corner `orig`, edge `len2`; 0 = a point
        light) per primary sample of [sample0, sample0 + nsamples) (default: all from sample0) that are visible from the first
        hit, 1.0 where every sample missed.  irradiance: the mean of n . dir over those visible samples.  unbounded: anything
        along the shadow ray shadows, even beyond the light.  The primary rays are walk_rays' own (same seed, same jitter);
        v.maxdepth is not used.  None takes the library's default.  shadow / irradiance: True allocates the plane, an array
        is filled in place, False / None leaves it out (not both).  Returns (shadow, irradiance, ctx)."""
        k0, n, a = self._light_args(v, sample0, nsamples, orig, len2, rays, unbounded, bias)
        shape = (v.height, v.width)
        planes = []
        for name, x in (("shadow", shadow), ("irradiance", irradiance)):
            if x is True:
                x = np.zeros(shape, np.float32)
            elif x is False or x is None:
                x = None
            elif not isinstance(x, np.ndarray) or x.dtype != np.float32 or not x.flags.c_contiguous or x.shape != shape:
                raise ValueError(f"{name} must be a C-contiguous float32 array of shape {shape}")
            planes.append(x)
        if planes[0] is None and planes[1] is None:
            raise ValueError("at least one of shadow and irradiance is needed")
        if planes[0] is not None and planes[1] is not None and np.shares_memory(planes[0], planes[1]):
            raise ValueError("shadow and irradiance must not alias")
        self._config(s)
        st = _ffi.Stats()
        wall = C.c_double(0)
        ptr = [_p(x) if x is not None else None for x in planes]
        _chk(_ffi.lib().rth_caster_walk_light(s.h, v.width, v.height, _p(v.vp12), v.maxdepth, v.samples_per_pixel, 0, v.height, k0, n,
                                              C.byref(a), ptr[0], ptr[1], C.byref(st), C.byref(wall)))
        return planes[0], planes[1], ProgressCtx(st.rays, wall.value, st.as_dict())

    def walk_rays_light_device(self, v, s, shadow, irradiance, tile=None, orig=None, len2=None, rays=None, unbounded=False, bias=None,
                               sample0=0, nsamples=None, stream=None):
        """The same into torch tensors on the scene's device (rtmi_render_light_device) for a striped row set tile = (row0,
        nrows, stripe_rows, stripe_step) (default: the whole frame): `shadow` and `irradiance` are contiguous float32 tensors
        of nrows * width elements each (either may be None, not both, and they must not overlap), written by work enqueued on
        `stream` (a torch stream, a raw HIP stream pointer or None).  Returns ctx."""
        k0, n, a = self._light_args(v, sample0, nsamples, orig, len2, rays, unbounded, bias)
        t = _ffi.Tile(*[int(x) for x in (tile if tile is not None else (0, v.height, v.height, 0))])
        want = int(t.nrows) * int(v.width)
        if shadow is None and irradiance is None:
            raise ValueError("at least one of shadow and irradiance is needed")
        for name, x in (("shadow", shadow), ("irradiance", irradiance)):
            if x is not None and (not hasattr(x, "data_ptr") or not x.is_cuda or str(x.dtype) != "torch.float32" or not x.is_contiguous()
                                  or x.numel() != want):
                raise ValueError(f"{name} must be a contiguous float32 tensor of {want} elements on the device")
        if shadow is not None and irradiance is not None and abs(shadow.data_ptr() - irradiance.data_ptr()) < 4 * want:
            raise ValueError("shadow and irradiance must not overlap")
        self._config(s)
        st = _ffi.Stats()
        wall = C.c_double(0)
        ptr = [C.c_void_p(x.data_ptr()) if x is not None else None for x in (shadow, irradiance)]
        _chk(_ffi.lib().rth_caster_walk_light_device(s.h, v.width, v.height, _p(v.vp12), v.maxdepth, v.samples_per_pixel, C.byref(t), k0, n,
                                                     C.byref(a), ptr[0], ptr[1], C.c_void_p(getattr(stream, "cuda_stream", stream) or 0),
                                                     C.byref(st), C.byref(wall)))
        return ProgressCtx(st.rays, wall.value, st.as_dict())

    def _shadowed_args(self, v, sample0, nsamples, orig, len2, unbounded, bias):
        k0, n = self._feature_samples(v, sample0, nsamples)
        if orig is None:
            raise ValueError("orig (the light's corner) is needed")
        return k0, n, self.light_params(orig, len2, 1, unbounded, bias)

    def walk_rays_shadowed(self, v, s, data=None, orig=None, len2=None, unbounded=False, bias=None, sample0=0, nsamples=None, accum=None):
        """Path tracing of the whole frame with the reference's shadow rays switched on (rtmi_render_shadowed; include/rtmi.h
        defines it): walk_rays' paths, with every surface hit of every bounce tested against one box light (corner `orig`,
        edge `len2`; 0 = a point light; one shadow ray per hit) and shown black where it is shadowed.  Samples [sample0,
        sample0 + nsamples) (default: all from sample0) of the frame's v.samples_per_pixel; accum ((H, W, 4) float32, None
        allocates it) holds the running per-pixel sums as in walk_samples: read when sample0 > 0, always rewritten.  data
        ((H, W, 4) float32, None allocates it) receives accum * (1 / (sample0 + nsamples)): the image once every sample is in.
        unbounded: anything along a shadow ray shadows, even beyond the light.  Returns (data, ctx); ctx.accum is the sums."""
        k0, n, a = self._shadowed_args(v, sample0, nsamples, orig, len2, unbounded, bias)
        shape = (v.height, v.width, 4)
        bufs = []
        for name, x in (("data", data), ("accum", accum)):
            if x is None:
                x = np.zeros(shape, np.float32)
            elif not isinstance(x, np.ndarray) or x.dtype != np.float32 or not x.flags.c_contiguous or x.size != v.height * v.width * 4:
                raise ValueError(f"{name} must be a C-contiguous float32 array of height*width*4 elements")
            bufs.append(x)
        if np.shares_memory(bufs[0], bufs[1]):
            raise ValueError("data and accum must not alias")
        if k0 > 0 and accum is None:
            raise ValueError("sample0 > 0 continues the sums of the earlier samples: pass their accum")
        self._config(s)
        st = _ffi.Stats()
        wall = C.c_double(0)
        _chk(_ffi.lib().rth_caster_walk_shadowed(s.h, v.width, v.height, _p(v.vp12), v.maxdepth, v.samples_per_pixel, 0, v.height, k0, n,
                                                 C.byref(a), _p(bufs[1]), _p(bufs[0]), C.byref(st), C.byref(wall)))
        ctx = ProgressCtx(st.rays, wall.value, st.as_dict())
        ctx.accum = bufs[1]
        return bufs[0], ctx

    def walk_rays_shadowed_device(self, v, s, accum, out=None, tile=None, orig=None, len2=None, unbounded=False, bias=None, sample0=0,
                                  nsamples=None, stream=None):
        """The same on torch tensors on the scene's device (rtmi_render_shadowed_device) for a striped row set tile = (row0,
        nrows, stripe_rows, stripe_step) (default: the whole frame): `accum` and `out` (may be None: no preview) are contiguous
        float32 tensors of nrows * width * 4 elements that do not overlap, read and written by work enqueued on `stream` (a
        torch stream, a raw HIP stream pointer or None).  Returns ctx."""
        k0, n, a = self._shadowed_args(v, sample0, nsamples, orig, len2, unbounded, bias)
        t = _ffi.Tile(*[int(x) for x in (tile if tile is not None else (0, v.height, v.height, 0))])
        want = int(t.nrows) * int(v.width) * 4
        for name, x in (("accum", accum), ("out", out)):
            if (x is not None or name == "accum") and (not hasattr(x, "data_ptr") or not x.is_cuda or str(x.dtype) != "torch.float32"
                                                       or not x.is_contiguous() or x.numel() != want):
                raise ValueError(f"{name} must be a contiguous float32 tensor of {want} elements on the device")
        if out is not None and abs(accum.data_ptr() - out.data_ptr()) < 4 * want:
            raise ValueError("accum and out must not overlap")
        self._config(s)
        st = _ffi.Stats()
        wall = C.c_double(0)
        _chk(_ffi.lib().rth_caster_walk_shadowed_device(s.h, v.width, v.height, _p(v.vp12), v.maxdepth, v.samples_per_pixel, C.byref(t), k0, n,
                                                        C.byref(a), C.c_void_p(accum.data_ptr()), C.c_void_p(out.data_ptr() if out is not None else 0),
                                                        C.c_void_p(getattr(stream, "cuda_stream", stream) or 0), C.byref(st), C.byref(wall)))
        return ProgressCtx(st.rays, wall.value, st.as_dict())

    @staticmethod
    def envlight_params(bias=None):
        """rtmi_envlight_t from the library's defaults (bias 0.001) with the given field replaced; ValueError for what the library
        would refuse"""
        a = _ffi.Envlight()
        _ffi.lib().rtmi_envlight_defaults(C.byref(a))
        if bias is not None:
            if not np.isfinite(float(bias)):
                raise ValueError("bias must be finite")
            a.bias = float(bias)
        return a

    def walk_rays_envlight(self, v, s, data=None, bias=None, sample0=0, nsamples=None, accum=None):
        """Path tracing of the whole frame with the scene's environment sampled at every Matte hit that bounces
        (rtmi_render_envlight; include/rtmi.h defines it): walk_rays' paths and, in expectation, walk_rays' image of a scene with
        an environment, with less noise where a small bright region of the map lights matte surfaces.  Samples [sample0, sample0 +
        nsamples) (default: all from sample0) of the frame's v.samples_per_pixel; data and accum as in walk_rays_shadowed.  bias:
        the offset of a shadow ray's origin along the bounce vector (default 0.001, the reference's own for a bounce ray: any other
        value is biased against walk_rays).
        Returns (data, ctx); ctx.accum is the sums."""
        k0, n = self._feature_samples(v, sample0, nsamples)
        a = self.envlight_params(bias)
        shape = (v.height, v.width, 4)
        bufs = []
        for name, x in (("data", data), ("accum", accum)):
            if x is None:
                x = np.zeros(shape, np.float32)
            elif not isinstance(x, np.ndarray) or x.dtype != np.float32 or not x.flags.c_contiguous or x.size != v.height * v.width * 4:
                raise ValueError(f"{name} must be a C-contiguous float32 array of height*width*4 elements")
            bufs.append(x)
        if np.shares_memory(bufs[0], bufs[1]):
            raise ValueError("data and accum must not alias")
        if k0 > 0 and accum is None:
            raise ValueError("sample0 > 0 continues the sums of the earlier samples: pass their accum")
        self._config(s)
        st = _ffi.Stats()
        wall = C.c_double(0)
        _chk(_ffi.lib().rth_caster_walk_envlight(s.h, v.width, v.height, _p(v.vp12), v.maxdepth, v.samples_per_pixel, 0, v.height, k0, n,
                                                 C.byref(a), _p(bufs[1]), _p(bufs[0]), C.byref(st), C.byref(wall)))
        ctx = ProgressCtx(st.rays, wall.value, st.as_dict())
        ctx.accum = bufs[1]
        return bufs[0], ctx

    def walk_rays_envlight_device(self, v, s, accum, out=None, tile=None, bias=None, sample0=0, nsamples=None, stream=None):
        """The same on torch tensors on the scene's device (rtmi_render_envlight_device) for a striped row set tile = (row0,
        nrows, stripe_rows, stripe_step) (default: the whole frame); accum, out and stream as in walk_rays_shadowed_device.
        Returns ctx."""
        k0, n = self._feature_samples(v, sample0, nsamples)
        a = self.envlight_params(bias)
        t = _ffi.Tile(*[int(x) for x in (tile if tile is not None else (0, v.height, v.height, 0))])
        want = int(t.nrows) * int(v.width) * 4
        for name, x in (("accum", accum), ("out", out)):
            if (x is not None or name == "accum") and (not hasattr(x, "data_ptr") or not x.is_cuda or str(x.dtype) != "torch.float32"
                                                       or not x.is_contiguous() or x.numel() != want):
                raise ValueError(f"{name} must be a contiguous float32 tensor of {want} elements on the device")
        if out is not None and abs(accum.data_ptr() - out.data_ptr()) < 4 * want:
            raise ValueError("accum and out must not overlap")
        self._config(s)
        st = _ffi.Stats()
        wall = C.c_double(0)
        _chk(_ffi.lib().rth_caster_walk_envlight_device(s.h, v.width, v.height, _p(v.vp12), v.maxdepth, v.samples_per_pixel, C.byref(t), k0, n,
                                                        C.byref(a), C.c_void_p(accum.data_ptr()), C.c_void_p(out.data_ptr() if out is not None else 0),
                                                        C.c_void_p(getattr(stream, "cuda_stream", stream) or 0), C.byref(st), C.byref(wall)))
        return ProgressCtx(st.rays, wall.value, st.as_dict())

    def env_sampler(self, s):
        """The sampler table of the scene's environment as the first device holds it (rtmi_scene_get_env_sampler): (q (n, n) uint32,
        total), or None when the scene has no environment.  Uploads, and builds the table, if need be."""
        self._config(s)
        n = C.c_uint32(0)
        _chk(_ffi.lib().rth_scene_environment_size(s.h, C.byref(n)))
        if n.value == 0:
            return None
        q = np.zeros((n.value, n.value), np.uint32)
        total = C.c_uint64(0)
        _chk(_ffi.lib().rth_caster_env_sampler(s.h, _p(q), q.size, C.byref(total), C.byref(n)))
        return q, int(total.value)

    def walk_rays_emissive(self, v, s, data=None, sample0=0, nsamples=None, accum=None):
        """Path tracing of the whole frame with the scene's lamps (Scene.set_emitters) sampled at every Matte hit that bounces
        (rtmi_render_emissive; include/rtmi.h defines it): walk_rays' paths and, in expectation, walk_rays' image, with less noise
        where small bright Solid triangles light matte surfaces.  Samples [sample0, sample0 + nsamples) (default: all from sample0)
        of the frame's v.samples_per_pixel; data and accum as in walk_rays_shadowed.
        Returns (data, ctx); ctx.accum is the sums."""
        k0, n = self._feature_samples(v, sample0, nsamples)
        shape = (v.height, v.width, 4)
        bufs = []
        for name, x in (("data", data), ("accum", accum)):
            if x is None:
                x = np.zeros(shape, np.float32)
            elif not isinstance(x, np.ndarray) or x.dtype != np.float32 or not x.flags.c_contiguous or x.size != v.height * v.width * 4:
                raise ValueError(f"{name} must be a C-contiguous float32 array of height*width*4 elements")
            bufs.append(x)
        if np.shares_memory(bufs[0], bufs[1]):
            raise ValueError("data and accum must not alias")
        if k0 > 0 and accum is None:
            raise ValueError("sample0 > 0 continues the sums of the earlier samples: pass their accum")
        self._config(s)
        st = _ffi.Stats()
        wall = C.c_double(0)
        _chk(_ffi.lib().rth_caster_walk_emissive(s.h, v.width, v.height, _p(v.vp12), v.maxdepth, v.samples_per_pixel, 0, v.height, k0, n,
                                                 _p(bufs[1]), _p(bufs[0]), C.byref(st), C.byref(wall)))
        ctx = ProgressCtx(st.rays, wall.value, st.as_dict())
        ctx.accum = bufs[1]
        return bufs[0], ctx

    def walk_rays_emissive_device(self, v, s, accum, out=None, tile=None, sample0=0, nsamples=None, stream=None):
        """The same on torch tensors on the scene's device (rtmi_render_emissive_device) for a striped row set tile = (row0,
        nrows, stripe_rows, stripe_step) (default: the whole frame); accum, out and stream as in walk_rays_shadowed_device.
        Returns ctx."""
        k0, n = self._feature_samples(v, sample0, nsamples)
        t = _ffi.Tile(*[int(x) for x in (tile if tile is not None else (0, v.height, v.height, 0))])
        want = int(t.nrows) * int(v.width) * 4
        for name, x in (("accum", accum), ("out", out)):
            if (x is not None or name == "accum") and (not hasattr(x, "data_ptr") or not x.is_cuda or str(x.dtype) != "torch.float32"
                                                       or not x.is_contiguous() or x.numel() != want):
                raise ValueError(f"{name} must be a contiguous float32 tensor of {want} elements on the device")
        if out is not None and abs(accum.data_ptr() - out.data_ptr()) < 4 * want:
            raise ValueError("accum and out must not overlap")
        self._config(s)
        st = _ffi.Stats()
        wall = C.c_double(0)
        _chk(_ffi.lib().rth_caster_walk_emissive_device(s.h, v.width, v.height, _p(v.vp12), v.maxdepth, v.samples_per_pixel, C.byref(t), k0, n,
                                                        C.c_void_p(accum.data_ptr()), C.c_void_p(out.data_ptr() if out is not None else 0),
                                                        C.c_void_p(getattr(stream, "cuda_stream", stream) or 0), C.byref(st), C.byref(wall)))
        return ProgressCtx(st.rays, wall.value, st.as_dict())

    def emitter_sampler(self, s):
        """The lamps' tables of the scene as the first device holds them (rtmi_scene_get_emitter_sampler): a namespace q (L,) uint32,
        cum (L,) uint64, lamp_of_tri (ntris,) uint32 (0 = not a lamp), lamps (L, 5, 4) float32 -- (c0, A), (e1, w), (e2, 0), (n, 0),
        (radiance, 0) -- and total, or None when the scene has no lamps.  Uploads, and builds the tables, if need be."""
        self._config(s)
        n, total = C.c_uint32(0), C.c_uint64(0)
        _chk(_ffi.lib().rth_caster_emitter_sampler(s.h, None, None, None, None, 0, 0, C.byref(total), C.byref(n)))
        if n.value == 0:
            return None
        L, nt = n.value, s.num_tris()
        q, cum, idx, lamps = np.zeros(L, np.uint32), np.zeros(L, np.uint64), np.zeros(nt, np.uint32), np.zeros((L, 5, 4), np.float32)
        _chk(_ffi.lib().rth_caster_emitter_sampler(s.h, _p(q), _p(cum), _p(idx), _p(lamps), L, nt, C.byref(total), C.byref(n)))
        return SimpleNamespace(q=q, cum=cum, lamp_of_tri=idx, lamps=lamps, total=int(total.value))

    LIT_MAX_LIGHTS = _ffi.LIT_MAX_LIGHTS
    LIT_INVERSE_SQUARE = _ffi.LIT_INVERSE_SQUARE
    LIT_SURFACES = _ffi.LIT_SURFACES

    @staticmethod
    def lit_params(lights=(), inverse_square=False, surfaces=False):
        """rtmi_lit_t from the library's defaults (rtmi_lit_defaults: no lights, white, one ray each) with the given lights: up to
        four dicts of orig, len2, bias (light_params' arguments), color = three finite numbers (default white) and either
        unbounded=True or flags=LIGHT_UNBOUNDED, as preview_params takes them (one shadow ray per light and hit: no rays key).
        inverse_square: the light's cosine is divided by the squared distance.  surfaces: RTMI_LIT_SURFACES, the call takes scenes
        with a dielectric, vertex normals, textures and normal maps (include/rtmi.h "BOX LIGHTS ON SHADED SURFACES"); every lit
        call that is given the result carries it.  Raises ValueError for what the library would refuse."""
        p = _ffi.Lit()
        _ffi.lib().rtmi_lit_defaults(C.byref(p))
        lights = list(lights)
        if len(lights) > HipRayCaster.LIT_MAX_LIGHTS:
            raise ValueError(f"at most {HipRayCaster.LIT_MAX_LIGHTS} lights")
        for l, li in enumerate(lights):
            kw = dict(li)
            unknown = set(kw) - {"orig", "len2", "unbounded", "flags", "bias", "color"}
            if unknown:
                raise ValueError(f"light {l}: unknown keys {sorted(unknown)}")
            col = kw.pop("color", None)
            flags = kw.pop("flags", None)
            if flags is not None:
                if int(flags) & ~HipRayCaster.LIGHT_UNBOUNDED:
                    raise ValueError(f"light {l}: unknown flags")
                kw["unbounded"] = bool(kw.get("unbounded")) or bool(int(flags) & HipRayCaster.LIGHT_UNBOUNDED)
            if kw.get("orig") is None:
                raise ValueError(f"light {l}: orig (the light's corner) is needed")
            try:
                p.lights[l] = HipRayCaster.light_params(rays=1, **kw)
            except ValueError as e:
                raise ValueError(f"light {l}: {e}") from None
            if col is not None:
                c = [float(x) for x in col]
                if len(c) != 3 or not all(np.isfinite(x) for x in c):
                    raise ValueError(f"light {l}: color must be three finite numbers")
                p.light_color[l][0], p.light_color[l][1], p.light_color[l][2] = c
        p.nlights = len(lights)
        p.flags = (HipRayCaster.LIT_INVERSE_SQUARE if inverse_square else 0) | (HipRayCaster.LIT_SURFACES if surfaces else 0)
        return p

    def walk_rays_lit(self, v, s, lit, data=None, sample0=0, nsamples=None, accum=None):
        """Path tracing of the whole frame with box lights sampled at every Matte hit that bounces (rtmi_render_lit; include/rtmi.h
        defines it): walk_rays' paths, and at each such hit one shadow ray per light of `lit` (lit_params' result, or its lights
        argument) whose unoccluded light is added to what the surface passes on.  Samples [sample0, sample0 + nsamples) (default:
        all from sample0) of the frame's v.samples_per_pixel; data and accum as in walk_rays_shadowed.
        Returns (data, ctx); ctx.accum is the sums."""
        k0, n = self._feature_samples(v, sample0, nsamples)
        a = lit if isinstance(lit, _ffi.Lit) else self.lit_params(lit)
        shape = (v.height, v.width, 4)
        bufs = []
        for name, x in (("data", data), ("accum", accum)):
            if x is None:
                x = np.zeros(shape, np.float32)
            elif not isinstance(x, np.ndarray) or x.dtype != np.float32 or not x.flags.c_contiguous or x.size != v.height * v.width * 4:
                raise ValueError(f"{name} must be a C-contiguous float32 array of height*width*4 elements")
            bufs.append(x)
        if np.shares_memory(bufs[0], bufs[1]):
            raise ValueError("data and accum must not alias")
        if k0 > 0 and accum is None:
            raise ValueError("sample0 > 0 continues the sums of the earlier samples: pass their accum")
        self._config(s)
        st = _ffi.Stats()
        wall = C.c_double(0)
        _chk(_ffi.lib().rth_caster_walk_lit(s.h, v.width, v.height, _p(v.vp12), v.maxdepth, v.samples_per_pixel, 0, v.height, k0, n,
                                            C.byref(a), _p(bufs[1]), _p(bufs[0]), C.byref(st), C.byref(wall)))
        ctx = ProgressCtx(st.rays, wall.value, st.as_dict())
        ctx.accum = bufs[1]
        return bufs[0], ctx

    def walk_rays_lit_device(self, v, s, lit, accum, out=None, tile=None, sample0=0, nsamples=None, stream=None):
        """The same on torch tensors on the scene's device (rtmi_render_lit_device) for a striped row set tile = (row0, nrows,
        stripe_rows, stripe_step) (default: the whole frame); accum, out and stream as in walk_rays_shadowed_device.
        Returns ctx."""
        k0, n = self._feature_samples(v, sample0, nsamples)
        a = lit if isinstance(lit, _ffi.Lit) else self.lit_params(lit)
        t = _ffi.Tile(*[int(x) for x in (tile if tile is not None else (0, v.height, v.height, 0))])
        want = int(t.nrows) * int(v.width) * 4
        for name, x in (("accum", accum), ("out", out)):
            if (x is not None or name == "accum") and (not hasattr(x, "data_ptr") or not x.is_cuda or str(x.dtype) != "torch.float32"
                                                       or not x.is_contiguous() or x.numel() != want):
                raise ValueError(f"{name} must be a contiguous float32 tensor of {want} elements on the device")
        if out is not None and abs(accum.data_ptr() - out.data_ptr()) < 4 * want:
            raise ValueError("accum and out must not overlap")
        self._config(s)
        st = _ffi.Stats()
        wall = C.c_double(0)
        _chk(_ffi.lib().rth_caster_walk_lit_device(s.h, v.width, v.height, _p(v.vp12), v.maxdepth, v.samples_per_pixel, C.byref(t), k0, n,
                                                   C.byref(a), C.c_void_p(accum.data_ptr()), C.c_void_p(out.data_ptr() if out is not None else 0),
                                                   C.c_void_p(getattr(stream, "cuda_stream", stream) or 0), C.byref(st), C.byref(wall)))
        return ProgressCtx(st.rays, wall.value, st.as_dict())

    PREVIEW_MAX_LIGHTS = _ffi.PREVIEW_MAX_LIGHTS
    _PREVIEW_OUTPUTS = ("color", "albedo", "normal", "ids", "ao", "shadow", "irradiance")  # rtmi_preview_out_t's order

    @staticmethod
    def preview_params(ambient=None, ao=None, lights=()):
        """rtmi_preview_t from the library's defaults (rtmi_preview_defaults: ambient 0.3, AO of 4 rays, no lights, white
        lights) with the given fields replaced.  ao: None keeps the default AO, False switches it off (rays = 0), a dict of
        ao_params' arguments (rays, radius, bias) replaces it; rays = 0 in the dict switches it off too.  lights: up to four
        dicts of light_params' arguments (orig, len2, rays, unbounded, bias) plus color = three finite numbers (default
        white).  Raises ValueError for what the library would refuse."""
        p = _ffi.Preview()
        _ffi.lib().rtmi_preview_defaults(C.byref(p))
        if ambient is not None:
            a = [float(x) for x in ambient]
            if len(a) != 3 or not all(np.isfinite(x) for x in a):
                raise ValueError("ambient must be three finite numbers")
            p.ambient[0], p.ambient[1], p.ambient[2] = a
        if ao is False:
            p.ao.rays = 0
        elif ao is not None:
            kw = dict(ao)
            unknown = set(kw) - {"rays", "radius", "bias"}
            if unknown:
                raise ValueError(f"ao: unknown keys {sorted(unknown)}")
            off = kw.get("rays") is not None and int(kw["rays"]) == 0
            if off:
                kw.pop("rays")
            p.ao = HipRayCaster.ao_params(**kw)
            if off:
                p.ao.rays = 0
        lights = list(lights)
        if len(lights) > HipRayCaster.PREVIEW_MAX_LIGHTS:
            raise ValueError(f"at most {HipRayCaster.PREVIEW_MAX_LIGHTS} lights")
        for l, li in enumerate(lights):
            kw = dict(li)
            unknown = set(kw) - {"orig", "len2", "rays", "unbounded", "bias", "color"}
            if unknown:
                raise ValueError(f"light {l}: unknown keys {sorted(unknown)}")
            col = kw.pop("color", None)
            try:
                p.lights[l] = HipRayCaster.light_params(**kw)
            except ValueError as e:
                raise ValueError(f"light {l}: {e}") from None
            if col is not None:
                c = [float(x) for x in col]
                if len(c) != 3 or not all(np.isfinite(x) for x in c):
                    raise ValueError(f"light {l}: color must be three finite numbers")
                p.light_color[l][0], p.light_color[l][1], p.light_color[l][2] = c
        p.nlights = len(lights)
        return p

    def _preview_args(self, v, sample0, nsamples, ambient, ao, lights, wanted):
        """(sample0, nsamples, rtmi_preview_t) after the checks the library would make; wanted: the outputs asked for, by name"""
        k0, n = self._feature_samples(v, sample0, nsamples)
        p = self.preview_params(ambient, ao, lights)
        if n * p.ao.rays >= 1 << 24 or any(n * p.lights[l].rays >= 1 << 24 for l in range(p.nlights)):
            raise ValueError("nsamples * rays must stay below 2^24")
        if not wanted:
            raise ValueError("at least one output is needed")
        if "ao" in wanted and p.ao.rays == 0:
            raise ValueError("the ao output needs AO rays")
        if ("shadow" in wanted or "irradiance" in wanted) and p.nlights == 0:
            raise ValueError("the shadow and irradiance outputs need at least one light")
        return k0, n, p

    def walk_rays_preview(self, v, s, ambient=None, ao=None, lights=(), sample0=0, nsamples=None, color=True, albedo=False, normal=False,
                          ids=False, ao_out=False, shadow=False, irradiance=False):
        """A shaded preview of the whole frame in one call (rtmi_render_preview; include/rtmi.h defines it): per sample
        albedo * (ambient * ao + sum of light colour * irradiance), averaged per pixel, from one primary pass and one any-hit
        walk of the AO rays and every light's shadow rays.  ambient / ao / lights: preview_params' arguments.  Each output:
        True allocates it, an array is filled in place, False / None leaves it out (not all).  color, albedo, normal: (H, W, 4)
        float32; ids: (H, W) uint32; ao_out: (H, W) float32; shadow, irradiance: (L, H, W) float32, one plane per light.  The
        layers are bit for bit what walk_rays_features, walk_rays_ao and walk_rays_light return for the same parameters.
        Returns a namespace of the requested arrays (None for one left out; the AO plane is .ao) plus ctx."""
        h, w, nl = v.height, v.width, len(list(lights))
        spec = (("color", color, (h, w, 4), np.float32), ("albedo", albedo, (h, w, 4), np.float32), ("normal", normal, (h, w, 4), np.float32),
                ("ids", ids, (h, w), np.uint32), ("ao", ao_out, (h, w), np.float32), ("shadow", shadow, (nl, h, w), np.float32),
                ("irradiance", irradiance, (nl, h, w), np.float32))
        bufs = {}
        for name, x, shape, dt in spec:
            if x is True:
                x = np.zeros(shape, dt)
            elif x is False or x is None:
                x = None
            elif not isinstance(x, np.ndarray) or x.dtype != dt or not x.flags.c_contiguous or x.shape != shape:
                raise ValueError(f"{name} must be a C-contiguous {np.dtype(dt).name} array of shape {shape}")
            bufs[name] = x
        given = [x for x in bufs.values() if x is not None]
        k0, n, p = self._preview_args(v, sample0, nsamples, ambient, ao, lights, {k for k, x in bufs.items() if x is not None})
        if any(np.shares_memory(a, b) for i, a in enumerate(given) for b in given[i + 1:]):
            raise ValueError("the outputs must not overlap")
        self._config(s)
        out = _ffi.PreviewOut(*[x.ctypes.data if x is not None and x.size else None for x in bufs.values()])
        st = _ffi.Stats()
        wall = C.c_double(0)
        _chk(_ffi.lib().rth_caster_walk_preview(s.h, v.width, v.height, _p(v.vp12), v.maxdepth, v.samples_per_pixel, 0, v.height, k0, n,
                                                C.byref(p), C.byref(out), C.byref(st), C.byref(wall)))
        return SimpleNamespace(ctx=ProgressCtx(st.rays, wall.value, st.as_dict()), **bufs)

    def walk_rays_preview_device(self, v, s, tile=None, ambient=None, ao=None, lights=(), sample0=0, nsamples=None, color=None,
                                 albedo=None, normal=None, ids=None, ao_out=None, shadow=None, irradiance=None, stream=None):
        """The same into torch tensors on the scene's device (rtmi_render_preview_device) for a striped row set tile = (row0,
        nrows, stripe_rows, stripe_step) (default: the whole frame).  Each output is a contiguous tensor or None (not all):
        color, albedo, normal float32 of nrows * width * 4 elements, ids int32 or uint32 of nrows * width, ao_out float32 of
        nrows * width, shadow and irradiance float32 of L * nrows * width (one plane per light); no two may overlap.  They
        are written by work enqueued on `stream` (a torch stream, a raw HIP stream pointer or None).  color, albedo and
        normal are what denoise_device takes.  Returns ctx."""
        t = _ffi.Tile(*[int(x) for x in (tile if tile is not None else (0, v.height, v.height, 0))])
        npix, nl = int(t.nrows) * int(v.width), len(list(lights))
        spec = (("color", color, 4 * npix, ("torch.float32",)), ("albedo", albedo, 4 * npix, ("torch.float32",)),
                ("normal", normal, 4 * npix, ("torch.float32",)), ("ids", ids, npix, ("torch.int32", "torch.uint32")),
                ("ao", ao_out, npix, ("torch.float32",)), ("shadow", shadow, nl * npix, ("torch.float32",)),
                ("irradiance", irradiance, nl * npix, ("torch.float32",)))
        for name, x, want, dts in spec:
            if x is not None and (not hasattr(x, "data_ptr") or not x.is_cuda or str(x.dtype) not in dts or not x.is_contiguous()
                                  or x.numel() != want):
                raise ValueError(f"{name} must be a contiguous {dts[0][6:]} tensor of {want} elements on the device")
        k0, n, p = self._preview_args(v, sample0, nsamples, ambient, ao, lights, {name for name, x, _, _ in spec if x is not None})
        spans = sorted((x.data_ptr(), x.data_ptr() + 4 * want) for _, x, want, _ in spec if x is not None)
        if any(a[1] > b[0] for a, b in zip(spans, spans[1:])):
            raise ValueError("the outputs must not overlap")
        self._config(s)
        out = _ffi.PreviewOut(*[x.data_ptr() if x is not None else None for _, x, _, _ in spec])
        st = _ffi.Stats()
        wall = C.c_double(0)
        _chk(_ffi.lib().rth_caster_walk_preview_device(s.h, v.width, v.height, _p(v.vp12), v.maxdepth, v.samples_per_pixel, C.byref(t), k0, n,
                                                       C.byref(p), C.byref(out), C.c_void_p(getattr(stream, "cuda_stream", stream) or 0),
                                                       C.byref(st), C.byref(wall)))
        return ProgressCtx(st.rays, wall.value, st.as_dict())

    DENOISE_DEMODULATE = 1

    @staticmethod
    def denoise_params(iterations=None, demodulate=None, sigma_color=None, sigma_normal=None, sigma_depth=None, sigma_albedo=None):
        """rtmi_denoise_t from the library's defaults (rtmi_denoise_defaults: 3 iterations, no demodulation, sigma_color 1,
        sigma_normal 0.5, sigma_depth 0.1, sigma_albedo +inf) with the given fields replaced.  A sigma of +inf switches its
        term off.  Raises ValueError for what the library would refuse."""
        d = _ffi.Denoise()
        _ffi.lib().rtmi_denoise_defaults(C.byref(d))
        if iterations is not None:
            if not 1 <= int(iterations) <= 8:
                raise ValueError("iterations must be in [1, 8]")
            d.iterations = int(iterations)
        if demodulate is not None:
            d.flags = HipRayCaster.DENOISE_DEMODULATE if demodulate else 0
        for name, val in (("sigma_color", sigma_color), ("sigma_normal", sigma_normal), ("sigma_depth", sigma_depth),
                          ("sigma_albedo", sigma_albedo)):
            if val is not None:
                if not float(val) > 0.0:
                    raise ValueError(f"{name} must be > 0 (+inf switches the term off)")
                setattr(d, name, float(val))
        return d

    def _denoise_scene(self, scene):
        s = self._scene if scene is None else scene
        if s is None:
            raise ValueError("no scene: pass scene=, or render with this caster first (the filter runs on a scene's device handle)")
        return s

    @staticmethod
    def _denoise_images(bufs, nin):
        """The host images of denoise() / denoise_var(): bufs is [(name, array)], colour first, the outputs from index nin on;
        an output of None is allocated.  Raises ValueError for an image that is not C-contiguous (H, W, 4) float32 of colour's
        shape.  Returns (shape, the arrays, the name of the first output that shares memory with a buffer before it, or None)."""
        color = bufs[0][1]
        if not isinstance(color, np.ndarray) or color.ndim != 3 or color.shape[2] != 4 or color.shape[0] < 1 or color.shape[1] < 1:
            raise ValueError("color must be a C-contiguous float32 array of shape (H, W, 4)")
        shape = color.shape
        arrays = [np.zeros(shape, np.float32) if a is None and k >= nin else a for k, (_, a) in enumerate(bufs)]
        for (name, _), a in zip(bufs, arrays):
            if not isinstance(a, np.ndarray) or a.dtype != np.float32 or not a.flags.c_contiguous or a.shape != shape:
                raise ValueError(f"{name} must be a C-contiguous float32 array of shape {shape}")
        shared = next((bufs[k][0] for k in range(nin, len(bufs)) if any(np.shares_memory(arrays[k], a) for a in arrays[:k])), None)
        return shape, arrays, shared

    @staticmethod
    def _denoise_ptrs(w, h, ptrs, names):
        """The device images of denoise_device() / denoise_var_device() as a list of int; all are required."""
        if int(w) < 1 or int(h) < 1:
            raise ValueError("w and h must be >= 1")
        ptrs = [int(p or 0) for p in ptrs]
        if not all(ptrs):
            raise ValueError(f"{names} must all be given")
        return ptrs

    def denoise(self, color, albedo, normal, out=None, scene=None, **params):
        """The feature-guided a-trous filter (rtmi_denoise; include/rtmi.h defines it) on host arrays: color as walk_rays
        writes it, albedo and normal as walk_rays_features returns them for the whole frame, all C-contiguous (H, W, 4)
        float32.  out (same shape; allocated when None; not one of the inputs) receives the result and is returned.
        scene: the Scene whose device handle runs the filter and keeps its scratch image (default: the one this caster
        last worked on); the result does not depend on it.
        params: iterations, demodulate, sigma_color, sigma_normal, sigma_depth, sigma_albedo (denoise_params)."""
        d = self.denoise_params(**params)
        shape, (_, _, _, out), shared = self._denoise_images([("color", color), ("albedo", albedo), ("normal", normal), ("out", out)], 3)
        if shared:
            raise ValueError("out must not share memory with an input: the filter is never in place")
        s = self._denoise_scene(scene)
        self._config(s)
        _chk(_ffi.lib().rth_caster_denoise(s.h, shape[1], shape[0], _p(color), _p(albedo), _p(normal), C.byref(d), _p(out)))
        return out

    def denoise_device(self, w, h, color_ptr, albedo_ptr, normal_ptr, out_ptr, stream=None, scene=None, **params):
        """The same on device memory (rtmi_denoise_device): four images of w * h float4, one launch per iteration enqueued
        on HIP stream `stream`; nothing is synchronised and nothing crosses to the host."""
        d = self.denoise_params(**params)
        ptrs = self._denoise_ptrs(w, h, (color_ptr, albedo_ptr, normal_ptr, out_ptr), "color_ptr, albedo_ptr, normal_ptr and out_ptr")
        if ptrs[3] in ptrs[:3]:
            raise ValueError("out_ptr must not be one of the inputs: the filter is never in place")
        s = self._denoise_scene(scene)
        self._config(s)
        _chk(_ffi.lib().rth_caster_denoise_device(s.h, int(w), int(h), C.c_void_p(ptrs[0]), C.c_void_p(ptrs[1]), C.c_void_p(ptrs[2]),
                                                  C.byref(d), C.c_void_p(ptrs[3]), C.c_void_p(stream or 0)))

    def walk_rays_denoised(self, v, s, data, **params):
        """walk_rays, the features of all v.samples_per_pixel samples and the denoiser in one call (rtmi_render_denoised):
        all three run on the device and only the filtered image ((H, W, 4) float32) is copied into data.  Equals denoise() of
        walk_rays' image and walk_rays_features' albedo and normal.  Returns the render's ProgressCtx."""
        d = self.denoise_params(**params)
        if not isinstance(data, np.ndarray) or data.dtype != np.float32 or not data.flags.c_contiguous or data.size != v.height * v.width * 4:
            raise ValueError("data must be a C-contiguous float32 array of height*width*4 elements")
        self._config(s)
        st = _ffi.Stats()
        wall = C.c_double(0)
        _chk(_ffi.lib().rth_caster_walk_denoised(s.h, v.width, v.height, _p(v.vp12), v.maxdepth, v.samples_per_pixel, C.byref(d),
                                                 _p(data), C.byref(st), C.byref(wall)))
        return ProgressCtx(st.rays, wall.value, st.as_dict())

    @staticmethod
    def denoise_var_params(iterations=None, demodulate=None, sigma_color=None, sigma_normal=None, sigma_depth=None, sigma_albedo=None):
        """rtmi_denoise_t of the variance-guided filter from the library's defaults (rtmi_denoise_var_defaults: 1 iteration, no
        demodulation, sigma_color 3 STANDARD DEVIATIONS OF THE PIXEL, sigma_normal 0.5, sigma_depth 0.1, sigma_albedo +inf)
        with the given fields replaced.  Raises ValueError for what the library would refuse."""
        base = _ffi.Denoise()
        _ffi.lib().rtmi_denoise_var_defaults(C.byref(base))
        d = HipRayCaster.denoise_params(iterations, demodulate, sigma_color, sigma_normal, sigma_depth, sigma_albedo)
        if iterations is None:
            d.iterations = base.iterations
        if sigma_color is None:
            d.sigma_color = base.sigma_color
        return d

    def variance(self, accum, sumsq, counts, out=None, scene=None):
        """The variance of every pixel's mean (rtmi_variance; include/rtmi.h defines it) from the moments of an adaptive
        render: accum and sumsq C-contiguous (..., 4) float32 of one shape, counts uint32 of that shape without the last axis.
        out (same shape as accum; allocated when None; none of the inputs) receives (vm_r, vm_g, vm_b, their sum) per pixel,
        +inf where count < 2, and is returned."""
        if not isinstance(accum, np.ndarray) or accum.dtype != np.float32 or accum.ndim < 1 or accum.shape[-1] != 4 or not accum.flags.c_contiguous:
            raise ValueError("accum must be a C-contiguous float32 array of shape (..., 4)")
        if out is None:
            out = np.zeros(accum.shape, np.float32)
        for name, a in (("sumsq", sumsq), ("out", out)):
            if not isinstance(a, np.ndarray) or a.dtype != np.float32 or not a.flags.c_contiguous or a.shape != accum.shape:
                raise ValueError(f"{name} must be a C-contiguous float32 array of shape {accum.shape}")
        if not isinstance(counts, np.ndarray) or counts.dtype != np.uint32 or not counts.flags.c_contiguous or counts.shape != accum.shape[:-1]:
            raise ValueError(f"counts must be a C-contiguous uint32 array of shape {accum.shape[:-1]}")
        if any(np.shares_memory(out, a) for a in (accum, sumsq, counts)):
            raise ValueError("out must not share memory with an input")
        s = self._denoise_scene(scene)
        self._config(s)
        _chk(_ffi.lib().rth_caster_variance(s.h, _p(accum), _p(sumsq), _p(counts), counts.size, _p(out)))
        return out

    def variance_device(self, accum_ptr, sumsq_ptr, counts_ptr, npixels, variance_ptr, stream=None, scene=None):
        """The same on device memory (rtmi_variance_device): npixels float4 / float4 / uint32 in, npixels float4 out, one
        launch enqueued on HIP stream `stream`; nothing is synchronised."""
        ptrs = [int(p or 0) for p in (accum_ptr, sumsq_ptr, counts_ptr, variance_ptr)]
        if int(npixels) < 0:
            raise ValueError("npixels must be >= 0")
        if not all(ptrs):
            raise ValueError("accum_ptr, sumsq_ptr, counts_ptr and variance_ptr must all be given")
        if ptrs[3] in ptrs[:3]:
            raise ValueError("variance_ptr must not be one of the inputs")
        s = self._denoise_scene(scene)
        self._config(s)
        _chk(_ffi.lib().rth_caster_variance_device(s.h, C.c_void_p(ptrs[0]), C.c_void_p(ptrs[1]), C.c_void_p(ptrs[2]), int(npixels),
                                                   C.c_void_p(ptrs[3]), C.c_void_p(stream or 0)))

    def denoise_var(self, color, albedo, normal, variance, out=None, var_out=None, scene=None, **params):
        """The variance-guided a-trous filter (rtmi_denoise_var; include/rtmi.h defines it) on host arrays: denoise()'s three
        images and variance as variance() returns it for the frame, all C-contiguous (H, W, 4) float32.  out (allocated when
        None) receives the result and is returned.  var_out: None leaves the propagated variance out, True allocates it, an
        array is filled; with it the call returns (out, var_out).  No output may share memory with another buffer.
        params: iterations, demodulate, sigma_color (in standard deviations of the pixel), sigma_normal, sigma_depth,
        sigma_albedo (denoise_var_params)."""
        d = self.denoise_var_params(**params)
        bufs = [("color", color), ("albedo", albedo), ("normal", normal), ("variance", variance), ("out", out)]
        if var_out is not None:
            bufs.append(("var_out", None if var_out is True else var_out))
        shape, arrays, shared = self._denoise_images(bufs, 4)
        if shared:
            raise ValueError(f"{shared} must not share memory with another buffer: the filter is never in place")
        out, var_out = arrays[4], arrays[5] if var_out is not None else None
        s = self._denoise_scene(scene)
        self._config(s)
        _chk(_ffi.lib().rth_caster_denoise_var(s.h, shape[1], shape[0], _p(color), _p(albedo), _p(normal), _p(variance), C.byref(d),
                                               _p(out), _p(var_out) if var_out is not None else None))
        return out if var_out is None else (out, var_out)

    def denoise_var_device(self, w, h, color_ptr, albedo_ptr, normal_ptr, variance_ptr, out_ptr, var_out_ptr=None, stream=None,
                           scene=None, **params):
        """The same on device memory (rtmi_denoise_var_device): images of w * h float4, one launch per iteration enqueued on
        HIP stream `stream`; nothing is synchronised and nothing crosses to the host.  var_out_ptr None/0: not produced."""
        d = self.denoise_var_params(**params)
        ptrs = self._denoise_ptrs(w, h, (color_ptr, albedo_ptr, normal_ptr, variance_ptr, out_ptr),
                                  "color_ptr, albedo_ptr, normal_ptr, variance_ptr and out_ptr")
        vo = int(var_out_ptr or 0)
        if ptrs[4] in ptrs[:4] or (vo and vo in ptrs):
            raise ValueError("out_ptr and var_out_ptr must not be another buffer of the call: the filter is never in place")
        s = self._denoise_scene(scene)
        self._config(s)
        _chk(_ffi.lib().rth_caster_denoise_var_device(s.h, int(w), int(h), C.c_void_p(ptrs[0]), C.c_void_p(ptrs[1]), C.c_void_p(ptrs[2]),
                                                      C.c_void_p(ptrs[3]), C.byref(d), C.c_void_p(ptrs[4]), C.c_void_p(vo),
                                                      C.c_void_p(stream or 0)))

    def walk_rays_adaptive_denoised(self, v, s, data, min_samples=8, pass_samples=8, rel_tol=None, abs_tol=None, counts=None, **params):
        """walk_rays_adaptive, variance() of its moments, the features of samples [0, min_samples) and denoise_var() in one
        call (rtmi_render_adaptive_denoised): all four run on the device and only the filtered image ((H, W, 4) float32, into
        data) and the count map are copied out.  Adaptive arguments and ctx as walk_rays_adaptive, params as denoise_var."""
        d = self.denoise_var_params(**params)
        if not isinstance(data, np.ndarray) or data.dtype != np.float32 or not data.flags.c_contiguous or data.size != v.height * v.width * 4:
            raise ValueError("data must be a C-contiguous float32 array of height*width*4 elements")
        if counts is None:
            counts = np.zeros((v.height, v.width), np.uint32)
        elif not isinstance(counts, np.ndarray) or counts.dtype != np.uint32 or not counts.flags.c_contiguous or counts.size != v.height * v.width:
            raise ValueError("counts must be a C-contiguous uint32 array of height*width elements")
        ad = self._adaptive(v, min_samples, pass_samples, self.ADAPTIVE_REL_TOL if rel_tol is None else rel_tol,
                            self.ADAPTIVE_ABS_TOL if abs_tol is None else abs_tol)
        self._config(s)
        st = _ffi.Stats()
        wall = C.c_double(0)
        _chk(_ffi.lib().rth_caster_walk_adaptive_denoised(s.h, v.width, v.height, _p(v.vp12), v.maxdepth, v.samples_per_pixel,
                                                          C.byref(ad), C.byref(d), _p(data), _p(counts), C.byref(st), C.byref(wall)))
        ctx = self._adaptive_ctx(st, wall, ad)
        ctx.counts = counts
        return ctx

    def quantize_device(self, s, rgba_ptr, npixels, rgb_ptr, stream_ptr=None):
        """write_png's `(c * 255.) as u8` on device memory (f32x4 -> u8x3), enqueued on the stream."""
        self._config(s)
        _chk(_ffi.lib().rth_caster_quantize_device(s.h, C.c_void_p(rgba_ptr), npixels, C.c_void_p(rgb_ptr), C.c_void_p(stream_ptr or 0)))

    def upload(self, s):
        """Make the scene, and its environment if it has one, resident on every device of the caster"""
        self._config(s)
        _chk(_ffi.lib().rth_caster_upload(s.h))

    def environment(self, s):
        """The environment table as the first device holds it (rtmi_scene_get_environment): (n, n, 3) f32, or None when the
        scene has none.  Uploads first if need be."""
        self._config(s)
        n = C.c_uint32(0)
        _chk(_ffi.lib().rth_scene_environment_size(s.h, C.byref(n)))
        if n.value == 0:
            return None
        rgb = np.zeros((n.value, n.value, 3), np.float32)
        _chk(_ffi.lib().rth_caster_environment(s.h, _p(rgb), rgb.size, C.byref(n)))
        return rgb

    def vertex_normals(self, s):
        """The vertex normals as the first device holds them (rtmi_scene_get_normals): (ntris, 3, 3) f32, or None when the scene
        has none.  Uploads first if need be."""
        self._config(s)
        n = C.c_uint64(0)
        _chk(_ffi.lib().rth_scene_normals_size(s.h, C.byref(n)))
        if n.value == 0:
            return None
        out = np.zeros((n.value, 3, 3), np.float32)
        _chk(_ffi.lib().rth_caster_normals(s.h, _p(out), out.size, C.byref(n)))
        return out

    def textures(self, s):
        """The textures as the first device holds them (rtmi_scene_get_uvs, rtmi_scene_get_texture): (images, uvs (ntris, 3, 2) f32,
        tex_of_tri (ntris,) u32; a degenerate triangle reads as texture 0), or None when the scene has no images.  Uploads first if
        need be."""
        self._config(s)
        ntex, n = C.c_uint32(0), C.c_uint64(0)
        _chk(_ffi.lib().rth_scene_textures_size(s.h, C.byref(ntex), C.byref(n)))
        if ntex.value == 0:
            return None
        uv, tt = np.zeros((n.value, 3, 2), np.float32), np.zeros(n.value, np.uint32)
        _chk(_ffi.lib().rth_caster_uvs(s.h, _p(uv), _p(tt), n.value, C.byref(n)))
        images = []
        for k in range(1, ntex.value + 1):
            w, h = C.c_uint32(0), C.c_uint32(0)
            _chk(_ffi.lib().rth_scene_get_texture(s.h, k, None, 0, C.byref(w), C.byref(h)))
            im = np.zeros((h.value, w.value, 3), np.float32)
            _chk(_ffi.lib().rth_caster_texture(s.h, k, _p(im), im.size, C.byref(w), C.byref(h)))
            images.append(im)
        return images, uv, tt

    def normal_maps(self, s):
        """The normal maps as the first device holds them (rtmi_scene_get_normal_maps): (nmap_of_tri (ntris,) u32, strength; a
        triangle without a tangent frame reads as map 0), or None when the scene has none.  Uploads first if need be."""
        self._config(s)
        n = C.c_uint64(0)
        _chk(_ffi.lib().rth_scene_normal_maps_size(s.h, C.byref(n)))
        if n.value == 0:
            return None
        nm, st = np.zeros(n.value, np.uint32), C.c_float(0)
        _chk(_ffi.lib().rth_caster_normal_maps(s.h, _p(nm), C.byref(st), n.value, C.byref(n)))
        return nm[:n.value], float(st.value)

    def trace(self, s, orig4, dir4):
        """Closest hit per explicit ray (rtmi_trace): -> tri, t, face, stats."""
        o4, d4 = _f(orig4).reshape(-1, 4), _f(dir4).reshape(-1, 4)
        n = o4.shape[0]
        tri, t, face = np.zeros(n, np.uint32), np.zeros(n, np.float32), np.zeros(n, np.uint32)
        self._config(s)
        st = _ffi.Stats()
        _chk(_ffi.lib().rth_caster_trace(s.h, n, _p(o4), _p(d4), _p(tri), _p(t), _p(face), C.byref(st)))
        return tri, t, face, st.as_dict()

    def occluded(self, s, orig4, dir4, tmax=None):
        """Any-hit occlusion per explicit ray (rtmi_occluded; include/rtmi.h defines it): -> (uint8 array of 0 / 1, stats).
        Ray i is occluded iff its closest hit (trace) has tri != 0 and t < tmax[i] in float32; tmax None means +inf for every
        ray.  No epsilon and no exclusion of the triangle the origin lies on: offset the origins yourself."""
        o4, d4 = _f(orig4).reshape(-1, 4), _f(dir4).reshape(-1, 4)
        n = o4.shape[0]
        if d4.shape[0] != n:
            raise ValueError("orig4 and dir4 must hold the same number of rays")
        tm = None
        if tmax is not None:
            tm = _f(tmax).reshape(-1)
            if tm.shape[0] != n:
                raise ValueError("tmax must hold one float per ray")
        out = np.zeros(n, np.uint8)
        self._config(s)
        st = _ffi.Stats()
        _chk(_ffi.lib().rth_caster_occluded(s.h, n, _p(o4), _p(d4), _p(tm) if tm is not None else None, _p(out), C.byref(st)))
        return out, st.as_dict()

    def occluded_device(self, s, n, orig4_ptr, dir4_ptr, tmax_ptr, occluded_ptr, stream=None):
        """The same on device memory (rtmi_occluded_device): n float4 origins, n float4 directions and n floats of tmax
        (tmax_ptr None/0: +inf) are read in place, n bytes are written at occluded_ptr.  The work starts after what is
        queued on HIP stream `stream`, and that stream waits for it; the call returns once the counters are read back.
        -> stats."""
        ptrs = [int(p or 0) for p in (orig4_ptr, dir4_ptr, occluded_ptr)]
        if int(n) < 0:
            raise ValueError("n must be >= 0")
        if not all(ptrs):
            raise ValueError("orig4_ptr, dir4_ptr and occluded_ptr must all be given")
        tm = int(tmax_ptr or 0)
        if ptrs[2] in (ptrs[0], ptrs[1]) or (tm and ptrs[2] == tm):
            raise ValueError("occluded_ptr must not be one of the inputs")
        self._config(s)
        st = _ffi.Stats()
        _chk(_ffi.lib().rth_caster_occluded_device(s.h, int(n), C.c_void_p(ptrs[0]), C.c_void_p(ptrs[1]), C.c_void_p(tm),
                                                   C.c_void_p(ptrs[2]), C.c_void_p(stream or 0), C.byref(st)))
        return st.as_dict()

    def trace_device(self, s, orig4, dir4, tri, t, face, stream=None):
        """trace() on torch tensors on the scene's device (rtmi_trace_device): orig4 and dir4 are contiguous float32 tensors of
        n * 4 elements, read in place; tri and face (int32 or uint32) and t (float32) are contiguous tensors of n elements,
        written in place.  The work starts after what is queued on `stream` (a torch stream, a raw HIP stream pointer or None)
        and that stream waits for it.  -> stats."""
        n = self._ray_tensors(orig4, dir4)
        for name, x, dts in (("tri", tri, ("torch.int32", "torch.uint32")), ("t", t, ("torch.float32",)), ("face", face, ("torch.int32", "torch.uint32"))):
            self._tensor(name, x, n, dts)
        self._config(s)
        st = _ffi.Stats()
        _chk(_ffi.lib().rth_caster_trace_device(s.h, n, C.c_void_p(orig4.data_ptr()), C.c_void_p(dir4.data_ptr()), C.c_void_p(tri.data_ptr()),
                                                C.c_void_p(t.data_ptr()), C.c_void_p(face.data_ptr()),
                                                C.c_void_p(getattr(stream, "cuda_stream", stream) or 0), C.byref(st)))
        return st.as_dict()

    RAYS_MAKE_RAY = 1
    RAYS_OUTPUTS = ("color", "mean", "albedo", "normal", "ids")

    @staticmethod
    def _tensor(name, x, want, dts):
        if not hasattr(x, "data_ptr") or not x.is_cuda or str(x.dtype) not in dts or not x.is_contiguous() or x.numel() != want:
            raise ValueError(f"{name} must be a contiguous {dts[0][6:]} tensor of {want} elements on the device")

    @classmethod
    def _ray_tensors(cls, orig4, dir4):
        if not hasattr(orig4, "data_ptr") or orig4.numel() % 4:
            raise ValueError("orig4 must be a contiguous float32 tensor of n * 4 elements on the device")
        n = orig4.numel() // 4
        cls._tensor("orig4", orig4, 4 * n, ("torch.float32",))
        cls._tensor("dir4", dir4, 4 * n, ("torch.float32",))
        return n

    @classmethod
    def _rays_args(cls, n, maxdepth, group, pixel0, make_ray, keyed):
        maxdepth, group, pixel0 = int(maxdepth), int(group), int(pixel0)
        if not 0 <= maxdepth <= 32:
            raise ValueError("maxdepth must be in [0, 32]")
        if not 1 <= group <= 65536:
            raise ValueError("group must be in [1, 65536]")
        if n % group:
            raise ValueError("the number of rays must be a multiple of group")
        if n >= 1 << 31:
            raise ValueError("at most 2^31 - 1 rays per call")
        if pixel0 < 0 or (not keyed and n and pixel0 + n // group - 1 >= 1 << 32):
            raise ValueError("pixel0 + n / group - 1 must stay below 2^32")
        return _ffi.Rays(maxdepth, group, pixel0 & 0xFFFFFFFF, cls.RAYS_MAKE_RAY if make_ray else 0)

    def walk_rays_explicit(self, s, orig4, dir4, maxdepth, group=1, keys=None, pixel0=0, make_ray=False, color=True, mean=False,
                           albedo=False, normal=False, ids=False, _lit=None):
        """Path tracing of caller-supplied rays (rtmi_render_rays; include/rtmi.h defines it): orig4 and dir4 are (n, 4) float32
        arrays, a ray's origin and unit direction as make_ray stores them (make_ray=True: the library normalises the
        directions).  The RNG key of ray i is keys[i] = (pixel, sample) ((n, 2) uint32) or, without keys, (pixel0 + i // group,
        i % group).  Outputs, each produced when its flag is true: color (n, 4) float32, the colour project_ray returns for each
        ray at depth `maxdepth`; mean (n // group, 4), the f32 mean of each group of `group` consecutive rays in walk_ray_set's
        order; albedo and normal (n // group, 4) and ids (n // group) uint32, the first-hit feature buffers with a group
        standing for a pixel.  Returns (dict of the requested arrays, ctx)."""
        o4, d4 = _f(orig4).reshape(-1, 4), _f(dir4).reshape(-1, 4)
        n = o4.shape[0]
        if d4.shape[0] != n:
            raise ValueError("orig4 and dir4 must hold the same number of rays")
        kk = None
        if keys is not None:
            kk = np.ascontiguousarray(keys, dtype=np.uint32).reshape(-1, 2)
            if kk.shape[0] != n:
                raise ValueError("keys must hold one (pixel, sample) pair per ray")
        r = self._rays_args(n, maxdepth, group, pixel0, make_ray, kk is not None)
        ng = n // r.group
        shapes = {"color": ((n, 4), np.float32), "mean": ((ng, 4), np.float32), "albedo": ((ng, 4), np.float32),
                  "normal": ((ng, 4), np.float32), "ids": ((ng,), np.uint32)}
        want = dict(color=color, mean=mean, albedo=albedo, normal=normal, ids=ids)
        bufs = {k: np.zeros(*shapes[k]) for k in self.RAYS_OUTPUTS if want[k]}
        if not bufs:
            raise ValueError("at least one of color, mean, albedo, normal and ids must be produced")
        out = _ffi.RaysOut(*[_p(bufs[k]) if k in bufs else None for k in self.RAYS_OUTPUTS])
        self._config(s)
        st = _ffi.Stats()
        wall = C.c_double(0)
        if _lit is not None:
            _chk(_ffi.lib().rth_caster_walk_rays_explicit_lit(s.h, n, _p(o4), _p(d4), _p(kk) if kk is not None else None, C.byref(r),
                                                              C.byref(_lit), C.byref(out), C.byref(st), C.byref(wall)))
        else:
            _chk(_ffi.lib().rth_caster_walk_rays_explicit(s.h, n, _p(o4), _p(d4), _p(kk) if kk is not None else None, C.byref(r), C.byref(out),
                                                          C.byref(st), C.byref(wall)))
        return bufs, ProgressCtx(st.rays, wall.value, st.as_dict())

    def walk_rays_explicit_device(self, s, orig4, dir4, maxdepth, group=1, keys=None, pixel0=0, make_ray=False, color=None, mean=None,
                                  albedo=None, normal=None, ids=None, stream=None, _lit=None):
        """The same on torch tensors on the scene's device (rtmi_render_rays_device), read and written in place: orig4 and dir4
        contiguous float32 of n * 4 elements, keys None or contiguous int32 / uint32 of n * 2; each output a contiguous tensor or
        None (not all): color float32 of n * 4, mean, albedo and normal float32 of (n // group) * 4, ids int32 or uint32 of
        n // group; no two buffers may overlap.  The work starts after what is queued on `stream` (a torch stream, a raw HIP
        stream pointer or None) and that stream waits for it.  Returns ctx."""
        n = self._ray_tensors(orig4, dir4)
        if keys is not None:
            self._tensor("keys", keys, 2 * n, ("torch.int32", "torch.uint32"))
        r = self._rays_args(n, maxdepth, group, pixel0, make_ray, keys is not None)
        ng = n // r.group
        spec = (("color", color, 4 * n, ("torch.float32",)), ("mean", mean, 4 * ng, ("torch.float32",)),
                ("albedo", albedo, 4 * ng, ("torch.float32",)), ("normal", normal, 4 * ng, ("torch.float32",)),
                ("ids", ids, ng, ("torch.int32", "torch.uint32")))
        for name, x, want, dts in spec:
            if x is not None:
                self._tensor(name, x, want, dts)
        if all(x is None for _, x, _, _ in spec):
            raise ValueError("at least one of color, mean, albedo, normal and ids must be given")
        spans = [(orig4.data_ptr(), 16 * n), (dir4.data_ptr(), 16 * n)] + ([(keys.data_ptr(), 8 * n)] if keys is not None else [])
        spans = sorted(spans + [(x.data_ptr(), 4 * want) for _, x, want, _ in spec if x is not None])
        if any(a[0] + a[1] > b[0] for a, b in zip(spans, spans[1:]) if a[1] and b[1]):
            raise ValueError("the buffers must not overlap")
        self._config(s)
        out = _ffi.RaysOut(*[x.data_ptr() if x is not None else None for _, x, _, _ in spec])
        st = _ffi.Stats()
        wall = C.c_double(0)
        kp = C.c_void_p(keys.data_ptr()) if keys is not None else None
        sp = C.c_void_p(getattr(stream, "cuda_stream", stream) or 0)
        if _lit is not None:
            _chk(_ffi.lib().rth_caster_walk_rays_explicit_lit_device(s.h, n, C.c_void_p(orig4.data_ptr()), C.c_void_p(dir4.data_ptr()), kp,
                                                                     C.byref(r), C.byref(_lit), C.byref(out), sp, C.byref(st), C.byref(wall)))
        else:
            _chk(_ffi.lib().rth_caster_walk_rays_explicit_device(s.h, n, C.c_void_p(orig4.data_ptr()), C.c_void_p(dir4.data_ptr()), kp,
                                                                 C.byref(r), C.byref(out), sp, C.byref(st), C.byref(wall)))
        return ProgressCtx(st.rays, wall.value, st.as_dict())

    def walk_rays_explicit_lit(self, s, orig4, dir4, maxdepth, lit, **kw):
        """walk_rays_explicit with box lights sampled at every Matte hit that bounces (rtmi_render_rays_lit; include/rtmi.h defines
        it): the same rays, keys, groups and outputs, and at each such hit one shadow ray per light of `lit` (lit_params' result,
        or its lights argument) whose unoccluded light is added to what the surface passes on.  Returns (dict, ctx)."""
        a = lit if isinstance(lit, _ffi.Lit) else self.lit_params(lit)
        return self.walk_rays_explicit(s, orig4, dir4, maxdepth, _lit=a, **kw)

    def walk_rays_explicit_lit_device(self, s, orig4, dir4, maxdepth, lit, **kw):
        """The same on torch tensors on the scene's device (rtmi_render_rays_lit_device): walk_rays_explicit_device's arguments.
        Returns ctx."""
        a = lit if isinstance(lit, _ffi.Lit) else self.lit_params(lit)
        return self.walk_rays_explicit_device(s, orig4, dir4, maxdepth, _lit=a, **kw)

    BAKE_MODES = {"points": _ffi.BAKE_POINTS, "triangles": _ffi.BAKE_TRIANGLES}
    BAKE_OUTPUTS = ("light", "open", "orig", "dir")

    @staticmethod
    def bake_params(mode="points", rays=None, maxdepth=None, pixel0=None, bias=None):
        """rtmi_bake_t from the library's defaults (rtmi_bake_defaults: points, 64 rays, maxdepth 4, pixel0 0, bias 0.001) with
        the given fields replaced.  Raises ValueError for what the library would refuse."""
        if mode not in HipRayCaster.BAKE_MODES:
            raise ValueError(f"mode must be one of {sorted(HipRayCaster.BAKE_MODES)}")
        b = _ffi.Bake()
        _ffi.lib().rtmi_bake_defaults(C.byref(b))
        b.mode = HipRayCaster.BAKE_MODES[mode]
        if rays is not None:
            if not 1 <= int(rays) <= 65536:
                raise ValueError("rays must be in [1, 65536]")
            b.rays = int(rays)
        if maxdepth is not None:
            if not 0 <= int(maxdepth) <= 32:
                raise ValueError("maxdepth must be in [0, 32]")
            b.maxdepth = int(maxdepth)
        if pixel0 is not None:
            if not 0 <= int(pixel0) < 1 << 32:
                raise ValueError("pixel0 must be in [0, 2^32)")
            b.pixel0 = int(pixel0)
        if bias is not None:
            if not np.isfinite(float(bias)):
                raise ValueError("bias must be finite")
            b.bias = float(bias)
        return b

    @staticmethod
    def _bake_count(b, npos, nnrm):
        """M of a bake call whose pos4 holds npos float4 and nrm4 nnrm float4"""
        per = 3 if b.mode == _ffi.BAKE_TRIANGLES else 1
        if npos != per * nnrm:
            raise ValueError("pos4 must hold one float4 per element (points) or three (triangles), nrm4 one per element")
        if nnrm * b.rays >= 1 << 31:
            raise ValueError("elements * rays must stay below 2^31")
        if nnrm and b.pixel0 + nnrm - 1 >= 1 << 32:
            raise ValueError("pixel0 + M - 1 must stay below 2^32")
        return nnrm

    def bake(self, s, pos4, nrm4, params, light=True, open=False, orig=False, dir=False, _lit=None, _direct=False):
        """Light baked at surface points or over triangles (rtmi_bake; include/rtmi.h defines it).  params: bake_params().
        nrm4: (M, 4) float32, the side to bake of each element, used as given.  pos4: (M, 4) float32 points, or (3 M, 4), the
        corners of M triangles.  Per element params.rays gather rays are made on the device and path-traced at depth
        params.maxdepth.  Outputs, each produced when its flag is true: light (M, 4) float32, the mean colour arriving; open (M,)
        float32, the share of the element's rays that hit nothing; orig and dir (M * rays, 4), the gather rays themselves.
        Returns (dict of the requested arrays, ctx)."""
        p4, n4 = _f(pos4).reshape(-1, 4), _f(nrm4).reshape(-1, 4)
        m = self._bake_count(params, p4.shape[0], n4.shape[0])
        n = m * params.rays
        shapes = {"light": (m, 4), "open": (m,), "orig": (n, 4), "dir": (n, 4)}
        want = dict(light=light, open=open, orig=orig, dir=dir)
        names = self.BAKE_OUTPUTS
        if _lit is not None:
            shapes["direct"], want["direct"], names = (m, 4), _direct, self.BAKE_LIT_OUTPUTS
        bufs = {k: np.zeros(shapes[k], np.float32) for k in names if want[k]}
        if not bufs:
            raise ValueError("at least one of " + ", ".join(names[:-1]) + " and " + names[-1] + " must be produced")
        ptrs = [_p(bufs[k]) if k in bufs else None for k in names]
        self._config(s)
        st = _ffi.Stats()
        wall = C.c_double(0)
        if _lit is not None:
            out = _ffi.BakeLitOut(*ptrs)
            _chk(_ffi.lib().rth_caster_bake_lit(s.h, m, _p(p4), _p(n4), C.byref(params), C.byref(_lit), C.byref(out), C.byref(st),
                                                C.byref(wall)))
        else:
            out = _ffi.BakeOut(*ptrs)
            _chk(_ffi.lib().rth_caster_bake(s.h, m, _p(p4), _p(n4), C.byref(params), C.byref(out), C.byref(st), C.byref(wall)))
        return bufs, ProgressCtx(st.rays, wall.value, st.as_dict())

    def bake_device(self, s, pos4, nrm4, params, light=None, open=None, orig=None, dir=None, stream=None, _lit=None, _direct=None):
        """The same on torch tensors on the scene's device (rtmi_bake_device), read and written in place: nrm4 contiguous
        float32 of M * 4 elements, pos4 of M * 4 (points) or 3 M * 4 (triangles); each output a contiguous float32 tensor or None
        (not all): light of M * 4, open of M, orig and dir of M * rays * 4; no two buffers may overlap.  The work starts after
        what is queued on `stream` (a torch stream, a raw HIP stream pointer or None) and that stream waits for it.
        Returns ctx."""
        for name, x in (("pos4", pos4), ("nrm4", nrm4)):
            if not hasattr(x, "data_ptr") or x.numel() % 4:
                raise ValueError(f"{name} must be a contiguous float32 tensor of whole float4 on the device")
            self._tensor(name, x, x.numel(), ("torch.float32",))
        m = self._bake_count(params, pos4.numel() // 4, nrm4.numel() // 4)
        n = m * params.rays
        spec = (("light", light, 4 * m), ("open", open, m), ("orig", orig, 4 * n), ("dir", dir, 4 * n))
        if _lit is not None:
            spec += (("direct", _direct, 4 * m),)
        for name, x, want in spec:
            if x is not None:
                self._tensor(name, x, want, ("torch.float32",))
        if all(x is None for _, x, _ in spec):
            raise ValueError("at least one of " + ", ".join(k for k, _, _ in spec[:-1]) + " and " + spec[-1][0] + " must be given")
        spans = sorted([(pos4.data_ptr(), 4 * pos4.numel()), (nrm4.data_ptr(), 16 * m)] +
                       [(x.data_ptr(), 4 * want) for _, x, want in spec if x is not None])
        if any(a[0] + a[1] > b[0] for a, b in zip(spans, spans[1:]) if a[1] and b[1]):
            raise ValueError("the buffers must not overlap")
        self._config(s)
        ptrs = [x.data_ptr() if x is not None else None for _, x, _ in spec]
        st = _ffi.Stats()
        wall = C.c_double(0)
        sp = C.c_void_p(getattr(stream, "cuda_stream", stream) or 0)
        if _lit is not None:
            out = _ffi.BakeLitOut(*ptrs)
            _chk(_ffi.lib().rth_caster_bake_lit_device(s.h, m, C.c_void_p(pos4.data_ptr()), C.c_void_p(nrm4.data_ptr()), C.byref(params),
                                                       C.byref(_lit), C.byref(out), sp, C.byref(st), C.byref(wall)))
        else:
            out = _ffi.BakeOut(*ptrs)
            _chk(_ffi.lib().rth_caster_bake_device(s.h, m, C.c_void_p(pos4.data_ptr()), C.c_void_p(nrm4.data_ptr()), C.byref(params),
                                                   C.byref(out), sp, C.byref(st), C.byref(wall)))
        return ProgressCtx(st.rays, wall.value, st.as_dict())

    BAKE_LIT_OUTPUTS = BAKE_OUTPUTS + ("direct",)

    def bake_lit(self, s, pos4, nrm4, params, lit, light=True, open=False, orig=False, dir=False, direct=True):
        """bake() with box lights (rtmi_bake_lit; include/rtmi.h defines it).  lit: lit_params' result, or its lights argument.
        light is then the indirect light with the lamps lighting every Matte bounce of every gather path, and direct (M, 4)
        float32 the lamps' light arriving at the element itself; a lightmap texel of a surface (color, alpha) is
        mix_color(color, light + direct, alpha).  Pass unit normals: direct scales with their length.
        Returns (dict of the requested arrays, ctx)."""
        a = lit if isinstance(lit, _ffi.Lit) else self.lit_params(lit)
        return self.bake(s, pos4, nrm4, params, light=light, open=open, orig=orig, dir=dir, _lit=a, _direct=direct)

    def bake_lit_device(self, s, pos4, nrm4, params, lit, light=None, open=None, orig=None, dir=None, direct=None, stream=None):
        """The same on torch tensors on the scene's device (rtmi_bake_lit_device): bake_device's arguments and direct, a
        contiguous float32 tensor of M * 4 or None.  Returns ctx."""
        a = lit if isinstance(lit, _ffi.Lit) else self.lit_params(lit)
        return self.bake_device(s, pos4, nrm4, params, light=light, open=open, orig=orig, dir=dir, stream=stream, _lit=a, _direct=direct)

    def bake_triangles(self, s, corners, normals, rays=None, maxdepth=None, pixel0=None, bias=None, light=True, open=False,
                       orig=False, dir=False, _lit=None, _direct=False):
        """bake() over whole triangles: corners (M, 3, 3) or (M, 3, 4) float32, normals (M, 3) or (M, 4), the side of each
        triangle to bake (its `norm` or the negative); three-component vectors get lane 3 = +0.  One colour per face, for a
        flat-shaded view of the scene.  Returns (dict of the requested arrays, ctx)."""
        c = _f(corners)
        if c.ndim != 3 or c.shape[1] != 3 or c.shape[2] not in (3, 4):
            raise ValueError("corners must be (M, 3, 3) or (M, 3, 4)")
        nn = _f(normals)
        if nn.ndim != 2 or nn.shape[0] != c.shape[0] or nn.shape[1] not in (3, 4):
            raise ValueError("normals must be (M, 3) or (M, 4), one per triangle")
        p4 = np.zeros((c.shape[0] * 3, 4), np.float32)
        p4[:, : c.shape[2]] = c.reshape(-1, c.shape[2])
        n4 = np.zeros((c.shape[0], 4), np.float32)
        n4[:, : nn.shape[1]] = nn
        return self.bake(s, p4, n4, self.bake_params("triangles", rays, maxdepth, pixel0, bias), light=light, open=open, orig=orig, dir=dir,
                         _lit=_lit, _direct=_direct)

    def bake_triangles_lit(self, s, corners, normals, lit, direct=True, **kw):
        """bake_triangles() with box lights (bake_lit over whole triangles): bake_triangles' arguments, lit as bake_lit takes it.
        Returns (dict of the requested arrays, ctx)."""
        a = lit if isinstance(lit, _ffi.Lit) else self.lit_params(lit)
        return self.bake_triangles(s, corners, normals, _lit=a, _direct=direct, **kw)

    def _records(self, n, call, pixel=None):
        """Size query, then the fill (rth_caster_*_records)"""
        recs = np.zeros(n, REC_DTYPE)
        total, st = C.c_uint64(0), _ffi.Stats()
        _chk(call(_p(recs), None, 0, C.byref(total), C.byref(st)))
        ids = np.zeros(max(total.value, 1), np.uint32)
        if total.value:
            _chk(call(_p(recs), _p(ids), total.value, C.byref(total), C.byref(st)))
        return RayRecords(recs, ids[: total.value], pixel, st.as_dict())

    def trace_records(self, s, orig4, dir4):
        """Per-ray records of the exact octree walk for explicit rays (rtmi_trace_records) -> RayRecords (.stats: the
        call's rtmi_stats_t of the fill)."""
        o4, d4 = _f(orig4).reshape(-1, 4), _f(dir4).reshape(-1, 4)
        self._config(s)
        return self._records(o4.shape[0], lambda r, ids, cap, tot, st: _ffi.lib().rth_caster_trace_records(
            s.h, o4.shape[0], _p(o4), _p(d4), r, ids, cap, tot, st))

    def primary_records(self, v, s, row0=0, nrows=None, sample=0):
        """Records of the primary rays of sample `sample` of every pixel of rows [row0, row0 + nrows) (rtmi_primary_records):
        record i is pixel (row0 + i // width, i % width), its ray bit-identical to the renderer's."""
        nrows = v.height - row0 if nrows is None else int(nrows)
        self._config(s)
        n = nrows * v.width
        i = np.arange(n, dtype=np.uint64)
        pixel = np.stack([row0 + i // v.width, i % v.width], axis=1).astype(np.uint32)
        return self._records(n, lambda r, ids, cap, tot, st: _ffi.lib().rth_caster_primary_records(
            s.h, v.width, v.height, _p(v.vp12), v.maxdepth, v.samples_per_pixel, row0, nrows, sample, r, ids, cap, tot, st), pixel)


def quantize(rgba):
    """write_png's `(c * 255.) as u8` (raytrace.rs:1468-1473)."""
    rgba = _f(rgba).reshape(-1, 4)
    out = np.zeros((rgba.shape[0], 3), np.uint8)
    _ffi.lib().rth_quantize(_p(rgba), rgba.shape[0], _p(out))
    return out


def normal_map_from_height(height, scale=1.0):
    """A normal map (h, w, 3) f32 from a height field (h, w) (rtmi_normal_map_from_height): repeat-wrapped central differences,
    n = unit(-dx, -dy, 1), rgb = n * 0.5 + 0.5.  Host code; needs no device."""
    hh = _f(height)
    if hh.ndim != 2:
        raise ValueError(f"height must be (h, w), not {hh.shape}")
    out = np.zeros(hh.shape + (3,), np.float32)
    _chk(_ffi.lib().rth_normal_map_from_height(_p(hh), hh.shape[1], hh.shape[0], float(scale), _p(out)))
    return out


# ---------------------------------------------------------------- scenes of the benchmark configs
def canonical_scene(obj_path, accel="octree", maxdepth=10, minobjs=19, teapot_surface=None, threads=0, gpu_build=None, smooth=False,
                    texture=None, normal_map=None):
    """The scene of raytrace/src/main.rs:116-164.  smooth (an extension): the teapot gets generated vertex normals.  texture (an
    extension): an (h, w, 3) f32 image the teapot gets through box-projected uvs.  normal_map (an extension): an (h, w, 3) f32
    tangent-space normal map for the teapot, appended to the scene's images; the teapot is box-projected if it has no uvs yet."""
    s = Scene(with_dummy=True)
    tsurf = teapot_surface or SurfaceKind.Matte(make_color(252, 119, 0), 0.2)
    s.extend_parse_obj(obj_path, [0.0, 0.5, 5.0], 1.0, create_transform(unit([0.0, 0.3, 1.0]), to_radians(270.0)), tsurf, 0.05,
                       normals="smooth" if smooth else None, uvs=None if texture is None and normal_map is None else "box",
                       texture=0 if texture is None else 1)
    if texture is not None or normal_map is not None:
        s.set_textures([im for im in (texture, normal_map) if im is not None], None, None)
    if normal_map is not None:
        nteapot = s.num_tris() - 1
        s.set_normal_maps(np.full(nteapot, 1 if texture is None else 2, np.uint32))
    side = SurfaceKind.Matte(make_color(40, 40, 40), 0.2)
    s.extend_make_disk([4.0, 4.0, 7.0], unit([-0.3, -0.55, -0.5]), 2.0, 0.1, 50,
                       SurfaceKind.Reflective(0.0002, make_color(230, 230, 230), 0.7), side, -1.0)
    s.extend_make_disk([4.0, -3.0, 5.0], unit([-0.5, 2.0, -0.5]), 1.0, 0.04, 50,
                       SurfaceKind.Reflective(0.002, make_color(230, 230, 230), 0.7), side, -1.0)
    s.populate_triangle_numbers()
    if accel == "octree":
        s.build_bounding_box([0.0, 0.0, 20.1], 20.0, maxdepth, minobjs, threads, gpu_device=gpu_build)
    elif accel == "trivial":
        s.build_trivial_bounding_box([0.0, 0.0, 0.0], 20.0)
    return s


def grid_scene(obj_path, maxdepth=10, minobjs=19, n=8, threads=0, gpu_build=None):
    """BASELINE config 5: n instances of teapot_tri.obj on a 2x2x2 grid (spacing 9 units) inside the canonical
    root box — the octree-traversal stress scene (8 x 6320 + 1 = 50 561 triangles)."""
    s = Scene(with_dummy=True)
    surfs = [SurfaceKind.Matte(make_color(252, 119, 0), 0.2), SurfaceKind.Reflective(0.01, make_color(200, 200, 220), 0.6),
             SurfaceKind.Solid(make_color(30, 160, 60)), SurfaceKind.Matte(make_color(200, 40, 40), 0.35)]
    k = 0
    for iz in range(2):
        for iy in range(2):
            for ix in range(2):
                if k >= n:
                    break
                off = [-4.5 + 9.0 * ix, -4.5 + 9.0 * iy, 9.0 + 9.0 * iz]
                s.extend_parse_obj(obj_path, off, 1.0, create_transform(unit([0.0, 0.3, 1.0]), to_radians(270.0 + 20.0 * k)),
                                   surfs[k % 4], 0.05 if k % 2 == 0 else 0.0)
                k += 1
    s.populate_triangle_numbers()
    s.build_bounding_box([0.0, 0.0, 20.1], 20.0, maxdepth, minobjs, threads, gpu_device=gpu_build)
    return s


def canonical_viewport(w, h, maxdepth=5, samples=1):
    """main.rs:166-173"""
    aspect = np.float32(h) / np.float32(w)
    return create_viewport((w, h), (1.0, float(np.float32(1.0) * aspect)), [2.0, 0.0, 0.0], unit([0.0, 0.0, 1.0]), 90.0,
                           to_radians(0.0), maxdepth, samples)
