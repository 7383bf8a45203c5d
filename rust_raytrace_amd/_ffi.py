"""ctypes loader for librtmi.so (HIP kernels + C ABI + C++ host mirror).

The product path has no CPU fallback: if the library is missing this module
raises, and every render entry point fails with the library's own error when
no HIP device is visible.
"""
import ctypes as C
import os
import subprocess

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
LIB_PATH = os.path.join(_CSRC, "librtmi.so")


class Stats(C.Structure):
    """rtmi_stats_t (include/rtmi.h)."""
    _fields_ = [("rays", C.c_uint64), ("box_tests", C.c_uint64), ("tri_tests", C.c_uint64),
                ("full_tests", C.c_uint64), ("nodes", C.c_uint64), ("leaves", C.c_uint64),
                ("kernel_ms", C.c_double), ("trace_ms", C.c_double), ("trace_launches", C.c_uint32),
                ("streams", C.c_uint32), ("render_ms", C.c_double), ("band_copy_ms", C.c_double),
                ("deinterleave_ms", C.c_double), ("primary_ms", C.c_double), ("bounce_ms", C.c_double),
                ("peer_access", C.c_int32), ("pipeline", C.c_uint32), ("slow_paths", C.c_uint32), ("reserved", C.c_uint32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class RayRecord(C.Structure):
    """rtmi_ray_record_t (include/rtmi.h)."""
    _fields_ = [("orig", C.c_float * 4), ("dir", C.c_float * 4), ("tri", C.c_uint32), ("t", C.c_float), ("face", C.c_uint32),
                ("nleaves", C.c_uint32), ("leaf_first", C.c_uint64), ("box_tests", C.c_uint32), ("tri_tests", C.c_uint32),
                ("full_tests", C.c_uint32), ("nodes", C.c_uint32)]


class Tile(C.Structure):
    """rtmi_tile_t (include/rtmi.h)."""
    _fields_ = [("row0", C.c_uint32), ("nrows", C.c_uint32), ("stripe_rows", C.c_uint32), ("stripe_step", C.c_uint32)]


class Adaptive(C.Structure):
    """rtmi_adaptive_t (include/rtmi.h)."""
    _fields_ = [("min_samples", C.c_uint32), ("pass_samples", C.c_uint32), ("rel_tol", C.c_float), ("abs_tol", C.c_float),
                ("passes", C.c_uint32), ("unconverged", C.c_uint32), ("samples", C.c_uint64)]


class Denoise(C.Structure):
    """rtmi_denoise_t (include/rtmi.h)."""
    _fields_ = [("iterations", C.c_uint32), ("flags", C.c_uint32), ("sigma_color", C.c_float), ("sigma_normal", C.c_float),
                ("sigma_depth", C.c_float), ("sigma_albedo", C.c_float)]


class Ao(C.Structure):
    """rtmi_ao_t (include/rtmi.h)."""
    _fields_ = [("rays", C.c_uint32), ("flags", C.c_uint32), ("radius", C.c_float), ("bias", C.c_float)]


class Light(C.Structure):
    """rtmi_light_t (include/rtmi.h)."""
    _fields_ = [("orig", C.c_float * 3), ("len2", C.c_float), ("rays", C.c_uint32), ("flags", C.c_uint32), ("bias", C.c_float)]


PREVIEW_MAX_LIGHTS = 4  # RTMI_PREVIEW_MAX_LIGHTS


class Preview(C.Structure):
    """rtmi_preview_t (include/rtmi.h): 196 bytes."""
    _fields_ = [("ambient", C.c_float * 3), ("nlights", C.c_uint32), ("flags", C.c_uint32), ("ao", Ao),
                ("lights", Light * PREVIEW_MAX_LIGHTS), ("light_color", (C.c_float * 3) * PREVIEW_MAX_LIGHTS)]


LIT_MAX_LIGHTS = 4        # RTMI_LIT_MAX_LIGHTS
LIT_INVERSE_SQUARE = 1    # RTMI_LIT_INVERSE_SQUARE
LIT_SURFACES = 4          # RTMI_LIT_SURFACES (bit 1 is not assigned)


class Lit(C.Structure):
    """rtmi_lit_t (include/rtmi.h): 168 bytes."""
    _fields_ = [("nlights", C.c_uint32), ("flags", C.c_uint32), ("lights", Light * LIT_MAX_LIGHTS),
                ("light_color", (C.c_float * 3) * LIT_MAX_LIGHTS)]


class PreviewOut(C.Structure):
    """rtmi_preview_out_t (include/rtmi.h): seven pointers, any may be NULL."""
    _fields_ = [("color", C.c_void_p), ("albedo", C.c_void_p), ("normal", C.c_void_p), ("ids", C.c_void_p), ("ao", C.c_void_p),
                ("shadow", C.c_void_p), ("irradiance", C.c_void_p)]


class Texture(C.Structure):
    """rtmi_texture_t (include/rtmi.h): a pointer to width * height * 3 floats, and three u32."""
    _fields_ = [("rgb", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32), ("flags", C.c_uint32)]


class NormalMaps(C.Structure):
    """rtmi_normal_maps_t (include/rtmi.h): a float and a u32."""
    _fields_ = [("strength", C.c_float), ("flags", C.c_uint32)]


class Rays(C.Structure):
    """rtmi_rays_t (include/rtmi.h): 16 bytes."""
    _fields_ = [("maxdepth", C.c_uint32), ("group", C.c_uint32), ("pixel0", C.c_uint32), ("flags", C.c_uint32)]


class RaysOut(C.Structure):
    """rtmi_rays_out_t (include/rtmi.h): five pointers, any may be NULL."""
    _fields_ = [("color", C.c_void_p), ("mean", C.c_void_p), ("albedo", C.c_void_p), ("normal", C.c_void_p), ("ids", C.c_void_p)]


class Bake(C.Structure):
    """rtmi_bake_t (include/rtmi.h): 24 bytes."""
    _fields_ = [("mode", C.c_uint32), ("rays", C.c_uint32), ("maxdepth", C.c_uint32), ("pixel0", C.c_uint32), ("flags", C.c_uint32),
                ("bias", C.c_float)]


class BakeOut(C.Structure):
    """rtmi_bake_out_t (include/rtmi.h): four pointers, any may be NULL."""
    _fields_ = [("light", C.c_void_p), ("open", C.c_void_p), ("orig", C.c_void_p), ("dir", C.c_void_p)]


class BakeLitOut(C.Structure):
    """rtmi_bake_lit_out_t (include/rtmi.h): rtmi_bake_out_t's four pointers and direct, any may be NULL."""
    _fields_ = [("light", C.c_void_p), ("open", C.c_void_p), ("orig", C.c_void_p), ("dir", C.c_void_p), ("direct", C.c_void_p)]


BAKE_POINTS, BAKE_TRIANGLES = 0, 1  # RTMI_BAKE_*


class Camera(C.Structure):
    """rtmi_camera_t (include/rtmi.h): 16 bytes."""
    _fields_ = [("model", C.c_uint32), ("flags", C.c_uint32), ("lens_radius", C.c_float), ("focus", C.c_float)]


class CameraOut(C.Structure):
    """rtmi_camera_out_t (include/rtmi.h): three pointers, each may be NULL."""
    _fields_ = [("albedo", C.c_void_p), ("normal", C.c_void_p), ("ids", C.c_void_p)]


CAMERA_PINHOLE, CAMERA_THIN_LENS, CAMERA_ORTHO = 0, 1, 2  # RTMI_CAMERA_*


class Environment(C.Structure):
    """rtmi_environment_t (include/rtmi.h): 40 bytes."""
    _fields_ = [("frame", C.c_float * 9), ("flags", C.c_uint32)]


class Envlight(C.Structure):
    """rtmi_envlight_t (include/rtmi.h): 8 bytes."""
    _fields_ = [("bias", C.c_float), ("flags", C.c_uint32)]


class Sky(C.Structure):
    """rtmi_sky_t (include/rtmi.h): 76 bytes."""
    _fields_ = [("up", C.c_float * 3), ("sun_dir", C.c_float * 3), ("sun_cos", C.c_float), ("zenith", C.c_float * 3),
                ("horizon", C.c_float * 3), ("ground", C.c_float * 3), ("sun_color", C.c_float * 3)]


class Tuning(C.Structure):
    """rtmi_tuning_t (include/rtmi.h)."""
    _fields_ = [("batch_paths", C.c_uint64), ("streams", C.c_uint32), ("subtile_min_paths", C.c_uint32),
                ("oct_waves_per_cu", C.c_uint32), ("refill_min0", C.c_uint32), ("refill_min", C.c_uint32),
                ("xcd_aware", C.c_uint32), ("kernel", C.c_uint32), ("pipeline", C.c_uint32), ("slow_path_off", C.c_uint32)]


def build(force=False):
    """Compile librtmi.so in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    if force:
        subprocess.check_call(["make", "-C", _CSRC, "clean"], stdout=subprocess.DEVNULL)
    subprocess.check_call(["make", "-C", _CSRC, "-j4"], stdout=subprocess.DEVNULL)
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(make -C rust_raytrace_amd/csrc). There is no CPU fallback for the render path.")
    # One HIP runtime per process: torch bundles its own libamdhip64 (SONAME libamdhip64.so.7) and
    # librtmi.so needs that SONAME, so with torch loaded FIRST both share torch's runtime (streams and
    # device pointers are then interchangeable).  Loaded the other way round the process ends up with
    # two runtimes and torch sees no GPU.  Without torch the system /opt/rocm runtime is used.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    vp, u64, u32, f32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_float, C.c_int
    L.rtmi_last_error.restype = C.c_char_p
    L.rth_last_error.restype = C.c_char_p
    L.rtmi_device_count.restype = i32
    L.rth_to_radians.restype = f32
    L.rth_to_radians.argtypes = [f32]
    L.rth_scene_new.restype = vp
    L.rth_scene_new.argtypes = [i32]
    L.rth_scene_free.argtypes = [vp]
    L.rth_num_tris.restype = u64
    L.rth_num_tris.argtypes = [vp]
    L.rth_make_color.argtypes = [C.c_uint8, C.c_uint8, C.c_uint8, vp]
    L.rth_unit.argtypes = [vp, vp]
    L.rth_create_transform.argtypes = [vp, f32, vp]
    L.rth_create_viewport.argtypes = [u32, u32, f32, f32, vp, vp, f32, f32, vp]
    L.rth_add_triangle.argtypes = [vp, vp, u32, vp, f32, f32, f32]
    L.rth_add_triangles_gpu.argtypes = [vp, vp, u64, u32, vp, f32, f32, f32, i32]
    L.rth_add_obj.argtypes = [vp, C.c_char_p, vp, f32, vp, u32, vp, f32, f32, f32]
    L.rth_add_obj_mode.argtypes = [vp, C.c_char_p, vp, f32, vp, u32, vp, f32, f32, f32, u32]
    L.rth_add_disk.argtypes = [vp, vp, vp, f32, f32, u64, u32, vp, f32, f32, u32, vp, f32, f32, f32]
    L.rth_add_sphere.argtypes = [vp, vp, f32, u64, u64, u32, vp, f32, f32, f32]
    L.rth_populate_triangle_numbers.argtypes = [vp]
    L.rtmi_environment_defaults.restype = None
    L.rtmi_environment_defaults.argtypes = [vp]
    L.rtmi_sky_defaults.restype = None
    L.rtmi_sky_defaults.argtypes = [vp]
    L.rtmi_scene_set_environment.argtypes = [vp, vp, u32, vp]
    L.rtmi_scene_get_environment.argtypes = [vp, vp, vp]
    L.rtmi_scene_set_sky.argtypes = [vp, u32, vp]
    L.rth_scene_set_environment.argtypes = [vp, vp, u32, vp]
    L.rth_scene_set_sky.argtypes = [vp, u32, vp]
    L.rth_scene_environment_size.argtypes = [vp, vp]
    L.rth_caster_environment.argtypes = [vp, vp, u64, vp]
    L.rtmi_scene_set_normals.argtypes = [vp, vp, vp, u64]
    L.rtmi_scene_get_normals.argtypes = [vp, vp, vp]
    L.rtmi_smooth_normals.argtypes = [vp, vp, u64, f32, vp]
    L.rth_scene_set_normals.argtypes = [vp, vp, u64, u64]
    L.rth_scene_smooth_normals.argtypes = [vp, u64, u64, f32]
    L.rth_scene_normals_size.argtypes = [vp, vp]
    L.rth_scene_get_normals.argtypes = [vp, vp, u64]
    L.rth_caster_normals.argtypes = [vp, vp, u64, vp]
    L.rth_add_obj_normals.argtypes = [vp, C.c_char_p, vp, f32, vp, u32, vp, f32, f32, f32, u32, u32, f32]
    L.rtmi_scene_set_textures.argtypes = [vp, vp, u32, vp, vp, vp, u64]
    L.rtmi_scene_get_uvs.argtypes = [vp, vp, vp, vp]
    L.rtmi_scene_get_texture.argtypes = [vp, u32, vp, vp, vp]
    L.rtmi_project_uvs.argtypes = [vp, vp, u64, vp, f32, vp]
    L.rth_scene_set_textures.argtypes = [vp, vp, u32]
    L.rth_scene_set_uvs.argtypes = [vp, vp, vp, u64, u64]
    L.rth_scene_project_uvs.argtypes = [vp, u64, u64, vp, f32, u32]
    L.rth_scene_textures_size.argtypes = [vp, vp, vp]
    L.rth_scene_get_uvs.argtypes = [vp, vp, vp, u64]
    L.rth_scene_get_texture.argtypes = [vp, u32, vp, u64, vp, vp]
    L.rth_caster_uvs.argtypes = [vp, vp, vp, u64, vp]
    L.rth_caster_texture.argtypes = [vp, u32, vp, u64, vp, vp]
    L.rth_add_obj_uvs.argtypes = [vp, C.c_char_p, vp, f32, vp, u32, vp, f32, f32, f32, u32, u32]
    L.rtmi_normal_maps_defaults.argtypes = [vp]
    L.rtmi_normal_maps_defaults.restype = None
    L.rtmi_scene_set_normal_maps.argtypes = [vp, vp, vp, u64, vp]
    L.rtmi_scene_get_normal_maps.argtypes = [vp, vp, vp, vp]
    L.rtmi_normal_map_frames.argtypes = [vp, vp, vp, vp, u64, vp]
    L.rtmi_normal_map_from_height.argtypes = [vp, u32, u32, f32, vp]
    L.rth_scene_set_normal_maps.argtypes = [vp, vp, u64, u64, f32, u32]
    L.rth_scene_normal_maps_size.argtypes = [vp, vp]
    L.rth_scene_get_normal_maps.argtypes = [vp, vp, vp, u64]
    L.rth_scene_normal_map_frames.argtypes = [vp, vp, u64]
    L.rth_caster_normal_maps.argtypes = [vp, vp, vp, u64, vp]
    L.rth_normal_map_from_height.argtypes = [vp, u32, u32, f32, vp]
    L.rth_add_analytic_sphere.argtypes = [vp, vp, f32, u32, vp, f32, f32]
    L.rth_build_bounding_box.argtypes = [vp, vp, f32, u64, u64, u32]
    L.rth_build_bounding_box_gpu.argtypes = [vp, vp, f32, u64, u64, i32]
    L.rth_build_trivial_bounding_box.argtypes = [vp, vp, f32]
    L.rth_box_contains_polygon.argtypes = [vp, vp, f32, u64]
    L.rth_face_contains_triangle.argtypes = [vp, vp, vp, f32, u64]
    L.rth_get_triangles.argtypes = [vp, vp, vp, vp]
    L.rth_tree_sizes.argtypes = [vp, vp, vp]
    L.rth_tree_get.argtypes = [vp, vp, vp, vp]
    L.rth_caster_config.argtypes = [vp, u64, i32, u32]
    L.rth_caster_upload.argtypes = [vp]
    L.rth_caster_set_tuning.argtypes = [vp, vp]
    L.rth_caster_set_devices.argtypes = [vp, vp, u32]
    L.rth_caster_walk_frame_multi.argtypes = [vp, u32, u32, vp, u64, u64, u32, u32, vp, vp, vp, vp, u32, vp]
    L.rth_caster_walk_rows.argtypes = [vp, u32, u32, vp, u64, u64, u64, u64, vp, vp, vp]
    L.rth_caster_walk_rows_device.argtypes = [vp, u32, u32, vp, u64, u64, u64, u64, vp, vp, vp, vp]
    L.rth_caster_walk_tile_device.argtypes = [vp, u32, u32, vp, u64, u64, vp, vp, vp, vp, vp]
    L.rth_caster_walk_samples.argtypes = [vp, u32, u32, vp, u64, u64, u64, u64, u32, u32, vp, vp, vp, vp]
    L.rth_caster_walk_samples_device.argtypes = [vp, u32, u32, vp, u64, u64, vp, u32, u32, vp, vp, vp, vp, vp]
    L.rtmi_render_samples.argtypes = [vp, vp, u64, u32, u32, u32, u32, vp, vp, vp]
    L.rtmi_render_samples_device.argtypes = [vp, vp, u64, vp, u32, u32, vp, vp, vp, vp]
    L.rth_caster_walk_features.argtypes = [vp, u32, u32, vp, u64, u64, u64, u64, u32, u32, vp, vp, vp, vp, vp]
    L.rth_caster_walk_features_device.argtypes = [vp, u32, u32, vp, u64, u64, vp, u32, u32, vp, vp, vp, vp, vp, vp]
    L.rtmi_render_features.argtypes = [vp, vp, u64, u32, u32, u32, u32, vp, vp, vp, vp]
    L.rtmi_render_features_device.argtypes = [vp, vp, u64, vp, u32, u32, vp, vp, vp, vp, vp]
    L.rth_caster_walk_adaptive.argtypes = [vp, u32, u32, vp, u64, u64, u64, u64, vp, vp, vp, vp, vp]
    L.rth_caster_walk_adaptive_device.argtypes = [vp, u32, u32, vp, u64, u64, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.rtmi_render_adaptive.argtypes = [vp, vp, u64, u32, u32, vp, vp, vp, vp]
    L.rtmi_render_adaptive_device.argtypes = [vp, vp, u64, vp, vp, vp, vp, vp, vp, vp, vp]
    L.rtmi_denoise_defaults.restype = None
    L.rtmi_denoise_defaults.argtypes = [vp]
    L.rtmi_denoise.argtypes = [vp, u32, u32, vp, vp, vp, vp, vp]
    L.rtmi_denoise_device.argtypes = [vp, u32, u32, vp, vp, vp, vp, vp, vp]
    L.rtmi_render_denoised.argtypes = [vp, vp, u64, vp, vp, vp]
    L.rth_caster_denoise.argtypes = [vp, u32, u32, vp, vp, vp, vp, vp]
    L.rth_caster_denoise_device.argtypes = [vp, u32, u32, vp, vp, vp, vp, vp, vp]
    L.rth_caster_walk_denoised.argtypes = [vp, u32, u32, vp, u64, u64, vp, vp, vp, vp]
    L.rtmi_denoise_var_defaults.restype = None
    L.rtmi_denoise_var_defaults.argtypes = [vp]
    L.rtmi_variance.argtypes = [vp, vp, vp, vp, u64, vp]
    L.rtmi_variance_device.argtypes = [vp, vp, vp, vp, u64, vp, vp]
    L.rtmi_denoise_var.argtypes = [vp, u32, u32, vp, vp, vp, vp, vp, vp, vp]
    L.rtmi_denoise_var_device.argtypes = [vp, u32, u32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.rtmi_render_adaptive_denoised.argtypes = [vp, vp, u64, vp, vp, vp, vp, vp]
    L.rth_caster_variance.argtypes = [vp, vp, vp, vp, u64, vp]
    L.rth_caster_variance_device.argtypes = [vp, vp, vp, vp, u64, vp, vp]
    L.rth_caster_denoise_var.argtypes = [vp, u32, u32, vp, vp, vp, vp, vp, vp, vp]
    L.rth_caster_denoise_var_device.argtypes = [vp, u32, u32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.rth_caster_walk_adaptive_denoised.argtypes = [vp, u32, u32, vp, u64, u64, vp, vp, vp, vp, vp, vp]
    L.rtmi_render_views.argtypes = [vp, vp, vp, u32, vp, vp]
    L.rtmi_render_views_device.argtypes = [vp, vp, vp, u32, vp, vp, vp, vp]
    L.rth_caster_walk_views.argtypes = [vp, u32, u32, u32, vp, u64, u64, vp, vp, vp, vp]
    L.rth_caster_walk_views_device.argtypes = [vp, u32, u32, u32, vp, u64, u64, vp, vp, vp, vp, vp, vp]
    L.rth_caster_quantize_device.argtypes = [vp, vp, u64, vp, vp]
    L.rth_caster_trace.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp]
    L.rth_quantize.argtypes = [vp, u64, vp]
    L.rtmi_occluded.argtypes = [vp, u64, vp, vp, vp, vp, vp]
    L.rtmi_occluded_device.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp]
    L.rth_caster_occluded.argtypes = [vp, u64, vp, vp, vp, vp, vp]
    L.rth_caster_occluded_device.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp]
    L.rtmi_trace_device.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp, vp]
    L.rth_caster_trace_device.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp, vp]
    L.rtmi_render_rays.argtypes = [vp, u64, vp, vp, vp, u64, vp, vp, vp]
    L.rtmi_render_rays_device.argtypes = [vp, u64, vp, vp, vp, u64, vp, vp, vp, vp]
    L.rth_caster_walk_rays_explicit.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp, vp]
    L.rth_caster_walk_rays_explicit_device.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp, vp, vp]
    L.rtmi_bake_defaults.restype = None
    L.rtmi_bake_defaults.argtypes = [vp]
    L.rtmi_bake.argtypes = [vp, u64, vp, vp, u64, vp, vp, vp]
    L.rtmi_bake_device.argtypes = [vp, u64, vp, vp, u64, vp, vp, vp, vp]
    L.rth_caster_bake.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp]
    L.rth_caster_bake_device.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp, vp]
    L.rtmi_camera_defaults.restype = None
    L.rtmi_camera_defaults.argtypes = [vp]
    L.rtmi_render_camera.argtypes = [vp, vp, u64, u32, u32, vp, u32, u32, vp, vp, vp, vp]
    L.rtmi_render_camera_device.argtypes = [vp, vp, u64, vp, vp, u32, u32, vp, vp, vp, vp, vp]
    L.rth_caster_walk_camera.argtypes = [vp, u32, u32, vp, u64, u64, u64, u64, vp, u32, u32, vp, vp, vp, vp, vp]
    L.rth_caster_walk_camera_device.argtypes = [vp, u32, u32, vp, u64, u64, vp, vp, u32, u32, vp, vp, vp, vp, vp, vp]
    L.rtmi_ao_defaults.restype = None
    L.rtmi_ao_defaults.argtypes = [vp]
    L.rtmi_render_ao.argtypes = [vp, vp, u64, u32, u32, u32, u32, vp, vp, vp]
    L.rtmi_render_ao_device.argtypes = [vp, vp, u64, vp, u32, u32, vp, vp, vp, vp]
    L.rth_caster_walk_ao.argtypes = [vp, u32, u32, vp, u64, u64, u64, u64, u32, u32, vp, vp, vp, vp]
    L.rth_caster_walk_ao_device.argtypes = [vp, u32, u32, vp, u64, u64, vp, u32, u32, vp, vp, vp, vp, vp]
    L.rtmi_light_defaults.restype = None
    L.rtmi_light_defaults.argtypes = [vp]
    L.rtmi_render_light.argtypes = [vp, vp, u64, u32, u32, u32, u32, vp, vp, vp, vp]
    L.rtmi_render_light_device.argtypes = [vp, vp, u64, vp, u32, u32, vp, vp, vp, vp, vp]
    L.rth_caster_walk_light.argtypes = [vp, u32, u32, vp, u64, u64, u64, u64, u32, u32, vp, vp, vp, vp, vp]
    L.rth_caster_walk_light_device.argtypes = [vp, u32, u32, vp, u64, u64, vp, u32, u32, vp, vp, vp, vp, vp, vp]
    L.rtmi_render_shadowed.argtypes = [vp, vp, u64, u32, u32, u32, u32, vp, vp, vp, vp]
    L.rtmi_render_shadowed_device.argtypes = [vp, vp, u64, vp, u32, u32, vp, vp, vp, vp, vp]
    L.rth_caster_walk_shadowed.argtypes = [vp, u32, u32, vp, u64, u64, u64, u64, u32, u32, vp, vp, vp, vp, vp]
    L.rth_caster_walk_shadowed_device.argtypes = [vp, u32, u32, vp, u64, u64, vp, u32, u32, vp, vp, vp, vp, vp, vp]
    L.rtmi_envlight_defaults.restype = None
    L.rtmi_envlight_defaults.argtypes = [vp]
    L.rtmi_scene_get_env_sampler.argtypes = [vp, vp, vp, vp]
    L.rtmi_render_envlight.argtypes = [vp, vp, u64, u32, u32, u32, u32, vp, vp, vp, vp]
    L.rtmi_render_envlight_device.argtypes = [vp, vp, u64, vp, u32, u32, vp, vp, vp, vp, vp]
    L.rth_caster_walk_envlight.argtypes = [vp, u32, u32, vp, u64, u64, u64, u64, u32, u32, vp, vp, vp, vp, vp]
    L.rth_caster_walk_envlight_device.argtypes = [vp, u32, u32, vp, u64, u64, vp, u32, u32, vp, vp, vp, vp, vp, vp]
    L.rth_caster_env_sampler.argtypes = [vp, vp, u64, vp, vp]
    L.rtmi_scene_set_emitters.argtypes = [vp, vp, vp, u64]
    L.rtmi_scene_get_emitter_sampler.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.rtmi_render_emissive.argtypes = [vp, vp, u64, u32, u32, u32, u32, vp, vp, vp]
    L.rtmi_render_emissive_device.argtypes = [vp, vp, u64, vp, u32, u32, vp, vp, vp, vp]
    L.rth_scene_set_emitters.argtypes = [vp, vp, u64, u64]
    L.rth_scene_get_emitters.argtypes = [vp, vp, u64]
    L.rth_caster_walk_emissive.argtypes = [vp, u32, u32, vp, u64, u64, u64, u64, u32, u32, vp, vp, vp, vp]
    L.rth_caster_walk_emissive_device.argtypes = [vp, u32, u32, vp, u64, u64, vp, u32, u32, vp, vp, vp, vp, vp]
    L.rth_caster_emitter_sampler.argtypes = [vp, vp, vp, vp, vp, u64, u64, vp, vp]
    L.rtmi_lit_defaults.restype = None
    L.rtmi_lit_defaults.argtypes = [vp]
    L.rtmi_render_lit.argtypes = [vp, vp, u64, u32, u32, u32, u32, vp, vp, vp, vp]
    L.rtmi_render_lit_device.argtypes = [vp, vp, u64, vp, u32, u32, vp, vp, vp, vp, vp]
    L.rth_caster_walk_lit.argtypes = [vp, u32, u32, vp, u64, u64, u64, u64, u32, u32, vp, vp, vp, vp, vp]
    L.rth_caster_walk_lit_device.argtypes = [vp, u32, u32, vp, u64, u64, vp, u32, u32, vp, vp, vp, vp, vp, vp]
    L.rtmi_render_rays_lit.argtypes = [vp, u64, vp, vp, vp, u64, vp, vp, vp, vp]
    L.rtmi_render_rays_lit_device.argtypes = [vp, u64, vp, vp, vp, u64, vp, vp, vp, vp, vp]
    L.rth_caster_walk_rays_explicit_lit.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp, vp, vp]
    L.rth_caster_walk_rays_explicit_lit_device.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.rtmi_bake_lit.argtypes = [vp, u64, vp, vp, u64, vp, vp, vp, vp]
    L.rtmi_bake_lit_device.argtypes = [vp, u64, vp, vp, u64, vp, vp, vp, vp, vp]
    L.rth_caster_bake_lit.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp, vp]
    L.rth_caster_bake_lit_device.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp, vp, vp]
    L.rtmi_preview_defaults.restype = None
    L.rtmi_preview_defaults.argtypes = [vp]
    L.rtmi_render_preview.argtypes = [vp, vp, u64, u32, u32, u32, u32, vp, vp, vp]
    L.rtmi_render_preview_device.argtypes = [vp, vp, u64, vp, u32, u32, vp, vp, vp, vp]
    L.rth_caster_walk_preview.argtypes = [vp, u32, u32, vp, u64, u64, u64, u64, u32, u32, vp, vp, vp, vp]
    L.rth_caster_walk_preview_device.argtypes = [vp, u32, u32, vp, u64, u64, vp, u32, u32, vp, vp, vp, vp, vp]
    L.rtmi_trace_records.argtypes = [vp, u64, vp, vp, vp, vp, u64, vp, vp]
    L.rtmi_primary_records.argtypes = [vp, vp, u64, u32, u32, u32, vp, vp, u64, vp, vp]
    L.rth_caster_trace_records.argtypes = [vp, u64, vp, vp, vp, vp, u64, vp, vp]
    L.rth_caster_primary_records.argtypes = [vp, u32, u32, vp, u64, u64, u32, u32, u32, vp, vp, u64, vp, vp]
    L.rth_scene_set_debug.argtypes = [vp, i32]
    L.rth_scene_debug_records.argtypes = [vp, vp, vp, vp, vp, vp]
    _lib = L
    return L


# every symbol include/rtmi.h and include/rtmi_host.h declare
RTMI_SYMBOLS = ["rtmi_device_count", "rtmi_scene_create", "rtmi_scene_destroy", "rtmi_scene_set_options",
                "rtmi_scene_get_tuning", "rtmi_scene_set_tuning", "rtmi_scene_set_spheres", "rtmi_environment_defaults", "rtmi_scene_set_environment", "rtmi_scene_get_environment", "rtmi_sky_defaults", "rtmi_scene_set_sky", "rtmi_scene_set_normals", "rtmi_scene_get_normals", "rtmi_smooth_normals", "rtmi_scene_set_textures", "rtmi_scene_get_uvs", "rtmi_scene_get_texture", "rtmi_project_uvs", "rtmi_normal_maps_defaults", "rtmi_scene_set_normal_maps", "rtmi_scene_get_normal_maps", "rtmi_normal_map_frames", "rtmi_normal_map_from_height", "rtmi_scene_set_corners", "rtmi_render", "rtmi_render_frame_multi",
                "rtmi_render_device", "rtmi_render_tile_device", "rtmi_render_samples", "rtmi_render_samples_device", "rtmi_render_features", "rtmi_render_features_device", "rtmi_denoise_defaults", "rtmi_denoise", "rtmi_denoise_device", "rtmi_render_denoised", "rtmi_denoise_var_defaults", "rtmi_variance", "rtmi_variance_device", "rtmi_denoise_var", "rtmi_denoise_var_device", "rtmi_render_adaptive_denoised", "rtmi_render_adaptive", "rtmi_render_adaptive_device", "rtmi_render_views", "rtmi_render_views_device", "rtmi_trace", "rtmi_occluded", "rtmi_occluded_device", "rtmi_trace_device", "rtmi_render_rays", "rtmi_render_rays_device", "rtmi_bake_defaults", "rtmi_bake", "rtmi_bake_device", "rtmi_camera_defaults", "rtmi_render_camera", "rtmi_render_camera_device", "rtmi_ao_defaults", "rtmi_render_ao", "rtmi_render_ao_device", "rtmi_light_defaults", "rtmi_render_light", "rtmi_render_light_device", "rtmi_render_shadowed", "rtmi_render_shadowed_device", "rtmi_envlight_defaults", "rtmi_scene_get_env_sampler", "rtmi_render_envlight", "rtmi_render_envlight_device", "rtmi_scene_set_emitters", "rtmi_scene_get_emitter_sampler", "rtmi_render_emissive", "rtmi_render_emissive_device", "rtmi_lit_defaults", "rtmi_render_lit", "rtmi_render_lit_device", "rtmi_render_rays_lit", "rtmi_render_rays_lit_device", "rtmi_bake_lit", "rtmi_bake_lit_device", "rtmi_preview_defaults", "rtmi_render_preview", "rtmi_render_preview_device", "rtmi_trace_records", "rtmi_primary_records", "rtmi_quantize", "rtmi_quantize_device", "rtmi_make_triangles", "rtmi_builder_create", "rtmi_builder_filter", "rtmi_builder_destroy", "rtmi_last_error"]
RTH_SYMBOLS = ["rth_last_error", "rth_make_color", "rth_unit", "rth_to_radians", "rth_create_transform",
               "rth_create_viewport", "rth_scene_new", "rth_scene_free", "rth_num_tris", "rth_add_triangle", "rth_add_triangles_gpu", "rth_add_obj", "rth_add_obj_mode",
               "rth_add_disk", "rth_add_sphere", "rth_add_analytic_sphere", "rth_scene_set_environment", "rth_scene_set_sky", "rth_scene_environment_size", "rth_caster_environment", "rth_scene_set_normals", "rth_scene_smooth_normals", "rth_scene_normals_size", "rth_scene_get_normals", "rth_caster_normals", "rth_add_obj_normals", "rth_scene_set_textures", "rth_scene_set_uvs", "rth_scene_project_uvs", "rth_scene_textures_size", "rth_scene_get_uvs", "rth_scene_get_texture", "rth_caster_uvs", "rth_caster_texture", "rth_add_obj_uvs", "rth_scene_set_normal_maps", "rth_scene_normal_maps_size", "rth_scene_get_normal_maps", "rth_scene_normal_map_frames", "rth_caster_normal_maps", "rth_normal_map_from_height", "rth_populate_triangle_numbers", "rth_build_bounding_box", "rth_build_bounding_box_gpu",
               "rth_build_trivial_bounding_box", "rth_box_contains_polygon", "rth_face_contains_triangle",
               "rth_get_triangles", "rth_tree_sizes", "rth_tree_get", "rth_caster_config", "rth_caster_walk_rows",
               "rth_caster_walk_rows_device", "rth_caster_walk_tile_device", "rth_caster_walk_samples", "rth_caster_walk_samples_device", "rth_caster_walk_features", "rth_caster_walk_features_device", "rth_caster_denoise", "rth_caster_denoise_device", "rth_caster_walk_denoised", "rth_caster_variance", "rth_caster_variance_device", "rth_caster_denoise_var", "rth_caster_denoise_var_device", "rth_caster_walk_adaptive_denoised", "rth_caster_walk_adaptive", "rth_caster_walk_adaptive_device", "rth_caster_walk_views", "rth_caster_walk_views_device", "rth_caster_trace", "rth_caster_occluded", "rth_caster_occluded_device", "rth_caster_trace_device", "rth_caster_walk_rays_explicit", "rth_caster_walk_rays_explicit_device", "rth_caster_bake", "rth_caster_bake_device", "rth_caster_walk_camera", "rth_caster_walk_camera_device", "rth_caster_walk_ao", "rth_caster_walk_ao_device", "rth_caster_walk_light", "rth_caster_walk_light_device", "rth_caster_walk_shadowed", "rth_caster_walk_shadowed_device", "rth_caster_walk_envlight", "rth_caster_walk_envlight_device", "rth_caster_env_sampler", "rth_scene_set_emitters", "rth_scene_get_emitters", "rth_caster_walk_emissive", "rth_caster_walk_emissive_device", "rth_caster_emitter_sampler", "rth_caster_walk_lit", "rth_caster_walk_lit_device", "rth_caster_walk_rays_explicit_lit", "rth_caster_walk_rays_explicit_lit_device", "rth_caster_bake_lit", "rth_caster_bake_lit_device", "rth_caster_walk_preview", "rth_caster_walk_preview_device", "rth_caster_trace_records", "rth_caster_primary_records", "rth_scene_set_debug", "rth_scene_debug_records", "rth_caster_upload", "rth_caster_set_tuning", "rth_caster_set_devices", "rth_caster_walk_frame_multi", "rth_caster_quantize_device", "rth_quantize"]
