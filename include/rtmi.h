/* rtmi.h — C ABI of the MI355X path-tracing core (librtmi.so).
 *
 * Drop-in boundary for rust_raytrace's `RayCaster` plug-in
 * (raytrace_lib/src/raytrace.rs:1128-1165).  A Rust `impl RayCaster for
 * HipRayCaster` flattens `Scene` once, calls rtmi_scene_create(), then
 * rtmi_render() from walk_rays_internal(); see INTEGRATION.md for the shim.
 *
 * Plain C: pointers and sizes only, no C++/torch types.  Every function
 * returns RTMI_OK (0) or an error code; the message for the calling thread is
 * available from rtmi_last_error().  No C++ exception crosses this boundary.
 * All functions are callable from any host thread (the reference enters its
 * caster from a scoped worker thread, raytrace.rs:1141-1146); one in-flight
 * render per scene handle.
 */
#ifndef RTMI_H
#define RTMI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    RTMI_OK = 0,
    RTMI_ERR_INVALID = 1,      /* bad argument / malformed scene            */
    RTMI_ERR_NO_DEVICE = 2,    /* no HIP device visible / bad device index  */
    RTMI_ERR_UNSUPPORTED = 3,  /* valid input outside what the kernels take */
    RTMI_ERR_OOM = 4,          /* host or device allocation failed          */
    RTMI_ERR_DEVICE = 5        /* any other HIP runtime / kernel failure    */
};

/* SurfaceKind (raytrace.rs:303-308), and one kind the reference does not have: RTMI_DIELECTRIC, clear or tinted glass, whose
 * `scattering` field carries the INDEX OF REFRACTION (the definition follows the sphere record below). */
enum { RTMI_SOLID = 0, RTMI_MATTE = 1, RTMI_REFLECTIVE = 2, RTMI_DIELECTRIC = 3 };

/* One `Triangle` (raytrace.rs:326-337) reduced to the fields the hot path
 * reads (intersects/normal/getsurface, raytrace.rs:399-461).  Lane 3 of every
 * Vec3 is +0 for records produced by make_triangle (raytrace.rs:340-383) and
 * is not transported. */
typedef struct rtmi_triangle {
    float incenter[3];
    float norm[3];
    float bounding_r2;
    float sides[3][3];
    float side_lens[3];
    float edge_thickness;
    uint32_t surface_kind; /* RTMI_SOLID / RTMI_MATTE / RTMI_REFLECTIVE / RTMI_DIELECTRIC */
    float color[3];
    float alpha;      /* Matte, Reflective, Dielectric */
    float scattering; /* Reflective; Dielectric: the index of refraction `ior`, finite and > 0 */
} rtmi_triangle_t;

/* One `BoundingBox` (raytrace.rs:618-623), flattened.  Inner box: its children
 * are boxes[first .. first+count) in the order of `BBSubobj::Boxes`.  Leaf:
 * its triangle indices are tri_refs[first .. first+count) in the order of
 * `BBSubobj::Tris`.  boxes[0] is the root (`Scene.boxes`). */
typedef struct rtmi_box {
    float orig[3];
    float len2; /* half edge length */
    uint32_t first;
    uint32_t count;
    uint32_t is_leaf;
    uint32_t depth;
} rtmi_box_t;

/* `Viewport` (raytrace.rs:1305-1318).  orig/cam/vu/vv are private in the
 * reference; the shim recomputes them with create_viewport's formula
 * (raytrace.rs:1343-1370) or the host crate makes them `pub`. */
typedef struct rtmi_viewport {
    uint32_t width, height;
    float orig[3], cam[3], vu[3], vv[3];
    uint32_t maxdepth;
    uint32_t samples_per_pixel;
} rtmi_viewport_t;

/* Work counters of one render/trace call.  `rays` is the reference's "Rays"
 * statistic: project_ray calls with depth > 0 (raytrace.rs:1278). */
typedef struct rtmi_stats {
    uint64_t rays;
    uint64_t box_tests, tri_tests, full_tests, nodes, leaves; /* filled only when counting is enabled */
    double kernel_ms;  /* device time span of the call (HIP events on the caller's stream)               */
    double trace_ms;   /* sum of the durations of the closest-hit launches (HIP events on their streams)  */
    uint32_t trace_launches;
    uint32_t streams;  /* internal streams that ran concurrently (1..4): launches overlap when > 1       */
    /* rtmi_render_frame_multi only (0 elsewhere): host wall-clock milliseconds of this scene's steps, so that a slow
     * link or a refused peer mapping is visible per device instead of only in the frame time */
    double render_ms;       /* rtmi_render_tile_device of this scene's tile                                  */
    double band_copy_ms;    /* (quantise +) the band's one crossing to the root device, synchronised           */
    double deinterleave_ms; /* scenes[0] only: k_deinterleave (+ the copy to out_host)                         */
    /* pipeline 3 (rtmi_tuning_t.pipeline): trace_ms split into its two parts, summed over streams and batches        */
    double primary_ms;      /* k_path_primary launches (pixel_ray + closest hit + color_ray of the primary rays;
                             * it also traces the mirror reflections of primary hits in place:
                             * RTMI_MIRROR_INPLACE)                                            */
    double bounce_ms;       /* the bounce passes' closest-hit launches (k_trace_oct)                               */
    /* (rtmi_render_ao*: primary_ms = the primary rays' closest-hit launches, bounce_ms = the AO rays' walk launches)     */
    /* (rtmi_render_light*: likewise, bounce_ms = the live shadow rays' walk launches)                                    */
    /* (rtmi_render_shadowed*: primary_ms = the closest-hit launches of ALL passes, bounce_ms = the shadow rays' walk launches) */
    int32_t peer_access;    /* 1 = this device writes the root device's memory directly (peer access enabled, or the
                             * same device); 0 = the runtime refused: the band is staged (rtmi_last_error() carries a
                             * warning although the call returns RTMI_OK)                                      */
    uint32_t pipeline;      /* which pipeline rendered (rtmi_tuning_t.pipeline: 1 or 3)                            */
    uint32_t slow_paths;    /* paths handed to k_path_slow (rtmi_tuning_t.slow_path_off)                           */
    uint32_t reserved;
} rtmi_stats_t;

/* A set of image rows: `nrows` rows taken in stripes of `stripe_rows`
 * consecutive rows, the k-th stripe starting at row0 + k*stripe_step.
 * {row0, nrows, nrows, 0} is the contiguous band [row0, row0+nrows).
 * Interleaved stripes are how a frame is tiled over the GPUs of a node: rank r
 * of N takes {r*S, H/N, S, N*S}; cost per row is very uneven (sky vs teapot). */
typedef struct rtmi_tile {
    uint32_t row0, nrows, stripe_rows, stripe_step;
} rtmi_tile_t;

/* Analytic sphere.  NOT part of the reference at this revision (its only `Collidable` is `Triangle`, raytrace.rs:399;
 * spheres are tessellated by make_sphere, raytrace.rs:464-529); BASELINE's north_star names an analytic ray-sphere
 * test, so this build defines one -- parity with the Rust binary is unpinned by construction.  Semantics (DESIGN.md 4.6 states
 * them operation by operation): standard quadratic in the reference's Vec3 arithmetic, `t < 0` is a miss like
 * for triangles, the far root counts as a Back-face hit from inside, normal = (point - center).unit(); no edge faces.
 * A scene's spheres are a flat list: every ray is tested against every sphere AFTER the box tree and a sphere replaces
 * the tree's hit iff it is strictly closer.  Reported hit index = ntris + sphere index.
 * Intended, not an oversight: there is no origin-primitive exclusion and no epsilon, exactly as for the reference's
 * triangles (`t < 0` is the only rejection, raytrace.rs:402-405; bounce origins are moved 0.001 along the NEW direction's
 * random part, raytrace.rs:284-296, which can leave them a rounding error inside the surface).  A bounce ray whose
 * rounded origin lies just inside its sphere therefore re-hits it from inside at t ~ 0 (Back face), as a reference
 * bounce ray can re-hit the plane of the triangle it left; Matte/Reflective spheres are darker for it. */
typedef struct rtmi_sphere {
    float center[3];
    float radius;
    uint32_t surface_kind; /* RTMI_SOLID / RTMI_MATTE / RTMI_REFLECTIVE / RTMI_DIELECTRIC */
    float color[3];
    float alpha;
    float scattering; /* Reflective; Dielectric: the index of refraction `ior`, finite and > 0 */
} rtmi_sphere_t;

/* RTMI_DIELECTRIC: refraction and Fresnel reflection.  NOT part of the reference, which has no surface that
 * transmits light, so this build defines one, operation by operation like the camera models and the bake.  `color` and `alpha`
 * mean what they mean for Matte and Reflective -- the level's terms in color_ray's mix_color(color, c, alpha): alpha = 1 is clear
 * glass, smaller values tint it -- and `scattering` carries the index of refraction `ior`.  rtmi_scene_create and
 * rtmi_scene_set_spheres refuse an ior that is NaN, infinite or <= 0 with RTMI_ERR_INVALID and name the first offender; kinds
 * above 3 stay "unknown surface kind".  The surface table's key of a dielectric includes alpha and ior, so distinct glasses stay
 * distinct surfaces.
 *
 * Everything but the bounce ray is Matte's: the surface is pushed on the path's stack, an exhausted depth is black, the fold
 * is the existing loop, the edge faces of a glass triangle stay Solid black.  The bounce ray of the hit of a path's ray number
 * `pass` with remaining depth maxdepth - pass - 1 != 0 -- (ro, rd) the ray, point = rd * t + ro, norm the surface's normal
 * (already * -1.f on a back face, `face & 1`; an analytic sphere's is (point - center).unit(), and its far root is the back
 * face, so a glass ball refracts in and out), rv = random_vec of RNG block pass + 1 -- uses only + - * / and sqrt in f32, no
 * contraction, every step rounded on all four lanes:
 *     ci   = fabsf(vdot(rd, norm))                         (reflect_ray's ddot)
 *     eta  = (face & 1) ? ior : 1.f / ior                  (front face: entering the solid; back face: leaving it)
 *     s2   = 1.f - ci * ci
 *     k    = 1.f - (eta * eta) * s2
 *     tir  = !(k >= 0.f)                                   (total internal reflection; a NaN reflects)
 *     ct   = sqrtf(k)                                      (cosine of the transmitted angle; unused when tir)
 *     cs   = (face & 1) ? ct : ci                          (Schlick takes the cosine on the thin side)
 *     r0   = (1.f - ior) / (1.f + ior);  r0 = r0 * r0
 *     x    = 1.f - cs;  x2 = x * x;  x5 = (x2 * x2) * x
 *     R    = r0 + (1.f - r0) * x5
 *     u    = unit float (top 24 bits * 2^-24) of WORD 3 of RNG block pass + 1 of (seed, pixel, sample): the block random_vec
 *            already draws words 0-2 of; no new block, and no other draw moves
 *     reflect iff tir || u < R
 * Reflected ray: reflect_ray's statements (raytrace.rs:278-290) with scattering = 0.f, the double normalisation included.
 * Refracted ray:
 *     perp = vmul(vadd(rd, vmul(norm, ci)), eta)
 *     par  = vmul(norm, -ct)
 *     td   = vunit(vadd(perp, par))
 *     ray  = make_ray(vadd(point, vmul(td, 0.001f)), td)   (the origin is offset along the new direction, as every bounce's)
 * There are no clamps and no special cases.  As a consequence a ci that is a rounding error above 1 gives a slightly negative s2
 * and x, and ior = 1.f runs the same arithmetic (eta = 1, r0 = 0, R = x5).
 * FRONT MEANS OUTSIDE: the front face of a triangle (the side its `norm` points to) is taken to be the outside of the solid.  A
 * mesh whose norms point into the solid behaves as a bubble of the inverse index.
 *
 * A scene with at least one dielectric triangle or sphere renders on the per-pass pipeline (stats.pipeline = 1, slow_paths = 0;
 * zero-component rays are traced in place) with the glass shading kernels (k_shade*_glass), whatever the scene kind and options:
 * rtmi_render, _device, _tile_device, rtmi_render_samples*, rtmi_render_adaptive*, rtmi_render_views*, rtmi_render_frame_multi,
 * rtmi_render_camera*, rtmi_render_rays*, rtmi_bake* and the two denoised wrappers all gain it.  Scenes without one take exactly
 * the path they took before the kind existed.
 * Unchanged: rtmi_trace*, rtmi_occluded* and the records; rtmi_render_features*, _ao*, _light*, _preview*, which read first hits
 * only -- glass shows its `color` as albedo and occludes AO and shadow rays like any other surface.
 * rtmi_render_shadowed* returns RTMI_ERR_UNSUPPORTED for a scene with a dielectric, before any HIP call.
 * Not here: transparent shadows, Beer-Lambert absorption, rough glass, nested media (no stack of indices: every back face leaves
 * into ior 1), glass in the path kernels (pipeline 3), glass under rtmi_render_shadowed*. */

typedef struct rtmi_scene rtmi_scene_t;

/* Number of visible HIP devices (0 when none); never fails. */
int rtmi_device_count(void);

/* Upload a scene to `device` and keep it resident until rtmi_scene_destroy().
 * tris[0] is the never-rendered sentinel (raytrace.rs:791, :849); a hit index
 * of 0 means "miss".  Replaces the per-batch cudaMalloc/cudaMemcpy of
 * exec_cuda_raytrace (cuda_raytrace_lib/src/cuda_rt.cu:381-425). */
int rtmi_scene_create(const rtmi_triangle_t* tris, uint64_t ntris,
                      const rtmi_box_t* boxes, uint64_t nboxes,
                      const uint32_t* tri_refs, uint64_t nrefs,
                      int device, rtmi_scene_t** out);
int rtmi_scene_destroy(rtmi_scene_t* scene);

/* Replace the scene's list of analytic spheres (n may be 0).  At most 4096 spheres (they are not in the tree). */
int rtmi_scene_set_spheres(rtmi_scene_t* scene, const rtmi_sphere_t* spheres, uint64_t n);

/* THE ENVIRONMENT OF A SCENE: an HDR map looked up where a path escapes.  NOT part of the reference, whose
 * color_ray returns one constant for every miss ((128, 180, 255) / 255, raytrace.rs:1264), so this build defines it, operation
 * by operation like the camera models and the dielectric.  A scene with an environment starts the fold of a path that leaves it
 * at the map's colour in the direction of the path's last ray.  Nothing else of color_ray's chain moves: no RNG draw, no ray
 * count, black at exhausted depth and at edge faces.
 *
 * The map is an n x n table over the octahedral map of the directions (pole axis: map-space z), 1 <= n <= 4096; `rgb` is
 * n * n * 3 floats, row-major, texel (i, j) = row j, column i at rgb[3 * (j * n + i)].  Texels may be any float: values above 1
 * are the point, the float image carries them and rtmi_quantize* clamps as it always did.  `frame` holds the rows r0, r1, r2 that
 * take a world direction to map space.  On the device the table is one float4 per texel with lane 3 +0.f, as the sky
 * constant's is; so is lane 3 of r0..r2.
 *
 * The lookup for a unit direction d, float32 throughout, + - * /, fabsf, floorf and comparisons only, every step rounded (no
 * fused multiply-add), plain loads (no texture unit, whose fixed-point weights could not be restated), mix_color =
 * c1 * (1.f - a) + c2 * a lane by lane (raytrace.rs:299-301), vdot the ordered sum seeded with +0 (raytrace.rs:65-77):
 *     m  = (vdot(r0, d), vdot(r1, d), vdot(r2, d))
 *     a  = (|m.x| + |m.y|) + |m.z|;  px = m.x / a;  py = m.y / a
 *     if m.z < 0.f:  (px, py) = ((1.f - |py|) * sg(px), (1.f - |px|) * sg(py)), both from the old values, sg(v) = v >= 0.f ? 1.f : -1.f
 *     fx = (px * 0.5f + 0.5f) * (float)n - 0.5f;  fy likewise from py
 *     cx = !(fx >= -1.f) ? -1.f : (fx > (float)n ? (float)n : fx);  cy likewise     (a NaN becomes -1)
 *     ix = (int)floorf(cx);  iy = (int)floorf(cy);  tx = fx - floorf(fx);  ty = fy - floorf(fy)
 *     texel(i, j):  ox = i < 0 || i >= n;  oy = j < 0 || j >= n;  ic = clamp(i, 0, n - 1);  jc = clamp(j, 0, n - 1);
 *                   if ox: jc = n - 1 - jc;  if oy: ic = n - 1 - ic;  the table's entry jc * n + ic
 *     c  = mix_color(mix_color(texel(ix, iy), texel(ix + 1, iy), tx), mix_color(texel(ix, iy + 1), texel(ix + 1, iy + 1), tx), ty)
 * The border rule is the octahedral map's: points x and -x of an outer edge of the square are the same direction, so the filter
 * stays continuous across the fold instead of clamping to the edge.  The indices come from the clamped coordinates, so no
 * direction reads outside the table; the weights come from the unclamped ones.  For every direction that is not NaN the clamp
 * changes nothing (|px|, |py| <= 1, so fx lies in [-0.5, n - 0.5]) and the two are the same numbers; a NaN, infinite or zero
 * direction reads four texels of the table's corners and yields a NaN colour.
 *
 * rtmi_scene_set_environment: rgb == NULL or n == 0 removes the environment, and the scene is exactly the scene it was before.
 * env == NULL: the defaults (identity frame, flags 0).  n > 4096, a frame entry that is not finite or flags != 0:
 * RTMI_ERR_INVALID before any HIP call.  Setting, replacing or removing waits for the scene's work to finish first (one call at
 * a time per handle, as everywhere).
 * rtmi_scene_set_sky fills the table on the device (k_env_sky) under the identity frame, so that the feature is usable without
 * an HDR file.  Texel (i, j) runs the inverse of the map:
 *     px = ((float)i + 0.5f) / (float)n * 2.f - 1.f;  py likewise from j;  z = (1.f - |px|) - |py|
 *     if z < 0.f: the same swap-and-sign rule on the old (px, py);  dir = vunit(px, py, z)
 *     h = vdot(dir, vunit(up));  c = h < 0.f ? ground : mix_color(horizon, zenith, h)
 *     if vdot(dir, vunit(sun_dir)) >= sun_cos:  c = c + sun_color
 * sun_cos is the cosine of the sun disc's angular radius.  n outside 1..4096, a zero or non-finite up or sun_dir:
 * RTMI_ERR_INVALID before any HIP call.
 * rtmi_scene_get_environment copies the device table back as rgb (rgb_out may be NULL); *n_out = 0 means there is none.
 *
 * A scene with an environment renders on the per-pass pipeline (stats.pipeline = 1, slow_paths = 0) with the environment shading
 * kernels (k_shade*_env, which also know RTMI_DIELECTRIC), whatever the scene kind and options: rtmi_render, _device,
 * _tile_device, rtmi_render_samples*, rtmi_render_adaptive*, rtmi_render_views*, rtmi_render_frame_multi (each scene handle
 * carries its own table), rtmi_render_camera*, rtmi_render_rays*, rtmi_bake* (`light`; `open` counts misses as before) and the
 * two denoised wrappers all gain it.  Scenes without one take exactly the path they took before.
 * Unchanged: rtmi_trace*, rtmi_occluded*, the records; rtmi_render_features*, _ao*, _light*, _preview* and the guide buffers of
 * the camera and explicit-ray calls, which read first hits only: a miss's albedo stays the sky constant with coverage 0.
 * rtmi_render_shadowed* returns RTMI_ERR_UNSUPPORTED for a scene with an environment, before any HIP call.
 * Importance sampling of the map, with next-event estimation towards its bright texels: rtmi_render_envlight*, "SAMPLING THE
 * ENVIRONMENT" below.
 * Not here: an environment in the path kernels (pipeline 3), image file loading, equirectangular input, mip-mapped lookups. */
typedef struct rtmi_environment { float frame[9]; uint32_t flags; /* 0 */ } rtmi_environment_t;
void rtmi_environment_defaults(rtmi_environment_t* env); /* identity frame, flags 0 */
int rtmi_scene_set_environment(rtmi_scene_t* scene, const float* rgb /* n * n * 3, or NULL */, uint32_t n,
                               const rtmi_environment_t* env /* or NULL = defaults */);
int rtmi_scene_get_environment(rtmi_scene_t* scene, float* rgb_out /* n * n * 3, or NULL */, uint32_t* n_out);
typedef struct rtmi_sky {
    float up[3], sun_dir[3], sun_cos;
    float zenith[3], horizon[3], ground[3], sun_color[3];
} rtmi_sky_t;
void rtmi_sky_defaults(rtmi_sky_t* sky); /* up +y, a sun of 5.7 degrees radius up and to the left behind the canonical camera */
int rtmi_scene_set_sky(rtmi_scene_t* scene, uint32_t n, const rtmi_sky_t* sky /* or NULL = defaults */);

/* VERTEX NORMALS OF A SCENE: smooth shading, per-vertex normals interpolated at every hit.  NOT part of the
 * reference, which shades every hit with its triangle's one geometric normal, so this build defines it, operation by operation
 * like the camera models, the dielectric and the environment.  A scene may carry, per triangle, its three corners c0, c1, c2 and
 * three corner normals n0, n1, n2: 9 + 9 floats per triangle, n = ntris, entry 0 the sentinel's and ignored.  Lane 3 of every
 * vector is +0 on the device.  A triangle whose nine normal floats are all zero is flat.
 *
 * All arithmetic is f32, + - * / and sqrt only, no contraction, every step rounded on all lanes; vdot (the ordered sum seeded
 * with +0), vunit (multiply by 1.f / sqrtf(vdot(a, a))), vadd, vsub, vmul are the reference's Vec3 operations.
 * Per triangle, once, when the normals are set:
 *     e1 = c1 - c0;  e2 = c2 - c0
 *     d00 = vdot(e1, e1);  d01 = vdot(e1, e2);  d11 = vdot(e2, e2);  den = d00 * d11 - d01 * d01
 * At a hit of a triangle (not an analytic sphere, not an edge face), with point = rd * t + ro as color_ray computes it and ng the
 * record's normal, already * -1.f on a back face:
 *     w   = point - c0;  d20 = vdot(w, e1);  d21 = vdot(w, e2)
 *     b1  = (d11 * d20 - d01 * d21) / den;  b2 = (d00 * d21 - d01 * d20) / den;  b0 = (1.f - b1) - b2
 *     ns  = vunit(vadd(vadd(vmul(n0, b0), vmul(n1, b1)), vmul(n2, b2)));  if (face & 1) ns = vmul(ns, -1.f)
 *     use = vdot(ns, ng) > 0.f && vdot(rd, ns) < 0.f
 *     norm = use ? ns : ng
 * There are no clamps and no special cases.  A flat triangle gives vunit(0) = NaN, so `use` is false and it is shaded exactly as
 * without normals; so is a degenerate one (den = 0).  A shading normal that faces away from the incoming ray, or away from the
 * geometric side that was hit, falls back to ng.  Hits in the edge band extrapolate slightly (b outside [0, 1]).
 * `norm` feeds the bounce unchanged: lambertian_ray, reflect_ray, the whole RTMI_DIELECTRIC arm.  One more rule keeps a bounce ray
 * on the right side of the real surface.  Evaluate the kind's bounce with `norm`; let dir be the direction as passed to make_ray
 * (Matte: norm + rv; reflection: vunit(reflect + rv * scattering); refraction: td) and side = -1.f for a refracted ray, +1.f
 * otherwise.  If use && !(side * vdot(dir, ng) > 0.f), evaluate the whole bounce again from the top with norm = ng: the same rv,
 * the same u, no new draw.  No RNG draw moves; the fold, the stack push, black at exhausted depth and at edge faces are untouched.
 * Only hits that bounce (not Solid, remaining depth not exhausted) look at the normals.
 * Guide normals (rtmi_render_features*, the guides of rtmi_render_camera*, rtmi_render_rays* and rtmi_render_preview*): a triangle
 * hit's normal is `norm` as above, from the primary ray's ro and rd, whatever the surface kind (no second rule: nothing bounces).
 * Albedo, coverage, depth and ids do not change.
 *
 * rtmi_scene_set_normals: n must equal ntris.  normals9 == NULL or n == 0 removes the normals, and the scene is exactly the scene
 * it was before.  A corner or normal that is not finite (entry 0 aside): RTMI_ERR_INVALID before any HIP call.  Setting,
 * replacing or removing waits for the scene's work to finish first.  The corners must be the ones the records came from.
 * rtmi_scene_get_normals copies the device table's normals back (normals9_out may be NULL; entry 0 reads as zeros); *n_out = 0
 * means there are none.
 *
 * rtmi_smooth_normals generates corner normals from shared corner POSITIONS (host code, no device needed; no sentinel: all n
 * triangles count).  facenorm3: the records' normals.  Per triangle g: x = cross(c1 - c0, c2 - c0), components written out as
 * a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x; a_g = sqrtf(vdot(x, x)); w_g = vmul(facenorm_g, a_g).
 * Corner k of triangle f: s = +0; for g in increasing index, if some corner of g compares == to c_fk in all three components, and
 * g == f or vdot(facenorm_f, facenorm_g) >= crease_cos, then s = vadd(s, w_g), each g at most once per corner; n_fk = vunit(s).
 * Area-weighted, so slivers do not tilt a vertex; crease_cos keeps edges sharper than its angle sharp (1: every corner gets its own
 * face's normal; -1: everything that shares the position is averaged).  crease_cos outside [-1, 1] or NaN: RTMI_ERR_INVALID.
 *
 * A scene with vertex normals renders on the per-pass pipeline (stats.pipeline = 1, slow_paths = 0) with the smooth shading
 * kernels (k_shade*_smooth, which also know RTMI_DIELECTRIC and the environment) and k_features_smooth, whatever the scene kind
 * and options: every call that gains glass gains this.  rtmi_bake*'s generator takes the caller's normal as before; its traced
 * paths bounce smoothly.  Unchanged: rtmi_trace*, rtmi_occluded*, the records, rtmi_render_ao*, _light* and the AO and light of
 * _preview*, which use the geometric normal.  rtmi_render_shadowed* returns RTMI_ERR_UNSUPPORTED, before any HIP call.
 * Not here: vertex normals in AO, light and preview shading; in the path kernels (pipeline 3); under rtmi_render_shadowed*; a
 * softened shadow terminator.  (Normal maps: the section after the textures'.) */
int rtmi_scene_set_normals(rtmi_scene_t* scene, const float* corners9, const float* normals9 /* or NULL */, uint64_t n);
int rtmi_scene_get_normals(rtmi_scene_t* scene, float* normals9_out /* n * 9, or NULL */, uint64_t* n_out);
int rtmi_smooth_normals(const float* corners9, const float* facenorm3, uint64_t n, float crease_cos, float* normals9_out);

/* TEXTURES OF A SCENE: per-corner texture coordinates and a bilinear image lookup at every hit.  NOT part of the
 * reference, which has neither uvs nor images, so this build defines it, operation by operation like the environment and the
 * vertex normals.  All arithmetic is f32: + - * /, floorf and comparisons only, plain loads (not the texture unit), no
 * contraction, every step rounded.  vdot, mix_color are the reference's.
 *
 * Images: rtmi_texture_t.rgb is width * height * 3 floats, row-major, texel (i, j) at rgb[3 * (j * width + i)], row 0 is v = 0.
 * Any float value is allowed.  On the device a texel is one float4 with lane 3 = +0; all images sit in one buffer behind a table
 * of (offset, width, height) per image.  Limits: ntex <= 256, width and height 1..8192, at most 2^26 texels in all; flags = 0.
 * UVs: n must equal ntris, entry 0 the sentinel's and ignored; uvs6 = (u0, v0, u1, v1, u2, v2) per triangle; tex_of_tri[i] = 0 for
 * no texture or 1..ntex; corners9 as in rtmi_scene_set_normals.  Per triangle, once, by exactly that section's statements:
 *     e1 = c1 - c0;  e2 = c2 - c0
 *     d00 = vdot(e1, e1);  d01 = vdot(e1, e2);  d11 = vdot(e2, e2);  den = d00 * d11 - d01 * d01
 * A triangle with den == 0.f is stored with texture 0.
 *
 * The colour of a hit of a triangle (not an analytic sphere, not an edge face) with tex_of_tri != 0, image W x H, with
 * point = rd * t + ro as color_ray computes it:
 *     w = point - c0;  d20 = vdot(w, e1);  d21 = vdot(w, e2)
 *     b1 = (d11 * d20 - d01 * d21) / den;  b2 = (d00 * d21 - d01 * d20) / den;  b0 = (1.f - b1) - b2
 *     u = (u0 * b0 + u1 * b1) + u2 * b2;  v = (v0 * b0 + v1 * b1) + v2 * b2
 *     fu = u - floorf(u);  fv = v - floorf(v)                                                        (repeat)
 *     fx = fu * (float)W - 0.5f;  fy = fv * (float)H - 0.5f
 *     cx = !(fx >= -1.f) ? -1.f : (fx > (float)W - 1.f ? (float)W - 1.f : fx);  cy likewise with H    (indices only; a NaN gives -1)
 *     ix = (int)floorf(cx);  iy = (int)floorf(cy);  tx = fx - floorf(fx);  ty = fy - floorf(fy)      (weights: the unclamped values)
 *     wrap(i, N) = i < 0 ? i + N : (i >= N ? i - N : i);  T(i, j) = texel (wrap(i, W), wrap(j, H))
 *     tc = mix_color(mix_color(T(ix, iy), T(ix + 1, iy), tx), mix_color(T(ix, iy + 1), T(ix + 1, iy + 1), tx), ty)
 *     colour = (material.color.x * tc.x, material.color.y * tc.y, material.color.z * tc.z, +0)
 * For every value that is not NaN the clamp changes no index: fx lies in [-0.5, W - 0.5] (fu == 1.f, which a tiny negative u rounds
 * to, included), so ix is in [-1, W - 1] and one wrap step is enough down to W = 1.  A NaN coordinate reads texels near index
 * W - 1 or 0 and gives a NaN colour.  alpha, scattering and the kind stay the material's; an untextured hit's colour is the
 * material's, unmodified.  The four loads are issued together.
 * Where the colour goes: a Solid hit ends its path with `colour`.  Every other hit pushes (colour.rgb, material.alpha) on a colour
 * stack beside the surface stack, and the fold of the nested mix_color calls reads the level's colour and alpha there.  No draw and
 * no ray count moves; black at edge faces and at exhausted depth (the level is still pushed and coloured).  Guides: the albedo of
 * rtmi_render_features* and of the guides of rtmi_render_camera* and rtmi_render_rays* is `colour` for such a hit; coverage, normal,
 * depth and ids are unchanged.
 *
 * rtmi_scene_set_textures: tex == NULL or ntex == 0 removes everything, and the scene is exactly the scene it was before.
 * RTMI_ERR_INVALID before any HIP call, naming the first offender: flags != 0, a limit exceeded, a tex_of_tri above ntex, a corner
 * or uv of a textured triangle that is not finite.  Setting, replacing or removing waits for the scene's work to finish first.
 * rtmi_scene_get_uvs copies the device table's uvs and texture numbers back (either may be NULL; *n_out = 0: no textures; a
 * degenerate triangle reads as texture 0).  rtmi_scene_get_texture: image k = 1..ntex of the device's buffer (rgb_out may be NULL
 * for the size alone).
 * rtmi_project_uvs (host code, no device needed; no sentinel: all n triangles count) is a box projection.  Per triangle the axis a
 * is that of the largest |facenorm| component: x if |x| >= |y| and |x| >= |z|, else y if |y| >= |z|, else z.  Corner p gets
 * (u, v) = ((p[j] - lo[j]) * scale, (p[k] - lo[k]) * scale) with (j, k) = (y, z) for a = x, (z, x) for a = y, (x, y) for a = z.
 *
 * A scene with textures renders on the per-pass pipeline (stats.pipeline = 1, slow_paths = 0) with the k_shade*_tex kernels (which
 * also know RTMI_DIELECTRIC, the environment and vertex normals) and k_features_tex, whatever the scene kind and options: every call
 * that gains vertex normals gains this.  Unchanged: rtmi_trace*, rtmi_occluded*, the records, rtmi_render_ao*, _light*.
 * rtmi_render_shadowed* and rtmi_render_preview* return RTMI_ERR_UNSUPPORTED, before any HIP call.
 * rtmi_scene_set_textures (set, replace or remove) also removes the scene's normal maps (the next section): the image numbers they
 * name are gone.  A scene without maps behaves as it always did.
 * Not here: mip maps and any minification filter, clamp or mirror wrap modes, textures on analytic spheres, roughness and alpha
 * maps, sRGB decoding and image file loading, textures in the path kernels (pipeline 3), under the preview and the shadowed
 * call. */
typedef struct rtmi_texture { const float* rgb; uint32_t width, height, flags /* 0 */; } rtmi_texture_t;
int rtmi_scene_set_textures(rtmi_scene_t* scene, const rtmi_texture_t* tex /* or NULL */, uint32_t ntex, const float* corners9,
                            const float* uvs6, const uint32_t* tex_of_tri, uint64_t n);
int rtmi_scene_get_uvs(rtmi_scene_t* scene, float* uvs6_out /* n * 6, or NULL */, uint32_t* tex_of_tri_out /* n, or NULL */, uint64_t* n_out);
int rtmi_scene_get_texture(rtmi_scene_t* scene, uint32_t k, float* rgb_out /* or NULL */, uint32_t* w_out, uint32_t* h_out);
int rtmi_project_uvs(const float* corners9, const float* facenorm3, uint64_t n, const float lo[3], float scale, float* uvs6_out);

/* NORMAL MAPS OF A SCENE: tangent-space normals looked up at every bouncing hit.  NOT part of the reference, which
 * has nothing of the kind, so this build defines it, operation by operation like its neighbours.  All arithmetic is f32: + - * /,
 * sqrt, floorf and comparisons only, plain loads, no contraction, every step rounded, lane 3 of every vector +0.  vdot, vunit,
 * vadd, vsub, vmul are the reference's; cross(a, b) is written out component by component as in rtmi_smooth_normals:
 * (a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x, +0).
 *
 * A normal map is one of the images rtmi_scene_set_textures stored; its texel rgb encodes a tangent-space vector as 2 * rgb - 1.
 * A triangle names its map by nmap_of_tri (0 = none, 1..ntex), independent of tex_of_tri: a triangle may have a map and no colour
 * texture, and its colour is then the material's, bit for bit.  The uvs are the ones rtmi_scene_set_textures stored.
 * Per triangle, once, on the host, when the maps are set; e1, e2, den by the texture section's statements from corners9, (u0, v0),
 * (u1, v1), (u2, v2) the stored uvs, ngeom the record's (front) normal:
 *     du1 = u1 - u0;  du2 = u2 - u0;  dv1 = v1 - v0;  dv2 = v2 - v0
 *     det = du1 * dv2 - du2 * dv1
 *     T = vsub(vmul(e1, dv2), vmul(e2, dv1));  B = vsub(vmul(e2, du1), vmul(e1, du2));  if (det < 0.f) both vmul(., -1.f)
 *     hand = vdot(cross(ngeom, T), B) >= 0.f ? 1.f : -1.f
 * A triangle with det == 0.f or den == 0.f is stored with map 0.  T is stored as computed (not normalised); B is used for hand only.
 *
 * At a hit that bounces (a triangle, not an analytic sphere, not an edge face, not Solid, remaining depth not exhausted) of a
 * triangle with a map: N is the vertex-normal section's `norm` (ns or ng, already on the hit side; ng without vertex normals),
 * (u, v) the texture section's, M that section's bilinear lookup (tc) of image nmap_of_tri at (u, v):
 *     x = (M.x * 2.f - 1.f) * strength;  y = (M.y * 2.f - 1.f) * strength;  z = M.z * 2.f - 1.f
 *     t = vunit(vsub(T, vmul(N, vdot(N, T))))
 *     b = vmul(cross(N, t), (face & 1) ? -hand : hand)          (t and b are the same world vectors seen from either face)
 *     nm = vunit(vadd(vadd(vmul(t, x), vmul(b, y)), vmul(N, z)))
 *     usem = vdot(nm, ng) > 0.f && vdot(rd, nm) < 0.f
 *     norm = usem ? nm : N
 * There are no clamps and no special cases.  A texel of (0.5, 0.5, 0.5), or T parallel to N, gives vunit(0) = NaN; usem is then
 * false and the hit is shaded exactly as without the map.  A mapped normal that faces away from the ray or from the side that was
 * hit falls back to N.  The wrong-side rule of the vertex-normal section is unchanged with (use || usem) where it says use: if the
 * bounce evaluated with `norm` leaves on the wrong side of ng, the whole bounce is evaluated again with ng, the same rv, the same
 * u, no new draw.  No RNG draw moves; the fold, the surface and colour stacks, black at edge faces and at exhausted depth are
 * untouched.  A triangle with map 0 is shaded bit for bit as before.  NOT promised: that a flat map (texel (0.5, 0.5, 1)) is
 * bit-identical to no map -- vunit(N) need not return N's bits.
 * Guides: the normal of rtmi_render_features*, and of the guides of rtmi_render_camera* and rtmi_render_rays*, is `norm` as above,
 * from the primary ray, whatever the surface kind.  Albedo, coverage, depth and ids do not change.
 *
 * rtmi_scene_set_normal_maps: n must equal ntris, entry 0 the sentinel's; corners9 as in rtmi_scene_set_normals; opt == NULL: the
 * defaults (strength 1.f, flags 0).  nmap_of_tri == NULL or n == 0 removes the maps, and the scene is exactly what it was.
 * RTMI_ERR_INVALID before any HIP call, naming the first offender: the scene has no textures, flags != 0, a strength that is not
 * finite, an entry above ntex, a corner of a mapped triangle that is not finite.  Setting, replacing or removing waits for the
 * scene's work first.  rtmi_scene_set_textures (set, replace or remove) removes the maps.  rtmi_scene_get_normal_maps copies the
 * device table's numbers back (*n_out = 0: no maps; a degenerate triangle reads as map 0).
 * rtmi_normal_map_frames (host code, no device needed; no sentinel: all n triangles count) is the per-triangle part alone, which
 * rtmi_scene_set_normal_maps applies: frames4_out gets (T.x, T.y, T.z, bits) per triangle, bits 0-30 the stored map number and
 * bit 31 set when hand = -1.f; all zero for a triangle stored with map 0.  facenorm3: the records' normals.
 * rtmi_normal_map_from_height (host code, no device needed) makes a map from a height field h(i, j) = height[j * w + i] with
 * repeat-wrapped central differences:
 *     dx = ((h(i + 1, j) - h(i - 1, j)) * 0.5f) * scale;  dy = ((h(i, j + 1) - h(i, j - 1)) * 0.5f) * scale
 *     n = vunit((-dx, -dy, 1.f));  rgb = (n.x * 0.5f + 0.5f, n.y * 0.5f + 0.5f, n.z * 0.5f + 0.5f)
 * A null pointer with w * h > 0 is refused; a size of 0 succeeds.
 *
 * A scene with normal maps renders on the per-pass pipeline with the k_shade*_nmap kernels (which know everything the _tex kernels
 * do) and k_features_nmap: every call that gains textures gains this.  Unchanged: rtmi_trace*, rtmi_occluded*, the records,
 * rtmi_render_ao*, _light*, which use the geometric normal; rtmi_bake*'s generator takes the caller's normal as before and its
 * traced paths bounce about mapped normals; rtmi_render_shadowed* and rtmi_render_preview* refuse a textured scene as before.
 * Not here: roughness and alpha maps, object-space normal maps, per-vertex tangents from a file, mip maps, normal maps on spheres,
 * in AO, light, preview and shadowed shading, in the path kernels (pipeline 3), a softened shadow terminator. */
typedef struct rtmi_normal_maps { float strength; /* 1.f */ uint32_t flags; /* 0 */ } rtmi_normal_maps_t;
void rtmi_normal_maps_defaults(rtmi_normal_maps_t* opt);
int rtmi_scene_set_normal_maps(rtmi_scene_t* scene, const float* corners9, const uint32_t* nmap_of_tri /* n, or NULL */, uint64_t n,
                               const rtmi_normal_maps_t* opt /* or NULL */);
int rtmi_scene_get_normal_maps(rtmi_scene_t* scene, uint32_t* nmap_of_tri_out /* or NULL */, float* strength_out /* or NULL */, uint64_t* n_out);
int rtmi_normal_map_frames(const float* corners9, const float* uvs6, const float* facenorm3, const uint32_t* nmap_of_tri, uint64_t n,
                           float* frames4_out);
int rtmi_normal_map_from_height(const float* height, uint32_t w, uint32_t h, float scale, float* rgb_out);

/* Optional: the corners the triangle records were made from (`Triangle.corners`, raytrace.rs:326-337), 9 floats per
 * triangle, n = ntris (entry 0 = the sentinel's, ignored).  Accepted and checked for size, no longer used: the BVH's boxes
 * are the triangles' own boxes (intersected with the bounding-radius disc's) for every scene, the corners solved from the
 * records' edge tests at scene creation, so that no render depends on the caller's corners being right. */
int rtmi_scene_set_corners(rtmi_scene_t* scene, const float* corners9, uint64_t n);

/* Option switches (all default 0): */
enum {
    RTMI_OPT_COUNTERS = 1u << 0, /* fill box/tri/node counters in rtmi_stats_t (slower) */
    RTMI_OPT_GENERIC = 1u << 1,  /* force the generic-tree traversal kernel              */
    RTMI_OPT_FAST = 1u << 2,     /* NOT bit-exact: skip boxes entirely behind the ray origin (octree kernel only).
                                  * The reference visits them; results differ only where a hit would have been found
                                  * first through such a box (exact ties between triangles, rays exactly parallel to a
                                  * triangle's plane).  Measured on config 3 (2048x2048 @ 64 spp): 17 of 4 194 304
                                  * pixels differ from exact mode, 1.6x the rays/s.  Never the default.              */
    RTMI_OPT_BVH = 1u << 3       /* "fast mode", NOT the reference's octree traversal: the closest hit over ALL triangles
                                  * with the lowest index winning exact ties, i.e. what the reference computes for a
                                  * build_trivial_bounding_box scene (raytrace.rs:847-856, :1012-1050), found through a
                                  * 4-wide SAH BVH the library builds over the triangles at scene creation (the
                                  * boxes/tri_refs passed in are ignored for tracing).  Bit-equal to the linear-list
                                  * render except for the reference's t = +-inf / NaN "hits" of triangles a ray does not
                                  * come near; differs from the octree render where the octree builder lost a triangle
                                  * or two triangles tie.  Never the default, never the headline.                     */
};
int rtmi_scene_set_options(rtmi_scene_t* scene, uint32_t options);

/* Launch tuning of one scene handle.  Defaults are taken ONCE, at rtmi_scene_create(), from the environment
 * (RTMI_BATCH_PATHS, RTMI_STREAMS, RTMI_SUBTILE_MIN_PATHS, RTMI_OCT_WAVES_PER_CU, RTMI_REFILL_MIN0,
 * RTMI_REFILL_MIN, RTMI_XCD_AWARE, RTMI_PIPELINE; RTMI_VERBOSE=1 prints per-pass timings to stderr) and can be read and changed
 * here.  None of them changes a pixel: any batch size, stream count or stripe split gives the same image. */
typedef struct rtmi_tuning {
    uint64_t batch_paths;       /* paths (pixel samples) per batch of the wavefront pipeline, all streams together; default 256 Mi.
                                   A tile up to 1/8 larger is still rendered as one batch.                    */
    uint32_t streams;           /* 1..4 internal HIP streams (interleaved sub-tiles of a tile); 0 (default) = automatic:
                                   one stream for tiles of 2^26 paths and more that run the path kernels
                                   (pipeline 3) and for rtmi_render_features*, three otherwise (renders of
                                   linear-list, generic-tree, BVH and sphere scenes always get three)        */
    uint32_t subtile_min_paths; /* tiles with fewer paths are not split over streams; default 32768           */
    uint32_t oct_waves_per_cu;  /* persistent waves per CU and launch of the octree kernel; 0 = automatic: what
                                   fits with one stream, at most 16 when several streams share the CUs       */
    uint32_t refill_min0;       /* idle lanes before a wave refills, primary pass (64 = whole wave); default 64 */
    uint32_t refill_min;        /* the same for bounce passes; default 16                                      */
    uint32_t xcd_aware;         /* 1 = one ray-queue range per XCD (by XCC_ID), 2 = by block index, 0 = one queue (default) */
    uint32_t kernel;            /* unused: the octree closest-hit kernel is always k_trace_oct.  0 and 1 are accepted;
                                 * 2 (a removed kernel) is refused with RTMI_ERR_UNSUPPORTED                            */
    uint32_t pipeline;          /* 0 = automatic (= 3), 1 = one launch per pass (k_gen, then k_trace* + k_shade per pass),
                                 * 3 = the path kernels: primary rays generated, traced and shaded in one kernel
                                 * (k_path_primary), then one closest-hit + one shading launch per bounce pass.  3 applies
                                 * to octree scenes; anything else (linear list, generic tree, BVH mode, analytic spheres)
                                 * runs 1.  Same image whichever runs.  2 (a removed pipeline) is refused with
                                 * RTMI_ERR_UNSUPPORTED.  Environment: RTMI_PIPELINE (2 there is read as 0).            */
    uint32_t slow_path_off;     /* 0 (default): in pipeline 3 a ray whose unit direction has an exactly-zero component
                                 * (BoundingBox::collides then skips that axis' slab, raytrace.rs:872-900: ~150 x the work of an
                                 * ordinary ray, 14 ms for the lane that traces it) is set aside and its path is traced by
                                 * k_path_slow on a side stream, one path per wave, beside the following passes; 1: such rays
                                 * are traced where they arise (they can hold a small tile's launches for ~10 % of its time).
                                 * Environment: RTMI_SLOW_PATH_OFF.                                                    */
} rtmi_tuning_t;
int rtmi_scene_get_tuning(rtmi_scene_t* scene, rtmi_tuning_t* out);
int rtmi_scene_set_tuning(rtmi_scene_t* scene, const rtmi_tuning_t* in);

/* Render image rows [row0, row0+nrows) of the viewport into `out`
 * (nrows*width*4 floats, row-major, RGB + a zero lane == `[Color]`,
 * raytrace.rs:1183, :1426).  Same pixel values for any row partition.
 * Replaces RayCaster::walk_rays_internal (raytrace.rs:1129-1131, :1175-1196)
 * with the RNG of the build (seed) injected at rand::random's call sites.
 * rtmi_render writes host memory; rtmi_render_device writes device memory on
 * `hip_stream` (a hipStream_t, or NULL for the default stream) and returns
 * after the work is enqueued and the counters are read back. */
/* Internally a tile is rendered as rtmi_tuning_t.streams sub-tiles (rows dealt out one by one), each on its own HIP stream
 * of the library (the tail of one sub-tile's persistent kernels overlaps the bulk of another's; large tiles use one);
 * they start after the work already queued on `hip_stream` and that stream is made to wait for them. */
int rtmi_render(rtmi_scene_t* scene, const rtmi_viewport_t* vp, uint64_t seed,
                uint32_t row0, uint32_t nrows, float* out_host, rtmi_stats_t* stats);
int rtmi_render_device(rtmi_scene_t* scene, const rtmi_viewport_t* vp, uint64_t seed,
                       uint32_t row0, uint32_t nrows, void* out_device, void* hip_stream,
                       rtmi_stats_t* stats);
/* Same for a striped row set; output row i is the i-th row of the tile. */
int rtmi_render_tile_device(rtmi_scene_t* scene, const rtmi_viewport_t* vp, uint64_t seed,
                            const rtmi_tile_t* tile, void* out_device, void* hip_stream,
                            rtmi_stats_t* stats);

/* Progressive rendering: samples [sample0, sample0 + nsamples) of every pixel of the tile, where vp->samples_per_pixel = S
 * is the frame's total (it decides the centred-ray rule of pixel_ray, raytrace.rs:1374-1394, and the final 1/S).
 * accum: one float4 per pixel of the tile (same layout as out) holding the running per-pixel sum of the samples done; read
 * when sample0 > 0, ignored (not read) when sample0 == 0, always rewritten.  out (optional, may be NULL; never the same
 * buffer as accum): the preview accum * (1/(sample0 + nsamples)).
 * Exactness: the RNG is keyed by (seed, pixel, sample, block), not by S, and a pixel's samples are summed in sample order
 * from 0.f, so passes that cover [0, S) in order leave in out exactly the bits of rtmi_render_tile_device.  The preview
 * after k samples equals a render at samples_per_pixel = k when k >= 2 or S == 1; with k == 1 < S it does not (sample 0 of
 * an S-sample frame is jittered, a 1-sample frame's is centred).
 * Passes must be issued in sample order, each continuing the previous one on the same accum: the library does not check.
 * stats describe this call only; summed over the passes of a frame they equal the single call's.  maxdepth == 0 writes
 * zeros to accum and out.  RTMI_ERR_INVALID also for nsamples == 0, sample0 + nsamples > S and a NULL accum.
 * The device variant enqueues on hip_stream like rtmi_render_tile_device and copies nothing.  The host variant renders
 * rows [row0, row0 + nrows) and copies accum in (only when sample0 > 0) and out again: 2 x 16 B per pixel of host-link
 * traffic per pass (+ 16 B when out_host is given). */
int rtmi_render_samples_device(rtmi_scene_t* scene, const rtmi_viewport_t* vp, uint64_t seed, const rtmi_tile_t* tile,
                               uint32_t sample0, uint32_t nsamples, void* accum_device, void* out_device,
                               void* hip_stream, rtmi_stats_t* stats);
int rtmi_render_samples(rtmi_scene_t* scene, const rtmi_viewport_t* vp, uint64_t seed, uint32_t row0, uint32_t nrows,
                        uint32_t sample0, uint32_t nsamples, float* accum_host, float* out_host, rtmi_stats_t* stats);

/* First-hit feature buffers: per-pixel albedo, shading normal, depth, coverage and hit id of the PRIMARY
 * rays, for denoisers, compositing and picking.  The rays are the renderer's own: samples [sample0, sample0 + nsamples) of
 * every pixel of the tile, of a frame of S = vp->samples_per_pixel samples, exactly as rtmi_render_samples_device generates
 * them (RNG keyed by (seed, pixel, sample, block 0); jittered iff S != 1).  vp->maxdepth is not consulted: only the primary
 * ray is traced, and its closest hit (tri, t, face) is what rtmi_trace returns for it.  Per sample, in f32:
 *   miss (tri == 0):          a = sky (128, 180, 255)/255,       c = 0,  n = (0, 0, 0),                          d = 0
 *   edge face (face & 2):     a = (0, 0, 0),                     c = 1,  n = the triangle's norm, * (-1.f) when face & 1,  d = t
 *   any other hit:            a = the surface's color (Solid, Matte, Reflective alike),  c, n, d as for an edge face
 * albedo: one float4 per pixel = (mean a.r, mean a.g, mean a.b, mean c: coverage / alpha).
 * normal: one float4 per pixel = (mean n.x, mean n.y, mean n.z, mean d).  The mean normal is not renormalised, and the mean
 *         depth of the samples that hit is normal.w / albedo.w where coverage is non-zero: the division is the caller's.
 * ids:    one uint32 per pixel = tri | face << 30 of sample `sample0` of the pixel (0 = miss): the first-hit id map (with
 *         S == 1 the centred ray's hit).
 * "mean" is walk_ray_set's arithmetic (raytrace.rs:1414-1426): acc = 0.f; acc = acc + x in sample order; acc * (1.f /
 * (float)nsamples).  A non-finite t of a degenerate "hit" (raytrace.rs:402-405) propagates into normal.w; nothing filters it.
 * Layout: the tile's, as rtmi_render_tile_device (row-major over the tile's rows).  Any of the three pointers may be NULL
 * (that buffer is not produced), but not all three; no two may alias.
 * stats: rays = pixels * nsamples, kernel_ms, trace_ms, trace_launches, streams, pipeline = 1, slow_paths = 0 (rays with a
 * zero component are traced in place, as rtmi_trace does); with RTMI_OPT_COUNTERS the five work counters.
 * Scenes: octree, generic tree (RTMI_OPT_GENERIC) and linear list; RTMI_OPT_FAST / RTMI_OPT_BVH give those modes' hits.
 * RTMI_ERR_UNSUPPORTED for a scene with analytic spheres: that primitive is build-defined (rtmi_sphere_t) and its normal
 * needs the hit point, which this call does not compute.
 * RTMI_ERR_INVALID, before any HIP call and before the scene is used: a NULL scene, viewport or tile; all three outputs
 * NULL; aliased outputs; nsamples == 0; sample0 + nsamples > S; every viewport and tile check of
 * rtmi_render_samples_device.  An empty tile returns RTMI_OK and touches nothing.  stats come back cleared on failure.
 * The device variant enqueues on hip_stream like rtmi_render_tile_device; the host variant renders rows [row0, row0 + nrows)
 * and copies the requested buffers out once (16 + 16 + 4 B per pixel).  Batches, streams and sub-tiles apply as for a
 * progressive pass (automatic streams: one); no tuning changes a bit of the result.
 * Not here: features of batches of views or of rtmi_render_frame_multi, sums continued across calls. */
int rtmi_render_features_device(rtmi_scene_t* scene, const rtmi_viewport_t* vp, uint64_t seed, const rtmi_tile_t* tile,
                                uint32_t sample0, uint32_t nsamples, void* albedo_device, void* normal_device,
                                void* ids_device, void* hip_stream, rtmi_stats_t* stats);
int rtmi_render_features(rtmi_scene_t* scene, const rtmi_viewport_t* vp, uint64_t seed, uint32_t row0, uint32_t nrows,
                         uint32_t sample0, uint32_t nsamples, float* albedo_host, float* normal_host, uint32_t* ids_host,
                         rtmi_stats_t* stats);

/* Feature-guided a-trous denoiser for low-sample frames: an edge-avoiding wavelet filter (Dammertz et al.
 * 2010) guided by the buffers of rtmi_render_features*.  NOT part of the reference, which has no denoiser: build-defined like
 * the analytic sphere, so what follows IS the definition, and the tests pin it bit for bit.  Only + - * / and comparisons in
 * f32, no contraction, no exp (neither the device's nor a host library's is correctly rounded).
 * Edge-stopping function (Tukey's biweight): g(x2, s2) = (x2 < s2) ? (1 - x2/s2)^2 : 0.  A NaN argument gives 0 (the
 * comparison is false); s2 = +inf gives exactly 1 for finite x2, so a term is switched off by passing +inf for its sigma.
 * Inputs: whole width x height row-major images (not striped tiles), one float4 per pixel:
 *   color   rgb, lane 3 ignored:          what rtmi_render_device writes
 *   albedo  a = rgb, cov = lane 3:        rtmi_render_features_device's albedo buffer  } of a features call with tile
 *   normal  n = xyz, d = lane 3 (depth):  rtmi_render_features_device's normal buffer  } {0, height, height, 0}
 *   out     rgb, lane 3 = 0; must not be one of the inputs.
 * Start value: u = color.rgb; with RTMI_DENOISE_DEMODULATE u = color.rgb / (albedo.rgb + 1/256) per channel.
 * Iteration i = 0 .. iterations-1, for every pixel p, with k = {1/16, 1/4, 3/8, 1/4, 1/16}:
 *   num = (0, 0, 0); den = 0; the taps q = p + 2^i * (dx, dy) are visited with dy outer, dx inner, both from -2 to 2;
 *   a tap outside the image is skipped;
 *   the centre tap has w = k[2] * k[2], always;
 *   when cov_p == 0 && cov_q == 0 (sky beside sky): w = (k[dy+2] * k[dx+2]) * g(|u_p - u_q|^2, sc2_i);
 *   any other tap: w = k[dy+2] * k[dx+2];  w = w * g(|n_p - n_q|^2, sigma_normal * sigma_normal);
 *                  w = w * g((d_p - d_q) * (d_p - d_q), (sigma_depth * d_p) * (sigma_depth * d_p));
 *                  w = w * g((cov_p - cov_q) * (cov_p - cov_q), 0.25);  w = w * g(|a_p - a_q|^2, sigma_albedo * sigma_albedo);
 *                  w = w * g(|u_p - u_q|^2, sc2_i);
 *   sc2_i = (sigma_color * sigma_color) * 4^-i (4^-i is exact);  |v|^2 = ((0 + v.x * v.x) + v.y * v.y) + v.z * v.z;
 *   a tap with w == 0 is not added (a NaN or inf neighbour cannot poison the sums: its g is 0); otherwise, per channel,
 *   num = num + w * u_q and den = den + w;
 *   u'_p = num / den.  Every pixel reads this iteration's input u: the filter ping-pongs, it is never in place.
 * Result: out.rgb = u, with RTMI_DENOISE_DEMODULATE u * (albedo.rgb + 1/256); out.w = 0.
 * A NaN pixel stays NaN (its own centre tap) and makes no neighbour NaN.
 * Defaults (rtmi_denoise_defaults): iterations 3, flags 0, sigma_color 1.0, sigma_normal 0.5, sigma_depth 0.1, sigma_albedo
 * +inf.  Demodulation is a flag and not the default: it raised the error against a converged render on the textureless test
 * scenes (DESIGN.md 4.12 has the figures). */
enum { RTMI_DENOISE_DEMODULATE = 1u << 0 };
typedef struct rtmi_denoise {
    uint32_t iterations;   /* 1..8; iteration i uses tap spacing 2^i */
    uint32_t flags;        /* RTMI_DENOISE_DEMODULATE */
    float sigma_color, sigma_normal, sigma_depth, sigma_albedo;
} rtmi_denoise_t;
void rtmi_denoise_defaults(rtmi_denoise_t* params);
/* rtmi_denoise_device: device images; one kernel launch per iteration is enqueued on hip_stream (like rtmi_quantize_device:
 * nothing is synchronised).  With more than one iteration the handle keeps one width*height*16 B ping-pong image, grown on
 * demand (growing it frees the old one, which waits for the device) and freed by rtmi_scene_destroy; no render workspace is
 * touched.  One denoise call per handle at a time.  rtmi_denoise: host images, copied in, filtered and copied out.
 * rtmi_render_denoised: rtmi_render_tile_device of the whole frame, rtmi_render_features_device over all
 * vp->samples_per_pixel samples and the filter, on device images the handle keeps; only the result is copied to out_host.
 * stats (optional) are the render call's.
 * RTMI_ERR_INVALID, before any HIP call and before the scene is used: a NULL scene, params or image; out aliasing an input;
 * width or height 0; iterations 0 or above 8; unknown flag bits; a sigma that is NaN or <= 0 (+inf is valid).
 * RTMI_ERR_UNSUPPORTED: width * height >= 2^32; rtmi_render_denoised on a scene with analytic spheres (no features).
 * Not here: temporal accumulation, variance guidance, striped tiles, batches of views, rtmi_render_frame_multi. */
int rtmi_denoise_device(rtmi_scene_t* scene, uint32_t width, uint32_t height, const void* color_device,
                        const void* albedo_device, const void* normal_device, const rtmi_denoise_t* params, void* out_device,
                        void* hip_stream);
int rtmi_denoise(rtmi_scene_t* scene, uint32_t width, uint32_t height, const float* color_host, const float* albedo_host,
                 const float* normal_host, const rtmi_denoise_t* params, float* out_host);
int rtmi_render_denoised(rtmi_scene_t* scene, const rtmi_viewport_t* vp, uint64_t seed, const rtmi_denoise_t* params,
                         float* out_host, rtmi_stats_t* stats);

/* Adaptive sampling: every pixel stops at its own sample count n, between min_samples and
 * vp->samples_per_pixel = S (the maximum, >= 2), and its value is exactly the pixel of a uniform render at spp = n.
 * Pass 0 renders samples [0, m) of every pixel of the tile (m = min_samples, 2 <= m <= S).  After each pass the stop rule
 * is applied to every pixel still active; one that goes on gets samples [n, min(n + pass_samples, S)) in the next pass
 * (all active pixels share the same n).  A pixel with n = S stops whatever the rule says.  The stop rule, in f32 and in
 * this order (s = sum, q = per-lane sum of squares of the pixel's samples; max(a, b) = a < b ? b : a):
 *   inv = 1/(float)n;  m_c = s_c * inv;  v_c = (q_c - s_c * m_c) / (float)(n - 1)   (c = r, g, b)
 *   e = max(max(v_r, v_g), v_b) / (float)n;  L = max(max(m_r, m_g), m_b);  t = abs_tol + rel_tol * L
 *   stop iff e <= t * t;  a NaN anywhere means "not stopped" (abs_tol = NaN: every pixel runs to S, in passes;
 *   abs_tol = +inf: every pixel stops at m).
 * passes, unconverged (pixels that reached S without the rule stopping them) and samples (the sum of counts) are outputs. */
typedef struct rtmi_adaptive {
    uint32_t min_samples, pass_samples; float rel_tol, abs_tol;  /* in  */
    uint32_t passes, unconverged; uint64_t samples;              /* out */
} rtmi_adaptive_t;

/* accum, sumsq: one float4 per pixel of the tile (the layout of out): the running sum, and the per-lane sum of squares
 * q = q + c * c in sample order from 0.f (lane 3 is 0); counts: one uint32 per pixel, its sample count; out (optional, may
 * be NULL) = accum * (1/count) per pixel, k_accum's arithmetic.  No two of the four buffers may alias.  The device variant
 * enqueues on hip_stream and reads back 4 bytes per pass (the number of active pixels, which sizes the next pass).  The
 * host variant renders rows [row0, row0 + nrows), keeps accum and sumsq on the device and copies out and counts once.
 * stats cover the whole call, summed over its passes: with abs_tol = NaN they are a single rtmi_render call's.
 * maxdepth == 0: zeros, count = m.  RTMI_ERR_INVALID (before any HIP call) for m < 2, m > S, pass_samples == 0, S < 2, a
 * NULL or aliased buffer, a NULL scene, viewport or ad. */
int rtmi_render_adaptive_device(rtmi_scene_t* scene, const rtmi_viewport_t* vp, uint64_t seed, const rtmi_tile_t* tile,
                                rtmi_adaptive_t* ad, void* accum_device, void* sumsq_device, void* counts_device,
                                void* out_device, void* hip_stream, rtmi_stats_t* stats);
int rtmi_render_adaptive(rtmi_scene_t* scene, const rtmi_viewport_t* vp, uint64_t seed, uint32_t row0, uint32_t nrows,
                         rtmi_adaptive_t* ad, float* out_host, uint32_t* counts_host, rtmi_stats_t* stats);

/* Variance-guided denoising: the a-trous filter above with a colour width that follows each pixel's own
 * measured variance, which is what an adaptive frame needs (its noise level differs by pixel by construction): the spatial
 * half of SVGF (Schied et al. 2017).  Build-defined like rtmi_denoise, so what follows IS the definition, and
 * tests/denoise_var_ref.py pins it bit for bit.  Only + - * / and comparisons in f32, no contraction, no exp, no sqrt.
 *
 * rtmi_variance*: the variance of every pixel's mean from the moments rtmi_render_adaptive_device leaves.  Per pixel: s =
 * accum, q = sumsq (one float4 each), n = count (uint32); output one float4.  For c = r, g, b (the first line is the stop
 * rule's own arithmetic):
 *   inv = 1.f / (float)n;  m_c = s_c * inv;  v_c = (q_c - s_c * m_c) / (float)(n - 1)
 *   vm_c = v_c / (float)n;  vm_c = vm_c < 0.f ? 0.f : vm_c      (a NaN stays NaN)
 *   lane 3 = ((0.f + vm_r) + vm_g) + vm_b
 *   n < 2 (nothing is known): all four lanes +inf.
 * The arithmetic is per pixel, so the call takes npixels and any layout, like rtmi_quantize_device.  The device variant
 * enqueues one launch on hip_stream and synchronises nothing; the host variant copies in, runs the kernel and copies out.
 * npixels == 0: RTMI_OK, nothing is touched (checked after the scene, before the buffers).  RTMI_ERR_INVALID, before any HIP
 * call and before the scene is used: a NULL scene or buffer, an output that is one of the inputs.  RTMI_ERR_UNSUPPORTED: the
 * host variant with npixels >= 2^32.
 *
 * rtmi_denoise_var*: rtmi_denoise_device's arguments plus
 *   variance  the image above for the whole width x height frame: vm = lanes 0-2, vs = lane 3
 *   var_out   optional (NULL: not produced): the propagated variance after the last iteration, same layout; must not be any
 *             other buffer of the call.
 * params: an rtmi_denoise_t with the same checks and the same accepted flags, but sigma_color is in STANDARD DEVIATIONS OF THE
 * PIXEL, not in colour units.  Defaults (rtmi_denoise_var_defaults): iterations 1, flags 0, sigma_color 3.0, sigma_normal 0.5,
 * sigma_depth 0.1, sigma_albedo +inf (DESIGN.md 4.13 has the measurement they come from).
 * Start value: u = color.rgb and (vm, vs) = variance; with RTMI_DENOISE_DEMODULATE u as for rtmi_denoise, vm_c = (vm_c /
 * (albedo_c + 1/256)) / (albedo_c + 1/256) (two divisions) and vs = ((0 + vm_r) + vm_g) + vm_b of those.
 * Iteration i is rtmi_denoise's iteration i with three differences:
 *  1. Colour width per pixel.  For the centre pixel p, gv_p is the 3 x 3 prefilter of this iteration's input vs: taps
 *     (dx, dy) in {-1, 0, 1}^2 at spacing 1 in every iteration, dy outer, dx inner, k3 = {1/4, 1/2, 1/4}; a tap outside the
 *     image is skipped; num = num + (k3[dy+1] * k3[dx+1]) * vs_q, den = den + k3[dy+1] * k3[dx+1] for every tap inside (zeros
 *     too); gv_p = num / den.  The colour term of every tap of p is g(|u_p - u_q|^2, s2c_p) with
 *     s2c_p = (sigma_color * sigma_color) * gv_p + 0x1p-40f.  There is no 4^-i factor: the variance shrinks by itself under 2.
 *     Everything else is unchanged: the sky-beside-sky rule, the other four factors and their order, "a tap with w == 0 is not
 *     added", the centre tap's fixed weight, u'_p = num / den.
 *  2. Variance propagation.  Alongside num and den, per channel, nv_c = nv_c + (w * w) * vm_{q,c} for exactly the taps that are
 *     added; the centre tap is one of them, with w = k[2] * k[2].  The iteration's output is vm'_c = nv_c / (den * den) and
 *     vs' = ((0 + vm'_r) + vm'_g) + vm'_b.  Colour and variance both ping-pong; no iteration is in place.
 *  3. Result: out as for rtmi_denoise; var_out = (vm, vs), with RTMI_DENOISE_DEMODULATE vm_c = (vm_c * (albedo_c + 1/256)) *
 *     (albedo_c + 1/256) and vs their ordered sum.
 * Consequences:
 *   a pixel of zero variance (sky, a Solid surface: s2c = 2^-40) mixes only with taps of identical colour, so converged
 *   pixels are not blurred; with sigma_color = +inf such a pixel has s2c = inf * 0 = NaN and mixes with nothing;
 *   +inf variance makes the colour term exactly 1 for finite colours: the guides alone decide;
 *   a NaN variance gives s2c = NaN and g = 0: every pixel whose 3 x 3 neighbourhood holds it is left unfiltered in that
 *   iteration (its centre tap alone).  No NaN ever enters a neighbour's colour; a neighbour's variance does take the NaN of a
 *   tap it adds, which freezes that neighbour in the next iteration.
 * Scratch: with more than one iteration the handle keeps one colour and two variance images (width*height*48 B), grown on
 * demand and freed by rtmi_scene_destroy; no render workspace and no image of rtmi_denoise is touched.  One call per handle at
 * a time.  RTMI_ERR_INVALID / RTMI_ERR_UNSUPPORTED as for rtmi_denoise*, and a NULL variance, out aliasing variance, var_out
 * aliasing any other buffer.
 *
 * rtmi_render_adaptive_denoised: on device images the handle keeps, (1) rtmi_render_adaptive_device of the whole frame, (2)
 * the variance image, (3) rtmi_render_features_device over samples [0, ad->min_samples), the samples every pixel has, (4) the
 * filter.  Only the result (out_host) and the counts (counts_host, optional) are copied out.  stats are the adaptive call's;
 * ad's outputs are filled.  RTMI_ERR_UNSUPPORTED on a scene with analytic spheres, as for rtmi_render_denoised.  Every
 * argument check of both component calls runs before any HIP call and before the scene is used.
 * Not here: temporal accumulation and reprojection, batches of views, striped tiles, rtmi_render_frame_multi, a sumsq output
 * of the uniform render calls (an adaptive call with min_samples = S yields the moments of a uniform S-spp frame). */
void rtmi_denoise_var_defaults(rtmi_denoise_t* params);
int rtmi_variance_device(rtmi_scene_t* scene, const void* accum_device, const void* sumsq_device, const void* counts_device,
                         uint64_t npixels, void* variance_device, void* hip_stream);
int rtmi_variance(rtmi_scene_t* scene, const float* accum_host, const float* sumsq_host, const uint32_t* counts_host,
                  uint64_t npixels, float* variance_host);
int rtmi_denoise_var_device(rtmi_scene_t* scene, uint32_t width, uint32_t height, const void* color_device,
                            const void* albedo_device, const void* normal_device, const void* variance_device,
                            const rtmi_denoise_t* params, void* out_device, void* var_out_device, void* hip_stream);
int rtmi_denoise_var(rtmi_scene_t* scene, uint32_t width, uint32_t height, const float* color_host, const float* albedo_host,
                     const float* normal_host, const float* variance_host, const rtmi_denoise_t* params, float* out_host,
                     float* var_out_host);
int rtmi_render_adaptive_denoised(rtmi_scene_t* scene, const rtmi_viewport_t* vp, uint64_t seed, rtmi_adaptive_t* ad,
                                  const rtmi_denoise_t* params, float* out_host, uint32_t* counts_host, rtmi_stats_t* stats);

/* A batch of views of one scene in one call: a camera move, a stereo pair, the faces of a cube map, many
 * small windows.  vps[k] and seeds[k] are view k: what rtmi_render(scene, &vps[k], seeds[k], 0, H, ...) would render, bit
 * for bit (the RNG of a pixel is keyed by its view's seed and its pixel index inside the view, its primary rays come from
 * its view's camera; everything else is shared).  All views share width, height, maxdepth and samples_per_pixel
 * (RTMI_ERR_INVALID naming the first view that differs); orig/cam/vu/vv and the seed are per view.
 * The batch is ONE stacked image of nviews * H rows: row k*H + r is row r of view k.  rtmi_render_views renders the whole
 * stack into out_host (nviews * H * W * 4 floats).  rtmi_render_views_device renders `tile` of the stack (rtmi_tile_t rules;
 * stripes may cross view boundaries) and enqueues on hip_stream like rtmi_render_tile_device.  Streams, batches and the
 * automatic stream rule apply to the stack as a whole.  stats cover the whole call: rays and the five work counters are
 * the sums over the views' single calls.  A batch of one view runs the single-view kernels (it is that view's call).
 * RTMI_ERR_INVALID, before any HIP call: nviews == 0; a NULL scene, vps, seeds or output; views that differ in a shared
 * field; a tile outside the stack; every check rtmi_render_tile_device makes for one view.  RTMI_ERR_UNSUPPORTED: nviews *
 * H * W >= 2^32.
 * Not for views (render them one call per view): progressive and adaptive passes, rtmi_render_frame_multi, per-ray
 * records. */
int rtmi_render_views_device(rtmi_scene_t* scene, const rtmi_viewport_t* vps, const uint64_t* seeds, uint32_t nviews,
                             const rtmi_tile_t* tile, void* out_device, void* hip_stream, rtmi_stats_t* stats);
int rtmi_render_views(rtmi_scene_t* scene, const rtmi_viewport_t* vps, const uint64_t* seeds, uint32_t nviews,
                      float* out_host, rtmi_stats_t* stats);

/* One whole frame over several devices of this process -- the fan-out the reference does over CPU threads
 * (DefaultRayCaster::walk_rays_internal, raytrace.rs:1175-1196: `threads` workers pulling rows from a queue) done
 * over GPUs, inside the library.  scenes[i] is the SAME scene uploaded to some device (rtmi_scene_create with
 * device = i; two handles may also share a device).  Scene i renders the interleaved stripes
 * {i*S, rows_i, S, n*S} (S = stripe_rows, 0 = default 16) on its own host thread and stream; every band then
 * crosses to scenes[0]'s device ONCE (hipMemcpyPeerAsync: one xGMI link per peer, all links at the same time),
 * where a kernel de-interleaves the stripes into the frame.  No other exchange: pixels are independent and the RNG
 * is keyed by (pixel, sample), so the frame is bit-identical to rtmi_render() of the whole image on one device.
 * flags: RTMI_FRAME_RGB8 quantises every band on its device first ((c*255.) as u8, raytrace.rs:1468-1473), so
 * 3 bytes per pixel cross the links instead of 16 and the output is height*width*3 bytes; otherwise the output is
 * height*width*4 floats (`[Color]`).  out_host and/or out_device (memory of scenes[0]'s device) receive the frame.
 * stats (optional) has nscenes entries, one per scene; "Rays" of the frame is their sum. */
enum {
    RTMI_FRAME_RGB8 = 1u << 0,
    RTMI_FRAME_RCCL = 1u << 1  /* the bands cross to scenes[0]'s device with ONE ncclGather (RCCL over xGMI; rccl.h) on a
                                * communicator the library makes for the scenes' devices (ncclCommInitAll, kept on scenes[0])
                                * instead of one hipMemcpyPeerAsync per band.  librccl.so.1 is loaded on first use (a process
                                * that holds PyTorch's RCCL gets that copy).  Every scene handle must sit on a device of its
                                * own.  Same frame either way; without the flag the library stays free of RCCL.            */
};
int rtmi_render_frame_multi(rtmi_scene_t* const* scenes, uint32_t nscenes, const rtmi_viewport_t* vp, uint64_t seed,
                            uint32_t stripe_rows, uint32_t flags, void* out_host, void* out_device, rtmi_stats_t* stats);

/* Closest hit for n explicit rays: orig (x,y,z,lane3) and unit dir
 * (x,y,z,lane3) as `make_ray` stores them (raytrace.rs:201-210).  Outputs per
 * ray: triangle index (0 = miss), hit time, face (0 front, 1 back, 2 edge
 * front, 3 edge back).  Same function as the reference's native entry point
 * exec_cuda_raytrace (cuda_raytrace_lib/src/cuda_raytrace.rs:20-58,
 * cuda_rt.h:8-15) but with the CPU path's semantics
 * (BoundingBox::get_object_intersection_for_ray, raytrace.rs:909-1010). */
int rtmi_trace(rtmi_scene_t* scene, uint64_t n, const float* orig4, const float* dir4,
               uint32_t* tri, float* t, uint32_t* face, rtmi_stats_t* stats);

/* Any-hit occlusion query: "is anything in the way?" for n explicit rays, each with its own limit -- shadow
 * and visibility tests, ambient occlusion, line of sight between two points (the shadow ray of LightSource::get_shadow_ray,
 * commented out at raytrace.rs:1203-1224, asks exactly this).  Rays as for rtmi_trace: float4 origin and float4 unit direction
 * as `make_ray` stores them.  Output: one byte per ray, 0 or 1.
 * Definition.  For ray i let (tri, t) be what rtmi_trace returns for that ray on this scene handle with its current options.
 *   occluded[i] = (tri != 0 && t < tmax[i]) ? 1 : 0        (the comparison in f32)
 * Consequences:
 *   a NaN t (a degenerate "hit", raytrace.rs:402-405) does not occlude;
 *   a hit at t == tmax does not occlude;
 *   tmax NaN or <= -0.f gives 0 for every ray (a hit has t >= 0 or NaN);
 *   a NULL tmax pointer means +inf for every ray: any hit of finite t occludes, a hit at t = +inf does not;
 *   the triangle the origin lies on is not excluded and there is no epsilon: offsetting the origin is the caller's job, as it is
 *   for bounce rays (raytrace.rs:284-296) and as the comment on rtmi_sphere_t says;
 *   analytic spheres take part exactly as in rtmi_trace: a sphere hit that replaces the tree's hit is the (tri, t) of the rule;
 *   RTMI_OPT_GENERIC, RTMI_OPT_FAST and RTMI_OPT_BVH each give their own mode's (tri, t).
 * How.  An exact octree and the linear list are walked by any-hit kernels (k_occluded_oct, k_occluded_linear): the closest-hit
 * walk's running best only ever moves to a smaller t, so a ray is answered 1 and leaves the walk as soon as that best is
 * < tmax; a ray that is not occluded is walked to the end, step for step as rtmi_trace walks it.  Rays with a zero direction
 * component are traced in place.  Generic trees, RTMI_OPT_GENERIC, RTMI_OPT_BVH and scenes with analytic spheres run
 * rtmi_trace's closest-hit launch followed by one elementwise kernel (k_occl_from_hits).  Same bytes either way.
 * rtmi_occluded: host buffers; orig4, dir4 and tmax are copied in, n bytes are copied out.
 * rtmi_occluded_device: device buffers, read in place (no staging copy of the rays).  The library's stream starts after the work
 * already queued on hip_stream and hip_stream is made to wait for it, as for rtmi_render_tile_device; the call returns once the
 * work is enqueued and the counters are read back.  One call per scene handle at a time, like every call on a handle.
 * stats: rays = n; kernel_ms, trace_ms (the walk kernel alone), trace_launches = 1, streams = 1 as rtmi_trace fills them (the
 * device variant's kernel_ms is the span on hip_stream).  With RTMI_OPT_COUNTERS the five work counters are the work the
 * any-hit walk actually did: each <= rtmi_trace's for the same rays, and equal to them when no ray is answered 1 (tmax all 0
 * or all NaN, say).
 * n == 0: RTMI_OK, nothing is touched (checked after the scene, before the buffers).  RTMI_ERR_INVALID, before any HIP call
 * and before the scene is used: a NULL scene, orig4, dir4 or occluded; an output that overlaps an input (as byte ranges of 16 n,
 * 16 n, 4 n and n bytes).  RTMI_ERR_UNSUPPORTED: n >= 2^31, as for rtmi_trace.  stats come back cleared on failure.
 * Not here: occlusion for batches of views and for rtmi_render_frame_multi.  (The
 * ambient-occlusion buffer is rtmi_render_ao*, the shadow layer of a box light rtmi_render_light*, shadow rays inside the
 * shading of every bounce rtmi_render_shadowed*, all below.) */
int rtmi_occluded(rtmi_scene_t* scene, uint64_t n, const float* orig4, const float* dir4, const float* tmax /* n floats or NULL */,
                  uint8_t* occluded, rtmi_stats_t* stats);
int rtmi_occluded_device(rtmi_scene_t* scene, uint64_t n, const void* orig4_device, const void* dir4_device,
                         const void* tmax_device /* or NULL */, void* occluded_device, void* hip_stream, rtmi_stats_t* stats);

/* rtmi_trace on device buffers: orig4 / dir4 (n float4 each, 16-byte aligned) are read where they are, with no staging copy;
 * tri / t / face (n uint32 / f32 / uint32) receive what rtmi_trace returns for the same rays on this handle.  One closest-hit
 * launch on the library's stream and one elementwise kernel that unpacks the hit records.  Stream semantics as for
 * rtmi_occluded_device: the library's stream starts after the work already queued on hip_stream, hip_stream is made to wait for
 * it, and the call returns once the counters are read back.  stats as rtmi_trace fills them (kernel_ms: the span on hip_stream).
 * n == 0: RTMI_OK, nothing is touched (checked after the scene, before the buffers).  RTMI_ERR_INVALID, before any HIP call and
 * before the scene is used, stats cleared: a NULL scene or buffer; two buffers that overlap as byte ranges (16 n, 16 n, 4 n, 4 n,
 * 4 n bytes).  RTMI_ERR_UNSUPPORTED: n >= 2^31. */
int rtmi_trace_device(rtmi_scene_t* scene, uint64_t n, const void* orig4_device, const void* dir4_device, void* tri_device,
                      void* t_device, void* face_device, void* hip_stream, rtmi_stats_t* stats);

/* Path tracing of caller-supplied rays: the colour project_ray (raytrace.rs:1199-1295) returns for each of n
 * explicit rays -- closest hit, color_ray, Lambert and mirror bounces, mix_color -- without Viewport::pixel_ray in front of it:
 * for fisheye, panoramic, orthographic and thin-lens cameras, light probes, lightmap and irradiance bakes, paths continued
 * from somebody else's G-buffer.  This is the reference's own function of a ray, not a build-defined one: the renderer's
 * primary rays fed back with their keys reproduce rtmi_render bit for bit, ray count and work counters included.
 * Rays: as for rtmi_trace, a float4 origin and a float4 unit direction per ray as `make_ray` stores them (raytrace.rs:201-210),
 * 16-byte aligned.  With RTMI_RAYS_MAKE_RAY the library applies make_ray itself: dir = vunit(dir), i.e. the ordered four-lane
 * dot ((((0 + x x) + y y) + z z) + w w), r = sqrt(.), dir * (1.f / r) (raytrace.rs:93-96); the origin is taken as given and
 * the caller's direction buffer is not written.
 * RNG key of ray i (what rand::random's call sites are keyed by, as in rtmi_render: (seed, pixel, sample, block)):
 *   keys != NULL:  (pixel, sample) = (keys[2 i], keys[2 i + 1]);
 *   keys == NULL:  (pixel, sample) = (pixel0 + i / G, i % G), G = rays->group.
 * Keys need not be distinct (two rays with one key draw the same numbers).  Block 0, pixel_ray's jitter, is never drawn; bounce k
 * of a path draws block k (k = 1 .. maxdepth - 1), exactly as a rendered path does.
 * Outputs (rtmi_rays_out_t; any may be NULL, not all), rays in groups of G consecutive rays, group g = rays [g G, (g + 1) G):
 *   color[i]   the colour of a path that starts with ray i, has ray i's key and depth rays->maxdepth; lane 3 = 0 (what a
 *              sample of rtmi_render contributes to its pixel);
 *   mean[g]    acc = 0.f; acc = acc + color[g G + s] for s = 0 .. G-1; acc * (1.f / (float)G): walk_ray_set's arithmetic
 *              (raytrace.rs:1414-1426), a group standing for a pixel and its rays for the pixel's samples;
 *   albedo[g], normal[g], ids[g]   rtmi_render_features*'s three buffers with a group for a pixel: the per-sample terms of the
 *              rays' closest hits (what rtmi_trace returns for them) folded in the same order; ids[g] is the id of ray g G.
 * maxdepth == 0: color and mean are zeros (project_ray returns black at depth 0, raytrace.rs:1261-1263); the guide buffers still
 * come from the closest hits: the rays are traced when a guide is asked for and not otherwise.
 * Scenes: every kind rtmi_render takes -- octree, linear list, generic tree, RTMI_OPT_GENERIC, RTMI_OPT_FAST, RTMI_OPT_BVH and
 * analytic spheres, each with its own mode's hits.  The guide buffers are refused with RTMI_ERR_UNSUPPORTED on a scene with
 * analytic spheres, as rtmi_render_features* is; the colours are not.
 * How: always the per-pass pipeline (rtmi_tuning_t.pipeline 1) on one stream of the library: per batch k_rays_begin (the queue's
 * count and identity path map; with RTMI_RAYS_MAKE_RAY the unit directions, into the workspace queue), then per pass the scene's
 * closest-hit launch and k_shade_rays, k_features after pass 0 when guides are asked for, k_accum for the means.  Rays with a
 * zero direction component are traced in place.  The device variant's pass 0 traces the caller's buffers where they are (no
 * staging copy of the rays; with the flag only the directions are rewritten, into the workspace) and, when color is asked for,
 * the sample colours are written straight into it.  A batch holds whole groups: rtmi_tuning_t.batch_paths rounded down to a
 * multiple of G, at least G.  Hit records and queues are the handle's render workspace; nothing new persists on the handle.  No
 * tuning changes a bit of the result.  An octree scene does not get k_path_primary's packet culling and in-place mirror pass
 * here: those need to know that the rays are a camera's (DESIGN.md 4.18 has the measured cost).
 * rtmi_render_rays_device: device buffers; stream semantics as for rtmi_occluded_device: the library's stream starts after the
 * work already queued on hip_stream, hip_stream is made to wait for it, and the call returns once the counters are read back.
 * rtmi_render_rays: host buffers; each batch's rays (and keys) are copied in and its outputs copied out.
 * stats: rays = the reference's "Rays" counter, every ray traced in any pass (with maxdepth == 0 and a guide: n); trace_launches
 * = passes x batches, trace_ms = the sum of those closest-hit launches' times, kernel_ms = the span of the call on hip_stream
 * (host variant: on the library's stream, copies included), streams = 1, pipeline = 1, slow_paths = 0; with RTMI_OPT_COUNTERS
 * the five work counters.
 * Checks, all before any HIP call, stats cleared; only the last one reads the scene.  In this order:
 *   RTMI_ERR_INVALID: a NULL scene, rays struct or out; group == 0; unknown flag bits; n % group != 0;
 *   n == 0: RTMI_OK, nothing is touched;
 *   RTMI_ERR_INVALID: a NULL orig4 or dir4; all five outputs NULL; two buffers overlapping as byte ranges, inputs and keys
 *     included (16 n, 16 n, 8 n; 16 n, and 16, 16, 16, 4 times n / G); keys == NULL and pixel0 + n / G - 1 >= 2^32;
 *   RTMI_ERR_UNSUPPORTED: n >= 2^31; maxdepth > 32; group > 65536; a guide buffer on a scene with analytic spheres.
 * Not here: the path kernels (pipeline 3) for explicit rays, several streams, rtmi_render_frame_multi, batches of views,
 * progressive or adaptive passes over explicit rays, a denoised one-call wrapper (mean, albedo and normal feed
 * rtmi_denoise_device directly when the groups form an image).  (Built-in thin-lens and orthographic cameras with progressive
 * passes are rtmi_render_camera*, below; fisheye and panoramic cameras need sin / cos and stay with this call.) */
enum { RTMI_RAYS_MAKE_RAY = 1u << 0 };
typedef struct rtmi_rays {
    uint32_t maxdepth;  /* project_ray's depth, 0..32                                                            */
    uint32_t group;     /* G >= 1: rays come in groups of G consecutive rays (the samples of one "pixel")        */
    uint32_t pixel0;    /* RNG key of group 0 when keys == NULL                                                  */
    uint32_t flags;     /* RTMI_RAYS_MAKE_RAY or 0                                                               */
} rtmi_rays_t;          /* 16 bytes */
typedef struct rtmi_rays_out {   /* any may be NULL, not all; no two may overlap, none may overlap an input */
    void* color;    /* n float4: the colour project_ray returns for ray i, lane 3 = 0                            */
    void* mean;     /* n/G float4: walk_ray_set's mean of each group                                             */
    void* albedo;   /* n/G float4 } rtmi_render_features*'s three buffers, a group standing for a pixel and      */
    void* normal;   /* n/G float4 } its rays for the pixel's samples                                             */
    void* ids;      /* n/G uint32 } (id of the group's first ray)                                                */
} rtmi_rays_out_t;
int rtmi_render_rays_device(rtmi_scene_t* scene, uint64_t n, const void* orig4_device, const void* dir4_device,
                            const void* keys_device /* n x 2 uint32 or NULL */, uint64_t seed, const rtmi_rays_t* rays,
                            const rtmi_rays_out_t* out_device, void* hip_stream, rtmi_stats_t* stats);
int rtmi_render_rays(rtmi_scene_t* scene, uint64_t n, const float* orig4, const float* dir4, const uint32_t* keys /* or NULL */,
                     uint64_t seed, const rtmi_rays_t* rays, const rtmi_rays_out_t* out_host, rtmi_stats_t* stats);

/* Light baked at surface points and over triangles: "how much light arrives here", asked at M elements of the
 * caller's choosing -- lightmap texels, vertices, probe positions (RTMI_BAKE_POINTS) or whole triangles, for per-face colours
 * (RTMI_BAKE_TRIANGLES).  Per element K gather rays are made on the device, path-traced as rtmi_render_rays* traces them and
 * folded; the rays never exist on the host.  The gather ray is the reference's Matte bounce (lambertian_ray's direction,
 * raytrace.rs:292-297) and its colour the reference's project_ray, so light[m] is the colour color_ray mixes a white Matte
 * surface at that point with.  The generator is NOT part of the reference: build-defined like rtmi_render_ao*, so what follows
 * IS the definition, and tests/bake_ref.py pins it bit for bit.  Only + - * / and sqrt in f32 (all correctly rounded), every
 * step rounded to f32 on all four lanes, no contraction, no transcendental function.
 * Inputs: nrm4 = M float4, the side to bake: used as given on all four lanes and NOT normalised (pass a triangle's `norm` or
 * its negative, lane 3 = +0).  pos4 = M float4 (POINTS), or 3 M float4 (TRIANGLES): corners c0, c1, c2 of element m at 3 m,
 * 3 m + 1, 3 m + 2 (the scene keeps no corners on the device, and the triangles need not be the scene's).  16-byte aligned.
 * Ray k of element m, k = 0 .. K-1, K = bake->rays; RNG key (seed, pixel = pixel0 + m, sample = k); vadd, vsub, vmul (vector *
 * scalar), vunit (the ordered four-lane dot (((0 + x x) + y y) + z z) + w w, r = sqrt(.), v * (1.f / r)) the reference's Vec3
 * operations (raytrace.rs:22-122), n = nrm4[m]:
 *   point  POINTS:    pos4[m].
 *          TRIANGLES: u, v = the unit floats (top 24 bits * 2^-24) of words 0 and 1 of RNG block 0x20000000 of the key;
 *                     if (u + v > 1.f) { u = 1.f - u; v = 1.f - v; }    (the area-preserving fold of the square onto the
 *                     triangle: no sqrt);  point = vadd(vadd(c0, vmul(vsub(c1, c0), u)), vmul(vsub(c2, c0), v)).
 *                     Block 0x20000000 is new with this call and used by nothing else (a path's bounces draw blocks 1..32,
 *                     the thin lens 0x40000000 | k, rtmi_render_ao* 0x80000000 | k, the lights 0xC0000000 | k).
 *   rv   = random_vec (raytrace.rs:188-192) from block 0 of the key: three uniforms - 0.5f, made a unit vector.  Block 0 is
 *          pixel_ray's jitter, which a path under rtmi_render_rays* never draws;
 *   orig = vadd(point, vmul(n, bias));   dir = vunit(vadd(n, rv)): rtmi_render_ao*'s two lines, the offset along n and not
 *          along rv for the reason measured in DESIGN.md 4.15.
 * Outputs (rtmi_bake_out_t; any may be NULL, not all):
 *   orig[m K + k], dir[m K + k]   the gather rays themselves;
 *   light[m]   the colour of ray m K + k is exactly what rtmi_render_rays* gives that ray with keys == NULL, group = K, the
 *              same pixel0, maxdepth and flags = 0 (bounce j of the path draws block j), and light[m] is that call's mean[m]:
 *              acc = 0.f; acc = acc + color[m K + k] for k = 0 .. K-1; acc * (1.f / (float)K) (walk_ray_set's arithmetic,
 *              raytrace.rs:1414-1426); lane 3 = 0;
 *   open[m]    (float)misses * (1.f / (float)K), misses = the number of the element's rays whose closest hit (what rtmi_trace
 *              returns for the ray under the handle's current options) has tri == 0: an integer count, so no order matters.
 * maxdepth == 0: light is zeros (project_ray returns black at depth 0); open, orig and dir are still produced, and the rays are
 * traced only if open is asked for.
 * Scenes: every kind rtmi_render_rays* takes, each with its own mode's hits, analytic spheres included (open needs no surface
 * record).  Stream semantics (device variant), stats and "no tuning changes a bit of the result" are rtmi_render_rays*'s: rays =
 * every ray traced in any pass, trace_launches = passes x batches, streams = 1, pipeline = 1.
 * How: always the per-pass pipeline on one stream of the library.  Per batch k_bake_rays stands where k_rays_begin stands (the
 * rays, the queue's count and the identity path map), then per pass the scene's closest-hit launch and k_shade_rays,
 * k_bake_open after pass 0 when open is asked for, k_accum for light.  The rays go into the workspace queue; the device
 * variant writes them straight into orig / dir when those are given and traces them there.  A batch holds whole elements:
 * rtmi_tuning_t.batch_paths rounded down to a multiple of K, at least K.  Nothing new persists on the handle.
 * rtmi_bake: host buffers; each batch's elements are copied in and its outputs copied out.
 * Checks, all before any HIP call and before the scene is used, stats cleared.  In this order:
 *   RTMI_ERR_INVALID: a NULL scene, bake struct or out; an unknown mode; rays == 0; non-zero flags; bias NaN or infinite;
 *   M == 0: RTMI_OK, nothing is touched;
 *   RTMI_ERR_INVALID: a NULL pos4 or nrm4; all four outputs NULL; two buffers overlapping as byte ranges, inputs included
 *     (16 M or 48 M, 16 M; 16 M, 4 M, 16 M K, 16 M K); pixel0 + M - 1 >= 2^32;
 *   RTMI_ERR_UNSUPPORTED: rays > 65536; maxdepth > 32; M K >= 2^31.
 * Not here: box lights (rtmi_bake_lit*, "BOX LIGHTS ON EXPLICIT RAYS AND IN THE BAKE" below, samples them at the element and at
 * every Matte bounce), the shadowed path variant (rtmi_render_shadowed*'s shading), the path kernels
 * (pipeline 3), several streams or devices, progressive continuation of a bake across calls, filtering of a lightmap. */
enum { RTMI_BAKE_POINTS = 0, RTMI_BAKE_TRIANGLES = 1 };
typedef struct rtmi_bake {
    uint32_t mode;      /* RTMI_BAKE_*                                                                           */
    uint32_t rays;      /* K gather rays per element, 1..65536                                                   */
    uint32_t maxdepth;  /* project_ray's depth of every gather ray, 0..32                                        */
    uint32_t pixel0;    /* RNG key of element 0                                                                  */
    uint32_t flags;     /* must be 0                                                                             */
    float    bias;      /* origin offset along the element's normal, finite                                      */
} rtmi_bake_t;          /* 24 bytes */
typedef struct rtmi_bake_out {   /* any may be NULL, not all; none may overlap another or an input */
    void* light;    /* M float4: mean colour arriving at element m, lane 3 = 0                                   */
    void* open;     /* M f32: share of the element's gather rays whose closest hit is a miss                     */
    void* orig;     /* M*K float4 } the gather rays themselves, ray m*K + k                                      */
    void* dir;      /* M*K float4 }                                                                              */
} rtmi_bake_out_t;
void rtmi_bake_defaults(rtmi_bake_t* bake);  /* POINTS, 64 rays, maxdepth 4, pixel0 0, flags 0, bias 0.001f */
int rtmi_bake_device(rtmi_scene_t* scene, uint64_t M, const void* pos4_device, const void* nrm4_device, uint64_t seed,
                     const rtmi_bake_t* bake, const rtmi_bake_out_t* out_device, void* hip_stream, rtmi_stats_t* stats);
int rtmi_bake(rtmi_scene_t* scene, uint64_t M, const float* pos4, const float* nrm4, uint64_t seed, const rtmi_bake_t* bake,
              const rtmi_bake_out_t* out_host, rtmi_stats_t* stats);

/* Built-in camera models rendered on the device: rtmi_render_samples[_device] with a ray generator that is
 * not only the reference's pinhole -- a thin lens (depth of field) and an orthographic camera -- and, optionally, the
 * denoiser's guide buffers of the very same rays.  The rays never leave the device: nothing is generated, keyed, stored or
 * folded by the caller.  The pinhole IS the reference's camera (Viewport::pixel_ray, raytrace.rs:1374-1394) and that mode is
 * rtmi_render_samples_device bit for bit; the other two models are NOT part of the reference (it has one camera): build-defined,
 * so what follows IS the definition, and tests/camera_ref.py pins it bit for bit.  Only + - * / and sqrt in f32 (all correctly
 * rounded), every step rounded to f32 on all four lanes, no contraction, no transcendental function.
 * Contract: rtmi_render_samples[_device]'s, word for word: samples [sample0, sample0 + nsamples) of every pixel of the tile of
 * a frame of S = vp->samples_per_pixel samples; accum (one float4 per pixel of the tile) is read only when sample0 > 0 and
 * always rewritten; out (optional, never the same buffer as accum) = accum * (1/(sample0 + nsamples)); passes must be issued
 * in sample order, each continuing the previous one on the same accum; striped tiles, streams, sub-tiles and batches apply
 * unchanged and no tuning changes a bit; maxdepth == 0 writes zeros to accum and out.
 * The ray of (row, col, sample), with pixel = row * width + col, orig / cam / vu / vv the viewport's vectors with lane 3 = +0,
 * and vadd, vsub, vmul (vector * scalar), vunit (the ordered four-lane dot (((0 + x x) + y y) + z z) + w w, r = sqrt(.),
 * v * (1.f / r)), make_ray(o, d) = (o, vunit(d)) the reference's Vec3 operations (raytrace.rs:22-122, :201-210):
 *   p = pixel_ray's image-plane point px_u, computed exactly as rtmi_render_samples_device computes it:
 *       vu_delta = vmul(vu, 1.f / (float)width);  vv_delta = vmul(vv, 1.f / (float)height);
 *       (u_off, v_off) = (0.5f, 0.5f) when S == 1, else the unit floats of words 0 and 1 of RNG block 0 of (seed, pixel, sample);
 *       p = vadd(vadd(orig, vmul(vu_delta, (float)col + u_off)), vmul(vv_delta, (float)row + v_off)).
 *   RTMI_CAMERA_PINHOLE:   make_ray(p, vunit(vsub(p, cam))): pixel_ray itself.
 *   RTMI_CAMERA_ORTHO:     c = vadd(vadd(orig, vmul(vu, 0.5f)), vmul(vv, 0.5f))   (the centre of the image plane);
 *                          axis = vunit(vsub(c, cam));  the ray is make_ray(p, axis).
 *     The image covers the image-plane rectangle itself, every ray parallel to the camera's axis.  An axis-aligned
 *     orthographic view makes EVERY ray a ray with exactly-zero direction components: the reference's expensive case
 *     (BoundingBox::collides skips that axis' slab, raytrace.rs:872-900, ~150 x the work of an ordinary ray), which the
 *     per-pass pipeline traces in place.  Tilt the camera by a hair when that cost matters.
 *   RTMI_CAMERA_THIN_LENS: lens axes eu = vunit(vu), ev = vunit(vv).
 *     Lens sample (x, y): for k = 0, 1 let w = RNG block 0x40000000 | k of (seed, pixel, sample); for j = 0, 1 the candidate
 *       x = 2.f * u(w[2 j]) - 1.f,  y = 2.f * u(w[2 j + 1]) - 1.f      (u = top 24 bits * 2^-24; a product, then a difference);
 *       the first candidate, in the order (k, j) = (0, 0), (0, 1), (1, 0), (1, 1), with (x * x) + (y * y) <= 1.f is taken.  If all
 *       four fail the sample is (0.f, 0.f): the pinhole's ray.  That happens with probability (1 - pi/4)^4 ~ 0.0021, a
 *       slight, stated over-weighting of the lens centre.  Blocks 0x40000000 | k are used by nothing else (bounces draw blocks
 *       1..32, rtmi_render_ao* 0x80000000 | k, the lights 0xC0000000 | k, rtmi_bake*'s point on a triangle the one block
 *       0x20000000, which is used by nothing else either).
 *     o = vadd(vmul(eu, x * lens_radius), vmul(ev, y * lens_radius))          (the point on the lens, relative to cam)
 *     e = vsub(p, cam);   F = vadd(cam, vmul(e, focus))                        (the point in focus)
 *     O = vadd(p, vmul(o, 1.f - 1.f / focus))       (where the lens ray crosses the image plane: rays start where the
 *                                                    reference's start, so what lies between eye and image plane stays unseen)
 *     the ray is make_ray(O, vunit(vsub(F, vadd(cam, o)))).
 *     lens_radius == 0.f runs the same arithmetic (it is not special-cased): the pinhole's picture, though signs of zero in
 *     the origin may differ from the pinhole's.  ORTHO and PINHOLE ignore lens_radius and focus.
 *   The RNG key of the path's bounces is unchanged: (seed, pixel, sample), blocks 1.. as in every render call.
 * Guides (rtmi_camera_out_t, or a NULL pointer for none; each buffer may be NULL): rtmi_render_features*'s albedo, normal
 * and ids (same layout, same arithmetic) for the samples of THIS call, computed by k_features from the hit records of pass 0,
 * i.e. from the very rays that are shaded.  They are not continued across calls.  They do not depend on vp->maxdepth: with
 * maxdepth == 0 the primary rays are traced for them alone.  Refused with RTMI_ERR_UNSUPPORTED on a scene with analytic
 * spheres, as rtmi_render_features* is; the colours are not.
 * Scenes: every kind rtmi_render takes, each with its own mode's hits.
 * How: always the per-pass pipeline (rtmi_tuning_t.pipeline is not consulted: k_path_primary's packet culls assume that the
 * samples of a pixel share one origin, and a lens breaks that).  Per batch k_gen_camera stands where k_gen_samples stands;
 * then per pass the scene's closest-hit launch and k_shade_samples, k_features after pass 0 when a guide is asked for, and
 * k_accum_samples.  Nothing new persists on the handle.
 * stats: as rtmi_render_samples_device fills them, pipeline = 1, slow_paths = 0, trace_launches = passes x batches (with
 * maxdepth == 0 and a guide: the features call's stats, rays = pixels * nsamples).
 * Checks, all before any HIP call and before the scene is used, stats cleared: everything rtmi_render_samples_device refuses
 * (a NULL scene, viewport, tile or accum; accum == out; nsamples == 0; sample0 + nsamples > S; the viewport and tile checks);
 * RTMI_ERR_INVALID for a NULL camera, an unknown model, non-zero flags, THIN_LENS with lens_radius negative or not finite or
 * focus not finite and > 0, and a guide buffer that is the same buffer as another buffer of the call.  An empty tile returns
 * RTMI_OK and touches nothing.
 * The device variant enqueues on hip_stream like rtmi_render_samples_device.  The host variant renders rows [row0, row0 +
 * nrows), copies accum in (only when sample0 > 0) and accum, out and the guides out.
 * Not here: fisheye and panoramic models (sin / cos cannot be pinned bit for bit; rtmi_render_rays* renders them), adaptive
 * passes, batches of views and rtmi_render_frame_multi for these cameras, a path-kernel (pipeline 3) variant, AO, light,
 * shadowed or preview calls through a lens. */
enum { RTMI_CAMERA_PINHOLE = 0, RTMI_CAMERA_THIN_LENS = 1, RTMI_CAMERA_ORTHO = 2 };
typedef struct rtmi_camera {
    uint32_t model;        /* RTMI_CAMERA_*                                                                              */
    uint32_t flags;        /* must be 0                                                                                  */
    float    lens_radius;  /* THIN_LENS: world units, >= 0, finite                                                       */
    float    focus;        /* THIN_LENS: distance of the plane in focus from the eye, in units of the image plane's
                              distance from the eye (> 0, finite; 1 = the image plane)                                   */
} rtmi_camera_t;           /* 16 bytes */
typedef struct rtmi_camera_out { void *albedo, *normal, *ids; } rtmi_camera_out_t;  /* each may be NULL */
void rtmi_camera_defaults(rtmi_camera_t* camera);  /* PINHOLE, 0, 0.f, 1.f */
int rtmi_render_camera_device(rtmi_scene_t* scene, const rtmi_viewport_t* vp, uint64_t seed, const rtmi_tile_t* tile,
                              const rtmi_camera_t* camera, uint32_t sample0, uint32_t nsamples, void* accum_device,
                              void* out_device /* or NULL */, const rtmi_camera_out_t* guides /* or NULL */, void* hip_stream,
                              rtmi_stats_t* stats);
int rtmi_render_camera(rtmi_scene_t* scene, const rtmi_viewport_t* vp, uint64_t seed, uint32_t row0, uint32_t nrows,
                       const rtmi_camera_t* camera, uint32_t sample0, uint32_t nsamples, float* accum_host,
                       float* out_host /* or NULL */, const rtmi_camera_out_t* guides_host /* or NULL */, rtmi_stats_t* stats);

/* Ambient occlusion rendered on the device: one f32 per pixel, the share of K hemisphere rays per primary
 * sample that reach `radius` unoccluded -- a shaded preview, a contact-shadow layer, a guide image.  NOT part of the reference,
 * which has no AO: build-defined like the denoiser, so what follows IS the definition, and tests/ao_ref.py pins it bit for bit.
 * Primary rays: exactly those of rtmi_render_features_device for the same (vp, seed, tile, sample0, nsamples): RNG block 0,
 * jittered iff S = vp->samples_per_pixel != 1, vp->maxdepth not consulted, and (tri, t, face) of a ray is what rtmi_trace
 * returns for it under the handle's current options.
 * Per sample s of pixel p (p = row * width + col of the image, the renderer's RNG key), with (ro, rd) the primary ray:
 *   a miss (tri == 0) contributes K visible rays;
 *   a hit, edge faces included:  n = the triangle's norm, * (-1.f) when face & 1 (the features call's normal);
 *                                point = rd * t + ro   (a multiplication, then an addition, all four lanes, no contraction);
 *   for k = 0 .. K-1:  rv   = random_vec (raytrace.rs:188-192) from RNG block 0x80000000 | k of (seed, p, s): three uniforms
 *                             - 0.5f, made a unit vector.  The block range is disjoint from a path's own blocks 0 .. maxdepth;
 *                      orig = point + n * bias;
 *                      dir  = unit(n + rv): lambertian_ray's direction (raytrace.rs:292-297) with one normalisation, unit(v)
 *                             = v * (1.f / sqrt(ordered dot)) as everywhere (raytrace.rs:93-96);
 *                      the ray is visible iff rtmi_occluded's definition gives 0 for (orig, dir, tmax = radius) on this handle.
 *   No case is special: a non-finite t produces whatever rays the arithmetic gives, and their answers are rtmi_occluded's.
 * The offset is along n, not along rv as lambertian_ray's is: with rv, 59 % of the AO rays of the canonical view re-hit the
 * surface they left (a flat open surface would read 0.5); with n, 11.7 % are occluded and none by its own triangle
 * (DESIGN.md 4.15 has the measurement).
 * Result: ao[p] = (float)visible * (1.f / (float)(nsamples * K)), visible = the number of visible rays over the pixel's
 * samples.  Every term is 0 or 1 and nsamples * K < 2^24, so the value does not depend on any order of summation.  A pixel
 * whose samples all missed reads 1.0.  Layout: the tile's, as rtmi_render_tile_device, one f32 per pixel.
 * Scenes: octree, linear list, generic tree and RTMI_OPT_GENERIC; RTMI_OPT_FAST / RTMI_OPT_BVH give their own modes' hits and
 * answers.  RTMI_ERR_UNSUPPORTED for a scene with analytic spheres, as for features, and for nsamples * rays >= 2^24.
 * RTMI_ERR_INVALID, before any HIP call and before the scene is used, stats cleared: a NULL scene, viewport, tile, ao or
 * output; rays 0 or above 256; non-zero flags; radius NaN or below 0; bias NaN or infinite; nsamples == 0; sample0 + nsamples
 * > S; every viewport and tile check of the features call.  An empty tile returns RTMI_OK and touches nothing.
 * stats: rays = pixels * nsamples + (samples that hit) * K; kernel_ms, streams, pipeline = 1 as for features; trace_launches
 * and trace_ms cover the primary closest-hit launches (their share: primary_ms) and the AO rays' walk launches (bounce_ms).
 * With RTMI_OPT_COUNTERS the five work counters are the primaries' closest-hit work plus the any-hit walk's actual work.
 * How: per batch, on one library stream, the features call's primary pass; k_ao_rays compacts the paths that hit and writes
 * their K rays (a sample that missed costs no walk); the ray count stays on the device; the scene's any-hit walk (or its
 * closest-hit launch, where rtmi_occluded uses that); k_ao_resolve counts per pixel.  The AO ray queue (37 B per ray at most)
 * lives on the handle, grows on demand and is freed by rtmi_scene_destroy; a batch holds at most batch_paths AO rays.  No
 * tuning changes a bit of the result.  The device variant enqueues on hip_stream like rtmi_render_tile_device; the host variant
 * renders rows [row0, row0 + nrows) and copies 4 B per pixel out.
 * Not here: AO for batches of views and for rtmi_render_frame_multi, AO as a guide of the denoisers, cosine-weighted or
 * otherwise importance-sampled variants.  (The shaded preview that multiplies this term in per sample, with the primary rays
 * traced once for AO and every light, is rtmi_render_preview*, below.) */
typedef struct rtmi_ao {
    uint32_t rays;    /* K: AO rays per primary sample that hits, 1..256 */
    uint32_t flags;   /* must be 0 */
    float radius;     /* tmax of every AO ray; +inf = unlimited; 0 is valid (nothing occludes) */
    float bias;       /* origin offset along the shading normal */
} rtmi_ao_t;
void rtmi_ao_defaults(rtmi_ao_t* ao);  /* rays 4, flags 0, radius +inf, bias 0.001f (the reference's bounce offset, raytrace.rs:284-296) */
int rtmi_render_ao_device(rtmi_scene_t* scene, const rtmi_viewport_t* vp, uint64_t seed, const rtmi_tile_t* tile,
                          uint32_t sample0, uint32_t nsamples, const rtmi_ao_t* ao, void* ao_device, void* hip_stream,
                          rtmi_stats_t* stats);
int rtmi_render_ao(rtmi_scene_t* scene, const rtmi_viewport_t* vp, uint64_t seed, uint32_t row0, uint32_t nrows,
                   uint32_t sample0, uint32_t nsamples, const rtmi_ao_t* ao, float* ao_host, rtmi_stats_t* stats);

/* Direct light rendered on the device: soft shadows from one box light, two f32 planes per pixel.
 *   shadow     the share of K light samples per primary sample that are visible from the first hit (1.0 where every sample
 *              missed): a shadow layer, a contact-shadow layer, a guide image;
 *   irradiance the mean of n . dir over those visible samples: the cosine-weighted light, so that a preview is
 *              albedo * (ambient * ao + light * irradiance) from device buffers with no bounce pass.
 * The reference declares the light (pub struct LightSource { orig, len2 }, raytrace.rs:595-598) and spells the shadow ray out
 * in a comment (_get_shadow_ray, raytrace.rs:600-610; its use in color_ray, :1203-1224) but never runs either, so the buffer is
 * build-defined like the denoiser and rtmi_render_ao*: what follows IS the definition, and tests/light_ref.py pins it bit for
 * bit.  All arithmetic is f32 on all four lanes, no contraction.
 * Primary rays: exactly those of rtmi_render_features_device for the same (vp, seed, tile, sample0, nsamples): RNG block 0,
 * jittered iff S = vp->samples_per_pixel != 1, vp->maxdepth not consulted, and (tri, t, face) of a ray is what rtmi_trace
 * returns for it under the handle's current options.
 * Per sample s of pixel p (p = row * width + col of the image, the renderer's RNG key), with (ro, rd) the primary ray and
 * K = light->rays:
 *   a miss (tri == 0) contributes K visible rays to shadow and nothing to irradiance;
 *   a hit, edge faces included:  n = the triangle's norm, * (-1.f) when face & 1 (the features call's normal);
 *                                point = rd * t + ro   (a multiplication, then an addition);
 *   for k = 0 .. K-1:  w    = RNG block 0xC0000000 | k of (seed, p, s), u_c = top 24 bits of w_c * 2^-24: one Philox block is
 *                             exactly the four rand::random draws of _get_shadow_ray.  The block range is disjoint from a
 *                             path's own blocks 0 .. maxdepth and from AO's 0x80000000 | k;
 *                      adj  = (orig.x + u_0 * len2, orig.y + u_1 * len2, orig.z + u_2 * len2, 0): per lane a multiplication,
 *                             then an addition;
 *                      v    = adj - point;
 *                      d2   = the ordered four-lane dot of v with itself ((((0 + x x) + y y) + z z) + w w, as `unit` has it);
 *                      r    = sqrt(d2);
 *                      dir  = v * (1.f / r);
 *                      o    = point + n * (bias * (u_3 + 1.f))   (the direction is taken from the unsmudged point, as in the
 *                             reference);
 *                      c    = the ordered four-lane dot of n and dir;
 *                      cull: if !(c > 0.f) the ray is not traced and is not visible (the light behind the surface, a NaN,
 *                             the light at the point);
 *                      otherwise the ray is visible iff rtmi_occluded's definition gives 0 for (o, dir, tmax = r) on this
 *                             handle; with RTMI_LIGHT_UNBOUNDED the limit is the NULL tmax instead: the reference's test as
 *                             written, where anything along the ray shadows, even beyond the light.
 * Results, with N = nsamples * K:
 *   shadow[p]     = (float)visible * (1.f / (float)N), visible = the number of visible rays over the pixel's samples: an
 *                   integer below 2^24, so the order of summation is free;
 *   irradiance[p] = acc * (1.f / (float)N), acc = 0.f, then acc = acc + c for every visible ray of a sample that hit, in
 *                   sample order, then in k order.
 * Different from the reference's comment: the own triangle is NOT excluded from the test (`id != obj.getid()`): the smudge
 * along n together with c > 0 takes its place; and the default limit is the light's distance, not infinity.
 * Layout: the tile's, as rtmi_render_ao*, one f32 per pixel in each plane.  Either plane may be NULL, not both; the two must
 * not be the same buffer.
 * Scenes: octree, linear list, generic tree and RTMI_OPT_GENERIC; RTMI_OPT_FAST / RTMI_OPT_BVH give their own modes' hits and
 * answers.  RTMI_ERR_UNSUPPORTED for a scene with analytic spheres, as for features, and for nsamples * rays >= 2^24.
 * RTMI_ERR_INVALID, before any HIP call and before the scene is used, stats cleared: a NULL scene, viewport, tile or light;
 * both outputs NULL, or the same pointer; rays 0 or above 256; unknown flag bits; len2 NaN, negative or infinite; a non-finite
 * orig or bias; nsamples == 0; sample0 + nsamples > S; every viewport and tile check of the features call.  An empty tile
 * returns RTMI_OK and touches nothing.
 * stats: rays = pixels * nsamples + live rays (live = not culled); kernel_ms, streams, pipeline = 1 as for features;
 * trace_launches and trace_ms cover the primary closest-hit launches (their share: primary_ms) and the shadow rays' walk
 * launches (bounce_ms).  With RTMI_OPT_COUNTERS the five work counters are the primaries' closest-hit work plus the any-hit
 * walk's actual work.
 * How: per batch, on one library stream, the features call's primary pass; k_light_rays builds the candidates of the paths
 * that hit and compacts the live ones per ray, its counter being the walk's ray count (it stays on the device; a batch whose
 * rays are all culled walks 0 rays); the scene's any-hit walk (or its closest-hit launch, where rtmi_occluded uses that);
 * k_light_resolve counts and folds per pixel in the defined order.  The light queue (40 B per live ray at most, 1 answer byte,
 * 4 B per candidate) lives on the handle, grows on demand and is freed by rtmi_scene_destroy; a batch holds at most
 * batch_paths candidates.  No tuning changes a bit of the result.  The device variant enqueues on hip_stream like
 * rtmi_render_tile_device; the host variant renders rows [row0, row0 + nrows) and copies 4 B per pixel and plane out.
 * Not here: batches of views and rtmi_render_frame_multi, the buffer as a denoiser guide, importance sampling.  (Shadow rays
 * inside color_ray, at every hit of every bounce: rtmi_render_shadowed*, below.)  (Several lights in one call, each with a colour, composed per sample with albedo and AO:
 * rtmi_render_preview*, below, which also returns these two planes for every light.) */
enum { RTMI_LIGHT_UNBOUNDED = 1u << 0 };
typedef struct rtmi_light {
    float orig[3];   /* LightSource.orig: the corner of the light's box                 */
    float len2;      /* LightSource.len2: its edge; 0 = a point light; >= 0, finite     */
    uint32_t rays;   /* K: light samples per primary sample that hits, 1..256           */
    uint32_t flags;  /* RTMI_LIGHT_UNBOUNDED or 0                                       */
    float bias;      /* the smudge factor; default 0.005f (raytrace.rs:607)             */
} rtmi_light_t;
void rtmi_light_defaults(rtmi_light_t* light);  /* orig (0,0,0), len2 0, rays 4, flags 0, bias 0.005f */
int rtmi_render_light_device(rtmi_scene_t* scene, const rtmi_viewport_t* vp, uint64_t seed, const rtmi_tile_t* tile,
                             uint32_t sample0, uint32_t nsamples, const rtmi_light_t* light, void* shadow_device,
                             void* irradiance_device, void* hip_stream, rtmi_stats_t* stats);
int rtmi_render_light(rtmi_scene_t* scene, const rtmi_viewport_t* vp, uint64_t seed, uint32_t row0, uint32_t nrows,
                      uint32_t sample0, uint32_t nsamples, const rtmi_light_t* light, float* shadow_host, float* irradiance_host,
                      rtmi_stats_t* stats);

/* Path tracing with the reference's shadow rays inside color_ray: a progressive pass in which every surface
 * hit of every bounce is tested against ONE box light and shows black where it is shadowed.  The reference spells the test
 * out in color_ray (raytrace.rs:1203-1224: `let shadowed = ...; if !shadowed {color} else {black}` for Solid, Matte and
 * Reflective alike) around _get_shadow_ray (:600-610) and never runs it, so the image is build-defined like
 * rtmi_render_light*: what follows IS the definition, and tests/shadowed_ref.py pins it bit for bit.  rtmi_render and
 * rtmi_render_samples* are unchanged.  All arithmetic is f32 on all four lanes, no contraction.
 * Contract: rtmi_render_samples[_device]'s in every respect -- samples [sample0, sample0 + nsamples) of a frame of S =
 * vp->samples_per_pixel samples, accum continued (read only when sample0 > 0) and rewritten, out (may be NULL) = accum *
 * (1.f / (float)(sample0 + nsamples)), the tile's layout, the stream's semantics, maxdepth == 0 writes zeros -- plus:
 * Paths: the rays of every pass are exactly those of rtmi_render_samples_device for the same arguments.  The shadow bit
 *   changes colours only: never a ray, never an RNG block 0 .. maxdepth, never the "Rays" a plain render counts.
 * Shadow test: made at the hit of a path's ray number j (j = the bounces behind it, 0 for the primary ray) when the hit is
 *   neither a miss nor an edge face (face & 2): Solid, Matte and Reflective, including the last ray of a path whose depth is
 *   exhausted.  With (ro, rd) that ray, (tri, t, face) its closest hit as rtmi_trace returns it under the handle's options,
 *   (p, s) the path's pixel (row * width + col) and sample number:
 *     point = rd * t + ro                          (a multiplication, then an addition);
 *     n     = the triangle's norm, * (-1.f) when face & 1;
 *     w     = RNG block 0xC0000000 | j of (seed, p, s), u_c = top 24 bits of w_c * 2^-24;
 *     adj, v, d2, r, dir, o, c                     exactly as rtmi_render_light* states them, from light->orig, len2, bias;
 *     shadowed_j = !(c > 0.f) || rtmi_occluded's answer for (o, dir, tmax = r), the NULL tmax with RTMI_LIGHT_UNBOUNDED.
 *   ONE candidate per hit: light->rays must be 1.  At j = 0 this is candidate k = 0 of rtmi_render_light* on the same sample.
 * Colour: color_ray's (shade_hit's), with the surface colour of level j replaced by (0, 0, 0) where shadowed_j:
 *   c = mix_color(shadowed_j ? black : color_j, c, alpha_j), evaluated inside-out over the path's Matte / Reflective levels;
 *   a terminal Solid shows shadowed ? black : color.  The sky, edge faces and the black of an exhausted depth are untouched.
 * Per pixel: rtmi_render_samples_device's sums (acc = acc + sample colour in sample order; * the reciprocal).
 * Scenes: octree, linear list, generic tree and RTMI_OPT_GENERIC are exact; RTMI_OPT_FAST / RTMI_OPT_BVH give their own
 *   modes' hits and answers.  RTMI_ERR_UNSUPPORTED for a scene with analytic spheres.
 * RTMI_ERR_INVALID, before any HIP call and before the scene is used, stats cleared: every check of
 *   rtmi_render_samples[_device] (NULL scene, viewport, tile or accum; accum == out; nsamples == 0; sample0 + nsamples > S;
 *   the viewport and tile checks), every parameter check of rtmi_render_light* on light (NULL; rays 0 or above 256; unknown
 *   flag bits; len2 NaN, negative or infinite; a non-finite orig or bias), and rays != 1.  An empty tile returns RTMI_OK.
 * stats: rays = the plain call's rays + the live shadow rays traced (live = c > 0.f); pipeline = 1, slow_paths = 0 (no slow
 *   queue: a ray with a zero direction component is traced in place); trace_launches counts, per batch and pass, the
 *   closest-hit launch and the shadow rays' walk launch (2 * maxdepth per batch); trace_ms is their summed time, primary_ms
 *   the closest-hit launches' share (all passes, not only the primary rays'), bounce_ms the walks' share.  With
 *   RTMI_OPT_COUNTERS the five work counters are the plain call's closest-hit work plus the walks' actual work.
 * How: always the per-pass pipeline (rtmi_tuning_t.pipeline is not consulted), batches, sub-tiles and streams as for
 *   rtmi_render_samples_device.  Per pass: the closest-hit launch; k_shadow_rays builds the candidates and compacts the live
 *   ones into a shadow queue whose counter stays on the device (a second control block per stream); the scene's any-hit walk
 *   of that queue (its closest-hit launch where rtmi_occluded uses that, with hit records of its own); k_shade_shadowed
 *   shades with the answers, keeping one mask word per path (bit j = shadowed_j).  Nothing is copied to the host between
 *   passes.  The buffers (45 B per path at most beside the plain workspace, plus 8 B per path on scenes without an any-hit
 *   kernel) live on the handle, grow on demand and are freed by rtmi_scene_destroy.  No tuning changes a bit of the result.
 * Not here: several or coloured lights inside the path, falloff or a cosine term (the reference's test is binary; light that
 *   ADDS energy, with both: rtmi_render_lit*, "BOX LIGHTS IN THE PATH" below), more than one light sample per hit, shadowed variants of rtmi_render_rays*, adaptive passes, batches of views,
 *   rtmi_render_frame_multi and the path kernels (pipeline 3). */
int rtmi_render_shadowed_device(rtmi_scene_t* scene, const rtmi_viewport_t* vp, uint64_t seed, const rtmi_tile_t* tile,
                                uint32_t sample0, uint32_t nsamples, const rtmi_light_t* light, void* accum_device,
                                void* out_device /* or NULL */, void* hip_stream, rtmi_stats_t* stats);
int rtmi_render_shadowed(rtmi_scene_t* scene, const rtmi_viewport_t* vp, uint64_t seed, uint32_t row0, uint32_t nrows,
                         uint32_t sample0, uint32_t nsamples, const rtmi_light_t* light, float* accum_host,
                         float* out_host /* or NULL */, rtmi_stats_t* stats);

/* SAMPLING THE ENVIRONMENT at matte hits: next-event estimation towards the map's bright texels.  A progressive
 * pass that renders, in expectation, the image rtmi_render_samples[_device] renders of a scene with an environment, with less
 * noise where a small bright region (a sun) lights matte surfaces: at every Matte hit that bounces, one shadow ray is also sent
 * towards a direction drawn from the map's brightness, and combined with the bounce's own escape by the balance heuristic.  NOT part
 * of the reference; build-defined like the environment itself: what follows IS the definition, tests/envlight_ref.py pins it bit
 * for bit.  float32 throughout, every step rounded (no fused multiply-add), vdot the ordered sum seeded with +0, all four lanes.
 *
 * The sampler table of an n x n environment, in integers, so that no summation order exists.  For texel (i, j) with colour (r, g, b):
 *     lum = (r + g) + b;  a lum that is not finite or not > 0.f counts as 0.f
 *     px = ((float)i + 0.5f) / (float)n * 2.f - 1.f;  py likewise from j;  z = (1.f - |px|) - |py|;  if z < 0.f: the fold on the
 *     old (px, py)                                   (the texel centre's map point as rtmi_scene_set_sky has it before vunit)
 *     r2 = (px * px + py * py) + z * z;  w = lum / (r2 * sqrtf(r2));  a w that is not finite (an overflow) counts as 0.f
 *     (a piece dpx dpy of the square covers the solid angle dpx dpy / r^3: w makes the pdf per solid angle proportional to lum)
 *     wmax = the maximum of w over the table
 *     s = w * (1048576.f / wmax);  s = !(s >= 0.f) ? 0.f : (s > 1048576.f ? 1048576.f : s);  q(i, j) = 1 + (uint32)s
 *     wmax == 0.f: q = 1 everywhere.  The + 1 keeps the pdf positive in every direction; the estimator is unbiased because of it.
 *     total = the sum of q (uint64);  C = the inclusive prefix sum of q in row-major order (uint64)
 * The table is built on the device on the first call that needs it, kept on the scene handle, and dropped by
 * rtmi_scene_set_environment and rtmi_scene_set_sky (setting, replacing or clearing).  rtmi_scene_get_env_sampler copies q back
 * (n * n uint32, row-major; q_out may be NULL) with total and n, building the table if need be; *n_out = 0: no environment.
 *
 * pe(d), the environment's pdf per solid angle of a world unit direction d:
 *     m, a, px, py and the fold exactly as the lookup above computes them
 *     gx = floorf((px * 0.5f + 0.5f) * (float)n);  gx = !(gx >= 0.f) ? 0.f : (gx > (float)n - 1.f ? (float)n - 1.f : gx);  i = (int)gx;
 *     j likewise from py
 *     pe = (((float)q(i, j) / (float)total) * (((float)n * (float)n) * 0.25f)) / ((a * a) * a)
 *   Right for a rotation frame only: RTMI_ERR_UNSUPPORTED, before any HIP call, when some |vdot(r_i, r_j) - delta_ij| > 1e-4f.
 * pb(n, d, s), the pdf per solid angle of the reference's Matte bounce dir = unit(n + s), s = random_vec (the unit vector of a
 * uniform point of the cube: density 1 / (24 m^3) per solid angle, m = max |s_c|; the map s -> unit(n + s) has the Jacobian 4 cos):
 *     cos = vdot(n, d);  m = fmaxf(fmaxf(|s.x|, |s.y|), |s.z|);  pb = cos > 0.f ? cos / (6.f * ((m * m) * m)) : 0.f
 *
 * The pass.  Contract: rtmi_render_samples[_device]'s in every respect, as rtmi_render_shadowed* states it.  The rays of every pass
 * are exactly those of rtmi_render_samples_device for the same arguments: no ray, no RNG block 0 .. maxdepth and no plain "Rays"
 * count moves.  At the hit of a path's ray number j, when the hit is a Matte surface (neither a miss nor an edge face) and the path
 * bounces (maxdepth - j - 1 != 0: an exhausted level gets no sample, as the plain render shows black there):
 *     point = rd * t + ro;  n = the triangle's norm, * (-1.f) when face & 1
 *     w = RNG block 0xC0000000 | j of (seed, pixel, sample);  T = the upper 64 bits of ((uint64)w0 << 32 | w1) * total
 *     texel (i, j'): the first k = j' * n + i with C[k] > T
 *     px = ((float)i + u(w2)) / (float)n * 2.f - 1.f;  py likewise from j' and u(w3);  u(x) = top 24 bits of x * 2^-24
 *     z = (1.f - |px|) - |py|;  if z < 0.f: the fold;  m = vunit(px, py, z)
 *     omega = vunit((r0 * m.x + r1 * m.y) + r2 * m.z)                                  (the transposed frame)
 *     cos = vdot(n, omega);  s = omega * (2.f * cos) - n                              (the random_vec whose bounce is omega)
 *     o = point + s * bias                  (where that bounce ray starts when bias = 0.001f: the shadow ray sees what it would)
 *     culled when !(cos > 0.f); otherwise L = the lookup of omega, wgt = pb(n, omega, s) / (pb + pe(omega))
 *     live when wgt > 0.f and some lane 0..2 of L != 0.f;  direct_j = L * wgt when live and rtmi_occluded's answer for
 *     (o, omega, no tmax) is 0, else (0, 0, 0)
 *   and with nr the bounce ray (lambertian_ray with rv = random_vec of block j + 1): wb = pb(n, nr.dir, rv) / (pb + pe(nr.dir)).
 *   A Reflective level has direct_j = 0 and wb = 1.f; so has the primary ray (wb) and an exhausted level (direct_j).
 * Colour: a miss is lookup(rd) * wb, wb that of the path's last bounce; the fold is c = mix_color(color_j, c + direct_j, alpha_j),
 *   inside-out over the path's Matte / Reflective levels.  Edge faces, Solid ends and the black of exhausted depth as in color_ray.
 * (The reference's Matte bounce starts at point + rv * 0.001f, which lies behind the surface for half of the draws and then hits
 *  that surface from behind; a shadow ray from point + n * bias sees a different scene, and the two estimators then differ in
 *  expectation.  Hence o above.)
 * bias: ONLY bias == 0.001f, the reference's own offset of a bounce ray and the default, renders rtmi_render_samples*'s image in
 *   expectation.  Every other finite value is accepted and is BIASED against it: the shadow rays then start elsewhere than the
 *   bounce rays they stand for and see a different scene.
 * RTMI_ERR_UNSUPPORTED, before any HIP call, for a scene without an environment, with analytic spheres, with a dielectric, with
 *   vertex normals, with textures or with normal maps, and for a frame that is no rotation.
 * RTMI_ERR_INVALID, before any HIP call and before the scene is used, stats cleared: every check of rtmi_render_samples[_device],
 *   a bias that is not finite, flags != 0.  env == NULL: the defaults.  An empty tile returns RTMI_OK.
 * stats: as rtmi_render_shadowed* fills them: rays = the plain rays + the live shadow rays, trace_launches = 2 per pass and batch,
 *   primary_ms the closest-hit launches' share, bounce_ms the walks'.
 * How: rtmi_render_shadowed*'s pass structure and buffers: k_envlight_rays, the occlusion walk, k_shade_envlight per pass (on an
 *   octree the walk is the scene's closest-hit launch, which is faster than the any-hit kernel on rays that mostly escape; the
 *   answers are the same; no launch but the shading at the exhausted pass); beside them
 *   16 B per shadow queue entry, 16 B per path and level (the direct stack) and 4 B per path, allocated by this call only.
 * Not here: smooth, textured, normal-mapped and glass scenes; samples at the exhausted level; more than one environment sample per
 *   hit; box lights in the same pass; adaptive variants, view batches and denoised wrappers; the path kernels (pipeline 3). */
typedef struct rtmi_envlight { float bias; /* default 0.001f */ uint32_t flags; /* 0 */ } rtmi_envlight_t;
void rtmi_envlight_defaults(rtmi_envlight_t* env);
int rtmi_scene_get_env_sampler(rtmi_scene_t* scene, uint32_t* q_out /* n * n, or NULL */, uint64_t* total_out /* or NULL */,
                               uint32_t* n_out);
int rtmi_render_envlight_device(rtmi_scene_t* scene, const rtmi_viewport_t* vp, uint64_t seed, const rtmi_tile_t* tile,
                                uint32_t sample0, uint32_t nsamples, const rtmi_envlight_t* env /* or NULL = defaults */,
                                void* accum_device, void* out_device /* or NULL */, void* hip_stream, rtmi_stats_t* stats);
int rtmi_render_envlight(rtmi_scene_t* scene, const rtmi_viewport_t* vp, uint64_t seed, uint32_t row0, uint32_t nrows,
                         uint32_t sample0, uint32_t nsamples, const rtmi_envlight_t* env /* or NULL = defaults */, float* accum_host,
                         float* out_host /* or NULL */, rtmi_stats_t* stats);

/* BOX LIGHTS IN THE PATH: direct light from up to four coloured box lights at every matte hit.  A box light
 * (rtmi_light_t, the reference's LightSource { orig, len2 }) is not geometry: no bounce ray can hit one.  This progressive pass puts
 * its light into the paths by next-event estimation: at every Matte hit that bounces, one shadow ray per light is sent to a point
 * of the light's box, and what arrives unoccluded is added to the light the surface passes on.  NOT part of the reference (which
 * declares the light and never uses it); build-defined like rtmi_render_light* and rtmi_render_envlight*: what follows IS the
 * definition, and tests/lit_ref.py pins it bit for bit.  All arithmetic is f32 on all four lanes, every step rounded (no fused
 * multiply-add), + - * / and sqrt only.
 * Contract: rtmi_render_samples[_device]'s in every respect, as rtmi_render_shadowed* states it: samples [sample0, sample0 +
 *   nsamples) of a frame of S samples, accum continued and rewritten, out (may be NULL) = accum * (1.f / (float)(sample0 +
 *   nsamples)), the tile's layout, the stream's semantics, maxdepth == 0 writes zeros, an empty tile returns RTMI_OK.
 * Paths: the rays of every pass are exactly those of rtmi_render_samples_device for the same arguments: no ray, no RNG block
 *   0 .. maxdepth and no plain "Rays" count moves.
 * Candidates: made at the hit of a path's ray number j when the hit is a Matte surface (neither a miss nor an edge face) and the
 *   path bounces there (maxdepth - j - 1 != 0: an exhausted level gets no sample, as in rtmi_render_envlight*).  With point and n
 *   as rtmi_render_shadowed* states them, for l = 0 .. nlights-1:
 *     w      = RNG block 0xC0000000 | (l << 16) | j of (seed, pixel, sample); for l = 0 that is rtmi_render_shadowed*'s block.
 *              Every light has a stream of its own: the lights' jitter is independent, unlike rtmi_render_preview*'s lights,
 *              which share their blocks so that each layer equals its single call;
 *     adj, v, d2, r, dir, o, c   exactly as rtmi_render_light* states them, from lights[l].orig, len2, bias;
 *     culled when !(c > 0.f); otherwise visible iff rtmi_occluded's definition gives 0 for (o, dir, tmax = r), the NULL limit
 *              when lights[l].flags has RTMI_LIGHT_UNBOUNDED;
 *     g_l    = c, or with RTMI_LIT_INVERSE_SQUARE  c / d2.
 * Direct light of a level: direct_j = (0, 0, 0, 0); then for l ascending over the live and visible candidates, per channel
 *   ch = 0 .. 2:  direct_j[ch] = direct_j[ch] + light_color[l][ch] * g_l  (a multiplication, then an addition); lane 3 stays 0.
 *   A Reflective level and an exhausted level have direct_j = 0.
 * Colour: the fold is c = mix_color(color_j, c + direct_j, alpha_j), inside-out over the path's Matte / Reflective levels, as
 *   in rtmi_render_envlight*.  A miss is the sky constant; on a scene with an environment it is the plain lookup of the ray's
 *   direction, unweighted (there is no second estimator to balance against).  Solid ends, edge faces and the black of exhausted
 *   depth as in color_ray.  No case is special: non-finite values propagate as the arithmetic gives them.
 * Per pixel: rtmi_render_samples_device's sums.
 * nlights == 0 is valid: no candidate kernel and no walk is launched.  The image is then rtmi_render_samples_device's wherever
 *   no inner colour of a fold is -0.f (c + 0.f turns a -0.f into +0.f, which mix_color may show in the sign of a zero).
 * Scenes: octree, linear list, generic tree and RTMI_OPT_GENERIC are exact; RTMI_OPT_FAST / RTMI_OPT_BVH give their own modes'
 *   hits and answers.  With or without an environment.  RTMI_ERR_UNSUPPORTED, before any HIP call, for a scene with analytic
 *   spheres, a dielectric, vertex normals, textures or normal maps; the handle stays usable.  (With RTMI_LIT_SURFACES only
 *   analytic spheres are refused: "BOX LIGHTS ON SHADED SURFACES" below.)
 * RTMI_ERR_INVALID, before any HIP call and before the scene is used, stats cleared: every check of
 *   rtmi_render_samples[_device]; lit == NULL; nlights > RTMI_LIT_MAX_LIGHTS; unknown flag bits; every parameter check of
 *   rtmi_render_light* on each used light (the message names the light's index), and rays != 1; a non-finite used colour.
 * stats: as rtmi_render_shadowed* fills them: rays = the plain rays + the live candidates traced, trace_launches = 2 per pass
 *   and batch (an empty event pair where no walk runs), primary_ms the closest-hit launches' share, bounce_ms the walks',
 *   pipeline = 1, slow_paths = 0.
 * How: rtmi_render_shadowed*'s pass structure: k_lit_rays builds a hit's candidates in registers and compacts the live ones
 *   of all lights into ONE shadow queue per pass (one atomic per block of 256 paths), with one limit array (r, or +inf for an
 *   unbounded light) and a float4 weight per entry; the occlusion walk of that queue (on an octree the scene's closest-hit
 *   launch, which is faster than the any-hit kernel here as it is for rtmi_render_envlight*; the answers are the same);
 *   k_shade_lit sums the weights of an entry's unoccluded candidates in l order and folds.  Beside the plain workspace, per
 *   path and light: 53 B of queue, 4 B of slot and, on an octree, 12 B of hit records; per path and level 16 B (the direct
 *   stack); allocated by this call only.  No tuning changes a bit.
 * Not here: more than one sample per light and hit; lights chosen
 *   by importance; rtmi_render_envlight*'s sampling in the same pass; lights at Reflective or exhausted levels; adaptive
 *   variants, view batches and denoised wrappers; the path kernels (pipeline 3).  (Explicit rays and the bake with these lights:
 *   rtmi_render_rays_lit*, rtmi_bake_lit*, below.) */
/* rtmi_lit_t.flags: bit 0 RTMI_LIT_INVERSE_SQUARE, bit 2 RTMI_LIT_SURFACES ("BOX LIGHTS ON SHADED SURFACES" below).  Bit 1 is not
 * assigned: it and every higher bit are unknown flags and refused. */
enum { RTMI_LIT_MAX_LIGHTS = 4, RTMI_LIT_INVERSE_SQUARE = 1u << 0, RTMI_LIT_SURFACES = 1u << 2 };
typedef struct rtmi_lit {
    uint32_t nlights;          /* 0: 0..RTMI_LIT_MAX_LIGHTS                                                       */
    uint32_t flags;            /* 4: RTMI_LIT_INVERSE_SQUARE, RTMI_LIT_SURFACES, both or 0                        */
    rtmi_light_t lights[4];    /* 8: entries >= nlights are ignored; rays must be 1; flags may hold               */
                               /*    RTMI_LIGHT_UNBOUNDED                                                         */
    float light_color[4][3];   /* 120: the radiance scale per light; any finite float                             */
} rtmi_lit_t;                  /* 168 bytes */
void rtmi_lit_defaults(rtmi_lit_t* lit);  /* nlights 0, flags 0, rtmi_light_defaults x 4 with rays = 1, colours 1 */
int rtmi_render_lit_device(rtmi_scene_t* scene, const rtmi_viewport_t* vp, uint64_t seed, const rtmi_tile_t* tile,
                           uint32_t sample0, uint32_t nsamples, const rtmi_lit_t* lit, void* accum_device,
                           void* out_device /* or NULL */, void* hip_stream, rtmi_stats_t* stats);
int rtmi_render_lit(rtmi_scene_t* scene, const rtmi_viewport_t* vp, uint64_t seed, uint32_t row0, uint32_t nrows,
                    uint32_t sample0, uint32_t nsamples, const rtmi_lit_t* lit, float* accum_host,
                    float* out_host /* or NULL */, rtmi_stats_t* stats);

/* BOX LIGHTS ON SHADED SURFACES: rtmi_render_lit*, rtmi_render_rays_lit* and rtmi_bake_lit* on scenes with a
 * dielectric, vertex normals, textures and normal maps.  Opt-in: a call whose rtmi_lit_t.flags has RTMI_LIT_SURFACES takes these
 * scenes; without the flag every call behaves as stated above, refusals and their wording included.  Analytic spheres stay refused
 * with the same message.  On a scene without any of these features the flag changes no bit and no stat.  Build-defined; what
 * follows IS the definition, and tests/lit_surfaces_ref.py pins it bit for bit.  f32 on all four lanes, every step rounded, no
 * fused multiply-add.
 * Everything of "BOX LIGHTS IN THE PATH" holds except what follows.  The paths, the RNG blocks 0 .. maxdepth, the queue order and
 *   the plain ray count are those of the plain render (rtmi_render_samples*, rtmi_render_rays*, rtmi_bake*) of the same scene on its
 *   own shading level.  Unchanged: the light blocks 0xC0000000 | l << 16 | j and their four draws; adj, v, d2, r, dir; the limit;
 *   g_l = c or c / d2; the sum over l ascending.
 * Normals at a Matte hit that bounces:
 *   ng = the record's normal, * -1.f on a back face;
 *   N  = the hit's shading normal, exactly the normal the bounce is first evaluated with: ng to start with; the result of "VERTEX
 *        NORMALS OF A SCENE" where it is usable (use); the result of "NORMAL MAPS OF A SCENE" about that where it is usable (usem).
 *        N does not depend on the bounce's random vector: the bounce's own fall-back to ng, when its ray leaves on the wrong side
 *        of the real surface, does not touch the lamp term.
 * Candidate l:
 *   c = vdot(N, dir);
 *   o = vadd(point, vmul(ng, bias_l * (u(w[3]) + 1.f))): the geometric normal, because an offset along a shading normal can start
 *       under a neighbouring facet;
 *   live when c > 0.f && vdot(ng, dir) > 0.f: the second test keeps a lamp behind the real surface from lighting it through a
 *       tilted normal.  On a hit with N == ng this is "BOX LIGHTS IN THE PATH"'s candidate bit for bit.
 * Other surface kinds: a Dielectric level gets no candidate and direct_j = 0, like a Reflective level.  Glass occludes a shadow
 *   ray like any other surface (no transparent shadows).
 * Colour: the fold c = mix_color(colour_j, c + direct_j, alpha_j) reads a level's colour where the plain render of the scene reads
 *   it: on a textured scene "TEXTURES OF A SCENE"'s colour of the hit.  A textured Solid hit ends with that colour.  The lamp's
 *   weight is not textured: the albedo acts in the fold.
 * Bounce: the plain render's, statement for statement: the same normal, the same wrong-side re-evaluation, RTMI_DIELECTRIC's
 *   reflect-or-refract draw from word 3 of the level's block.
 * rtmi_bake_lit*: direct keeps the caller's element normal for both roles (c and the offset), as stated above; the flag only lets
 *   it run on these scenes, and light is rtmi_render_rays_lit*'s with the flag.
 * stats: rays = the plain rays + the live candidates traced.
 * How: scenes whose shading level is above the environment's, or that have a dielectric, run k_lit_rays_surf and k_shade_lit_surf
 *   (and their _explicit forms): k_lit_rays' compaction with N computed once before the light loop, and k_shade_lit's slot loop in
 *   front of a lit arm of the top shading level, which computes N again and reads no record of the candidate kernel.  One set for
 *   every featured scene: a table the scene lacks is passed empty and tested at run time.  The colour stack is the plain render's,
 *   allocated on a textured scene only.  Every other scene runs the kernels it ran before, with or without the flag.
 * Not here: rtmi_render_emissive* and rtmi_render_envlight* on these scenes (their balance heuristic needs the bounce's density,
 *   which is a mixture under a shading normal with the wrong-side re-evaluation); transparent shadows; textured lamp weights;
 *   analytic spheres; adaptive, view-batch and denoised variants; the path kernels (pipeline 3). */

/* BOX LIGHTS ON EXPLICIT RAYS AND IN THE BAKE.  Build-defined like the calls they extend; what follows IS the
 * definition, and tests/bake_lit_ref.py pins it bit for bit.  f32 on all four lanes, every step rounded, no fused multiply-add.
 *
 * rtmi_render_rays_lit[_device]: rtmi_render_rays[_device] with "BOX LIGHTS IN THE PATH" above in every path.
 * Contract: rtmi_render_rays*'s in every respect: groups, RTMI_RAYS_MAKE_RAY, keys or the ray's place in its group, color / mean /
 *   albedo / normal / ids, batches of whole groups, the stream's semantics, maxdepth == 0.  The paths, the RNG blocks 0 .. maxdepth,
 *   the plain ray count and the guide buffers are rtmi_render_rays*'s for the same arguments.
 * Candidates: at the hit of a path's ray number j that is a Matte surface and bounces (maxdepth - j - 1 != 0), exactly as
 *   rtmi_render_lit* states them: w = RNG block 0xC0000000 | (l << 16) | j of the ray's key (seed, pixel, sample), the key
 *   rtmi_render_rays* gives the ray (its keys entry, or pixel0 + its group and its place in the group); adj, v, d2, r, dir, o, c;
 *   culled when !(c > 0.f); the limit r, or none for RTMI_LIGHT_UNBOUNDED; g_l, RTMI_LIT_INVERSE_SQUARE; direct_j and the fold
 *   c = mix_color(color_j, c + direct_j, alpha_j); a miss is the sky constant or the environment's plain lookup.
 * RTMI_ERR_INVALID: every check of rtmi_render_rays*, then every check rtmi_render_lit* makes on `lit`, before any HIP call, stats
 *   cleared.  RTMI_ERR_UNSUPPORTED: rtmi_render_rays*'s, then the scenes rtmi_render_lit* refuses, with its wording; the handle
 *   stays usable.
 * stats: rays = the plain rays + the live candidates traced; trace_launches = 2 per pass and batch (an empty event pair where no
 *   walk runs); otherwise rtmi_render_rays*'s.
 * How: rtmi_render_rays*'s batch loop with, per pass, k_lit_rays_explicit, the occlusion walk of its shadow queue (rtmi_render_lit*'s
 *   route: the closest-hit launch on an octree) and k_shade_lit_explicit: k_lit_rays' and k_shade_lit's bodies with rays_key's key.
 *
 * rtmi_bake_lit[_device]: rtmi_bake[_device] with lamps.  orig, dir and open are rtmi_bake*'s: the same bits for the same arguments.
 *   light[m]   exactly rtmi_render_rays_lit*'s mean[m] of the gather rays with keys == NULL, group = K, the same pixel0, maxdepth
 *              and lit: the indirect light, with the lamps lighting every Matte bounce of every gather path.
 *   direct[m]  M float4, lane 3 = 0: the lamps' light arriving at the element itself.  For ray index k = 0 .. K-1, key (seed,
 *              pixel0 + m, k), n = nrm4[m] as given on all four lanes and NOT normalised (c below scales with its length: pass a
 *              unit normal):
 *     point  POINTS: pos4[m].  TRIANGLES: the very point gather ray k starts from (the same draw of block 0x20000000, the same
 *            fold, the same vadd(vadd(c0, ..), ..));
 *     for l = 0 .. nlights-1, with vdot the ordered four-lane dot (((0 + x x) + y y) + z z) + w w:
 *       w    = RNG block 0xC000FFFF | (l << 16) of the key (level field 0xFFFF; see the list of blocks below);
 *       adj  = (orig[0] + u(w[0]) * len2, orig[1] + u(w[1]) * len2, orig[2] + u(w[2]) * len2, 0), u = top 24 bits * 2^-24;
 *       v = vsub(adj, point); d2 = vdot(v, v); r = sqrt(d2); dir = vmul(v, 1.f / r);
 *       o = vadd(point, vmul(n, bias_l * (u(w[3]) + 1.f))); c = vdot(n, dir)      (rtmi_render_light*'s arithmetic);
 *       culled when !(c > 0.f); otherwise visible iff rtmi_occluded's definition gives 0 for (o, dir, tmax = r), the NULL limit
 *       when lights[l].flags has RTMI_LIGHT_UNBOUNDED;  g_l = c, or with RTMI_LIT_INVERSE_SQUARE c / d2;
 *     d_k = (0, 0, 0, 0); then for l ascending over the live and visible candidates d_k[ch] = d_k[ch] + light_color[l][ch] * g_l;
 *     direct[m] = walk_ray_set's fold of d_0 .. d_{K-1}: acc = 0.f; acc = acc + d_k; acc * (1.f / (float)K).
 *   direct does not depend on maxdepth; like open it is produced at maxdepth == 0.  With every output but direct NULL no gather
 *   ray is traced.
 *   A lightmap texel of a surface (color, alpha) is then mix_color(color, light[m] + direct[m], alpha).
 * RNG blocks drawn under one key, pairwise distinct: 0 (the gather ray), 0x20000000 (the point), 1 .. 32 (the bounces),
 *   0xC0000000 | l << 16 | j with j <= 31 (the candidates of path level j) and 0xC000FFFF | l << 16 (the element's candidates):
 *   no path level has the level field 0xFFFF.
 * Checks, before any HIP call and before the scene is used, stats cleared: rtmi_bake*'s in their order, with "all five outputs
 *   NULL" and the overlap check extended to direct (16 M bytes); then rtmi_render_lit*'s checks of `lit`; then its scene refusals.
 * stats: rtmi_bake*'s, and rays also counts the live candidates of the paths and of the elements; trace_launches = 2 per pass
 *   and batch, + 1 per batch for the elements' walk when direct is asked for.
 * How: per batch, when direct is asked for: k_bake_lit_rays (k_bake_rays' staging, k_lit_rays' candidates and compaction, one
 *   thread per (element, k)), the occlusion walk, k_bake_lit_resolve (d_k), k_accum; then rtmi_bake*'s batch with the lit passes.
 *   The shadow queue, limits, weights, answers and slots are sized batch x nlights, the direct stack batch x depth, allocated by
 *   these calls only.  No tuning changes a bit.
 * Not here: more than one sample per light and hit; rtmi_render_envlight*'s
 *   sampling in the same pass; adaptive, view and denoised variants. */
typedef struct rtmi_bake_lit_out {   /* rtmi_bake_out_t and direct: any may be NULL, not all; none may overlap another or an input */
    void *light, *open, *orig, *dir;
    void* direct;   /* M float4: the lamps' light at element m, lane 3 = 0 */
} rtmi_bake_lit_out_t;
int rtmi_render_rays_lit_device(rtmi_scene_t* scene, uint64_t n, const void* orig4_device, const void* dir4_device,
                                const void* keys_device /* or NULL */, uint64_t seed, const rtmi_rays_t* rays, const rtmi_lit_t* lit,
                                const rtmi_rays_out_t* out_device, void* hip_stream, rtmi_stats_t* stats);
int rtmi_render_rays_lit(rtmi_scene_t* scene, uint64_t n, const float* orig4, const float* dir4, const uint32_t* keys /* or NULL */,
                         uint64_t seed, const rtmi_rays_t* rays, const rtmi_lit_t* lit, const rtmi_rays_out_t* out_host,
                         rtmi_stats_t* stats);
int rtmi_bake_lit_device(rtmi_scene_t* scene, uint64_t M, const void* pos4_device, const void* nrm4_device, uint64_t seed,
                         const rtmi_bake_t* bake, const rtmi_lit_t* lit, const rtmi_bake_lit_out_t* out_device, void* hip_stream,
                         rtmi_stats_t* stats);
int rtmi_bake_lit(rtmi_scene_t* scene, uint64_t M, const float* pos4, const float* nrm4, uint64_t seed, const rtmi_bake_t* bake,
                  const rtmi_lit_t* lit, const rtmi_bake_lit_out_t* out_host, rtmi_stats_t* stats);

/* EMISSIVE TRIANGLES sampled at matte hits: next-event estimation towards lamps that are part of the scene.  A
 * Solid triangle ends a path with its surface colour, and nothing limits that colour to 1: a bright Solid triangle IS an area
 * light in rtmi_render* (visible, reflected, with the penumbrae of its shape), found only by the bounces that happen to hit it.
 * rtmi_scene_set_emitters marks such triangles as lamps; rtmi_render_emissive[_device] is a progressive pass that renders, in
 * expectation, the image rtmi_render_samples[_device] renders of the same scene, with less noise where small lamps light matte
 * surfaces: at every Matte hit that bounces, one shadow ray is also sent to a point drawn on the lamps, and combined with the
 * bounce's own chance of hitting a lamp by the balance heuristic.  NOT part of the reference; build-defined: what follows IS the
 * definition, tests/emissive_ref.py pins it bit for bit.  float32 throughout, every step rounded (no fused multiply-add), vdot the
 * ordered sum seeded with +0, all four lanes; + - * /, sqrt, fabsf and comparisons only.
 *
 * rtmi_scene_set_emitters(scene, corners9, emit_of_tri, n): n == ntris bytes, entry 0 the sentinel's (ignored); a non-zero byte
 *   marks the triangle.  corners9 as in rtmi_scene_set_normals (read for the marked triangles only).  A marked triangle's surface
 *   must be Solid and its corners finite, else RTMI_ERR_INVALID naming the triangle and the marks stay as they were.  A lamp's
 *   radiance is its surface colour (any float; scene creation does not limit a colour).  emit_of_tri == NULL or
 *   n == 0 clears the marks.  Marking changes no other call: every other entry point renders the scene exactly as before.
 * The lamps are numbered e = 1 .. L in triangle order.  Per lamp, from its corners c0, c1, c2 and its radiance (r, g, b):
 *     e1 = c1 - c0;  e2 = c2 - c0;  x = (e1.y * e2.z - e1.z * e2.y, e1.z * e2.x - e1.x * e2.z, e1.x * e2.y - e1.y * e2.x)
 *     A = 0.5f * sqrtf(vdot(x, x));  n_e = the triangle record's norm (unit, as every shading statement uses it)
 *     w = A * ((r + g) + b);  a w that is not > 0.f (a NaN too) or not finite counts as 0.f
 *     wmax = the maximum of w over the lamps
 *     s = w * (1048576.f / wmax);  s = !(s >= 0.f) ? 0.f : (s > 1048576.f ? 1048576.f : s);  q_e = 1 + (uint32)s
 *     wmax == 0.f: q = 1 for every lamp.  total = the sum of q (uint64);  C = the inclusive prefix sum of q over e (uint64)
 *   The tables are built on the device on the first call that needs them, kept on the handle and dropped by
 *   rtmi_scene_set_emitters.  rtmi_scene_get_emitter_sampler copies them back, building them if need be (every pointer but
 *   nlamps_out may be NULL): q (L uint32), C (L uint64), the lamp number of every triangle (ntris uint32, 0 = not a lamp), the
 *   records (L * 20 floats: (c0, A), (e1, w), (e2, 0), (n_e, 0), (r, g, b, 0)), total and L.  *nlamps_out = 0: no lamps.
 *
 * pe(e, x2, dir) = ((((float)q_e / (float)total) / A) * x2) / fabsf(vdot(n_e, dir)): the density per solid angle of the point where
 *   a ray along dir meets lamp e, x2 the squared distance to it.
 * pb(n, d, s): rtmi_render_envlight*'s, the pdf per solid angle of the Matte bounce.
 *
 * The pass.  Contract: rtmi_render_samples[_device]'s in every respect, as rtmi_render_shadowed* states it.  The rays of every pass
 * are exactly those of rtmi_render_samples_device for the same arguments: no ray, no RNG block 0 .. maxdepth and no plain "Rays"
 * count moves.  At the hit of a path's ray number j, when the hit is a Matte surface (neither a miss nor an edge face) and the path
 * bounces (maxdepth - j - 1 != 0: an exhausted level gets no sample):
 *     point = rd * t + ro;  n = the triangle's norm, * (-1.f) when face & 1
 *     w = RNG block 0xC0040000 | j of (seed, pixel, sample)   (distinct from every block of rtmi_render_lit*, rtmi_render_rays_lit*
 *         and rtmi_bake_lit* under one key: those are 0xC0000000 | l << 16 | level with l <= 3)
 *     T = the upper 64 bits of ((uint64)w0 << 32 | w1) * total;  lamp e: the first e with C[e] > T
 *     a = u(w2);  b = u(w3);  if a + b > 1.f: a = 1.f - a, b = 1.f - b;  y = (c0 + e1 * a) + e2 * b
 *     dv = y - point;  d2 = vdot(dv, dv);  omega = vunit(dv);  cos = vdot(n, omega);  s = omega * (2.f * cos) - n
 *     o = point + s * 0.001f                      (where the bounce along omega starts: the shadow ray sees what it would)
 *     live when cos > 0.f and fabsf(vdot(n_e, omega)) > 0.f and some lane 0..2 of the radiance != 0.f
 *     the shadow ray (o, omega) is traced by the scene's closest-hit definition (rtmi_trace's); it counts when its first hit is
 *     lamp e itself on a non-edge face (tri == the lamp's triangle, !(face & 2)), at time ts:
 *       pbv = pb(n, omega, s);  pe' = pe(e, ts * ts, omega);  pet = pe(e, d2, omega);  wB = pe' / (pbv + pe')
 *       direct_j = radiance * ((pbv / pet) * wB);  otherwise direct_j = (0, 0, 0)
 *   and with nr the bounce ray (lambertian_ray with rv = random_vec of block j + 1): wp = pb(n, nr.dir, rv).
 *   A Reflective level has direct_j = 0 and wp = "no sample"; so has the primary ray (wp) and an exhausted level (direct_j).
 * Colour: a ray number j >= 1 whose hit is a lamp's non-edge face, with wp >= 0.f from the level before: the lamp's colour *
 *   (wp / (wp + pe(e, t * t, rd))), e and t from the hit.  Every other Solid end (a primary ray's, a mirror's, a Solid triangle
 *   that is no lamp), edge faces, misses (the sky constant, or the environment's plain lookup) and the black of exhausted depth as
 *   in color_ray.  The fold is c = mix_color(color_j, c + direct_j, alpha_j), inside-out over the path's Matte / Reflective levels.
 *   Both strategies evaluate pe from the hit record of their own ray by the same statements, so their weights sum to one for one
 *   ray.  (Occlusion, the edge band and lamps behind lamps need no limit and no epsilon: a candidate is paid exactly where the
 *   bounce ray along omega would have been.)  No case is special: non-finite values propagate as the arithmetic gives them.
 * Scenes: octree, linear list, generic tree and RTMI_OPT_GENERIC; with or without an environment.  RTMI_ERR_UNSUPPORTED, before
 *   any HIP call, stats cleared: a scene without lamps; with analytic spheres, a dielectric, vertex normals, textures or normal
 *   maps; RTMI_OPT_BVH (a non-exact first hit would break the "first hit is lamp e" test).  The handle stays usable.
 *   RTMI_OPT_FAST is taken and gives that mode's hits: path rays and shadow rays go through the same trace, so "first hit is
 *   lamp e" is decided on the hits the paths see (the frame is this definition on rtmi_trace's hits under the same option).
 * RTMI_ERR_INVALID, before any HIP call and before the scene is used, stats cleared: every check of rtmi_render_samples[_device].
 * stats: as rtmi_render_shadowed* fills them: rays = the plain rays + the live shadow rays, trace_launches = 2 per pass and batch
 *   (an empty event pair at the exhausted pass), primary_ms the path rays' closest-hit launches, bounce_ms the shadow rays'.
 * How: rtmi_render_envlight*'s pass structure: k_emissive_rays, the scene's closest-hit launch of the shadow queue into hit records
 *   of its own, k_shade_emissive per pass; beside the plain workspace 64 B per path (queue, weights, slot, hit records, wp; 4 B more on an octree) and 16 B
 *   per path and level (the direct stack), allocated by this call only.
 * Not here: lamps on smooth, textured, normal-mapped or glass scenes; Matte or textured emitters; more than one sample per hit; box
 *   lights or the environment's sampling in the same pass; explicit rays, bakes, adaptive variants, view batches and denoised
 *   wrappers; the path kernels (pipeline 3). */
int rtmi_scene_set_emitters(rtmi_scene_t* scene, const float* corners9, const uint8_t* emit_of_tri /* n bytes, or NULL: clear */,
                            uint64_t n);
int rtmi_scene_get_emitter_sampler(rtmi_scene_t* scene, uint32_t* q_out, uint64_t* cum_out, uint32_t* lamp_of_tri_out,
                                   float* lamps_out, uint64_t* total_out, uint32_t* nlamps_out);
int rtmi_render_emissive_device(rtmi_scene_t* scene, const rtmi_viewport_t* vp, uint64_t seed, const rtmi_tile_t* tile,
                                uint32_t sample0, uint32_t nsamples, void* accum_device, void* out_device /* or NULL */,
                                void* hip_stream, rtmi_stats_t* stats);
int rtmi_render_emissive(rtmi_scene_t* scene, const rtmi_viewport_t* vp, uint64_t seed, uint32_t row0, uint32_t nrows,
                         uint32_t sample0, uint32_t nsamples, float* accum_host, float* out_host /* or NULL */,
                         rtmi_stats_t* stats);

/* A shaded preview in one call: albedo, ambient occlusion and up to four coloured box lights composed PER
 * SAMPLE on the device, from one primary pass per batch and one any-hit walk of the AO rays and every light's live shadow
 * rays together.  The per-pixel buffers of rtmi_render_features*, rtmi_render_ao* and rtmi_render_light* are means over a
 * pixel's samples, and a product of means is not the mean of the products: a pixel half on a surface and half on the sky
 * would light its sky half.  The composition therefore needs the per-sample terms, which exist on the device only.
 * Build-defined like those three calls: what follows IS the definition, and tests/preview_ref.py pins it bit for bit.  All
 * arithmetic is f32, no contraction.
 * Primary rays, (tri, t, face), n and point: exactly those of rtmi_render_features_device for the same (vp, seed, tile,
 * sample0, nsamples); vp->maxdepth is not consulted.
 * AO rays of a sample that hit: exactly rtmi_render_ao*'s for preview->ao (RNG blocks 0x80000000 | k), Ka = ao.rays of them.
 * Candidates of light l: exactly rtmi_render_light*'s for preview->lights[l] (RNG blocks 0xC0000000 | k), K_l = lights[l].rays
 * of them.  The blocks are the same for every light: the lights' jitter is correlated, so that every layer equals its own
 * single call.
 * Per sample s of pixel p, with a = the features call's per-sample albedo (the sky's colour on a miss, 0 on an edge face):
 *   a miss:  e = a (the sky, unlit);
 *   a hit, edge faces included:
 *     f   = (float)v * (1.f / (float)Ka), v = the number of the sample's Ka AO rays that are visible; f = 1.f when Ka == 0;
 *     g_l = acc * (1.f / (float)K_l), acc = 0.f, then acc = acc + c for the live and visible candidates of light l in k order;
 *     per channel c:  L = ambient[c] * f;  for l = 0 .. nlights-1:  L = L + light_color[l][c] * g_l  (a multiplication, then
 *                     an addition);  e[c] = a[c] * L.
 *   No case is special: non-finite values propagate as the arithmetic gives them.
 * Per pixel: acc = 0.f, then acc = acc + e_s in sample order; color = acc * (1.f / (float)nsamples), lane 3 = 0.
 * Layers (rtmi_preview_out_t; any may be NULL, not all, and no two may overlap as byte ranges): each equals, bit for bit, what
 * the single call returns for the same parameters on the same handle: albedo / normal / ids are rtmi_render_features_device's
 * three buffers, ao is rtmi_render_ao_device's plane for preview->ao, plane l of shadow / irradiance (at l * tile pixels) is
 * rtmi_render_light_device's for lights[l].  color with albedo and normal feeds rtmi_denoise_device directly.
 * Scenes: as rtmi_render_ao* and rtmi_render_light*.  RTMI_ERR_UNSUPPORTED for a scene with analytic spheres and for
 * nsamples * Ka or any nsamples * K_l >= 2^24.
 * RTMI_ERR_INVALID, before any HIP call and before the scene is used, stats cleared: a NULL scene, viewport, tile, preview or
 * out; all outputs NULL, or two that overlap; nlights > RTMI_PREVIEW_MAX_LIGHTS; non-zero flags; a non-finite ambient or used
 * light colour; every parameter check of rtmi_render_ao* on `ao` except that rays == 0 is allowed (no AO rays, f = 1.f);
 * every parameter check of rtmi_render_light* on each used light (the message names the light's index); out->ao with ao.rays
 * == 0; out->shadow or out->irradiance with nlights == 0; nsamples == 0; sample0 + nsamples > S; every viewport and tile check
 * of the features call.  An empty tile returns RTMI_OK and touches nothing.  ao.rays == 0 && nlights == 0 is valid: a flat
 * albedo preview, and no walk is launched.
 * stats: rays = pixels * nsamples + (samples that hit) * Ka + the live rays of every light; pipeline = 1; primary_ms = the
 * primary closest-hit launches, bounce_ms = the shared walk, trace_ms their sum; trace_launches = 2 per batch, 1 per batch
 * without secondary rays.  With RTMI_OPT_COUNTERS the counters are the primaries' work plus the walk's actual work.
 * How: per batch, on one library stream: the features call's primary pass (and k_features when albedo, normal or ids are
 * asked for); k_preview_rays stages a block's hit paths once and writes their Ka AO rays and every light's live candidates
 * into ONE queue whose counter is the walk's ray count (it never leaves the device; one limit array: AO rays store radius,
 * bounded lights r, unbounded lights +inf, which rtmi_occluded's rule treats as the NULL limit), and each path's albedo; one
 * any-hit walk (or the closest-hit launch, where rtmi_occluded uses that); k_preview_resolve folds per pixel in the defined
 * order.  A path counts as Ka + the sum of K_l queue entries: a batch's entries stay within batch_paths.  The queue lives on
 * the handle, grows on demand and is freed by rtmi_scene_destroy.  No tuning changes a bit of the result.
 * Not here: previews of batches of views and of rtmi_render_frame_multi, sums continued across calls, importance sampling,
 * shadow rays inside color_ray (rtmi_render_shadowed*, above), a denoised-preview one-call wrapper. */
enum { RTMI_PREVIEW_MAX_LIGHTS = 4 };
typedef struct rtmi_preview {
    float ambient[3];          /* offset 0                                                  */
    uint32_t nlights;          /* 12: 0..RTMI_PREVIEW_MAX_LIGHTS                            */
    uint32_t flags;            /* 16: must be 0                                             */
    rtmi_ao_t ao;              /* 20: ao.rays == 0 is valid here: no AO rays, factor 1.f    */
    rtmi_light_t lights[4];    /* 36: entries >= nlights are ignored                        */
    float light_color[4][3];   /* 148                                                       */
} rtmi_preview_t;              /* 196 bytes */
typedef struct rtmi_preview_out {   /* any may be NULL, not all; no two may overlap as byte ranges */
    void* color;       /* float4 per pixel of the tile: rgb, lane 3 = 0 (what rtmi_render_device writes) */
    void* albedo;      /* float4  } exactly rtmi_render_features_device's three buffers                   */
    void* normal;      /* float4  }                                                                        */
    void* ids;         /* uint32  }                                                                        */
    void* ao;          /* f32 per pixel: exactly rtmi_render_ao_device's plane for preview->ao             */
    void* shadow;      /* nlights planes of f32, plane l at l * (tile pixels): rtmi_render_light_device's  */
    void* irradiance;  /* likewise                                         shadow / irradiance for lights[l] */
} rtmi_preview_out_t;
void rtmi_preview_defaults(rtmi_preview_t* preview);  /* ambient 0.3, nlights 0, flags 0, rtmi_ao_defaults, rtmi_light_defaults x 4, colours 1 */
int rtmi_render_preview_device(rtmi_scene_t* scene, const rtmi_viewport_t* vp, uint64_t seed, const rtmi_tile_t* tile,
                               uint32_t sample0, uint32_t nsamples, const rtmi_preview_t* preview,
                               const rtmi_preview_out_t* out_device, void* hip_stream, rtmi_stats_t* stats);
int rtmi_render_preview(rtmi_scene_t* scene, const rtmi_viewport_t* vp, uint64_t seed, uint32_t row0, uint32_t nrows,
                        uint32_t sample0, uint32_t nsamples, const rtmi_preview_t* preview, const rtmi_preview_out_t* out_host,
                        rtmi_stats_t* stats);

/* Per-ray debug records (the reference's Scene { debug_ctx, debug_en }, raytrace.rs:1297-1303, debug.rs): what the
 * octree walk did for each ray, taken from the production walk itself (k_trace_record: the walk of rtmi_trace in a
 * recording mode).  A leaf is named by its index in the `boxes` array rtmi_scene_create received (Scene.tree()'s
 * numbering); the leaves of a ray are listed in visiting order, a leaf entered twice twice, so their triangle lists
 * are the reference's `check_tris` and their sizes sum to the ray's tri_tests. */
typedef struct rtmi_ray_record {
    float orig[4], dir[4];   /* the ray as make_ray stores it (primary records: exactly what the renderer traces) */
    uint32_t tri;            /* closest hit, 0 = miss (then t = 0, face = 0)                                      */
    float t;
    uint32_t face;           /* 0 front, 1 back, 2 edge front, 3 edge back (as rtmi_trace)                        */
    uint32_t nleaves;        /* leaves visited = the reference's `leaves` counter for this ray                    */
    uint64_t leaf_first;     /* offset of this ray's leaf list in leaf_ids                                        */
    uint32_t box_tests, tri_tests, full_tests, nodes;  /* this ray's counters (its share of rtmi_stats_t)      */
} rtmi_ray_record_t;

/* rtmi_trace with a record per ray (recs: n entries).  Host buffers: these are diagnostics.  *leaf_total always receives
 * the number of leaf ids of the call.  leaf_ids == NULL: records and total only (a size query); otherwise leaf_ids
 * receives them (ray i's at recs[i].leaf_first), and leaf_cap < total is RTMI_ERR_INVALID with nothing written to
 * leaf_ids and the size needed in the message.  stats: rays = n, the five work counters (the sums over the records)
 * and kernel_ms.  RTMI_ERR_UNSUPPORTED for scenes k_trace_oct does not run (trivial one-leaf tree, generic tree,
 * RTMI_OPT_GENERIC), for RTMI_OPT_BVH and RTMI_OPT_FAST, and for scenes with analytic spheres. */
int rtmi_trace_records(rtmi_scene_t* scene, uint64_t n, const float* orig4, const float* dir4,
                       rtmi_ray_record_t* recs, uint32_t* leaf_ids, uint64_t leaf_cap, uint64_t* leaf_total,
                       rtmi_stats_t* stats);
/* The same for the primary rays of sample `sample` of every pixel of rows [row0, row0+nrows): record i is pixel
 * (row0 + i / width, i % width), its ray generated by the renderer's own ray generation, so its bits equal the
 * renderer's.  vp->maxdepth is not consulted (the record describes the primary ray's trace).  sample >= spp and rows
 * outside the frame are RTMI_ERR_INVALID. */
int rtmi_primary_records(rtmi_scene_t* scene, const rtmi_viewport_t* vp, uint64_t seed, uint32_t row0, uint32_t nrows,
                         uint32_t sample, rtmi_ray_record_t* recs, uint32_t* leaf_ids, uint64_t leaf_cap,
                         uint64_t* leaf_total, rtmi_stats_t* stats);

/* (c * 255.) as u8 per channel, RGB (raytrace.rs:1468-1473). */
int rtmi_quantize(rtmi_scene_t* scene, const float* rgba_host, uint64_t npixels, uint8_t* rgb_host);
/* Same on device memory, enqueued on `hip_stream`: lets a rank hand 3 bytes per pixel to the gather instead of 16. */
int rtmi_quantize_device(rtmi_scene_t* scene, const void* rgba_device, uint64_t npixels, void* rgb_device, void* hip_stream);

/* `make_triangle` (raytrace.rs:340-383) for n triangles on the GPU: corners (9 floats each) -> the geometric fields
 * of rtmi_triangle_t (incenter, norm, bounding_r2, sides, side_lens); edge_thickness and the surface fields are copied
 * from `proto`.  Bit-identical to the host computation.  Fails with RTMI_ERR_INVALID, naming the first offender, where
 * the reference panics on a degenerate triangle (unwrap at raytrace.rs:357). */
int rtmi_make_triangles(int device, const float* corners9_host, uint64_t n, const rtmi_triangle_t* proto,
                        rtmi_triangle_t* out_host);

/* Octree build on the GPU (raytrace.rs:753-845).  The builder's whole cost is box_contains_polygon (raytrace.rs:753-779)
 * on every (candidate child box, triangle of the parent's list) pair; rtmi_builder_filter evaluates it for all pairs of
 * one tree level, bit-identical to the host computation, so the resulting tree equals the reference builder's.  The
 * caller keeps the list bookkeeping (which is linear): see build_bounding_box_gpu in csrc/host/raytrace.cpp.
 * tris15: ntris x 15 floats (incenter, norm, corner 0, corner 1, corner 2), kept on the device by the handle.
 * boxes[b]: geometry + the range [cand_first, cand_first + cand_count) of `cand` (triangle indices) to test against it;
 * keep[keep_first + j] receives 1 when box b contains candidate j, else 0; flags outside every box's range are left as
 * they were.  Ranges of different boxes may overlap in `cand` (the 8 children of a box share their parent's list) but not
 * in `keep`.  Errors (RTMI_ERR_INVALID, nothing launched, `keep` untouched): a NULL builder; NULL boxes / cand / keep with
 * nboxes and nkeep non-zero; a candidate index >= ntris; a box whose range leaves `cand` or `keep`.  rtmi_builder_create:
 * RTMI_ERR_INVALID for ntris == 0, NULL tris15 / out, or a device index outside [0, rtmi_device_count()).
 * rtmi_builder_destroy(NULL) is RTMI_OK. */
typedef struct rtmi_build_box {
    float orig[3];
    float len2;
    uint32_t cand_first, cand_count;
    uint64_t keep_first;
} rtmi_build_box_t;
typedef struct rtmi_builder rtmi_builder_t;
int rtmi_builder_create(int device, const float* tris15, uint64_t ntris, rtmi_builder_t** out);
int rtmi_builder_filter(rtmi_builder_t* builder, const rtmi_build_box_t* boxes, uint64_t nboxes, const uint32_t* cand,
                        uint64_t ncand, uint8_t* keep, uint64_t nkeep);
int rtmi_builder_destroy(rtmi_builder_t* builder);

/* Message of the last error on the calling thread ("" if none). */
const char* rtmi_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* RTMI_H */
