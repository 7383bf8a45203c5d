/* rtmi_host.h — C view of the host-side mirror of the reference's scene API
 * (rust_raytrace_amd/csrc/host/raytrace.hpp) for language bindings (ctypes).
 *
 * This is NOT part of the drop-in boundary: in a real integration everything
 * declared here stays in the Rust `raytrace_lib` crate (make_triangle,
 * make_disk, parse_obj, build_bounding_box, create_viewport, the RayCaster
 * trait) and only include/rtmi.h is bound.  It exists because this image has
 * no Rust toolchain; the C++ mirror keeps the reference's names and semantics
 * so that tests read like the reference's own call sites (raytrace/src/main.rs).
 *
 * Functions returning int return 0 on success; the message of a failure (the
 * places where the reference panics) is read with rth_last_error().
 */
#ifndef RTMI_HOST_H
#define RTMI_HOST_H
#include <stdint.h>
#include "rtmi.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct rth_scene rth_scene_t; /* raytrace::Scene + a HipRayCaster bound to it */

const char* rth_last_error(void);

/* raytrace.rs:176-180, :93-96, f32::to_radians, :1320-1341, :1343-1370 */
void rth_make_color(uint8_t r, uint8_t g, uint8_t b, float* out3);
void rth_unit(const float* in3, float* out3);
float rth_to_radians(float deg);
void rth_create_transform(const float* dir3, float d_roll, float* out9);
void rth_create_viewport(uint32_t w, uint32_t h, float size0, float size1, const float* pos3, const float* dir3,
                         float fov, float c_roll, float* out12 /* orig cam vu vv */);

rth_scene_t* rth_scene_new(int with_dummy /* push make_dummy_triangle() first, main.rs:117 */);
void rth_scene_free(rth_scene_t* s);
uint64_t rth_num_tris(const rth_scene_t* s);

/* make_triangle / parse_obj / make_disk / make_sphere appended to Scene.tris */
int rth_add_triangle(rth_scene_t* s, const float* pts9, uint32_t kind, const float* color3, float alpha, float scattering, float edge);
int rth_add_obj(rth_scene_t* s, const char* path, const float* offset3, float scale, const float* basis9,
                uint32_t kind, const float* color3, float alpha, float scattering, float edge);
/* The same with robust != 0: opt-in loader extension (fan-triangulated polygons, negative indices, degenerate
 * triangles skipped).  robust == 0 is the reference's loader (first three corners, obj_parser.rs:63-65). */
int rth_add_obj_mode(rth_scene_t* s, const char* path, const float* offset3, float scale, const float* basis9, uint32_t kind,
                     const float* color3, float alpha, float scattering, float edge_thickness, uint32_t robust);
int rth_add_disk(rth_scene_t* s, const float* orig3, const float* norm3, float r, float d, uint64_t num_tris,
                 uint32_t kind, const float* color3, float alpha, float scattering,
                 uint32_t side_kind, const float* side_color3, float side_alpha, float side_scattering, float edge);
int rth_add_sphere(rth_scene_t* s, const float* orig3, float r, uint64_t num_lat, uint64_t num_lon,
                   uint32_t kind, const float* color3, float alpha, float scattering, float edge);
/* n triangles at once through the GPU make_triangle kernel (rtmi_make_triangles) */
int rth_add_triangles_gpu(rth_scene_t* s, const float* pts9, uint64_t n, uint32_t kind, const float* color3, float alpha,
                          float scattering, float edge, int device);
/* analytic sphere: a build-defined extension (rtmi_sphere_t in rtmi.h), not a reference API */
int rth_add_analytic_sphere(rth_scene_t* s, const float* center3, float radius, uint32_t kind, const float* color3, float alpha,
                            float scattering);
/* The environment of the scene (rtmi_scene_set_environment / rtmi_scene_set_sky in rtmi.h, which defines it): kept with the
 * scene and applied to its resident copy on every device at the next call that uses one; the scene is not uploaded again.
 * rgb == NULL or n == 0 removes it; frame9 == NULL is the identity; sky == NULL the defaults.  Refusals as in rtmi.h.
 * rth_scene_environment_size: n of what was set, 0 for none.  rth_caster_environment uploads if need be and reads the device's
 * table back (n * n * 3 floats, at most cap_floats). */
int rth_scene_set_environment(rth_scene_t* s, const float* rgb, uint32_t n, const float* frame9);
int rth_scene_set_sky(rth_scene_t* s, uint32_t n, const rtmi_sky_t* sky);
int rth_scene_environment_size(const rth_scene_t* s, uint32_t* n_out);
int rth_caster_environment(rth_scene_t* s, float* rgb_out, uint64_t cap_floats, uint32_t* n_out);
/* Vertex normals (rtmi_scene_set_normals / rtmi_smooth_normals in rtmi.h, which defines them): kept with the scene, 9 floats per
 * triangle, and applied with the triangles' own corners to its resident copy on every device at the next call that uses one; the
 * scene is not uploaded again.  Triangles that were never given normals, those appended later among them, are flat (zeros).
 * rth_scene_set_normals: normals of triangles [first, first + count), first >= 1; normals9 == NULL removes all of them.
 * rth_scene_smooth_normals: generated from the shared corner positions of that range alone (count = UINT64_MAX: to the end).
 * rth_scene_normals_size: the number of triangles when the scene has normals, else 0.  rth_scene_get_normals: the scene's copy,
 * ntris * 9 floats; rth_caster_normals uploads if need be and reads the device's table back.
 * rth_add_obj_normals: rth_add_obj_mode, then normals for the new triangles: 0 none, 1 the file's `vn` (each through the
 * transform and unit(); a corner without a normal index is an error), 2 generated with crease_cos. */
int rth_scene_set_normals(rth_scene_t* s, const float* normals9, uint64_t first, uint64_t count);
int rth_scene_smooth_normals(rth_scene_t* s, uint64_t first, uint64_t count, float crease_cos);
int rth_scene_normals_size(const rth_scene_t* s, uint64_t* n_out);
int rth_scene_get_normals(const rth_scene_t* s, float* normals9_out, uint64_t cap_floats);
int rth_caster_normals(rth_scene_t* s, float* normals9_out, uint64_t cap_floats, uint64_t* n_out);
int rth_add_obj_normals(rth_scene_t* s, const char* path, const float* offset3, float scale, const float* basis9, uint32_t kind,
                        const float* color3, float alpha, float scattering, float edge_thickness, uint32_t robust, uint32_t normals,
                        float crease_cos);
/* Textures (rtmi_scene_set_textures / rtmi_project_uvs in rtmi.h, which defines them): kept with the scene and applied with the
 * triangles' own corners to its resident copy on every device at the next call that uses one; the scene is not uploaded again.
 * Triangles that were never given uvs, those appended later among them, are untextured.
 * rth_scene_set_textures: the images (copied); tex == NULL or ntex == 0 removes the images, the uvs and the texture numbers.
 * rth_scene_set_uvs: uvs (6 floats) and texture numbers of triangles [first, first + count), first >= 1.
 * rth_scene_project_uvs: rtmi_project_uvs over that range (count = UINT64_MAX: to the end), which gets texture number `texture`.
 * rth_scene_textures_size: the number of images, and the number of triangles when the scene has images or uvs, else 0.
 * rth_scene_get_uvs / rth_scene_get_texture: the scene's copy; rth_caster_uvs / rth_caster_texture upload if need be and read the
 * device's tables back (k = 1..ntex; rgb_out = NULL in rth_scene_get_texture: the size alone).
 * rth_add_obj_uvs: rth_add_obj_mode, then the file's `vt` coordinates for the new triangles (the second field of every a/b or a/b/c
 * corner; a corner without one is an error), which get texture number `texture`. */
int rth_scene_set_textures(rth_scene_t* s, const rtmi_texture_t* tex, uint32_t ntex);
int rth_scene_set_uvs(rth_scene_t* s, const float* uvs6, const uint32_t* tex_of_tri, uint64_t first, uint64_t count);
int rth_scene_project_uvs(rth_scene_t* s, uint64_t first, uint64_t count, const float* lo3, float scale, uint32_t texture);
int rth_scene_textures_size(const rth_scene_t* s, uint32_t* ntex_out, uint64_t* n_out);
int rth_scene_get_uvs(const rth_scene_t* s, float* uvs6_out, uint32_t* tex_of_tri_out, uint64_t cap_tris);
int rth_scene_get_texture(const rth_scene_t* s, uint32_t k, float* rgb_out, uint64_t cap_floats, uint32_t* w_out, uint32_t* h_out);
int rth_caster_uvs(rth_scene_t* s, float* uvs6_out, uint32_t* tex_of_tri_out, uint64_t cap_tris, uint64_t* n_out);
int rth_caster_texture(rth_scene_t* s, uint32_t k, float* rgb_out, uint64_t cap_floats, uint32_t* w_out, uint32_t* h_out);
int rth_add_obj_uvs(rth_scene_t* s, const char* path, const float* offset3, float scale, const float* basis9, uint32_t kind,
                    const float* color3, float alpha, float scattering, float edge_thickness, uint32_t robust, uint32_t texture);
/* Normal maps (rtmi_scene_set_normal_maps in rtmi.h, which defines them): kept with the scene and applied, after the textures and
 * with the triangles' own corners, to its resident copy on every device at the next call that uses one.  A map is one of the
 * scene's texture images, so the scene needs images first, and rth_scene_set_textures (set or remove) removes the maps.
 * rth_scene_set_normal_maps: map numbers of triangles [first, first + count), first >= 1 (count = UINT64_MAX: to the end), and
 * the strength of all maps; nmap_of_tri == NULL or count == 0 removes the maps.  Refused: no images, flags != 0, a strength that
 * is not finite, a number above the number of images.
 * rth_scene_normal_maps_size: the number of triangles when the scene has maps, else 0.  rth_scene_get_normal_maps: the scene's
 * copy.  rth_scene_normal_map_frames: rtmi_normal_map_frames over the scene (4 floats per triangle, entry 0 zeros): what a device
 * stores.  rth_caster_normal_maps uploads if need be and reads the device's numbers back (a degenerate triangle reads as 0).
 * rth_normal_map_from_height: rtmi_normal_map_from_height. */
int rth_scene_set_normal_maps(rth_scene_t* s, const uint32_t* nmap_of_tri, uint64_t first, uint64_t count, float strength, uint32_t flags);
int rth_scene_normal_maps_size(const rth_scene_t* s, uint64_t* n_out);
int rth_scene_get_normal_maps(const rth_scene_t* s, uint32_t* nmap_of_tri_out, float* strength_out, uint64_t cap_tris);
int rth_scene_normal_map_frames(const rth_scene_t* s, float* frames4_out, uint64_t cap_tris);
int rth_caster_normal_maps(rth_scene_t* s, uint32_t* nmap_of_tri_out, float* strength_out, uint64_t cap_tris, uint64_t* n_out);
int rth_normal_map_from_height(const float* height, uint32_t w, uint32_t h, float scale, float* rgb_out);
void rth_populate_triangle_numbers(rth_scene_t* s);

/* build_bounding_box / build_trivial_bounding_box into Scene.boxes */
int rth_build_bounding_box(rth_scene_t* s, const float* orig3, float len2, uint64_t maxdepth, uint64_t minobjs, uint32_t threads);
/* The same tree with every level's box/triangle overlap tests on the GPU (rtmi_builder_*); bit-equal to the host build. */
int rth_build_bounding_box_gpu(rth_scene_t* s, const float* orig3, float len2, uint64_t maxdepth, uint64_t minobjs, int device);
int rth_build_trivial_bounding_box(rth_scene_t* s, const float* orig3, float len2);
int rth_box_contains_polygon(const rth_scene_t* s, const float* orig3, float len2, uint64_t tri);
int rth_face_contains_triangle(const rth_scene_t* s, const float* p3, const float* norm3, float len2, uint64_t tri);

/* inspection: 29 floats per triangle (incenter3 norm3 r2 sides9 side_lens3 edge corners9), kind, (color3 alpha scattering) */
void rth_get_triangles(const rth_scene_t* s, float* rec29, int32_t* kinds, float* surf5);
void rth_tree_sizes(const rth_scene_t* s, uint64_t* nboxes, uint64_t* nrefs);
void rth_tree_get(const rth_scene_t* s, float* geo4, uint32_t* topo4 /* first count is_leaf depth */, uint32_t* refs);

/* HipRayCaster (implements RayCaster, raytrace.rs:1128-1165) */
int rth_caster_config(rth_scene_t* s, uint64_t seed, int device, uint32_t rtmi_options);
int rth_caster_walk_rows(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp,
                         uint64_t row0, uint64_t nrows, float* out_host, rtmi_stats_t* stats, double* wall_seconds);
int rth_caster_walk_rows_device(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp,
                                uint64_t row0, uint64_t nrows, void* out_device, void* hip_stream, rtmi_stats_t* stats,
                                double* wall_seconds);
int rth_caster_walk_tile_device(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp,
                                const rtmi_tile_t* tile, void* out_device, void* hip_stream, rtmi_stats_t* stats,
                                double* wall_seconds);
/* Progressive rendering (rtmi_render_samples / rtmi_render_samples_device in rtmi.h): samples [sample0, sample0 + nsamples)
 * of the frame's spp, continuing the running per-pixel sums in accum; out (may be NULL) receives the preview. */
int rth_caster_walk_samples(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp,
                            uint64_t row0, uint64_t nrows, uint32_t sample0, uint32_t nsamples, float* accum_host, float* out_host,
                            rtmi_stats_t* stats, double* wall_seconds);
int rth_caster_walk_samples_device(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp,
                                   const rtmi_tile_t* tile, uint32_t sample0, uint32_t nsamples, void* accum_device,
                                   void* out_device, void* hip_stream, rtmi_stats_t* stats, double* wall_seconds);
/* First-hit feature buffers (rtmi_render_features / rtmi_render_features_device in rtmi.h): per-pixel means over samples
 * [sample0, sample0 + nsamples) of the primary rays' (albedo.rgb, coverage) and (normal.xyz, depth), and the hit id of sample
 * sample0; any of the three buffers may be NULL, not all.  maxdepth is not consulted. */
int rth_caster_walk_features(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp,
                             uint64_t row0, uint64_t nrows, uint32_t sample0, uint32_t nsamples, float* albedo_host,
                             float* normal_host, uint32_t* ids_host, rtmi_stats_t* stats, double* wall_seconds);
int rth_caster_walk_features_device(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp,
                                    const rtmi_tile_t* tile, uint32_t sample0, uint32_t nsamples, void* albedo_device,
                                    void* normal_device, void* ids_device, void* hip_stream, rtmi_stats_t* stats,
                                    double* wall_seconds);
/* Adaptive sampling (rtmi_render_adaptive / rtmi_render_adaptive_device in rtmi.h): spp is the maximum samples per pixel;
 * ad carries min_samples, pass_samples and the tolerances in and passes, unconverged and samples out.  out receives every
 * pixel at its own count, counts the per-pixel sample counts. */
int rth_caster_walk_adaptive(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp,
                             uint64_t row0, uint64_t nrows, rtmi_adaptive_t* ad, float* out_host, uint32_t* counts_host,
                             rtmi_stats_t* stats, double* wall_seconds);
int rth_caster_walk_adaptive_device(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp,
                                    const rtmi_tile_t* tile, rtmi_adaptive_t* ad, void* accum_device, void* sumsq_device,
                                    void* counts_device, void* out_device, void* hip_stream, rtmi_stats_t* stats,
                                    double* wall_seconds);
/* A batch of views (rtmi_render_views / rtmi_render_views_device in rtmi.h): nviews viewports of one size, maxdepth and spp,
 * vp12s = 12 floats per view; seeds (nviews entries, or NULL: the caster's seed for every view).  out receives the stacked
 * image, nviews * h rows (row k * h + r = row r of view k); the device variant renders `tile` of it. */
int rth_caster_walk_views(rth_scene_t* s, uint32_t nviews, uint32_t w, uint32_t h, const float* vp12s, uint64_t maxdepth, uint64_t spp,
                          const uint64_t* seeds, float* out_host, rtmi_stats_t* stats, double* wall_seconds);
int rth_caster_walk_views_device(rth_scene_t* s, uint32_t nviews, uint32_t w, uint32_t h, const float* vp12s, uint64_t maxdepth,
                                 uint64_t spp, const uint64_t* seeds, const rtmi_tile_t* tile, void* out_device, void* hip_stream,
                                 rtmi_stats_t* stats, double* wall_seconds);
int rth_caster_trace(rth_scene_t* s, uint64_t n, const float* orig4, const float* dir4, uint32_t* tri, float* t,
                     uint32_t* face, rtmi_stats_t* stats);
/* Any-hit occlusion (rtmi_occluded* in rtmi.h, which defines it) on the scene's resident copy: one byte per ray, 1 iff the
 * ray's closest hit lies before tmax (NULL: +inf for every ray). */
int rth_caster_occluded(rth_scene_t* s, uint64_t n, const float* orig4, const float* dir4, const float* tmax, uint8_t* occluded,
                        rtmi_stats_t* stats);
int rth_caster_occluded_device(rth_scene_t* s, uint64_t n, const void* orig4_device, const void* dir4_device,
                               const void* tmax_device, void* occluded_device, void* hip_stream, rtmi_stats_t* stats);
/* rtmi_trace on device buffers (rtmi_trace_device in rtmi.h): the rays are read in place, tri / t / face written in place. */
int rth_caster_trace_device(rth_scene_t* s, uint64_t n, const void* orig4_device, const void* dir4_device, void* tri_device,
                            void* t_device, void* face_device, void* hip_stream, rtmi_stats_t* stats);
/* Path tracing of caller-supplied rays (rtmi_render_rays / rtmi_render_rays_device in rtmi.h, which defines it) on the scene's
 * resident copy, with the caster's seed.  keys: n x 2 uint32 (pixel, sample) or NULL. */
int rth_caster_walk_rays_explicit(rth_scene_t* s, uint64_t n, const float* orig4, const float* dir4, const uint32_t* keys,
                                  const rtmi_rays_t* rays, const rtmi_rays_out_t* out_host, rtmi_stats_t* stats,
                                  double* wall_seconds);
int rth_caster_walk_rays_explicit_device(rth_scene_t* s, uint64_t n, const void* orig4_device, const void* dir4_device,
                                         const void* keys_device, const rtmi_rays_t* rays, const rtmi_rays_out_t* out_device,
                                         void* hip_stream, rtmi_stats_t* stats, double* wall_seconds);
/* Light baked at M surface points or over M triangles (rtmi_bake / rtmi_bake_device in rtmi.h, which defines it) on the scene's
 * resident copy, with the caster's seed: bake->rays gather rays per element made on the device, path-traced and folded.
 * pos4: M float4 (RTMI_BAKE_POINTS) or 3 M float4, a triangle's corners (RTMI_BAKE_TRIANGLES); nrm4: M float4. */
int rth_caster_bake(rth_scene_t* s, uint64_t M, const float* pos4, const float* nrm4, const rtmi_bake_t* bake,
                    const rtmi_bake_out_t* out_host, rtmi_stats_t* stats, double* wall_seconds);
int rth_caster_bake_device(rth_scene_t* s, uint64_t M, const void* pos4_device, const void* nrm4_device, const rtmi_bake_t* bake,
                           const rtmi_bake_out_t* out_device, void* hip_stream, rtmi_stats_t* stats, double* wall_seconds);
/* Both with box lights (rtmi_render_rays_lit* / rtmi_bake_lit* in rtmi.h, which defines them): rth_caster_walk_rays_explicit* and
 * rth_caster_bake* in every respect, the lamps sampled at every Matte hit of every path and, for the bake, at the element itself
 * (out->direct); lit must not be NULL. */
int rth_caster_walk_rays_explicit_lit(rth_scene_t* s, uint64_t n, const float* orig4, const float* dir4, const uint32_t* keys,
                                      const rtmi_rays_t* rays, const rtmi_lit_t* lit, const rtmi_rays_out_t* out_host,
                                      rtmi_stats_t* stats, double* wall_seconds);
int rth_caster_walk_rays_explicit_lit_device(rth_scene_t* s, uint64_t n, const void* orig4_device, const void* dir4_device,
                                             const void* keys_device, const rtmi_rays_t* rays, const rtmi_lit_t* lit,
                                             const rtmi_rays_out_t* out_device, void* hip_stream, rtmi_stats_t* stats,
                                             double* wall_seconds);
int rth_caster_bake_lit(rth_scene_t* s, uint64_t M, const float* pos4, const float* nrm4, const rtmi_bake_t* bake,
                        const rtmi_lit_t* lit, const rtmi_bake_lit_out_t* out_host, rtmi_stats_t* stats, double* wall_seconds);
int rth_caster_bake_lit_device(rth_scene_t* s, uint64_t M, const void* pos4_device, const void* nrm4_device, const rtmi_bake_t* bake,
                               const rtmi_lit_t* lit, const rtmi_bake_lit_out_t* out_device, void* hip_stream, rtmi_stats_t* stats,
                               double* wall_seconds);
/* Ambient occlusion (rtmi_render_ao / rtmi_render_ao_device in rtmi.h, which defines it): one f32 per pixel, the share of
 * ao->rays hemisphere rays per primary sample of [sample0, sample0 + nsamples) that are not occluded within ao->radius.
 * maxdepth is not consulted; the primary rays use the caster's seed. */
int rth_caster_walk_ao(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp, uint64_t row0,
                       uint64_t nrows, uint32_t sample0, uint32_t nsamples, const rtmi_ao_t* ao, float* ao_host,
                       rtmi_stats_t* stats, double* wall_seconds);
int rth_caster_walk_ao_device(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp,
                              const rtmi_tile_t* tile, uint32_t sample0, uint32_t nsamples, const rtmi_ao_t* ao, void* ao_device,
                              void* hip_stream, rtmi_stats_t* stats, double* wall_seconds);
/* Direct light (rtmi_render_light / rtmi_render_light_device in rtmi.h, which defines it): two f32 per pixel, the share of
 * light->rays samples of the box light (the host mirror's LightSource { orig, len2 }, raytrace.rs:595-598) per primary sample
 * of [sample0, sample0 + nsamples) that are visible from the first hit, and the mean of n . dir over them.  Either plane may
 * be NULL.  maxdepth is not consulted; the primary rays use the caster's seed. */
int rth_caster_walk_light(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp, uint64_t row0,
                          uint64_t nrows, uint32_t sample0, uint32_t nsamples, const rtmi_light_t* light, float* shadow_host,
                          float* irradiance_host, rtmi_stats_t* stats, double* wall_seconds);
int rth_caster_walk_light_device(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp,
                                 const rtmi_tile_t* tile, uint32_t sample0, uint32_t nsamples, const rtmi_light_t* light,
                                 void* shadow_device, void* irradiance_device, void* hip_stream, rtmi_stats_t* stats,
                                 double* wall_seconds);
/* Path tracing with the reference's shadow rays switched on (rtmi_render_shadowed / rtmi_render_shadowed_device in rtmi.h,
 * which defines it): rth_caster_walk_samples[_device] in every respect, with every surface hit of every bounce tested against
 * `light`, which becomes the scene's light (the host mirror's Scene::light, the reference's commented-out field).
 * light->rays must be 1. */
int rth_caster_walk_shadowed(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp, uint64_t row0,
                             uint64_t nrows, uint32_t sample0, uint32_t nsamples, const rtmi_light_t* light, float* accum_host,
                             float* out_host, rtmi_stats_t* stats, double* wall_seconds);
int rth_caster_walk_shadowed_device(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp,
                                    const rtmi_tile_t* tile, uint32_t sample0, uint32_t nsamples, const rtmi_light_t* light,
                                    void* accum_device, void* out_device, void* hip_stream, rtmi_stats_t* stats,
                                    double* wall_seconds);
/* Path tracing with the environment sampled at matte hits (rtmi_render_envlight / rtmi_render_envlight_device in rtmi.h, which
 * defines it): rth_caster_walk_samples[_device] in every respect; env may be NULL (the defaults).  rth_caster_env_sampler uploads
 * if need be and reads the sampler table back (rtmi_scene_get_env_sampler): n * n weights, at most cap of them, q_out may be NULL. */
int rth_caster_walk_envlight(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp, uint64_t row0,
                             uint64_t nrows, uint32_t sample0, uint32_t nsamples, const rtmi_envlight_t* env, float* accum_host,
                             float* out_host, rtmi_stats_t* stats, double* wall_seconds);
int rth_caster_walk_envlight_device(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp,
                                    const rtmi_tile_t* tile, uint32_t sample0, uint32_t nsamples, const rtmi_envlight_t* env,
                                    void* accum_device, void* out_device, void* hip_stream, rtmi_stats_t* stats,
                                    double* wall_seconds);
int rth_caster_env_sampler(rth_scene_t* s, uint32_t* q_out, uint64_t cap, uint64_t* total_out, uint32_t* n_out);
/* Emissive triangles (rtmi_scene_set_emitters in rtmi.h, which defines them).  rth_scene_set_emitters marks triangles first,
 * first + 1, ... (count bytes, non-zero = a lamp; a marked triangle must be Solid); NULL or count 0 clears every mark.  Kept with
 * the scene: a caster applies the marks to every resident copy.  rth_scene_get_emitters: one byte per triangle of the scene.
 * rth_caster_walk_emissive[_device] (rtmi_render_emissive / rtmi_render_emissive_device): rth_caster_walk_samples[_device] in every
 * respect.  rth_caster_emitter_sampler uploads if need be and reads the lamps' tables back (rtmi_scene_get_emitter_sampler): at
 * most cap_lamps lamps and cap_tris triangles; with every output pointer NULL it returns the lamp count and the total alone. */
int rth_scene_set_emitters(rth_scene_t* s, const uint8_t* emit_of_tri, uint64_t first, uint64_t count);
int rth_scene_get_emitters(const rth_scene_t* s, uint8_t* emit_of_tri_out, uint64_t cap_tris);
int rth_caster_walk_emissive(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp, uint64_t row0,
                             uint64_t nrows, uint32_t sample0, uint32_t nsamples, float* accum_host, float* out_host, rtmi_stats_t* stats,
                             double* wall_seconds);
int rth_caster_walk_emissive_device(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp,
                                    const rtmi_tile_t* tile, uint32_t sample0, uint32_t nsamples, void* accum_device, void* out_device,
                                    void* hip_stream, rtmi_stats_t* stats, double* wall_seconds);
int rth_caster_emitter_sampler(rth_scene_t* s, uint32_t* q_out, uint64_t* cum_out, uint32_t* lamp_of_tri_out, float* lamps_out,
                               uint64_t cap_lamps, uint64_t cap_tris, uint64_t* total_out, uint32_t* nlamps_out);
/* Path tracing with up to four coloured box lights sampled at every matte hit (rtmi_render_lit / rtmi_render_lit_device in rtmi.h,
 * which defines it): rth_caster_walk_samples[_device] in every respect; lit must not be NULL. */
int rth_caster_walk_lit(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp, uint64_t row0,
                        uint64_t nrows, uint32_t sample0, uint32_t nsamples, const rtmi_lit_t* lit, float* accum_host, float* out_host,
                        rtmi_stats_t* stats, double* wall_seconds);
int rth_caster_walk_lit_device(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp,
                               const rtmi_tile_t* tile, uint32_t sample0, uint32_t nsamples, const rtmi_lit_t* lit, void* accum_device,
                               void* out_device, void* hip_stream, rtmi_stats_t* stats, double* wall_seconds);
/* Built-in camera models (rtmi_render_camera / rtmi_render_camera_device in rtmi.h, which defines them):
 * rth_caster_walk_samples[_device] in every respect, with the rays of `camera` (pinhole, thin lens, orthographic) and, when
 * guides is not NULL, rth_caster_walk_features' buffers of those rays. */
int rth_caster_walk_camera(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp, uint64_t row0,
                           uint64_t nrows, const rtmi_camera_t* camera, uint32_t sample0, uint32_t nsamples, float* accum_host,
                           float* out_host, const rtmi_camera_out_t* guides_host, rtmi_stats_t* stats, double* wall_seconds);
int rth_caster_walk_camera_device(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp,
                                  const rtmi_tile_t* tile, const rtmi_camera_t* camera, uint32_t sample0, uint32_t nsamples,
                                  void* accum_device, void* out_device, const rtmi_camera_out_t* guides, void* hip_stream,
                                  rtmi_stats_t* stats, double* wall_seconds);
/* The shaded preview (rtmi_render_preview / rtmi_render_preview_device, which rtmi.h defines) on the scene's resident copy:
 * albedo, ambient occlusion and up to four coloured box lights composed per sample, with the layers `out` asks for.  maxdepth
 * is not consulted; the primary rays use the caster's seed. */
int rth_caster_walk_preview(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp, uint64_t row0,
                            uint64_t nrows, uint32_t sample0, uint32_t nsamples, const rtmi_preview_t* preview,
                            const rtmi_preview_out_t* out_host, rtmi_stats_t* stats, double* wall_seconds);
int rth_caster_walk_preview_device(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp,
                                   const rtmi_tile_t* tile, uint32_t sample0, uint32_t nsamples, const rtmi_preview_t* preview,
                                   const rtmi_preview_out_t* out_device, void* hip_stream, rtmi_stats_t* stats, double* wall_seconds);
/* Per-ray records (rtmi_trace_records / rtmi_primary_records, same buffers and size-query idiom) on the scene's
 * resident copy; the primary records use the caster's seed. */
int rth_caster_trace_records(rth_scene_t* s, uint64_t n, const float* orig4, const float* dir4, rtmi_ray_record_t* recs,
                             uint32_t* leaf_ids, uint64_t leaf_cap, uint64_t* leaf_total, rtmi_stats_t* stats);
int rth_caster_primary_records(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp,
                               uint32_t row0, uint32_t nrows, uint32_t sample, rtmi_ray_record_t* recs, uint32_t* leaf_ids,
                               uint64_t leaf_cap, uint64_t* leaf_total, rtmi_stats_t* stats);
/* Scene.debug_en, and Scene.debug as HipRayCaster::walk_rays_internal left it: *nrecs / *nleaf_ids always receive the
 * sizes; recs (nrecs entries), pixel2 ((row, col) per record) and leaf_ids are filled when not NULL. */
int rth_scene_set_debug(rth_scene_t* s, int on);
int rth_scene_debug_records(rth_scene_t* s, rtmi_ray_record_t* recs, uint32_t* pixel2, uint32_t* leaf_ids, uint64_t* nrecs,
                            uint64_t* nleaf_ids);
/* Multi-GPU inside the process (rtmi_render_frame_multi): the caster keeps one resident copy of the scene per entry of
 * `devices` (an entry may repeat a device); entry 0 is the root that receives the bands.  With more than one entry
 * walk_rays (rth_caster_walk_rows over the whole image) and rth_caster_walk_frame_multi stripe the frame over them. */
int rth_caster_set_devices(rth_scene_t* s, const int32_t* devices, uint32_t n);
int rth_caster_walk_frame_multi(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp,
                                uint32_t stripe_rows, uint32_t flags /* RTMI_FRAME_RGB8 */, void* out_host, void* out_device,
                                rtmi_stats_t* stats_sum, rtmi_stats_t* per_device, uint32_t per_device_cap, double* wall_seconds);
int rth_caster_upload(rth_scene_t* s);
/* The a-trous denoiser (rtmi_denoise / rtmi_denoise_device / rtmi_render_denoised in rtmi.h, which defines the filter) on
 * whole w x h images of this scene's caster: colour as rth_caster_walk_rows writes it, albedo and normal as
 * rth_caster_walk_features does.  rth_caster_walk_denoised renders the frame, takes the features of all its samples and
 * filters on the device; only the result is copied to out_host. */
int rth_caster_denoise(rth_scene_t* s, uint32_t w, uint32_t h, const float* color_host, const float* albedo_host,
                       const float* normal_host, const rtmi_denoise_t* params, float* out_host);
int rth_caster_denoise_device(rth_scene_t* s, uint32_t w, uint32_t h, const void* color_device, const void* albedo_device,
                              const void* normal_device, const rtmi_denoise_t* params, void* out_device, void* hip_stream);
int rth_caster_walk_denoised(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp,
                             const rtmi_denoise_t* params, float* out_host, rtmi_stats_t* stats, double* wall_seconds);
/* Variance-guided denoising (rtmi_variance* / rtmi_denoise_var* / rtmi_render_adaptive_denoised in rtmi.h, which defines it) on
 * this scene's caster: the variance image from the moments of an adaptive render (accum, sumsq, counts of npixels pixels), the
 * filter with that image beside rth_caster_denoise's (var_out may be NULL), and the adaptive render, its variance, the features
 * of its first ad->min_samples samples and the filter in one call: only the result and the counts (optional) are copied out. */
int rth_caster_variance(rth_scene_t* s, const float* accum_host, const float* sumsq_host, const uint32_t* counts_host,
                        uint64_t npixels, float* variance_host);
int rth_caster_variance_device(rth_scene_t* s, const void* accum_device, const void* sumsq_device, const void* counts_device,
                               uint64_t npixels, void* variance_device, void* hip_stream);
int rth_caster_denoise_var(rth_scene_t* s, uint32_t w, uint32_t h, const float* color_host, const float* albedo_host,
                           const float* normal_host, const float* variance_host, const rtmi_denoise_t* params, float* out_host,
                           float* var_out_host);
int rth_caster_denoise_var_device(rth_scene_t* s, uint32_t w, uint32_t h, const void* color_device, const void* albedo_device,
                                  const void* normal_device, const void* variance_device, const rtmi_denoise_t* params,
                                  void* out_device, void* var_out_device, void* hip_stream);
int rth_caster_walk_adaptive_denoised(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp,
                                      rtmi_adaptive_t* ad, const rtmi_denoise_t* params, float* out_host, uint32_t* counts_host,
                                      rtmi_stats_t* stats, double* wall_seconds);
/* Launch tuning for this scene's caster: fields that are 0 keep the library default, xcd_aware is passed as value + 1;
 * NULL restores all defaults.  Never changes a pixel. */
int rth_caster_set_tuning(rth_scene_t* s, const rtmi_tuning_t* tuning);
int rth_caster_quantize_device(rth_scene_t* s, const void* rgba_device, uint64_t npixels, void* rgb_device, void* hip_stream); /* make the scene resident now (otherwise on first use) */

/* write_png's quantisation on the host (raytrace.rs:1468-1473) */
void rth_quantize(const float* rgba, uint64_t npixels, uint8_t* rgb);

#ifdef __cplusplus
}
#endif
#endif
