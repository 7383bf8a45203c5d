// raytrace.hpp — host-side C++ mirror of the reference's scene/camera API
// (raytrace_lib/src/raytrace.rs, obj_parser.rs) plus the `RayCaster` plug-in
// whose MI355X implementation (`HipRayCaster`) calls the C ABI of
// include/rtmi.h.  In a real integration this layer stays in Rust (see
// INTEGRATION.md); it exists here because the image has no Rust toolchain.
//
// Same names, argument meaning and error behaviour as the reference; where the
// reference panics (`unwrap`, `assert!`) these functions throw
// std::runtime_error.  All arithmetic is strict IEEE f32 in the reference's
// operation order (compile with -ffp-contract=off).
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include <optional>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>

#include "../../../include/rtmi.h"

namespace raytrace {

// raytrace.rs:22-122 — Simd<f32,4>, lane 3 carried like the reference does.
struct Vec3 {
    float v[4];
    Vec3 add(const Vec3& o) const;
    Vec3 sub(const Vec3& o) const;
    Vec3 mult(float a) const;
    Vec3 mult_per(const Vec3& o) const;
    float len2() const;
    float len() const;
    float dot(const Vec3& o) const;
    Vec3 cross(const Vec3& o) const;
    Vec3 unit() const;
    Vec3 orthogonal() const;
    Vec3 change_basis(const std::tuple<Vec3, Vec3, Vec3>& b) const;
};
using Point = Vec3;
using Color = Vec3;

Vec3 make_vec(const float (&v)[3]);
inline Vec3 make_vec(float a, float b, float c) { const float t[3] = {a, b, c}; return make_vec(t); }
Color make_color(uint8_t r, uint8_t g, uint8_t b);  // raytrace.rs:176-180

// raytrace.rs:194-210
struct Ray { Point orig; Vec3 dir; Vec3 inv_dir; };
Ray make_ray(const Point& orig, const Vec3& dir);

// raytrace.rs:303-308, and Dielectric (include/rtmi.h, RTMI_DIELECTRIC: not in the reference), whose `scattering` is the
// index of refraction
struct SurfaceKind {
    enum Tag : uint32_t { Solid = RTMI_SOLID, Matte = RTMI_MATTE, Reflective = RTMI_REFLECTIVE, Dielectric = RTMI_DIELECTRIC } tag;
    Color color;
    float alpha;
    float scattering;  // Reflective; Dielectric: the index of refraction
    static SurfaceKind solid(const Color& c) { return SurfaceKind{Solid, c, 0.f, 0.f}; }
    static SurfaceKind matte(const Color& c, float alpha) { return SurfaceKind{Matte, c, alpha, 0.f}; }
    static SurfaceKind reflective(float scattering, const Color& c, float alpha) { return SurfaceKind{Reflective, c, alpha, scattering}; }
    static SurfaceKind dielectric(float ior, const Color& c, float alpha) { return SurfaceKind{Dielectric, c, alpha, ior}; }
};

// raytrace.rs:326-337
struct Triangle {
    Point incenter;
    Vec3 norm;
    float bounding_r2;
    Vec3 sides[3];
    float side_lens[3];
    Vec3 corners[3];
    SurfaceKind surface;
    float edge_thickness;
    size_t num;
};

Triangle make_triangle(const Vec3 (&points)[3], const SurfaceKind& surface, float edge_thickness);  // :340-383
// The same for many triangles on the GPU (rtmi_make_triangles): corners[i] = 3 points; bit-identical results.
std::vector<Triangle> make_triangles_gpu(const std::vector<Vec3>& corners, const SurfaceKind& surface, float edge_thickness,
                                         int device = 0);
Triangle make_dummy_triangle();                                                                      // :385-391
void populate_triangle_numbers(std::vector<Triangle>& tris);                                         // :393-397
std::vector<Triangle> make_sphere(const Point& orig, float r, std::pair<size_t, size_t> lat_lon,
                                  const SurfaceKind& surface, float edge_thickness);                 // :464-529
std::vector<Triangle> make_disk(const Point& orig, const Vec3& norm, float r, float d, size_t num_tris,
                                const SurfaceKind& surface, const SurfaceKind& side_surface,
                                float edge_thickness);                                               // :531-592

// raytrace.rs:612-634.  The reference's recursive `BoundingBox` is kept
// flattened, in the layout the C ABI transports (breadth-first, children of a
// box contiguous, triangle indices of a leaf contiguous).
struct BoundingBox {
    std::vector<rtmi_box_t> boxes;  // boxes[0] = root
    std::vector<uint32_t> tri_refs;
    size_t num_inner() const;
    size_t num_leaves() const;
    size_t max_depth() const;
};

bool box_contains_polygon(const Point& orig, float len2, const Triangle& t);                         // :753-779
bool face_contains_triangle(const Point& p, const Vec3& norm, float len2, const Triangle& t);        // :645-729
BoundingBox build_empty_box();                                                                       // :781-788
BoundingBox build_bounding_box(const std::vector<Triangle>& tris, const Point& orig, float len2,
                               size_t maxdepth, size_t minobjs, unsigned threads = 0);               // :790-845
// The same tree, the box/triangle overlap tests of every level evaluated on the GPU (rtmi_builder_*); bit-equal result.
BoundingBox build_bounding_box_gpu(const std::vector<Triangle>& tris, const Point& orig, float len2, size_t maxdepth,
                                   size_t minobjs, int device = 0);
BoundingBox build_trivial_bounding_box(const std::vector<Triangle>& tris, const Point& orig, float len2);  // :847-856

// raytrace.rs:595-598: a box light, `orig` its corner and `len2` its edge (0: a point light).  The reference declares it and
// spells its shadow ray out in a comment (_get_shadow_ray, :600-610) without running either; here it is the light of the
// direct-light buffer (HipRayCaster::walk_rays_light, rtmi_render_light* in rtmi.h, which defines the shadow ray) and, as
// Scene::light, of the shadowed path-trace (HipRayCaster::walk_rays_shadowed, rtmi_render_shadowed*).
struct LightSource {
    Point orig;
    float len2;
};

// Analytic sphere: NOT in the reference at this revision (only Triangle is Collidable, raytrace.rs:399; make_sphere
// tessellates).  A build-defined extension named by BASELINE's north_star; semantics in include/rtmi.h (rtmi_sphere_t)
// and, operation by operation, in DESIGN.md 4.6.  Parity with the Rust binary: unpinned.
struct Sphere {
    Point center;
    float radius;
    SurfaceKind surface;
};

// The environment of a scene (include/rtmi.h, rtmi_scene_set_environment / rtmi_scene_set_sky): NOT in the
// reference, whose paths that leave the scene all return one constant.  Either a table of n x n RGB texels with the frame that
// takes a world direction to map space, or (generated) the parameters of a sky the device fills the table from.
struct Environment {
    uint32_t n = 0;
    bool generated = false;
    std::vector<float> rgb;  // n * n * 3, row j, column i; empty when generated
    float frame[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
    rtmi_sky_t sky{};
};

// Per-ray records of the octree walk (rtmi_trace_records / rtmi_primary_records), the reference's DebugCtx (debug.rs):
// record i's leaves are leaf_ids[recs[i].leaf_first .. + recs[i].nleaves), indices into Scene.boxes.boxes.  pixel[i] =
// (row, col) of record i for primary records; empty for explicit rays.
struct RayRecords {
    std::vector<rtmi_ray_record_t> recs;
    std::vector<uint32_t> leaf_ids;
    std::vector<std::pair<uint32_t, uint32_t>> pixel;
};

// raytrace.rs:1297-1303
struct Scene {
    std::vector<Triangle> tris;
    BoundingBox boxes;
    std::vector<Sphere> spheres;  // analytic spheres: a flat list tested against every ray after the box tree
    // The reference's commented-out `light: LightSource` field.  walk_rays never looks at it (the reference's color_ray does not
    // either: its shadow block is commented out); walk_rays_shadowed / walk_shadowed_device need it.  Not part of the uploaded
    // scene: setting it needs no touch().
    std::optional<LightSource> light;
    // The environment, or none.  A HipRayCaster applies it to its resident copies on every device when env_generation differs
    // from the one it saw; the scene itself is not uploaded again, so code that edits `environment` bumps env_generation, not
    // generation.
    std::optional<Environment> environment;
    uint64_t env_generation = 0;
    // Vertex normals (include/rtmi.h, "VERTEX NORMALS OF A SCENE"), or none (empty): 9 floats per triangle, entry
    // i for tris[i], all zero = flat.  May be shorter than tris: triangles appended after the normals were set are flat.  Applied
    // like the environment: code that edits `normals` bumps normals_generation, not generation.
    std::vector<float> normals;
    uint64_t normals_generation = 0;
    // Textures (include/rtmi.h, "TEXTURES OF A SCENE"), or none (no images).  uvs: 6 floats per triangle
    // (u0, v0, u1, v1, u2, v2), entry i for tris[i]; tex_of_tri: 0 = none, or 1..images.  Both may be shorter than tris: triangles
    // appended later are untextured.  Applied like the normals: code that edits them bumps tex_generation, not generation.
    struct Texture { uint32_t width = 0, height = 0; std::vector<float> rgb; };
    std::vector<Texture> textures;
    std::vector<float> uvs;
    std::vector<uint32_t> tex_of_tri;
    uint64_t tex_generation = 0;
    // Normal maps (include/rtmi.h, "NORMAL MAPS OF A SCENE"), or none (empty): per triangle 0 = none, or the number
    // 1..images of the texture that is its map; may be shorter than tris.  Applied after the textures: code that edits them bumps
    // nmap_generation.  Setting or clearing the images clears them.
    std::vector<uint32_t> nmap_of_tri;
    float nmap_strength = 1.f;
    uint64_t nmap_generation = 0;
    // Emitters (include/rtmi.h, "EMISSIVE TRIANGLES"), or none (empty): one byte per triangle, non-zero = a lamp;
    // may be shorter than tris: triangles appended later are no lamps.  Applied like the normals: code that edits them bumps
    // emit_generation.
    std::vector<uint8_t> emitters;
    uint64_t emit_generation = 0;
    // debug_en: walk_rays also records sample 0's primary ray of every pixel into `debug` (the reference's debug_ctx, which
    // walk_rays fills through a &Scene: hence mutable).  Octree scenes only; walk_rays throws before rendering otherwise.
    bool debug_en = false;
    mutable RayRecords debug;
    // Bumped by touch(): a HipRayCaster keeps the uploaded copy of a Scene resident and re-uploads when the
    // generation it saw differs.  Code that edits tris/boxes in place must call touch() afterwards.
    uint64_t generation = 0;
    void touch() { generation++; }
};

// raytrace.rs:1305-1318
struct Viewport {
    size_t width, height;
    Point orig, cam;
    Vec3 vu, vv;
    size_t maxdepth, samples_per_pixel;
};
std::tuple<Vec3, Vec3, Vec3> create_transform(const Vec3& dir_in, float d_roll);                     // :1320-1341
Viewport create_viewport(std::pair<uint32_t, uint32_t> px, std::pair<float, float> size, const Point& pos,
                         const Vec3& dir, float fov, float c_roll, size_t maxdepth, size_t samples);  // :1343-1370
float to_radians(float deg);

// progress.rs:95-184 reduced to what print_stats reports.
struct ProgressCtx {
    uint64_t total_rays = 0;
    double seconds = 0.0;        // wall time of walk_rays (create_ctx -> finish)
    double kernel_seconds = 0.0; // device time of the render kernels
    rtmi_stats_t stats{};
    std::string stats_line() const;  // "Processed X million rays in Y seconds. Z million rays/s"
};

// raytrace.rs:1128-1165
class RayCaster {
public:
    virtual ~RayCaster() = default;
    virtual void walk_rays_internal(const Viewport& v, const Scene& s, Color* data, size_t threads, ProgressCtx& progress) = 0;
    ProgressCtx walk_rays(const Viewport& v, const Scene& s, Color* data, size_t threads, bool show_progress);
};

// The MI355X implementation of the plug-in.  `threads` is ignored like the
// reference's CudaRayCaster does (cuda_raytrace.rs:546-572).  Keeps the
// uploaded scene resident between calls on the same Scene object.
class HipRayCaster : public RayCaster {
public:
    explicit HipRayCaster(uint64_t seed = 1, int device = 0);
    ~HipRayCaster() override;
    HipRayCaster(const HipRayCaster&) = delete;
    HipRayCaster& operator=(const HipRayCaster&) = delete;
    void walk_rays_internal(const Viewport& v, const Scene& s, Color* data, size_t threads, ProgressCtx& progress) override;
    // Render only rows [row0, row0+nrows): the unit of multi-GPU image tiling.
    void walk_rows(const Viewport& v, const Scene& s, size_t row0, size_t nrows, Color* data, ProgressCtx& progress);
    void walk_rows_device(const Viewport& v, const Scene& s, size_t row0, size_t nrows, void* out_device,
                          void* hip_stream, ProgressCtx& progress);
    // Multi-GPU inside one process (rtmi_render_frame_multi): the frame is striped over `devices` (one uploaded copy
    // of the scene per entry; an entry may repeat a device), bands are copied once to devices[0] and de-interleaved
    // there.  With more than one entry walk_rays_internal() takes this path.  flags: RTMI_FRAME_RGB8 -> `data` is
    // height*width*3 bytes.
    void set_devices(const std::vector<int>& devices);
    void walk_frame_multi(const Viewport& v, const Scene& s, void* data_host, void* data_device, uint32_t stripe_rows,
                          uint32_t flags, ProgressCtx& progress, std::vector<rtmi_stats_t>* per_device = nullptr);
    // Striped row set (rtmi_tile_t): rank r of N renders {r*S, H/N, S, N*S}.
    void walk_tile_device(const Viewport& v, const Scene& s, const rtmi_tile_t& tile, void* out_device,
                          void* hip_stream, ProgressCtx& progress);
    // Progressive rendering (rtmi_render_samples / rtmi_render_samples_device): samples [sample0, sample0 + nsamples) of
    // the frame's v.samples_per_pixel, continuing the per-pixel running sums in `accum` (read only when sample0 > 0);
    // `out` (may be null) receives the preview.  Passes over [0, spp) in order end in the bits of walk_rows / walk_tile_device.
    void walk_samples(const Viewport& v, const Scene& s, size_t row0, size_t nrows, uint32_t sample0, uint32_t nsamples,
                      Color* accum, Color* out, ProgressCtx& progress);
    void walk_samples_device(const Viewport& v, const Scene& s, const rtmi_tile_t& tile, uint32_t sample0, uint32_t nsamples,
                             void* accum_device, void* out_device, void* hip_stream, ProgressCtx& progress);
    // First-hit feature buffers (rtmi_render_features / rtmi_render_features_device): per-pixel means over samples [sample0,
    // sample0 + nsamples) of the primary rays' (albedo.rgb, coverage) and (normal.xyz, depth), one Color each, and the hit id
    // (tri | face << 30) of each pixel's sample `sample0`.  Any of the three buffers may be null, not all; v.maxdepth is unused.
    void walk_rays_features(const Viewport& v, const Scene& s, size_t row0, size_t nrows, uint32_t sample0, uint32_t nsamples,
                            Color* albedo, Color* normal, uint32_t* ids, ProgressCtx& progress);
    void walk_features_device(const Viewport& v, const Scene& s, const rtmi_tile_t& tile, uint32_t sample0, uint32_t nsamples,
                              void* albedo_device, void* normal_device, void* ids_device, void* hip_stream, ProgressCtx& progress);
    // The a-trous denoiser (rtmi_denoise / rtmi_denoise_device / rtmi_render_denoised): whole width x height images, colour
    // as walk_rows writes it, albedo and normal as walk_rays_features does; out may not be one of the inputs.
    void denoise(const Scene& s, uint32_t width, uint32_t height, const Color* color, const Color* albedo, const Color* normal,
                 const rtmi_denoise_t& params, Color* out);
    void denoise_device(const Scene& s, uint32_t width, uint32_t height, const void* color_device, const void* albedo_device,
                        const void* normal_device, const rtmi_denoise_t& params, void* out_device, void* hip_stream);
    // walk_rows of the whole frame, the features of all its samples and the filter, on the device; out receives the result
    void walk_rays_denoised(const Viewport& v, const Scene& s, const rtmi_denoise_t& params, Color* out, ProgressCtx& progress);
    // Any-hit occlusion (rtmi_occluded*): occluded[i] = 1 iff ray i's closest hit lies before tmax[i] (tmax null: +inf); rays
    // as make_ray stores them, 8 floats each in two arrays.  The device variant reads device buffers in place.
    void occluded(const Scene& s, uint64_t n, const float* orig4, const float* dir4, const float* tmax, uint8_t* out,
                  rtmi_stats_t* stats = nullptr);
    void occluded_device(const Scene& s, uint64_t n, const void* orig4_device, const void* dir4_device, const void* tmax_device,
                         void* occluded_device, void* hip_stream, rtmi_stats_t* stats = nullptr);
    // rtmi_trace on device buffers (rtmi_trace_device): rays read in place, tri / t / face written in place.
    void trace_device(const Scene& s, uint64_t n, const void* orig4_device, const void* dir4_device, void* tri_device, void* t_device,
                      void* face_device, void* hip_stream, rtmi_stats_t* stats = nullptr);
    // Path tracing of caller-supplied rays (rtmi_render_rays / rtmi_render_rays_device, which rtmi.h defines) with the caster's
    // seed: per-ray colours, per-group means and the groups' first-hit guide buffers.  keys: n x 2 uint32 or null.
    void walk_rays_explicit(const Scene& s, uint64_t n, const float* orig4, const float* dir4, const uint32_t* keys, const rtmi_rays_t* rays,
                            const rtmi_rays_out_t* out_host, ProgressCtx& progress);
    void walk_rays_explicit_device(const Scene& s, uint64_t n, const void* orig4_device, const void* dir4_device, const void* keys_device,
                                   const rtmi_rays_t* rays, const rtmi_rays_out_t* out_device, void* hip_stream, ProgressCtx& progress);
    // Light baked at M surface points or over M triangles (rtmi_bake / rtmi_bake_device, which rtmi.h defines) with the caster's
    // seed: bake.rays gather rays per element made on the device, path-traced and folded to light / open; the rays themselves on
    // request.  pos4: M float4 (points) or 3 M float4 (triangle corners); nrm4: M float4, the side to bake.
    void bake(const Scene& s, uint64_t M, const float* pos4, const float* nrm4, const rtmi_bake_t& bake, const rtmi_bake_out_t& out_host,
              ProgressCtx& progress);
    void bake_device(const Scene& s, uint64_t M, const void* pos4_device, const void* nrm4_device, const rtmi_bake_t& bake,
                     const rtmi_bake_out_t& out_device, void* hip_stream, ProgressCtx& progress);
    // Both with box lights (rtmi_render_rays_lit* / rtmi_bake_lit*, which rtmi.h defines): the lamps sampled at every Matte hit
    // of every path, and for the bake at the element itself (out.direct).
    void walk_rays_explicit_lit(const Scene& s, uint64_t n, const float* orig4, const float* dir4, const uint32_t* keys, const rtmi_rays_t* rays,
                                const rtmi_lit_t* lit, const rtmi_rays_out_t* out_host, ProgressCtx& progress);
    void walk_rays_explicit_lit_device(const Scene& s, uint64_t n, const void* orig4_device, const void* dir4_device, const void* keys_device,
                                       const rtmi_rays_t* rays, const rtmi_lit_t* lit, const rtmi_rays_out_t* out_device, void* hip_stream,
                                       ProgressCtx& progress);
    void bake_lit(const Scene& s, uint64_t M, const float* pos4, const float* nrm4, const rtmi_bake_t& bake, const rtmi_lit_t& lit,
                  const rtmi_bake_lit_out_t& out_host, ProgressCtx& progress);
    void bake_lit_device(const Scene& s, uint64_t M, const void* pos4_device, const void* nrm4_device, const rtmi_bake_t& bake,
                         const rtmi_lit_t& lit, const rtmi_bake_lit_out_t& out_device, void* hip_stream, ProgressCtx& progress);
    // Ambient occlusion (rtmi_render_ao / rtmi_render_ao_device, which rtmi.h defines): one float per pixel, the share of
    // ao.rays hemisphere rays per primary sample of [sample0, sample0 + nsamples) that are not occluded within ao.radius.
    void walk_rays_ao(const Viewport& v, const Scene& s, size_t row0, size_t nrows, uint32_t sample0, uint32_t nsamples,
                      const rtmi_ao_t& ao, float* out, ProgressCtx& progress);
    void walk_ao_device(const Viewport& v, const Scene& s, const rtmi_tile_t& tile, uint32_t sample0, uint32_t nsamples,
                        const rtmi_ao_t& ao, void* ao_device, void* hip_stream, ProgressCtx& progress);
    // Direct light (rtmi_render_light / rtmi_render_light_device, which rtmi.h defines): two floats per pixel, the share of
    // `rays` samples of `light` per primary sample of [sample0, sample0 + nsamples) that are visible from the first hit, and
    // the mean of n . dir over them.  flags: RTMI_LIGHT_UNBOUNDED or 0; bias: the smudge factor.  Either plane may be null.
    void walk_rays_light(const Viewport& v, const Scene& s, size_t row0, size_t nrows, uint32_t sample0, uint32_t nsamples,
                         const LightSource& light, uint32_t rays, uint32_t flags, float bias, float* shadow, float* irradiance,
                         ProgressCtx& progress);
    void walk_light_device(const Viewport& v, const Scene& s, const rtmi_tile_t& tile, uint32_t sample0, uint32_t nsamples,
                           const LightSource& light, uint32_t rays, uint32_t flags, float bias, void* shadow_device,
                           void* irradiance_device, void* hip_stream, ProgressCtx& progress);
    // Path tracing with the reference's shadow rays switched on (rtmi_render_shadowed / rtmi_render_shadowed_device, which
    // rtmi.h defines): walk_samples / walk_samples_device in every respect, with every surface hit of every bounce tested
    // against s.light (one shadow ray per hit) and shown black where it is shadowed.  Throws when s.light is empty.
    // flags: RTMI_LIGHT_UNBOUNDED or 0; bias: the smudge factor (the reference's 0.005).
    void walk_rays_shadowed(const Viewport& v, const Scene& s, size_t row0, size_t nrows, uint32_t sample0, uint32_t nsamples,
                            uint32_t flags, float bias, Color* accum, Color* out, ProgressCtx& progress);
    void walk_shadowed_device(const Viewport& v, const Scene& s, const rtmi_tile_t& tile, uint32_t sample0, uint32_t nsamples,
                              uint32_t flags, float bias, void* accum_device, void* out_device, void* hip_stream,
                              ProgressCtx& progress);
    // Path tracing with the environment sampled at matte hits (rtmi_render_envlight / rtmi_render_envlight_device, which rtmi.h
    // defines): walk_samples / walk_samples_device in every respect.
    void walk_rays_envlight(const Viewport& v, const Scene& s, size_t row0, size_t nrows, uint32_t sample0, uint32_t nsamples,
                            const rtmi_envlight_t& env, Color* accum, Color* out, ProgressCtx& progress);
    void walk_envlight_device(const Viewport& v, const Scene& s, const rtmi_tile_t& tile, uint32_t sample0, uint32_t nsamples,
                              const rtmi_envlight_t& env, void* accum_device, void* out_device, void* hip_stream, ProgressCtx& progress);
    // Path tracing with box lights sampled at every matte hit (rtmi_render_lit / rtmi_render_lit_device, which rtmi.h defines):
    // walk_samples / walk_samples_device in every respect.
    void walk_rays_lit(const Viewport& v, const Scene& s, size_t row0, size_t nrows, uint32_t sample0, uint32_t nsamples,
                       const rtmi_lit_t& lit, Color* accum, Color* out, ProgressCtx& progress);
    void walk_lit_device(const Viewport& v, const Scene& s, const rtmi_tile_t& tile, uint32_t sample0, uint32_t nsamples,
                         const rtmi_lit_t& lit, void* accum_device, void* out_device, void* hip_stream, ProgressCtx& progress);
    // Path tracing with the scene's emissive triangles sampled at matte hits (rtmi_render_emissive / rtmi_render_emissive_device,
    // which rtmi.h defines): walk_samples / walk_samples_device in every respect.
    void walk_rays_emissive(const Viewport& v, const Scene& s, size_t row0, size_t nrows, uint32_t sample0, uint32_t nsamples, Color* accum,
                            Color* out, ProgressCtx& progress);
    void walk_emissive_device(const Viewport& v, const Scene& s, const rtmi_tile_t& tile, uint32_t sample0, uint32_t nsamples,
                              void* accum_device, void* out_device, void* hip_stream, ProgressCtx& progress);
    // The lamps' tables of the scene's resident copy on the first device (rtmi_scene_get_emitter_sampler): L weights, L prefix sums,
    // ntris lamp numbers, L * 20 floats of records and the total; all empty when the scene has no lamps.
    struct EmitterSampler { std::vector<uint32_t> q, lamp_of_tri; std::vector<uint64_t> cum; std::vector<float> lamps; uint64_t total = 0; };
    EmitterSampler emitter_sampler(const Scene& s);
    // The sampler table of the environment of the scene's resident copy on the first device (rtmi_scene_get_env_sampler): n * n
    // weights and their sum, empty and n = 0 when the scene has no environment.
    std::vector<uint32_t> env_sampler(const Scene& s, uint32_t& n, uint64_t& total);
    // Built-in camera models (rtmi_render_camera / rtmi_render_camera_device, which rtmi.h defines): walk_samples /
    // walk_samples_device in every respect, with the rays of `camera` (pinhole, thin lens, orthographic) and, when `guides` is
    // not null, the feature buffers of those rays.
    void walk_rays_camera(const Viewport& v, const Scene& s, size_t row0, size_t nrows, const rtmi_camera_t& camera, uint32_t sample0,
                          uint32_t nsamples, Color* accum, Color* out, const rtmi_camera_out_t* guides, ProgressCtx& progress);
    void walk_camera_device(const Viewport& v, const Scene& s, const rtmi_tile_t& tile, const rtmi_camera_t& camera, uint32_t sample0,
                            uint32_t nsamples, void* accum_device, void* out_device, const rtmi_camera_out_t* guides, void* hip_stream,
                            ProgressCtx& progress);
    // Shaded preview (rtmi_render_preview / rtmi_render_preview_device, which rtmi.h defines): albedo, AO and up to four
    // coloured box lights composed per sample from one primary pass; `out` names the colour image and the layers wanted.
    void walk_rays_preview(const Viewport& v, const Scene& s, size_t row0, size_t nrows, uint32_t sample0, uint32_t nsamples,
                           const rtmi_preview_t& preview, const rtmi_preview_out_t& out, ProgressCtx& progress);
    void walk_preview_device(const Viewport& v, const Scene& s, const rtmi_tile_t& tile, uint32_t sample0, uint32_t nsamples,
                             const rtmi_preview_t& preview, const rtmi_preview_out_t& out_device, void* hip_stream,
                             ProgressCtx& progress);
    // Variance-guided denoising (rtmi_variance* / rtmi_denoise_var* / rtmi_render_adaptive_denoised): variance() turns the
    // moments of an adaptive render (accum, sumsq, counts of npixels pixels) into the variance image the filter takes beside
    // denoise()'s images; var_out (may be null) receives the propagated variance.  walk_adaptive_denoised runs the adaptive
    // render, the variance image, the features of the first ad.min_samples samples and the filter on the device.
    void variance(const Scene& s, const Color* accum, const Color* sumsq, const uint32_t* counts, uint64_t npixels, Color* out);
    void variance_device(const Scene& s, const void* accum_device, const void* sumsq_device, const void* counts_device,
                         uint64_t npixels, void* variance_device, void* hip_stream);
    void denoise_var(const Scene& s, uint32_t width, uint32_t height, const Color* color, const Color* albedo, const Color* normal,
                     const Color* variance, const rtmi_denoise_t& params, Color* out, Color* var_out);
    void denoise_var_device(const Scene& s, uint32_t width, uint32_t height, const void* color_device, const void* albedo_device,
                            const void* normal_device, const void* variance_device, const rtmi_denoise_t& params, void* out_device,
                            void* var_out_device, void* hip_stream);
    void walk_adaptive_denoised(const Viewport& v, const Scene& s, rtmi_adaptive_t& ad, const rtmi_denoise_t& params, Color* out,
                                uint32_t* counts, ProgressCtx& progress);
    // Adaptive sampling (rtmi_render_adaptive / rtmi_render_adaptive_device): every pixel stops at its own count between
    // ad.min_samples and v.samples_per_pixel and equals the pixel of walk_rows at that many samples; counts receives them.
    void walk_adaptive(const Viewport& v, const Scene& s, size_t row0, size_t nrows, rtmi_adaptive_t& ad, Color* out,
                       uint32_t* counts, ProgressCtx& progress);
    void walk_adaptive_device(const Viewport& v, const Scene& s, const rtmi_tile_t& tile, rtmi_adaptive_t& ad, void* accum_device,
                              void* sumsq_device, void* counts_device, void* out_device, void* hip_stream, ProgressCtx& progress);
    // A batch of views of one scene (rtmi_render_views / rtmi_render_views_device): views[k] with seeds[k] is what walk_rows
    // of that view renders, bit for bit; the views share width, height, maxdepth and samples_per_pixel.  The batch is one
    // stacked image of views.size() * height rows (row k * height + r = row r of view k): walk_views writes all of it,
    // walk_views_device the rows of `tile`.  seeds empty: this caster's seed for every view.
    void walk_views(const std::vector<Viewport>& views, const Scene& s, const std::vector<uint64_t>& seeds, Color* data,
                    ProgressCtx& progress);
    void walk_views_device(const std::vector<Viewport>& views, const Scene& s, const std::vector<uint64_t>& seeds,
                           const rtmi_tile_t& tile, void* out_device, void* hip_stream, ProgressCtx& progress);
    void set_options(uint32_t opts) { options_ = opts; }
    // Per-ray records of the production walk (rtmi_trace_records / rtmi_primary_records, on the first device): explicit
    // rays (n x 4 floats each), or sample `sample` of every pixel of rows [row0, row0 + nrows).  Throws on unsupported scenes.
    RayRecords trace_records(const Scene& s, size_t n, const float* orig4, const float* dir4, rtmi_stats_t* stats = nullptr);
    RayRecords primary_records(const Viewport& v, const Scene& s, size_t row0, size_t nrows, uint32_t sample,
                               rtmi_stats_t* stats = nullptr);
    // Progress while rendering, as DefaultRayCaster reports it (raytrace.rs:1411, :1429-1435 send one tuple per finished
    // row / per 10 k rays: (thread, row, pixels done, {"Rays": n}); progress.rs:95-141 draws from them).  With a callback
    // set, walk_rays_internal renders the frame in `bands` row bands (default 16) and calls it after each one with
    // (thread = 0, last row of the band, pixels of the band, rays of the band).  Same image; a band is a render call of
    // its own (its launches do not overlap the next band's), so a frame costs a few per cent more than in one piece.
    using ProgressFn = std::function<void(size_t thread, size_t row, size_t pixels, uint64_t rays)>;
    void set_progress(ProgressFn fn, size_t bands = 16) { on_progress_ = std::move(fn); progress_bands_ = bands ? bands : 1; }
    // Launch tuning (rtmi_tuning_t); fields left 0 keep the library defaults.  Never changes a pixel.
    void set_tuning(const rtmi_tuning_t& t) { tuning_ = t; has_tuning_ = true; }
    void clear_tuning() { has_tuning_ = false; }
    // Uploads on first use, and again when another Scene object is passed or Scene::generation changed.
    rtmi_scene_t* resident(const Scene& s);
    void invalidate();
    // The environment table of the scene's resident copy on the first device (rtmi_scene_get_environment): n * n * 3 floats,
    // empty and n = 0 when the scene has none.
    std::vector<float> environment(const Scene& s, uint32_t& n);
    // The vertex normals of the scene's resident copy on the first device (rtmi_scene_get_normals): ntris * 9 floats, empty when
    // the scene has none.
    std::vector<float> vertex_normals(const Scene& s);
    // The uvs and texture numbers of the scene's resident copy on the first device (rtmi_scene_get_uvs): ntris * 6 floats and
    // ntris numbers, empty when the scene has no textures; and image k = 1.. of it (rtmi_scene_get_texture).
    void texture_uvs(const Scene& s, std::vector<float>& uvs6, std::vector<uint32_t>& tex_of_tri);
    std::vector<float> texture_image(const Scene& s, uint32_t k, uint32_t& width, uint32_t& height);
    // The map numbers and the strength of the scene's resident copy on the first device (rtmi_scene_get_normal_maps): ntris numbers,
    // empty when the scene has no normal maps.
    std::vector<uint32_t> normal_maps(const Scene& s, float& strength);
    uint64_t seed;
    int device;

private:
    rtmi_scene_t* handle_ = nullptr;
    std::vector<int> devices_;                 // multi-GPU: device of every extra handle (entry 0 = `device`)
    std::vector<rtmi_scene_t*> extra_;         // handles of devices_[1..]
    const Scene* key_scene_ = nullptr;
    uint64_t key_generation_ = 0;
    uint64_t key_env_generation_ = 0;
    bool env_applied_ = false;                 // the handles carry Scene::environment as of key_env_generation_
    void apply_environment(const Scene& s);
    uint64_t key_normals_generation_ = 0;
    bool normals_applied_ = false;             // the handles carry Scene::normals as of key_normals_generation_
    void apply_normals(const Scene& s);
    uint64_t key_tex_generation_ = 0;
    bool tex_applied_ = false;                 // the handles carry Scene::textures / uvs as of key_tex_generation_
    void apply_textures(const Scene& s);
    uint64_t key_nmap_generation_ = 0;
    bool nmap_applied_ = false;                // the handles carry Scene::nmap_of_tri as of key_nmap_generation_
    bool nmap_on_device_ = false;              // ... and that is a table, not "none"
    void apply_normal_maps(const Scene& s);
    uint64_t key_emit_generation_ = 0;
    bool emit_applied_ = false;                // the handles carry Scene::emitters as of key_emit_generation_
    bool emit_on_device_ = false;              // ... and that is a set of marks, not "none"
    void apply_emitters(const Scene& s);
    size_t key_ntris_ = 0, key_nboxes_ = 0, key_nrefs_ = 0;
    uint32_t options_ = 0;
    rtmi_tuning_t tuning_{}, defaults_{};
    bool has_tuning_ = false;
    ProgressFn on_progress_;
    size_t progress_bands_ = 16;
    void apply_settings();
    void render_frame(const Viewport& v, const Scene& s, Color* data, size_t threads, ProgressCtx& progress);  // walk_rays_internal without debug_en
};

void flatten_triangles(const std::vector<Triangle>& tris, std::vector<rtmi_triangle_t>& out);
rtmi_viewport_t to_abi(const Viewport& v);

namespace obj_parser {
// obj_parser.rs:47-73.  ObjMode::Reference (default) is the reference's loader exactly: first three corners of every
// face, 1-based positive indices.  ObjMode::Robust is an opt-in extension: polygons are fan-triangulated, negative
// (relative) indices are resolved, degenerate triangles are skipped.
enum class ObjMode { Reference = 0, Robust = 1 };
std::vector<Triangle> parse_obj(const std::string& path, const Vec3& offset, float scale,
                                const std::tuple<Vec3, Vec3, Vec3>& transform, const SurfaceKind& surface,
                                float edge_thickness, ObjMode mode = ObjMode::Reference, std::vector<float>* normals9 = nullptr,
                                std::vector<float>* uvs6 = nullptr);
// normals9 (an extension; NULL: the loader above exactly): also read the `vn` lines and the third field of every a/b/c or a//c
// face corner, in either mode, and append 9 floats per returned triangle: each corner's normal through change_basis(transform)
// and unit(), no scale and no offset.  A corner without a normal index, or one out of range, throws.
// uvs6 (an extension likewise): also read the `vt` lines (their first two numbers) and the second field of every a/b or a/b/c face
// corner, and append 6 floats per returned triangle, (u, v) per corner as the file has them.  A corner without one throws.
}  // namespace obj_parser

// raytrace.rs:1460-1478: quantisation only ((c*255.) as u8); PNG encoding stays with the caller.
void quantize_rgb8(const Color* data, size_t npixels, uint8_t* rgb);

}  // namespace raytrace
