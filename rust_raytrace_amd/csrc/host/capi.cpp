// capi.cpp — extern "C" view (include/rtmi_host.h) of the C++ host mirror.
#include <chrono>
#include <cmath>
#include <cstring>
#include <memory>

#include "../../../include/rtmi_host.h"
#include "raytrace.hpp"

using namespace raytrace;

struct rth_scene {
    Scene scene;
    std::unique_ptr<HipRayCaster> caster;
    uint32_t options = 0;
};

static thread_local std::string g_herr;
const char* rth_last_error(void) { return g_herr.c_str(); }

template <typename F>
static int guarded(F&& f) {
    try { f(); return 0; }
    catch (const std::exception& e) { g_herr = e.what(); return 1; }
    catch (...) { g_herr = "unknown C++ exception"; return 1; }
}
static Vec3 v3(const float* p) { return make_vec(p[0], p[1], p[2]); }
static SurfaceKind surf(uint32_t kind, const float* c, float alpha, float scat) {
    if (kind > RTMI_DIELECTRIC) throw std::runtime_error("unknown surface kind");
    if (kind == RTMI_DIELECTRIC && !(std::isfinite(scat) && scat > 0.f))
        throw std::runtime_error("a dielectric's index of refraction (scattering) must be finite and > 0");
    return SurfaceKind{(SurfaceKind::Tag)kind, v3(c), alpha, scat};
}
static HipRayCaster& caster_of(rth_scene* s) {
    if (!s->caster) s->caster.reset(new HipRayCaster(1, 0));
    return *s->caster;
}
static Viewport vp_from(uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp) {
    Viewport v;
    v.width = w; v.height = h;
    v.orig = v3(vp12); v.cam = v3(vp12 + 3); v.vu = v3(vp12 + 6); v.vv = v3(vp12 + 9);
    v.maxdepth = (size_t)maxdepth; v.samples_per_pixel = (size_t)spp;
    return v;
}

extern "C" {

void rth_make_color(uint8_t r, uint8_t g, uint8_t b, float* o) { Color c = make_color(r, g, b); memcpy(o, c.v, 12); }
void rth_unit(const float* in3, float* o) { Vec3 c = v3(in3).unit(); memcpy(o, c.v, 12); }
float rth_to_radians(float deg) { return to_radians(deg); }
void rth_create_transform(const float* dir3, float d_roll, float* out9) {
    auto b = create_transform(v3(dir3), d_roll);
    memcpy(out9, std::get<0>(b).v, 12); memcpy(out9 + 3, std::get<1>(b).v, 12); memcpy(out9 + 6, std::get<2>(b).v, 12);
}
void rth_create_viewport(uint32_t w, uint32_t h, float size0, float size1, const float* pos3, const float* dir3, float fov,
                         float c_roll, float* out12) {
    Viewport v = create_viewport({w, h}, {size0, size1}, v3(pos3), v3(dir3), fov, c_roll, 1, 1);
    memcpy(out12, v.orig.v, 12); memcpy(out12 + 3, v.cam.v, 12); memcpy(out12 + 6, v.vu.v, 12); memcpy(out12 + 9, v.vv.v, 12);
}

rth_scene_t* rth_scene_new(int with_dummy) {
    rth_scene* s = new rth_scene();
    if (with_dummy) s->scene.tris.push_back(make_dummy_triangle());
    return s;
}
void rth_scene_free(rth_scene_t* s) { delete s; }
uint64_t rth_num_tris(const rth_scene_t* s) { return s->scene.tris.size(); }

int rth_add_triangle(rth_scene_t* s, const float* p, uint32_t kind, const float* c, float alpha, float scat, float edge) {
    return guarded([&] {
        const Vec3 pts[3] = {v3(p), v3(p + 3), v3(p + 6)};
        s->scene.tris.push_back(make_triangle(pts, surf(kind, c, alpha, scat), edge));
        s->scene.touch();
    });
}
int rth_add_obj(rth_scene_t* s, const char* path, const float* off, float scale, const float* b9, uint32_t kind,
                const float* c, float alpha, float scat, float edge) {
    return rth_add_obj_mode(s, path, off, scale, b9, kind, c, alpha, scat, edge, 0);
}
int rth_add_obj_mode(rth_scene_t* s, const char* path, const float* off, float scale, const float* b9, uint32_t kind,
                     const float* c, float alpha, float scat, float edge, uint32_t robust) {
    return guarded([&] {
        auto t = obj_parser::parse_obj(path, v3(off), scale, std::make_tuple(v3(b9), v3(b9 + 3), v3(b9 + 6)),
                                       surf(kind, c, alpha, scat), edge, robust ? obj_parser::ObjMode::Robust : obj_parser::ObjMode::Reference);
        s->scene.tris.insert(s->scene.tris.end(), t.begin(), t.end());
        s->scene.touch();
    });
}
// rth_add_obj_mode, and (normals = 1) the file's vn normals for the new triangles, or (normals = 2) generated ones
// (rtmi_smooth_normals over the new triangles with crease_cos)
int rth_add_obj_normals(rth_scene_t* s, const char* path, const float* off, float scale, const float* b9, uint32_t kind, const float* c,
                        float alpha, float scat, float edge, uint32_t robust, uint32_t normals, float crease_cos) {
    if (normals == 0) return rth_add_obj_mode(s, path, off, scale, b9, kind, c, alpha, scat, edge, robust);
    if (normals > 2) return guarded([] { throw std::runtime_error("rth_add_obj_normals: normals must be 0 (none), 1 (file) or 2 (smooth)"); });
    if (normals == 2 && !(crease_cos >= -1.f && crease_cos <= 1.f))
        return guarded([] { throw std::runtime_error("smooth_normals: crease_cos must be in [-1, 1]"); });
    const uint64_t first = s->scene.tris.size();
    uint64_t count = 0;
    const int rc = guarded([&] {
        std::vector<float> n9;
        auto t = obj_parser::parse_obj(path, v3(off), scale, std::make_tuple(v3(b9), v3(b9 + 3), v3(b9 + 6)), surf(kind, c, alpha, scat), edge,
                                       robust ? obj_parser::ObjMode::Robust : obj_parser::ObjMode::Reference, normals == 1 ? &n9 : nullptr);
        count = t.size();
        if (first == 0 && count) throw std::runtime_error("vertex normals: the scene needs its sentinel triangle first");
        s->scene.tris.insert(s->scene.tris.end(), t.begin(), t.end());
        s->scene.touch();
        if (normals == 1 && count) {
            for (float x : n9)
                if (!std::isfinite(x)) throw std::runtime_error("parse_obj: a vn normal is zero or not finite");
            std::vector<float>& v = s->scene.normals;
            v.resize((first + count) * 9, 0.f);
            std::copy(n9.begin(), n9.end(), v.begin() + first * 9);
            s->scene.normals_generation++;
        }
    });
    if (rc != 0 || normals != 2 || count == 0) return rc;
    return rth_scene_smooth_normals(s, first, count, crease_cos);
}
int rth_add_disk(rth_scene_t* s, const float* orig3, const float* norm3, float r, float d, uint64_t n, uint32_t kind,
                 const float* c, float alpha, float scat, uint32_t skind, const float* sc, float salpha, float sscat, float edge) {
    return guarded([&] {
        auto t = make_disk(v3(orig3), v3(norm3), r, d, (size_t)n, surf(kind, c, alpha, scat), surf(skind, sc, salpha, sscat), edge);
        s->scene.tris.insert(s->scene.tris.end(), t.begin(), t.end());
        s->scene.touch();
    });
}
int rth_add_sphere(rth_scene_t* s, const float* orig3, float r, uint64_t nlat, uint64_t nlon, uint32_t kind, const float* c,
                   float alpha, float scat, float edge) {
    return guarded([&] {
        auto t = make_sphere(v3(orig3), r, {(size_t)nlat, (size_t)nlon}, surf(kind, c, alpha, scat), edge);
        s->scene.tris.insert(s->scene.tris.end(), t.begin(), t.end());
        s->scene.touch();
    });
}
int rth_add_triangles_gpu(rth_scene_t* s, const float* p, uint64_t n, uint32_t kind, const float* c, float alpha, float scat,
                          float edge, int device) {
    return guarded([&] {
        std::vector<Vec3> corners(n * 3);
        for (uint64_t i = 0; i < n * 3; i++) corners[i] = v3(p + 3 * i);
        auto t = make_triangles_gpu(corners, surf(kind, c, alpha, scat), edge, device);
        s->scene.tris.insert(s->scene.tris.end(), t.begin(), t.end());
        s->scene.touch();
    });
}
int rth_add_analytic_sphere(rth_scene_t* s, const float* center3, float r, uint32_t kind, const float* c, float alpha, float scat) {
    return guarded([&] {
        s->scene.spheres.push_back(Sphere{v3(center3), r, surf(kind, c, alpha, scat)});
        s->scene.touch();
    });
}
int rth_scene_set_environment(rth_scene_t* s, const float* rgb, uint32_t n, const float* frame9) {
    return guarded([&] {
        if (!rgb || n == 0) { s->scene.environment.reset(); s->scene.env_generation++; return; }
        if (n > 4096) throw std::runtime_error("environment: n must be 1 to 4096");
        Environment e;
        e.n = n;
        for (int k = 0; frame9 && k < 9; k++) {
            if (!std::isfinite(frame9[k])) throw std::runtime_error("environment: frame entry " + std::to_string(k) + " is not finite");
            e.frame[k] = frame9[k];
        }
        e.rgb.assign(rgb, rgb + (size_t)n * n * 3);
        s->scene.environment = std::move(e);
        s->scene.env_generation++;
    });
}
int rth_scene_set_sky(rth_scene_t* s, uint32_t n, const rtmi_sky_t* sky) {
    return guarded([&] {
        if (n < 1 || n > 4096) throw std::runtime_error("sky: n must be 1 to 4096");
        Environment e;
        e.n = n;
        e.generated = true;
        rtmi_sky_defaults(&e.sky);
        if (sky) e.sky = *sky;
        auto usable = [](const float* v) {
            return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]) && (v[0] != 0.f || v[1] != 0.f || v[2] != 0.f);
        };
        if (!usable(e.sky.up)) throw std::runtime_error("sky: up must be finite and not zero");
        if (!usable(e.sky.sun_dir)) throw std::runtime_error("sky: sun_dir must be finite and not zero");
        s->scene.environment = std::move(e);
        s->scene.env_generation++;
    });
}
int rth_scene_environment_size(const rth_scene_t* s, uint32_t* n_out) {
    *n_out = s->scene.environment ? s->scene.environment->n : 0u;
    return 0;
}
int rth_caster_environment(rth_scene_t* s, float* rgb_out, uint64_t cap_floats, uint32_t* n_out) {
    return guarded([&] {
        uint32_t n = 0;
        const std::vector<float> rgb = caster_of(s).environment(s->scene, n);
        if (rgb.size() > cap_floats) throw std::runtime_error("rth_caster_environment: the buffer is too small");
        if (!rgb.empty()) memcpy(rgb_out, rgb.data(), rgb.size() * sizeof(float));
        *n_out = n;
    });
}
// [first, first + count) clipped to the scene's triangles; count = UINT64_MAX: to the end.  The sentinel (0) is not a triangle.
static void normals_range(const rth_scene_t* s, uint64_t first, uint64_t& count, const std::string& what = "vertex normals") {
    const uint64_t n = s->scene.tris.size();
    if (first < 1 || first > n) throw std::runtime_error(what + ": first must be 1 to the number of triangles");
    if (count == UINT64_MAX) count = n - first;
    if (count > n - first) throw std::runtime_error(what + ": the range ends beyond the last triangle");
}
int rth_scene_set_normals(rth_scene_t* s, const float* normals9, uint64_t first, uint64_t count) {
    return guarded([&] {
        if (!normals9) { s->scene.normals.clear(); s->scene.normals_generation++; return; }
        normals_range(s, first, count);
        for (uint64_t k = 0; k < count * 9; k++)
            if (!std::isfinite(normals9[k])) throw std::runtime_error("vertex normals: a normal of triangle " + std::to_string(first + k / 9) + " is not finite");
        std::vector<float>& v = s->scene.normals;
        if (v.size() < (first + count) * 9) v.resize((first + count) * 9, 0.f);
        std::copy(normals9, normals9 + count * 9, v.begin() + first * 9);
        s->scene.normals_generation++;
    });
}
int rth_scene_smooth_normals(rth_scene_t* s, uint64_t first, uint64_t count, float crease_cos) {
    return guarded([&] {
        normals_range(s, first, count);
        std::vector<float> corners(count * 9), fn(count * 3), out(count * 9);
        for (uint64_t i = 0; i < count; i++) {
            const Triangle& t = s->scene.tris[first + i];
            for (int k = 0; k < 3; k++) memcpy(&corners[9 * i + 3 * k], t.corners[k].v, 12);
            memcpy(&fn[3 * i], t.norm.v, 12);
        }
        if (rtmi_smooth_normals(corners.data(), fn.data(), count, crease_cos, out.data()) != RTMI_OK)
            throw std::runtime_error(std::string("rtmi_smooth_normals: ") + rtmi_last_error());
        for (float x : out)
            if (!std::isfinite(x)) throw std::runtime_error("smooth_normals: a generated normal is not finite (a degenerate triangle?)");
        std::vector<float>& v = s->scene.normals;
        if (v.size() < (first + count) * 9) v.resize((first + count) * 9, 0.f);
        std::copy(out.begin(), out.end(), v.begin() + first * 9);
        s->scene.normals_generation++;
    });
}
int rth_scene_normals_size(const rth_scene_t* s, uint64_t* n_out) {
    *n_out = s->scene.normals.empty() ? 0u : s->scene.tris.size();
    return 0;
}
int rth_scene_get_normals(const rth_scene_t* s, float* normals9_out, uint64_t cap_floats) {
    return guarded([&] {
        const size_t want = s->scene.normals.empty() ? 0 : s->scene.tris.size() * 9;
        if (want > cap_floats) throw std::runtime_error("rth_scene_get_normals: the buffer is too small");
        std::fill(normals9_out, normals9_out + want, 0.f);
        std::copy(s->scene.normals.begin(), s->scene.normals.begin() + std::min(want, s->scene.normals.size()), normals9_out);
    });
}
int rth_caster_normals(rth_scene_t* s, float* normals9_out, uint64_t cap_floats, uint64_t* n_out) {
    return guarded([&] {
        const std::vector<float> v = caster_of(s).vertex_normals(s->scene);
        if (v.size() > cap_floats) throw std::runtime_error("rth_caster_normals: the buffer is too small");
        if (!v.empty()) memcpy(normals9_out, v.data(), v.size() * sizeof(float));
        *n_out = v.size() / 9;
    });
}
// --- textures (rtmi_scene_set_textures / rtmi_project_uvs in rtmi.h, which defines them)
static void uvs_grow(Scene& sc, uint64_t end) {
    if (sc.uvs.size() < end * 6) sc.uvs.resize(end * 6, 0.f);
    if (sc.tex_of_tri.size() < end) sc.tex_of_tri.resize(end, 0u);
}
int rth_scene_set_textures(rth_scene_t* s, const rtmi_texture_t* tex, uint32_t ntex) {
    return guarded([&] {
        Scene& sc = s->scene;
        if (!tex || ntex == 0) {  // everything goes: images, uvs, texture numbers
            sc.textures.clear(); sc.uvs.clear(); sc.tex_of_tri.clear(); sc.tex_generation++;
            sc.nmap_of_tri.clear(); sc.nmap_generation++;  // the maps name images by number
            return;
        }
        if (ntex > 256u) throw std::runtime_error("textures: more than 256 textures");
        uint64_t total = 0;
        std::vector<Scene::Texture> v(ntex);
        for (uint32_t k = 0; k < ntex; k++) {
            const std::string name = "textures: texture " + std::to_string(k + 1);
            if (tex[k].flags != 0u) throw std::runtime_error(name + " has flags != 0");
            if (!tex[k].rgb) throw std::runtime_error(name + " has no texels (rgb is NULL)");
            if (tex[k].width < 1u || tex[k].width > 8192u || tex[k].height < 1u || tex[k].height > 8192u)
                throw std::runtime_error(name + ": width and height must be 1 to 8192");
            total += (uint64_t)tex[k].width * tex[k].height;
            if (total > (1ull << 26)) throw std::runtime_error(name + ": more than 2^26 texels in all");
            v[k].width = tex[k].width; v[k].height = tex[k].height;
            v[k].rgb.assign(tex[k].rgb, tex[k].rgb + (size_t)tex[k].width * tex[k].height * 3);
        }
        for (size_t i = 1; i < sc.tex_of_tri.size(); i++)
            if (sc.tex_of_tri[i] > ntex) throw std::runtime_error("textures: tex_of_tri of triangle " + std::to_string(i) + " is above ntex");
        sc.textures = std::move(v);
        sc.tex_generation++;
        sc.nmap_of_tri.clear(); sc.nmap_generation++;  // the maps name images by number: new images, no maps
    });
}
int rth_scene_set_uvs(rth_scene_t* s, const float* uvs6, const uint32_t* tex_of_tri, uint64_t first, uint64_t count) {
    return guarded([&] {
        Scene& sc = s->scene;
        if (!uvs6 || !tex_of_tri) throw std::runtime_error("textures: uvs or tex_of_tri is NULL");
        normals_range(s, first, count, "textures");
        for (uint64_t i = 0; i < count; i++) {
            if (!sc.textures.empty() && tex_of_tri[i] > sc.textures.size())
                throw std::runtime_error("textures: tex_of_tri of triangle " + std::to_string(first + i) + " is above ntex");
            if (tex_of_tri[i] > 256u) throw std::runtime_error("textures: tex_of_tri of triangle " + std::to_string(first + i) + " is above 256");
            if (tex_of_tri[i] == 0u) continue;
            for (int k = 0; k < 6; k++)
                if (!std::isfinite(uvs6[6 * i + k])) throw std::runtime_error("textures: a uv of triangle " + std::to_string(first + i) + " is not finite");
        }
        uvs_grow(sc, first + count);
        std::copy(uvs6, uvs6 + count * 6, sc.uvs.begin() + first * 6);
        std::copy(tex_of_tri, tex_of_tri + count, sc.tex_of_tri.begin() + first);
        sc.tex_generation++;
    });
}
int rth_scene_project_uvs(rth_scene_t* s, uint64_t first, uint64_t count, const float* lo3, float scale, uint32_t texture) {
    return guarded([&] {
        Scene& sc = s->scene;
        normals_range(s, first, count, "textures");
        if (texture > 256u || (!sc.textures.empty() && texture > sc.textures.size())) throw std::runtime_error("textures: texture is above ntex");
        std::vector<float> corners(count * 9), fn(count * 3), out(count * 6);
        for (uint64_t i = 0; i < count; i++) {
            const Triangle& t = sc.tris[first + i];
            for (int k = 0; k < 3; k++) memcpy(&corners[9 * i + 3 * k], t.corners[k].v, 12);
            memcpy(&fn[3 * i], t.norm.v, 12);
        }
        if (rtmi_project_uvs(corners.data(), fn.data(), count, lo3, scale, out.data()) != RTMI_OK)
            throw std::runtime_error(std::string("rtmi_project_uvs: ") + rtmi_last_error());
        if (texture)
            for (float x : out)
                if (!std::isfinite(x)) throw std::runtime_error("project_uvs: a projected uv is not finite");
        uvs_grow(sc, first + count);
        std::copy(out.begin(), out.end(), sc.uvs.begin() + first * 6);
        std::fill(sc.tex_of_tri.begin() + first, sc.tex_of_tri.begin() + first + count, texture);
        sc.tex_generation++;
    });
}
int rth_scene_textures_size(const rth_scene_t* s, uint32_t* ntex_out, uint64_t* n_out) {
    *ntex_out = (uint32_t)s->scene.textures.size();
    *n_out = s->scene.textures.empty() && s->scene.uvs.empty() ? 0u : s->scene.tris.size();
    return 0;
}
int rth_scene_get_uvs(const rth_scene_t* s, float* uvs6_out, uint32_t* tex_of_tri_out, uint64_t cap_tris) {
    return guarded([&] {
        const Scene& sc = s->scene;
        const size_t n = sc.tris.size();
        if (n > cap_tris) throw std::runtime_error("rth_scene_get_uvs: the buffer is too small");
        std::fill(uvs6_out, uvs6_out + n * 6, 0.f);
        std::fill(tex_of_tri_out, tex_of_tri_out + n, 0u);
        std::copy(sc.uvs.begin(), sc.uvs.begin() + std::min(n * 6, sc.uvs.size()), uvs6_out);
        std::copy(sc.tex_of_tri.begin(), sc.tex_of_tri.begin() + std::min(n, sc.tex_of_tri.size()), tex_of_tri_out);
    });
}
int rth_scene_get_texture(const rth_scene_t* s, uint32_t k, float* rgb_out, uint64_t cap_floats, uint32_t* w_out, uint32_t* h_out) {
    return guarded([&] {
        const Scene& sc = s->scene;
        if (k < 1u || k > sc.textures.size()) throw std::runtime_error("rth_scene_get_texture: k must be 1 to the number of textures");
        const Scene::Texture& t = sc.textures[k - 1];
        *w_out = t.width; *h_out = t.height;
        if (!rgb_out) return;
        if (t.rgb.size() > cap_floats) throw std::runtime_error("rth_scene_get_texture: the buffer is too small");
        std::copy(t.rgb.begin(), t.rgb.end(), rgb_out);
    });
}
int rth_caster_uvs(rth_scene_t* s, float* uvs6_out, uint32_t* tex_of_tri_out, uint64_t cap_tris, uint64_t* n_out) {
    return guarded([&] {
        std::vector<float> uv;
        std::vector<uint32_t> tt;
        caster_of(s).texture_uvs(s->scene, uv, tt);
        if (tt.size() > cap_tris) throw std::runtime_error("rth_caster_uvs: the buffer is too small");
        if (!tt.empty()) {
            memcpy(uvs6_out, uv.data(), uv.size() * sizeof(float));
            memcpy(tex_of_tri_out, tt.data(), tt.size() * sizeof(uint32_t));
        }
        *n_out = tt.size();
    });
}
int rth_caster_texture(rth_scene_t* s, uint32_t k, float* rgb_out, uint64_t cap_floats, uint32_t* w_out, uint32_t* h_out) {
    return guarded([&] {
        const std::vector<float> v = caster_of(s).texture_image(s->scene, k, *w_out, *h_out);
        if (v.size() > cap_floats) throw std::runtime_error("rth_caster_texture: the buffer is too small");
        memcpy(rgb_out, v.data(), v.size() * sizeof(float));
    });
}
// rth_add_obj_mode, and the file's `vt` texture coordinates for the new triangles, which get texture number `texture`
int rth_add_obj_uvs(rth_scene_t* s, const char* path, const float* off, float scale, const float* b9, uint32_t kind, const float* c,
                    float alpha, float scat, float edge, uint32_t robust, uint32_t texture) {
    return guarded([&] {
        Scene& sc = s->scene;
        if (texture > 256u || (!sc.textures.empty() && texture > sc.textures.size())) throw std::runtime_error("textures: texture is above ntex");
        const uint64_t first = sc.tris.size();
        if (first == 0) throw std::runtime_error("textures: the scene needs its sentinel triangle first");
        std::vector<float> uv;
        auto t = obj_parser::parse_obj(path, v3(off), scale, std::make_tuple(v3(b9), v3(b9 + 3), v3(b9 + 6)), surf(kind, c, alpha, scat), edge,
                                       robust ? obj_parser::ObjMode::Robust : obj_parser::ObjMode::Reference, nullptr, &uv);
        for (float x : uv)
            if (!std::isfinite(x)) throw std::runtime_error("parse_obj: a vt texture coordinate is not finite");
        sc.tris.insert(sc.tris.end(), t.begin(), t.end());
        sc.touch();
        uvs_grow(sc, first + t.size());
        std::copy(uv.begin(), uv.end(), sc.uvs.begin() + first * 6);
        std::fill(sc.tex_of_tri.begin() + first, sc.tex_of_tri.end(), texture);
        sc.tex_generation++;
    });
}
// --- normal maps (rtmi_scene_set_normal_maps in rtmi.h, which defines them)
int rth_scene_set_normal_maps(rth_scene_t* s, const uint32_t* nmap_of_tri, uint64_t first, uint64_t count, float strength, uint32_t flags) {
    return guarded([&] {
        Scene& sc = s->scene;
        if (!nmap_of_tri || count == 0) {  // none
            sc.nmap_of_tri.clear(); sc.nmap_strength = 1.f; sc.nmap_generation++;
            return;
        }
        if (sc.textures.empty()) throw std::runtime_error("normal maps: the scene has no textures (a map is one of its images)");
        if (flags != 0u) throw std::runtime_error("normal maps: flags != 0");
        if (!std::isfinite(strength)) throw std::runtime_error("normal maps: strength is not finite");
        normals_range(s, first, count, "normal maps");
        for (uint64_t i = 0; i < count; i++)
            if (nmap_of_tri[i] > sc.textures.size())
                throw std::runtime_error("normal maps: nmap_of_tri of triangle " + std::to_string(first + i) + " is above ntex");
        if (sc.nmap_of_tri.size() < first + count) sc.nmap_of_tri.resize(first + count, 0u);
        std::copy(nmap_of_tri, nmap_of_tri + count, sc.nmap_of_tri.begin() + first);
        sc.nmap_strength = strength;
        sc.nmap_generation++;
    });
}
int rth_scene_normal_maps_size(const rth_scene_t* s, uint64_t* n_out) {
    *n_out = s->scene.nmap_of_tri.empty() ? 0u : s->scene.tris.size();
    return 0;
}
int rth_scene_get_normal_maps(const rth_scene_t* s, uint32_t* nmap_of_tri_out, float* strength_out, uint64_t cap_tris) {
    return guarded([&] {
        const Scene& sc = s->scene;
        const size_t n = sc.tris.size();
        if (n > cap_tris) throw std::runtime_error("rth_scene_get_normal_maps: the buffer is too small");
        std::fill(nmap_of_tri_out, nmap_of_tri_out + n, 0u);
        std::copy(sc.nmap_of_tri.begin(), sc.nmap_of_tri.begin() + std::min(n, sc.nmap_of_tri.size()), nmap_of_tri_out);
        *strength_out = sc.nmap_strength;
    });
}
// rtmi_normal_map_frames over the scene's triangles, with its corners, uvs and records' normals: what a device stores
int rth_scene_normal_map_frames(const rth_scene_t* s, float* frames4_out, uint64_t cap_tris) {
    return guarded([&] {
        const Scene& sc = s->scene;
        const size_t n = sc.tris.size();
        if (n > cap_tris) throw std::runtime_error("rth_scene_normal_map_frames: the buffer is too small");
        std::vector<float> corners(n * 9, 0.f), fn(n * 3, 0.f), uvs(n * 6, 0.f);
        std::vector<uint32_t> nm(n, 0u);
        for (size_t i = 1; i < n; i++) {
            for (int k = 0; k < 3; k++) memcpy(&corners[9 * i + 3 * k], sc.tris[i].corners[k].v, 12);
            memcpy(&fn[3 * i], sc.tris[i].norm.v, 12);
        }
        std::copy(sc.uvs.begin(), sc.uvs.begin() + std::min(sc.uvs.size(), uvs.size()), uvs.begin());
        std::copy(sc.nmap_of_tri.begin(), sc.nmap_of_tri.begin() + std::min(n, sc.nmap_of_tri.size()), nm.begin());
        std::fill(frames4_out, frames4_out + n * 4, 0.f);
        if (n > 1 && rtmi_normal_map_frames(corners.data() + 9, uvs.data() + 6, fn.data() + 3, nm.data() + 1, n - 1, frames4_out + 4) != RTMI_OK)
            throw std::runtime_error(std::string("rtmi_normal_map_frames: ") + rtmi_last_error());
    });
}
int rth_caster_normal_maps(rth_scene_t* s, uint32_t* nmap_of_tri_out, float* strength_out, uint64_t cap_tris, uint64_t* n_out) {
    return guarded([&] {
        float strength = 0.f;
        const std::vector<uint32_t> v = caster_of(s).normal_maps(s->scene, strength);
        if (v.size() > cap_tris) throw std::runtime_error("rth_caster_normal_maps: the buffer is too small");
        if (!v.empty()) memcpy(nmap_of_tri_out, v.data(), v.size() * sizeof(uint32_t));
        *strength_out = strength;
        *n_out = v.size();
    });
}
int rth_normal_map_from_height(const float* height, uint32_t w, uint32_t h, float scale, float* rgb_out) {
    return guarded([&] {
        if (rtmi_normal_map_from_height(height, w, h, scale, rgb_out) != RTMI_OK)
            throw std::runtime_error(std::string("rtmi_normal_map_from_height: ") + rtmi_last_error());
    });
}
void rth_populate_triangle_numbers(rth_scene_t* s) { populate_triangle_numbers(s->scene.tris); s->scene.touch(); }

int rth_build_bounding_box(rth_scene_t* s, const float* orig3, float len2, uint64_t maxdepth, uint64_t minobjs, uint32_t threads) {
    return guarded([&] {
        s->scene.boxes = build_bounding_box(s->scene.tris, v3(orig3), len2, (size_t)maxdepth, (size_t)minobjs, threads);
        s->scene.touch();
    });
}
int rth_build_bounding_box_gpu(rth_scene_t* s, const float* orig3, float len2, uint64_t maxdepth, uint64_t minobjs, int device) {
    return guarded([&] {
        s->scene.boxes = build_bounding_box_gpu(s->scene.tris, v3(orig3), len2, (size_t)maxdepth, (size_t)minobjs, device);
        s->scene.touch();
    });
}
int rth_build_trivial_bounding_box(rth_scene_t* s, const float* orig3, float len2) {
    return guarded([&] {
        s->scene.boxes = build_trivial_bounding_box(s->scene.tris, v3(orig3), len2);
        s->scene.touch();
    });
}
int rth_box_contains_polygon(const rth_scene_t* s, const float* orig3, float len2, uint64_t tri) {
    return box_contains_polygon(v3(orig3), len2, s->scene.tris.at(tri)) ? 1 : 0;
}
int rth_face_contains_triangle(const rth_scene_t* s, const float* p3, const float* norm3, float len2, uint64_t tri) {
    return face_contains_triangle(v3(p3), v3(norm3), len2, s->scene.tris.at(tri)) ? 1 : 0;
}

void rth_get_triangles(const rth_scene_t* s, float* out, int32_t* kinds, float* sf) {
    const auto& tris = s->scene.tris;
    for (size_t i = 0; i < tris.size(); i++) {
        const Triangle& t = tris[i];
        float* o = out + i * 29;
        memcpy(o, t.incenter.v, 12); memcpy(o + 3, t.norm.v, 12);
        o[6] = t.bounding_r2;
        for (int k = 0; k < 3; k++) { memcpy(o + 7 + 3 * k, t.sides[k].v, 12); o[16 + k] = t.side_lens[k]; memcpy(o + 20 + 3 * k, t.corners[k].v, 12); }
        o[19] = t.edge_thickness;
        kinds[i] = (int32_t)t.surface.tag;
        memcpy(sf + i * 5, t.surface.color.v, 12);
        sf[i * 5 + 3] = t.surface.alpha; sf[i * 5 + 4] = t.surface.scattering;
    }
}
void rth_tree_sizes(const rth_scene_t* s, uint64_t* nboxes, uint64_t* nrefs) {
    *nboxes = s->scene.boxes.boxes.size(); *nrefs = s->scene.boxes.tri_refs.size();
}
void rth_tree_get(const rth_scene_t* s, float* geo, uint32_t* topo, uint32_t* refs) {
    const auto& bb = s->scene.boxes;
    for (size_t i = 0; i < bb.boxes.size(); i++) {
        const rtmi_box_t& b = bb.boxes[i];
        memcpy(geo + i * 4, b.orig, 12); geo[i * 4 + 3] = b.len2;
        topo[i * 4] = b.first; topo[i * 4 + 1] = b.count; topo[i * 4 + 2] = b.is_leaf; topo[i * 4 + 3] = b.depth;
    }
    if (!bb.tri_refs.empty()) memcpy(refs, bb.tri_refs.data(), bb.tri_refs.size() * 4);
}

int rth_caster_config(rth_scene_t* s, uint64_t seed, int device, uint32_t options) {
    return guarded([&] {
        HipRayCaster& c = caster_of(s);
        if (c.device != device) { c.invalidate(); c.device = device; }
        c.seed = seed;
        c.set_options(options);
    });
}
int rth_caster_set_devices(rth_scene_t* s, const int32_t* devices, uint32_t n) {
    return guarded([&] { caster_of(s).set_devices(std::vector<int>(devices, devices + n)); });
}
int rth_caster_walk_frame_multi(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp,
                                uint32_t stripe_rows, uint32_t flags, void* out_host, void* out_device, rtmi_stats_t* stats,
                                rtmi_stats_t* per_device, uint32_t per_device_cap, double* wall) {
    return guarded([&] {
        const Viewport v = vp_from(w, h, vp12, maxdepth, spp);
        ProgressCtx ctx;
        std::vector<rtmi_stats_t> pd;
        const auto t0 = std::chrono::steady_clock::now();
        caster_of(s).walk_frame_multi(v, s->scene, out_host, out_device, stripe_rows, flags, ctx, &pd);
        if (wall) *wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (stats) *stats = ctx.stats;
        for (uint32_t k = 0; per_device && k < per_device_cap && k < pd.size(); k++) per_device[k] = pd[k];
    });
}
int rth_caster_set_tuning(rth_scene_t* s, const rtmi_tuning_t* t) {
    return guarded([&] {
        if (t) caster_of(s).set_tuning(*t);
        else caster_of(s).clear_tuning();
    });
}
int rth_caster_upload(rth_scene_t* s) { return guarded([&] { caster_of(s).resident(s->scene); }); }

int rth_caster_walk_rows(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp,
                         uint64_t row0, uint64_t nrows, float* out_host, rtmi_stats_t* stats, double* wall) {
    return guarded([&] {
        const Viewport v = vp_from(w, h, vp12, maxdepth, spp);
        ProgressCtx ctx;
        const auto t0 = std::chrono::steady_clock::now();
        caster_of(s).walk_rows(v, s->scene, (size_t)row0, (size_t)nrows, reinterpret_cast<Color*>(out_host), ctx);
        if (wall) *wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (stats) *stats = ctx.stats;
    });
}
int rth_caster_walk_rows_device(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp,
                                uint64_t row0, uint64_t nrows, void* out_device, void* hip_stream, rtmi_stats_t* stats, double* wall) {
    return guarded([&] {
        const Viewport v = vp_from(w, h, vp12, maxdepth, spp);
        ProgressCtx ctx;
        const auto t0 = std::chrono::steady_clock::now();
        caster_of(s).walk_rows_device(v, s->scene, (size_t)row0, (size_t)nrows, out_device, hip_stream, ctx);
        if (wall) *wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (stats) *stats = ctx.stats;
    });
}
int rth_caster_walk_tile_device(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp,
                                const rtmi_tile_t* tile, void* out_device, void* hip_stream, rtmi_stats_t* stats, double* wall) {
    return guarded([&] {
        const Viewport v = vp_from(w, h, vp12, maxdepth, spp);
        ProgressCtx ctx;
        const auto t0 = std::chrono::steady_clock::now();
        caster_of(s).walk_tile_device(v, s->scene, *tile, out_device, hip_stream, ctx);
        if (wall) *wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (stats) *stats = ctx.stats;
    });
}
int rth_caster_walk_samples(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp,
                            uint64_t row0, uint64_t nrows, uint32_t sample0, uint32_t nsamples, float* accum_host, float* out_host,
                            rtmi_stats_t* stats, double* wall) {
    return guarded([&] {
        const Viewport v = vp_from(w, h, vp12, maxdepth, spp);
        ProgressCtx ctx;
        const auto t0 = std::chrono::steady_clock::now();
        caster_of(s).walk_samples(v, s->scene, (size_t)row0, (size_t)nrows, sample0, nsamples, reinterpret_cast<Color*>(accum_host),
                                  reinterpret_cast<Color*>(out_host), ctx);
        if (wall) *wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (stats) *stats = ctx.stats;
    });
}
int rth_caster_walk_samples_device(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp,
                                   const rtmi_tile_t* tile, uint32_t sample0, uint32_t nsamples, void* accum_device,
                                   void* out_device, void* hip_stream, rtmi_stats_t* stats, double* wall) {
    return guarded([&] {
        if (!tile) throw std::runtime_error("NULL tile");
        const Viewport v = vp_from(w, h, vp12, maxdepth, spp);
        ProgressCtx ctx;
        const auto t0 = std::chrono::steady_clock::now();
        caster_of(s).walk_samples_device(v, s->scene, *tile, sample0, nsamples, accum_device, out_device, hip_stream, ctx);
        if (wall) *wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (stats) *stats = ctx.stats;
    });
}
int rth_caster_walk_features(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp,
                             uint64_t row0, uint64_t nrows, uint32_t sample0, uint32_t nsamples, float* albedo_host,
                             float* normal_host, uint32_t* ids_host, rtmi_stats_t* stats, double* wall) {
    return guarded([&] {
        const Viewport v = vp_from(w, h, vp12, maxdepth, spp);
        ProgressCtx ctx;
        const auto t0 = std::chrono::steady_clock::now();
        caster_of(s).walk_rays_features(v, s->scene, (size_t)row0, (size_t)nrows, sample0, nsamples, reinterpret_cast<Color*>(albedo_host),
                                        reinterpret_cast<Color*>(normal_host), ids_host, ctx);
        if (wall) *wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (stats) *stats = ctx.stats;
    });
}
int rth_caster_walk_features_device(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp,
                                    const rtmi_tile_t* tile, uint32_t sample0, uint32_t nsamples, void* albedo_device,
                                    void* normal_device, void* ids_device, void* hip_stream, rtmi_stats_t* stats, double* wall) {
    return guarded([&] {
        if (!tile) throw std::runtime_error("NULL tile");
        const Viewport v = vp_from(w, h, vp12, maxdepth, spp);
        ProgressCtx ctx;
        const auto t0 = std::chrono::steady_clock::now();
        caster_of(s).walk_features_device(v, s->scene, *tile, sample0, nsamples, albedo_device, normal_device, ids_device, hip_stream, ctx);
        if (wall) *wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (stats) *stats = ctx.stats;
    });
}
int rth_caster_walk_ao(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp, uint64_t row0,
                       uint64_t nrows, uint32_t sample0, uint32_t nsamples, const rtmi_ao_t* ao, float* ao_host, rtmi_stats_t* stats,
                       double* wall) {
    return guarded([&] {
        if (!ao) throw std::runtime_error("NULL rtmi_ao_t");
        const Viewport v = vp_from(w, h, vp12, maxdepth, spp);
        ProgressCtx ctx;
        const auto t0 = std::chrono::steady_clock::now();
        caster_of(s).walk_rays_ao(v, s->scene, (size_t)row0, (size_t)nrows, sample0, nsamples, *ao, ao_host, ctx);
        if (wall) *wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (stats) *stats = ctx.stats;
    });
}
int rth_caster_walk_ao_device(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp,
                              const rtmi_tile_t* tile, uint32_t sample0, uint32_t nsamples, const rtmi_ao_t* ao, void* ao_device,
                              void* hip_stream, rtmi_stats_t* stats, double* wall) {
    return guarded([&] {
        if (!tile) throw std::runtime_error("NULL tile");
        if (!ao) throw std::runtime_error("NULL rtmi_ao_t");
        const Viewport v = vp_from(w, h, vp12, maxdepth, spp);
        ProgressCtx ctx;
        const auto t0 = std::chrono::steady_clock::now();
        caster_of(s).walk_ao_device(v, s->scene, *tile, sample0, nsamples, *ao, ao_device, hip_stream, ctx);
        if (wall) *wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (stats) *stats = ctx.stats;
    });
}
int rth_caster_walk_light(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp, uint64_t row0,
                          uint64_t nrows, uint32_t sample0, uint32_t nsamples, const rtmi_light_t* light, float* shadow_host,
                          float* irradiance_host, rtmi_stats_t* stats, double* wall) {
    return guarded([&] {
        if (!light) throw std::runtime_error("NULL rtmi_light_t");
        const Viewport v = vp_from(w, h, vp12, maxdepth, spp);
        const LightSource ls{make_vec(light->orig), light->len2};
        ProgressCtx ctx;
        const auto t0 = std::chrono::steady_clock::now();
        caster_of(s).walk_rays_light(v, s->scene, (size_t)row0, (size_t)nrows, sample0, nsamples, ls, light->rays, light->flags, light->bias,
                                     shadow_host, irradiance_host, ctx);
        if (wall) *wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (stats) *stats = ctx.stats;
    });
}
int rth_caster_walk_light_device(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp,
                                 const rtmi_tile_t* tile, uint32_t sample0, uint32_t nsamples, const rtmi_light_t* light,
                                 void* shadow_device, void* irradiance_device, void* hip_stream, rtmi_stats_t* stats, double* wall) {
    return guarded([&] {
        if (!tile) throw std::runtime_error("NULL tile");
        if (!light) throw std::runtime_error("NULL rtmi_light_t");
        const Viewport v = vp_from(w, h, vp12, maxdepth, spp);
        const LightSource ls{make_vec(light->orig), light->len2};
        ProgressCtx ctx;
        const auto t0 = std::chrono::steady_clock::now();
        caster_of(s).walk_light_device(v, s->scene, *tile, sample0, nsamples, ls, light->rays, light->flags, light->bias, shadow_device,
                                       irradiance_device, hip_stream, ctx);
        if (wall) *wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (stats) *stats = ctx.stats;
    });
}
int rth_caster_walk_shadowed(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp, uint64_t row0,
                             uint64_t nrows, uint32_t sample0, uint32_t nsamples, const rtmi_light_t* light, float* accum_host,
                             float* out_host, rtmi_stats_t* stats, double* wall) {
    return guarded([&] {
        if (!light) throw std::runtime_error("NULL rtmi_light_t");
        if (light->rays != 1) throw std::runtime_error("shadowed: rays must be 1 (the reference draws one shadow ray per hit)");
        const Viewport v = vp_from(w, h, vp12, maxdepth, spp);
        s->scene.light = LightSource{make_vec(light->orig), light->len2};  // the reference's Scene.light; not uploaded, no touch()
        ProgressCtx ctx;
        const auto t0 = std::chrono::steady_clock::now();
        caster_of(s).walk_rays_shadowed(v, s->scene, (size_t)row0, (size_t)nrows, sample0, nsamples, light->flags, light->bias,
                                        reinterpret_cast<Color*>(accum_host), reinterpret_cast<Color*>(out_host), ctx);
        if (wall) *wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (stats) *stats = ctx.stats;
    });
}
int rth_caster_walk_shadowed_device(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp,
                                    const rtmi_tile_t* tile, uint32_t sample0, uint32_t nsamples, const rtmi_light_t* light,
                                    void* accum_device, void* out_device, void* hip_stream, rtmi_stats_t* stats, double* wall) {
    return guarded([&] {
        if (!tile) throw std::runtime_error("NULL tile");
        if (!light) throw std::runtime_error("NULL rtmi_light_t");
        if (light->rays != 1) throw std::runtime_error("shadowed: rays must be 1 (the reference draws one shadow ray per hit)");
        const Viewport v = vp_from(w, h, vp12, maxdepth, spp);
        s->scene.light = LightSource{make_vec(light->orig), light->len2};
        ProgressCtx ctx;
        const auto t0 = std::chrono::steady_clock::now();
        caster_of(s).walk_shadowed_device(v, s->scene, *tile, sample0, nsamples, light->flags, light->bias, accum_device, out_device,
                                          hip_stream, ctx);
        if (wall) *wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (stats) *stats = ctx.stats;
    });
}
static rtmi_envlight_t envlight_or_defaults(const rtmi_envlight_t* env) {
    rtmi_envlight_t e;
    rtmi_envlight_defaults(&e);
    if (env) e = *env;
    return e;
}
int rth_caster_walk_envlight(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp, uint64_t row0,
                             uint64_t nrows, uint32_t sample0, uint32_t nsamples, const rtmi_envlight_t* env, float* accum_host,
                             float* out_host, rtmi_stats_t* stats, double* wall) {
    return guarded([&] {
        const Viewport v = vp_from(w, h, vp12, maxdepth, spp);
        ProgressCtx ctx;
        const auto t0 = std::chrono::steady_clock::now();
        caster_of(s).walk_rays_envlight(v, s->scene, (size_t)row0, (size_t)nrows, sample0, nsamples, envlight_or_defaults(env),
                                        reinterpret_cast<Color*>(accum_host), reinterpret_cast<Color*>(out_host), ctx);
        if (wall) *wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (stats) *stats = ctx.stats;
    });
}
int rth_caster_walk_envlight_device(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp,
                                    const rtmi_tile_t* tile, uint32_t sample0, uint32_t nsamples, const rtmi_envlight_t* env,
                                    void* accum_device, void* out_device, void* hip_stream, rtmi_stats_t* stats, double* wall) {
    return guarded([&] {
        if (!tile) throw std::runtime_error("NULL tile");
        const Viewport v = vp_from(w, h, vp12, maxdepth, spp);
        ProgressCtx ctx;
        const auto t0 = std::chrono::steady_clock::now();
        caster_of(s).walk_envlight_device(v, s->scene, *tile, sample0, nsamples, envlight_or_defaults(env), accum_device, out_device,
                                          hip_stream, ctx);
        if (wall) *wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (stats) *stats = ctx.stats;
    });
}
int rth_caster_walk_lit(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp, uint64_t row0,
                        uint64_t nrows, uint32_t sample0, uint32_t nsamples, const rtmi_lit_t* lit, float* accum_host, float* out_host,
                        rtmi_stats_t* stats, double* wall) {
    return guarded([&] {
        if (!lit) throw std::runtime_error("NULL rtmi_lit_t");
        const Viewport v = vp_from(w, h, vp12, maxdepth, spp);
        ProgressCtx ctx;
        const auto t0 = std::chrono::steady_clock::now();
        caster_of(s).walk_rays_lit(v, s->scene, (size_t)row0, (size_t)nrows, sample0, nsamples, *lit, reinterpret_cast<Color*>(accum_host),
                                   reinterpret_cast<Color*>(out_host), ctx);
        if (wall) *wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (stats) *stats = ctx.stats;
    });
}
int rth_caster_walk_lit_device(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp,
                               const rtmi_tile_t* tile, uint32_t sample0, uint32_t nsamples, const rtmi_lit_t* lit, void* accum_device,
                               void* out_device, void* hip_stream, rtmi_stats_t* stats, double* wall) {
    return guarded([&] {
        if (!tile) throw std::runtime_error("NULL tile");
        if (!lit) throw std::runtime_error("NULL rtmi_lit_t");
        const Viewport v = vp_from(w, h, vp12, maxdepth, spp);
        ProgressCtx ctx;
        const auto t0 = std::chrono::steady_clock::now();
        caster_of(s).walk_lit_device(v, s->scene, *tile, sample0, nsamples, *lit, accum_device, out_device, hip_stream, ctx);
        if (wall) *wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (stats) *stats = ctx.stats;
    });
}
// --- emitters (rtmi_scene_set_emitters in rtmi.h, which defines them)
int rth_scene_set_emitters(rth_scene_t* s, const uint8_t* emit_of_tri, uint64_t first, uint64_t count) {
    return guarded([&] {
        Scene& sc = s->scene;
        if (!emit_of_tri || count == 0) { sc.emitters.clear(); sc.emit_generation++; return; }
        normals_range(s, first, count, "emitters");
        for (uint64_t i = 0; i < count; i++)
            if (emit_of_tri[i] && sc.tris[first + i].surface.tag != RTMI_SOLID)
                throw std::runtime_error("emitters: triangle " + std::to_string(first + i) + " is marked and its surface is not Solid");
        if (sc.emitters.size() < first + count) sc.emitters.resize(first + count, 0);
        for (uint64_t i = 0; i < count; i++) sc.emitters[first + i] = emit_of_tri[i] ? 1 : 0;
        sc.emit_generation++;
    });
}
int rth_scene_get_emitters(const rth_scene_t* s, uint8_t* emit_of_tri_out, uint64_t cap_tris) {
    return guarded([&] {
        const Scene& sc = s->scene;
        const size_t n = sc.tris.size();
        if (n > cap_tris) throw std::runtime_error("rth_scene_get_emitters: the buffer is too small");
        std::fill(emit_of_tri_out, emit_of_tri_out + n, (uint8_t)0);
        std::copy(sc.emitters.begin(), sc.emitters.begin() + std::min(n, sc.emitters.size()), emit_of_tri_out);
    });
}
int rth_caster_walk_emissive(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp, uint64_t row0,
                             uint64_t nrows, uint32_t sample0, uint32_t nsamples, float* accum_host, float* out_host, rtmi_stats_t* stats,
                             double* wall) {
    return guarded([&] {
        const Viewport v = vp_from(w, h, vp12, maxdepth, spp);
        ProgressCtx ctx;
        const auto t0 = std::chrono::steady_clock::now();
        caster_of(s).walk_rays_emissive(v, s->scene, (size_t)row0, (size_t)nrows, sample0, nsamples, reinterpret_cast<Color*>(accum_host),
                                        reinterpret_cast<Color*>(out_host), ctx);
        if (wall) *wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (stats) *stats = ctx.stats;
    });
}
int rth_caster_walk_emissive_device(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp,
                                    const rtmi_tile_t* tile, uint32_t sample0, uint32_t nsamples, void* accum_device, void* out_device,
                                    void* hip_stream, rtmi_stats_t* stats, double* wall) {
    return guarded([&] {
        if (!tile) throw std::runtime_error("NULL tile");
        const Viewport v = vp_from(w, h, vp12, maxdepth, spp);
        ProgressCtx ctx;
        const auto t0 = std::chrono::steady_clock::now();
        caster_of(s).walk_emissive_device(v, s->scene, *tile, sample0, nsamples, accum_device, out_device, hip_stream, ctx);
        if (wall) *wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (stats) *stats = ctx.stats;
    });
}
// The lamps' tables of the resident copy; sizes first (every pointer but nlamps_out NULL), then the copy
int rth_caster_emitter_sampler(rth_scene_t* s, uint32_t* q_out, uint64_t* cum_out, uint32_t* lamp_of_tri_out, float* lamps_out,
                               uint64_t cap_lamps, uint64_t cap_tris, uint64_t* total_out, uint32_t* nlamps_out) {
    return guarded([&] {
        if (!nlamps_out) throw std::runtime_error("rth_caster_emitter_sampler: NULL nlamps_out");
        const HipRayCaster::EmitterSampler e = caster_of(s).emitter_sampler(s->scene);
        *nlamps_out = (uint32_t)e.q.size();
        if (total_out) *total_out = e.total;
        if (!q_out && !cum_out && !lamp_of_tri_out && !lamps_out) return;
        if (e.q.size() > cap_lamps || e.lamp_of_tri.size() > cap_tris) throw std::runtime_error("rth_caster_emitter_sampler: the buffer is too small");
        if (q_out && !e.q.empty()) memcpy(q_out, e.q.data(), e.q.size() * sizeof(uint32_t));
        if (cum_out && !e.cum.empty()) memcpy(cum_out, e.cum.data(), e.cum.size() * sizeof(uint64_t));
        if (lamp_of_tri_out && !e.lamp_of_tri.empty()) memcpy(lamp_of_tri_out, e.lamp_of_tri.data(), e.lamp_of_tri.size() * sizeof(uint32_t));
        if (lamps_out && !e.lamps.empty()) memcpy(lamps_out, e.lamps.data(), e.lamps.size() * sizeof(float));
    });
}
int rth_caster_env_sampler(rth_scene_t* s, uint32_t* q_out, uint64_t cap, uint64_t* total_out, uint32_t* n_out) {
    return guarded([&] {
        if (!n_out) throw std::runtime_error("rth_caster_env_sampler: NULL n_out");
        uint32_t n = 0;
        uint64_t total = 0;
        const std::vector<uint32_t> q = caster_of(s).env_sampler(s->scene, n, total);
        if (q_out && q.size() > cap) throw std::runtime_error("rth_caster_env_sampler: the buffer is too small");
        if (q_out && !q.empty()) memcpy(q_out, q.data(), q.size() * sizeof(uint32_t));
        if (total_out) *total_out = total;
        *n_out = n;
    });
}
int rth_caster_walk_camera(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp, uint64_t row0,
                           uint64_t nrows, const rtmi_camera_t* camera, uint32_t sample0, uint32_t nsamples, float* accum_host,
                           float* out_host, const rtmi_camera_out_t* guides_host, rtmi_stats_t* stats, double* wall) {
    return guarded([&] {
        if (!camera) throw std::runtime_error("NULL rtmi_camera_t");
        const Viewport v = vp_from(w, h, vp12, maxdepth, spp);
        ProgressCtx ctx;
        const auto t0 = std::chrono::steady_clock::now();
        caster_of(s).walk_rays_camera(v, s->scene, (size_t)row0, (size_t)nrows, *camera, sample0, nsamples, reinterpret_cast<Color*>(accum_host),
                                      reinterpret_cast<Color*>(out_host), guides_host, ctx);
        if (wall) *wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (stats) *stats = ctx.stats;
    });
}
int rth_caster_walk_camera_device(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp,
                                  const rtmi_tile_t* tile, const rtmi_camera_t* camera, uint32_t sample0, uint32_t nsamples,
                                  void* accum_device, void* out_device, const rtmi_camera_out_t* guides, void* hip_stream,
                                  rtmi_stats_t* stats, double* wall) {
    return guarded([&] {
        if (!tile) throw std::runtime_error("NULL tile");
        if (!camera) throw std::runtime_error("NULL rtmi_camera_t");
        const Viewport v = vp_from(w, h, vp12, maxdepth, spp);
        ProgressCtx ctx;
        const auto t0 = std::chrono::steady_clock::now();
        caster_of(s).walk_camera_device(v, s->scene, *tile, *camera, sample0, nsamples, accum_device, out_device, guides, hip_stream, ctx);
        if (wall) *wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (stats) *stats = ctx.stats;
    });
}
int rth_caster_walk_preview(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp, uint64_t row0,
                            uint64_t nrows, uint32_t sample0, uint32_t nsamples, const rtmi_preview_t* preview,
                            const rtmi_preview_out_t* out_host, rtmi_stats_t* stats, double* wall) {
    return guarded([&] {
        if (!preview) throw std::runtime_error("NULL rtmi_preview_t");
        if (!out_host) throw std::runtime_error("NULL rtmi_preview_out_t");
        const Viewport v = vp_from(w, h, vp12, maxdepth, spp);
        ProgressCtx ctx;
        const auto t0 = std::chrono::steady_clock::now();
        caster_of(s).walk_rays_preview(v, s->scene, (size_t)row0, (size_t)nrows, sample0, nsamples, *preview, *out_host, ctx);
        if (wall) *wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (stats) *stats = ctx.stats;
    });
}
int rth_caster_walk_preview_device(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp,
                                   const rtmi_tile_t* tile, uint32_t sample0, uint32_t nsamples, const rtmi_preview_t* preview,
                                   const rtmi_preview_out_t* out_device, void* hip_stream, rtmi_stats_t* stats, double* wall) {
    return guarded([&] {
        if (!tile) throw std::runtime_error("NULL tile");
        if (!preview) throw std::runtime_error("NULL rtmi_preview_t");
        if (!out_device) throw std::runtime_error("NULL rtmi_preview_out_t");
        const Viewport v = vp_from(w, h, vp12, maxdepth, spp);
        ProgressCtx ctx;
        const auto t0 = std::chrono::steady_clock::now();
        caster_of(s).walk_preview_device(v, s->scene, *tile, sample0, nsamples, *preview, *out_device, hip_stream, ctx);
        if (wall) *wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (stats) *stats = ctx.stats;
    });
}
int rth_caster_denoise(rth_scene_t* s, uint32_t w, uint32_t h, const float* color_host, const float* albedo_host,
                       const float* normal_host, const rtmi_denoise_t* params, float* out_host) {
    return guarded([&] {
        if (!params) throw std::runtime_error("NULL rtmi_denoise_t");
        caster_of(s).denoise(s->scene, w, h, reinterpret_cast<const Color*>(color_host), reinterpret_cast<const Color*>(albedo_host),
                             reinterpret_cast<const Color*>(normal_host), *params, reinterpret_cast<Color*>(out_host));
    });
}
int rth_caster_denoise_device(rth_scene_t* s, uint32_t w, uint32_t h, const void* color_device, const void* albedo_device,
                              const void* normal_device, const rtmi_denoise_t* params, void* out_device, void* hip_stream) {
    return guarded([&] {
        if (!params) throw std::runtime_error("NULL rtmi_denoise_t");
        caster_of(s).denoise_device(s->scene, w, h, color_device, albedo_device, normal_device, *params, out_device, hip_stream);
    });
}
int rth_caster_walk_denoised(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp,
                             const rtmi_denoise_t* params, float* out_host, rtmi_stats_t* stats, double* wall) {
    return guarded([&] {
        if (!params) throw std::runtime_error("NULL rtmi_denoise_t");
        const Viewport v = vp_from(w, h, vp12, maxdepth, spp);
        ProgressCtx ctx;
        const auto t0 = std::chrono::steady_clock::now();
        caster_of(s).walk_rays_denoised(v, s->scene, *params, reinterpret_cast<Color*>(out_host), ctx);
        if (wall) *wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (stats) *stats = ctx.stats;
    });
}
int rth_caster_variance(rth_scene_t* s, const float* accum_host, const float* sumsq_host, const uint32_t* counts_host,
                        uint64_t npixels, float* variance_host) {
    return guarded([&] {
        caster_of(s).variance(s->scene, reinterpret_cast<const Color*>(accum_host), reinterpret_cast<const Color*>(sumsq_host),
                              counts_host, npixels, reinterpret_cast<Color*>(variance_host));
    });
}
int rth_caster_variance_device(rth_scene_t* s, const void* accum_device, const void* sumsq_device, const void* counts_device,
                               uint64_t npixels, void* variance_device, void* hip_stream) {
    return guarded([&] { caster_of(s).variance_device(s->scene, accum_device, sumsq_device, counts_device, npixels, variance_device, hip_stream); });
}
int rth_caster_denoise_var(rth_scene_t* s, uint32_t w, uint32_t h, const float* color_host, const float* albedo_host,
                           const float* normal_host, const float* variance_host, const rtmi_denoise_t* params, float* out_host,
                           float* var_out_host) {
    return guarded([&] {
        if (!params) throw std::runtime_error("NULL rtmi_denoise_t");
        caster_of(s).denoise_var(s->scene, w, h, reinterpret_cast<const Color*>(color_host), reinterpret_cast<const Color*>(albedo_host),
                                 reinterpret_cast<const Color*>(normal_host), reinterpret_cast<const Color*>(variance_host), *params,
                                 reinterpret_cast<Color*>(out_host), reinterpret_cast<Color*>(var_out_host));
    });
}
int rth_caster_denoise_var_device(rth_scene_t* s, uint32_t w, uint32_t h, const void* color_device, const void* albedo_device,
                                  const void* normal_device, const void* variance_device, const rtmi_denoise_t* params,
                                  void* out_device, void* var_out_device, void* hip_stream) {
    return guarded([&] {
        if (!params) throw std::runtime_error("NULL rtmi_denoise_t");
        caster_of(s).denoise_var_device(s->scene, w, h, color_device, albedo_device, normal_device, variance_device, *params, out_device,
                                        var_out_device, hip_stream);
    });
}
int rth_caster_walk_adaptive_denoised(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp,
                                      rtmi_adaptive_t* ad, const rtmi_denoise_t* params, float* out_host, uint32_t* counts_host,
                                      rtmi_stats_t* stats, double* wall) {
    return guarded([&] {
        if (!ad) throw std::runtime_error("NULL rtmi_adaptive_t");
        if (!params) throw std::runtime_error("NULL rtmi_denoise_t");
        const Viewport v = vp_from(w, h, vp12, maxdepth, spp);
        ProgressCtx ctx;
        const auto t0 = std::chrono::steady_clock::now();
        caster_of(s).walk_adaptive_denoised(v, s->scene, *ad, *params, reinterpret_cast<Color*>(out_host), counts_host, ctx);
        if (wall) *wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (stats) *stats = ctx.stats;
    });
}
int rth_caster_walk_adaptive(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp,
                             uint64_t row0, uint64_t nrows, rtmi_adaptive_t* ad, float* out_host, uint32_t* counts_host,
                             rtmi_stats_t* stats, double* wall) {
    return guarded([&] {
        if (!ad) throw std::runtime_error("NULL rtmi_adaptive_t");
        const Viewport v = vp_from(w, h, vp12, maxdepth, spp);
        ProgressCtx ctx;
        const auto t0 = std::chrono::steady_clock::now();
        caster_of(s).walk_adaptive(v, s->scene, (size_t)row0, (size_t)nrows, *ad, reinterpret_cast<Color*>(out_host), counts_host, ctx);
        if (wall) *wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (stats) *stats = ctx.stats;
    });
}
int rth_caster_walk_adaptive_device(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp,
                                    const rtmi_tile_t* tile, rtmi_adaptive_t* ad, void* accum_device, void* sumsq_device,
                                    void* counts_device, void* out_device, void* hip_stream, rtmi_stats_t* stats, double* wall) {
    return guarded([&] {
        if (!tile) throw std::runtime_error("NULL tile");
        if (!ad) throw std::runtime_error("NULL rtmi_adaptive_t");
        const Viewport v = vp_from(w, h, vp12, maxdepth, spp);
        ProgressCtx ctx;
        const auto t0 = std::chrono::steady_clock::now();
        caster_of(s).walk_adaptive_device(v, s->scene, *tile, *ad, accum_device, sumsq_device, counts_device, out_device,
                                          hip_stream, ctx);
        if (wall) *wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (stats) *stats = ctx.stats;
    });
}
// the views of a batch: nviews viewports of one size, vp12s = 12 floats per view
static std::vector<Viewport> views_from(uint32_t nviews, uint32_t w, uint32_t h, const float* vp12s, uint64_t maxdepth, uint64_t spp) {
    if (nviews && !vp12s) throw std::runtime_error("NULL viewports");
    std::vector<Viewport> views;
    for (uint32_t k = 0; k < nviews; k++) views.push_back(vp_from(w, h, vp12s + 12 * (size_t)k, maxdepth, spp));
    return views;
}
int rth_caster_walk_views(rth_scene_t* s, uint32_t nviews, uint32_t w, uint32_t h, const float* vp12s, uint64_t maxdepth, uint64_t spp,
                          const uint64_t* seeds, float* out_host, rtmi_stats_t* stats, double* wall) {
    return guarded([&] {
        const std::vector<Viewport> views = views_from(nviews, w, h, vp12s, maxdepth, spp);
        const std::vector<uint64_t> sd = seeds ? std::vector<uint64_t>(seeds, seeds + nviews) : std::vector<uint64_t>();
        ProgressCtx ctx;
        const auto t0 = std::chrono::steady_clock::now();
        caster_of(s).walk_views(views, s->scene, sd, reinterpret_cast<Color*>(out_host), ctx);
        if (wall) *wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (stats) *stats = ctx.stats;
    });
}
int rth_caster_walk_views_device(rth_scene_t* s, uint32_t nviews, uint32_t w, uint32_t h, const float* vp12s, uint64_t maxdepth,
                                 uint64_t spp, const uint64_t* seeds, const rtmi_tile_t* tile, void* out_device, void* hip_stream,
                                 rtmi_stats_t* stats, double* wall) {
    return guarded([&] {
        if (!tile) throw std::runtime_error("NULL tile");
        const std::vector<Viewport> views = views_from(nviews, w, h, vp12s, maxdepth, spp);
        const std::vector<uint64_t> sd = seeds ? std::vector<uint64_t>(seeds, seeds + nviews) : std::vector<uint64_t>();
        ProgressCtx ctx;
        const auto t0 = std::chrono::steady_clock::now();
        caster_of(s).walk_views_device(views, s->scene, sd, *tile, out_device, hip_stream, ctx);
        if (wall) *wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (stats) *stats = ctx.stats;
    });
}
int rth_caster_occluded(rth_scene_t* s, uint64_t n, const float* o4, const float* d4, const float* tmax, uint8_t* occluded,
                        rtmi_stats_t* stats) {
    return guarded([&] { caster_of(s).occluded(s->scene, n, o4, d4, tmax, occluded, stats); });
}
int rth_caster_occluded_device(rth_scene_t* s, uint64_t n, const void* orig4_device, const void* dir4_device, const void* tmax_device,
                               void* occluded_device, void* hip_stream, rtmi_stats_t* stats) {
    return guarded([&] { caster_of(s).occluded_device(s->scene, n, orig4_device, dir4_device, tmax_device, occluded_device, hip_stream, stats); });
}
int rth_caster_trace(rth_scene_t* s, uint64_t n, const float* o4, const float* d4, uint32_t* tri, float* t, uint32_t* face,
                     rtmi_stats_t* stats) {
    return guarded([&] {
        rtmi_scene_t* h = caster_of(s).resident(s->scene);
        if (rtmi_trace(h, n, o4, d4, tri, t, face, stats) != RTMI_OK)
            throw std::runtime_error(std::string("rtmi_trace: ") + rtmi_last_error());
    });
}

int rth_caster_trace_device(rth_scene_t* s, uint64_t n, const void* orig4_device, const void* dir4_device, void* tri_device, void* t_device,
                            void* face_device, void* hip_stream, rtmi_stats_t* stats) {
    return guarded([&] { caster_of(s).trace_device(s->scene, n, orig4_device, dir4_device, tri_device, t_device, face_device, hip_stream, stats); });
}
int rth_caster_walk_rays_explicit(rth_scene_t* s, uint64_t n, const float* o4, const float* d4, const uint32_t* keys, const rtmi_rays_t* rays,
                                  const rtmi_rays_out_t* out_host, rtmi_stats_t* stats, double* wall) {
    return guarded([&] {
        ProgressCtx ctx;
        const auto t0 = std::chrono::steady_clock::now();
        caster_of(s).walk_rays_explicit(s->scene, n, o4, d4, keys, rays, out_host, ctx);
        if (wall) *wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (stats) *stats = ctx.stats;
    });
}
int rth_caster_walk_rays_explicit_device(rth_scene_t* s, uint64_t n, const void* orig4_device, const void* dir4_device, const void* keys_device,
                                         const rtmi_rays_t* rays, const rtmi_rays_out_t* out_device, void* hip_stream, rtmi_stats_t* stats,
                                         double* wall) {
    return guarded([&] {
        ProgressCtx ctx;
        const auto t0 = std::chrono::steady_clock::now();
        caster_of(s).walk_rays_explicit_device(s->scene, n, orig4_device, dir4_device, keys_device, rays, out_device, hip_stream, ctx);
        if (wall) *wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (stats) *stats = ctx.stats;
    });
}

int rth_caster_bake(rth_scene_t* s, uint64_t M, const float* pos4, const float* nrm4, const rtmi_bake_t* bake, const rtmi_bake_out_t* out_host,
                    rtmi_stats_t* stats, double* wall) {
    return guarded([&] {
        if (!bake || !out_host) throw std::runtime_error("NULL bake or out");
        ProgressCtx ctx;
        const auto t0 = std::chrono::steady_clock::now();
        caster_of(s).bake(s->scene, M, pos4, nrm4, *bake, *out_host, ctx);
        if (wall) *wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (stats) *stats = ctx.stats;
    });
}
int rth_caster_bake_device(rth_scene_t* s, uint64_t M, const void* pos4_device, const void* nrm4_device, const rtmi_bake_t* bake,
                           const rtmi_bake_out_t* out_device, void* hip_stream, rtmi_stats_t* stats, double* wall) {
    return guarded([&] {
        if (!bake || !out_device) throw std::runtime_error("NULL bake or out");
        ProgressCtx ctx;
        const auto t0 = std::chrono::steady_clock::now();
        caster_of(s).bake_device(s->scene, M, pos4_device, nrm4_device, *bake, *out_device, hip_stream, ctx);
        if (wall) *wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (stats) *stats = ctx.stats;
    });
}

int rth_caster_walk_rays_explicit_lit(rth_scene_t* s, uint64_t n, const float* o4, const float* d4, const uint32_t* keys, const rtmi_rays_t* rays,
                                      const rtmi_lit_t* lit, const rtmi_rays_out_t* out_host, rtmi_stats_t* stats, double* wall) {
    return guarded([&] {
        ProgressCtx ctx;
        const auto t0 = std::chrono::steady_clock::now();
        caster_of(s).walk_rays_explicit_lit(s->scene, n, o4, d4, keys, rays, lit, out_host, ctx);
        if (wall) *wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (stats) *stats = ctx.stats;
    });
}
int rth_caster_walk_rays_explicit_lit_device(rth_scene_t* s, uint64_t n, const void* orig4_device, const void* dir4_device,
                                             const void* keys_device, const rtmi_rays_t* rays, const rtmi_lit_t* lit,
                                             const rtmi_rays_out_t* out_device, void* hip_stream, rtmi_stats_t* stats, double* wall) {
    return guarded([&] {
        ProgressCtx ctx;
        const auto t0 = std::chrono::steady_clock::now();
        caster_of(s).walk_rays_explicit_lit_device(s->scene, n, orig4_device, dir4_device, keys_device, rays, lit, out_device, hip_stream, ctx);
        if (wall) *wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (stats) *stats = ctx.stats;
    });
}
int rth_caster_bake_lit(rth_scene_t* s, uint64_t M, const float* pos4, const float* nrm4, const rtmi_bake_t* bake, const rtmi_lit_t* lit,
                        const rtmi_bake_lit_out_t* out_host, rtmi_stats_t* stats, double* wall) {
    return guarded([&] {
        if (!bake || !lit || !out_host) throw std::runtime_error("NULL bake, lit or out");
        ProgressCtx ctx;
        const auto t0 = std::chrono::steady_clock::now();
        caster_of(s).bake_lit(s->scene, M, pos4, nrm4, *bake, *lit, *out_host, ctx);
        if (wall) *wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (stats) *stats = ctx.stats;
    });
}
int rth_caster_bake_lit_device(rth_scene_t* s, uint64_t M, const void* pos4_device, const void* nrm4_device, const rtmi_bake_t* bake,
                               const rtmi_lit_t* lit, const rtmi_bake_lit_out_t* out_device, void* hip_stream, rtmi_stats_t* stats, double* wall) {
    return guarded([&] {
        if (!bake || !lit || !out_device) throw std::runtime_error("NULL bake, lit or out");
        ProgressCtx ctx;
        const auto t0 = std::chrono::steady_clock::now();
        caster_of(s).bake_lit_device(s->scene, M, pos4_device, nrm4_device, *bake, *lit, *out_device, hip_stream, ctx);
        if (wall) *wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (stats) *stats = ctx.stats;
    });
}

int rth_caster_trace_records(rth_scene_t* s, uint64_t n, const float* o4, const float* d4, rtmi_ray_record_t* recs, uint32_t* leaf_ids,
                             uint64_t leaf_cap, uint64_t* leaf_total, rtmi_stats_t* stats) {
    return guarded([&] {
        rtmi_scene_t* h = caster_of(s).resident(s->scene);
        if (rtmi_trace_records(h, n, o4, d4, recs, leaf_ids, leaf_cap, leaf_total, stats) != RTMI_OK)
            throw std::runtime_error(std::string("rtmi_trace_records: ") + rtmi_last_error());
    });
}
int rth_caster_primary_records(rth_scene_t* s, uint32_t w, uint32_t h, const float* vp12, uint64_t maxdepth, uint64_t spp,
                               uint32_t row0, uint32_t nrows, uint32_t sample, rtmi_ray_record_t* recs, uint32_t* leaf_ids,
                               uint64_t leaf_cap, uint64_t* leaf_total, rtmi_stats_t* stats) {
    return guarded([&] {
        const rtmi_viewport_t av = to_abi(vp_from(w, h, vp12, maxdepth, spp));
        HipRayCaster& c = caster_of(s);
        if (rtmi_primary_records(c.resident(s->scene), &av, c.seed, row0, nrows, sample, recs, leaf_ids, leaf_cap, leaf_total, stats) != RTMI_OK)
            throw std::runtime_error(std::string("rtmi_primary_records: ") + rtmi_last_error());
    });
}
int rth_scene_set_debug(rth_scene_t* s, int on) {
    return guarded([&] { s->scene.debug_en = on != 0; });
}
int rth_scene_debug_records(rth_scene_t* s, rtmi_ray_record_t* recs, uint32_t* pixel2, uint32_t* leaf_ids, uint64_t* nrecs,
                            uint64_t* nleaf_ids) {
    return guarded([&] {
        if (!nrecs || !nleaf_ids) throw std::runtime_error("NULL size argument");
        const RayRecords& d = s->scene.debug;
        *nrecs = d.recs.size();
        *nleaf_ids = d.leaf_ids.size();
        if (recs && !d.recs.empty()) memcpy(recs, d.recs.data(), d.recs.size() * sizeof(rtmi_ray_record_t));
        if (leaf_ids && !d.leaf_ids.empty()) memcpy(leaf_ids, d.leaf_ids.data(), d.leaf_ids.size() * 4);
        if (pixel2)
            for (size_t i = 0; i < d.pixel.size(); i++) { pixel2[2 * i] = d.pixel[i].first; pixel2[2 * i + 1] = d.pixel[i].second; }
    });
}

int rth_caster_quantize_device(rth_scene_t* s, const void* rgba_device, uint64_t npixels, void* rgb_device, void* hip_stream) {
    return guarded([&] {
        if (rtmi_quantize_device(caster_of(s).resident(s->scene), rgba_device, npixels, rgb_device, hip_stream) != RTMI_OK)
            throw std::runtime_error(std::string("rtmi_quantize_device: ") + rtmi_last_error());
    });
}

// development aid (tools/step_stats.py); not declared in rtmi_host.h
int rtmi_debug_counters(rtmi_scene_t* s, unsigned long long* out16);
int rth_debug_counters(rth_scene_t* s, unsigned long long* out16) {
    return guarded([&] { rtmi_debug_counters(caster_of(s).resident(s->scene), out16); });
}
int rtmi_debug_counters_n(rtmi_scene_t* s, unsigned long long* out, int n);
int rth_debug_counters_n(rth_scene_t* s, unsigned long long* out, int n) {
    return guarded([&] { rtmi_debug_counters_n(caster_of(s).resident(s->scene), out, n); });
}

int rtmi_debug_cert_stats(const rtmi_scene_t* s, unsigned long long* out);
int rth_debug_cert_stats(rth_scene_t* s, unsigned long long* out) {
    return guarded([&] { rtmi_debug_cert_stats(caster_of(s).resident(s->scene), out); });
}

int rtmi_debug_node_cull_stats(const rtmi_scene_t* s, unsigned long long* out);
int rth_debug_node_cull_stats(rth_scene_t* s, unsigned long long* out) {
    return guarded([&] { rtmi_debug_node_cull_stats(caster_of(s).resident(s->scene), out); });
}

// the statistics of the hybrid passes (device/hybrid.hpp) of the last batch of the resident scene's last call
int rtmi_debug_hybrid_counters(rtmi_scene_t* s, unsigned long long* out12, int* on);
int rth_debug_hybrid_counters(rth_scene_t* s, unsigned long long* out12, int* on) {
    int rc = 0;
    const int g = guarded([&] { rc = rtmi_debug_hybrid_counters(caster_of(s).resident(s->scene), out12, on); });
    return g ? g : rc;
}
// ... and of the shadow walks' own workspace (rtmi_render_shadowed* / _lit* / _envlight* / _emissive*)
int rtmi_debug_shadow_hybrid_counters(rtmi_scene_t* s, unsigned long long* out12);
int rth_debug_shadow_hybrid_counters(rth_scene_t* s, unsigned long long* out12) {
    int rc = 0;
    const int g = guarded([&] { rc = rtmi_debug_shadow_hybrid_counters(caster_of(s).resident(s->scene), out12); });
    return g ? g : rc;
}

void rth_quantize(const float* rgba, uint64_t npixels, uint8_t* rgb) {
    quantize_rgb8(reinterpret_cast<const Color*>(rgba), (size_t)npixels, rgb);
}

}  // extern "C"
