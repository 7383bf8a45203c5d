// shade.hpp — primary-ray generation and shading of one traced ray: Viewport::pixel_ray (raytrace_lib/src/raytrace.rs:
// 1374-1394), color_ray + the tail of project_ray (raytrace.rs:1199-1295), lambertian_ray / reflect_ray / random_vec /
// mix_color (raytrace.rs:278-301, :188-192) as device functions, shared by the per-pass kernels of rtmi_device.hip
// (k_gen, k_shade) and by the path kernels of trace_oct.hpp (k_path_primary, k_path_slow), so that every kernel that
// shades a ray executes the same arithmetic.  4-lane V4 values in the reference's operation order (vec4.hpp).
// Included by rtmi_device.hip.
#pragma once

namespace rtmi {

// Division of a u32 by a divisor that is constant for a launch (samples per pixel, image width, stripe height), without
// the ~40-instruction software division: Granlund & Montgomery, "Division by invariant integers using multiplication"
// (1994), figure 4.1 -- exact for every n < 2^32 and every d >= 1:
//   l = ceil(log2 d), m' = floor(2^32 (2^l - d) / d) + 1, sh1 = min(l, 1), sh2 = max(l - 1, 0)
//   q = (t + ((n - t) >> sh1)) >> sh2  with  t = mulhi(m', n)
struct FastDiv { uint32_t mul, sh1, sh2, d; };
inline FastDiv make_fastdiv(uint32_t d) {
    FastDiv f{1u, 0u, 0u, d ? d : 1u};
    uint32_t l = 0;
    while (l < 32 && (1ull << l) < f.d) l++;
    f.mul = (uint32_t)((((1ull << l) - f.d) << 32) / f.d) + 1u;
    f.sh1 = l < 1u ? l : 1u;
    f.sh2 = l > 0u ? l - 1u : 0u;
    return f;
}
__host__ __device__ inline uint32_t fdiv(uint32_t n, const FastDiv& f) {
    const uint32_t t = mulhi32(f.mul, n);
    return (t + ((n - t) >> f.sh1)) >> f.sh2;
}

struct DView {
    V4 orig, cam, vu, vv;
    uint32_t width, height, maxdepth, spp;         // spp: samples per pixel of THIS call (paths per pixel of a batch)
    uint32_t row0, stripe_rows, stripe_step;       // rtmi_tile_t: which image rows the tile's rows are
    // Samp::PASS / LIST only (the whole-frame kernels never read it): bits 0-30 sample0, the frame's sample number of the
    // call's first sample; bit 31 set when the FRAME has more than one sample per pixel (spp_frame != 1: pixel_ray
    // jitters).  view_set_sampling() fills it.
    uint32_t sample_key;
    uint32_t sub_mul, sub_off;                     // sub-tile of a stream: rows sub_off, sub_off + sub_mul, ... of the tile
    FastDiv dspp, dwidth, dstripe;                 // n / spp, n / width, n / stripe_rows
};
#define RTMI_KEY_JITTER 0x80000000u
inline void view_set_sampling(DView& v, uint32_t sample0, uint32_t spp_frame) {
    v.sample_key = sample0 | (spp_frame != 1u ? RTMI_KEY_JITTER : 0u);
}
inline void view_set_divisors(DView& v) {
    v.dspp = make_fastdiv(v.spp);
    v.dwidth = make_fastdiv(v.width);
    v.dstripe = make_fastdiv(v.stripe_rows);
}

// local pixel index of the sub-tile (row-major over ITS rows) -> image (row, col).  Row lr of the sub-tile is row
// lr * sub_mul + sub_off of the tile; row L of the tile is image row row0 + (L / stripe_rows) * stripe_step + L % stripe_rows.
__device__ inline void tile_pixel(const DView& v, uint32_t lp, uint32_t& row, uint32_t& col) {
    const uint32_t lr = fdiv(lp, v.dwidth);
    col = lp - lr * v.width;
    const uint32_t L = lr * v.sub_mul + v.sub_off;
    const uint32_t k = fdiv(L, v.dstripe);
    row = v.row0 + k * v.stripe_step + (L - k * v.stripe_rows);
}

// Sampling mode of a batch.  FRAME: all samples of the call's pixels (sample0 = 0, and the kernels do not spend the add and
// the register on it: 2 % of config 3's frame time when they did).  PASS: a progressive pass, samples [sample0, sample0 + spp)
// of its pixels (DView::sample_key).  LIST: an adaptive pass, a PASS whose pixels are entries pix0, pix0 + 1, ... of the
// active-pixel list, each a tile-local pixel index (row-major over the tile's rows; the launch's DView has sub_mul = 1,
// sub_off = 0).  The list pointer is an argument of the list kernels only, so the other kernels keep their launch constants.
// VIEWS: a batch of views of one scene (rtmi_render_views*), FRAME semantics over a stacked image whose row
// k * height + r is row r of view k; each view has its own camera and seed (ViewTab, an argument of the views kernels only).
// RAYS: caller-supplied rays (rtmi_render_rays*).  There is no camera and no tile: path i of a batch is its i-th
// ray and its RNG key comes from rays_key() below.  No generation kernel and no path kernel exists for this mode; only
// shade_pass is instantiated for it (k_shade_rays), in a branch of its own, so the other modes keep the code they had.
enum class Samp { FRAME, PASS, LIST, VIEWS, RAYS };
// Samp::VIEWS: view k's camera (lane 3 of every vector +0, as mk() makes them) and seed
struct VCam { float4 orig, cam, vu, vv; unsigned long long seed; uint32_t pad[2]; };
// the view table of a VIEWS launch: one VCam per view, and n / height (height = the rows of ONE view, DView::height)
struct ViewTab { const VCam* __restrict__ cams; FastDiv dh; };
// Samp::VIEWS: what the RNG and pixel_ray see of image row `row` of the stacked image -- its view k = row / height and its row
// inside that view -- and (key_seed) the view's seed.  Pixel (row, col) of the stack is then pixel key.row * width + col of
// view key.view, the RNG key of rtmi_render's call for that view.  The other modes render one view: view 0, the row itself,
// the launch's seed.  The callers compute the pixel key and read the seed where they pass them on, in the order they always
// did, so that those modes compile to the code they had before views existed (LLVM's reassociation orders the Philox
// xors by where their operands are defined).
struct PixKey { uint32_t view, row; };
template <Samp S>
__device__ inline PixKey pixel_key(const DView& v, uint32_t row, const ViewTab& vt) {
    if constexpr (S == Samp::VIEWS) {
        const uint32_t k = fdiv(row, vt.dh);
        return PixKey{k, row - k * v.height};
    } else {
        return PixKey{0u, row};
    }
}
template <Samp S>
__device__ inline uint64_t key_seed(const PixKey& key, const ViewTab& vt, uint64_t seed) {
    if constexpr (S == Samp::VIEWS) return vt.cams[key.view].seed;
    else return seed;
}
// path index of a batch that starts at local pixel pix0 -> image pixel index (row * width + col) and the FRAME's sample
// number (the RNG key)
template <Samp S>
__device__ inline void path_pixel(const DView& v, uint32_t pix0, uint32_t path, uint32_t& row, uint32_t& col, uint32_t& sample,
                                  const uint32_t* __restrict__ list) {
    const uint32_t q = fdiv(path, v.dspp);
    sample = (S != Samp::FRAME && S != Samp::VIEWS ? (v.sample_key & ~RTMI_KEY_JITTER) : 0u) + (path - q * v.spp);
    tile_pixel(v, S == Samp::LIST ? list[pix0 + q] : pix0 + q, row, col);
}

// Samp::RAYS: the RNG key (pixel, sample) of path `path` of a batch.  keys != null: the caller's pair for that ray (the batch's
// slice of the n x 2 array).  Otherwise rays come in groups of G = v.spp consecutive rays, group g of the batch is "pixel"
// pix0 + g (pix0: the key of the batch's first group) and a ray's sample is its place in its group.
__device__ inline void rays_key(const DView& v, uint32_t pix0, uint32_t path, const uint32_t* __restrict__ keys, uint32_t& pixel,
                                uint32_t& sample) {
    if (keys) {
        pixel = keys[2u * path];
        sample = keys[2u * path + 1u];
    } else {
        const uint32_t g = fdiv(path, v.dspp);
        pixel = pix0 + g;
        sample = path - g * v.spp;
    }
}

struct RayV { V4 orig, dir; };
// make_ray (raytrace.rs:201-210); inv_dir is recomputed by the trace kernel
__device__ inline RayV make_ray(V4 orig, V4 dir) { return RayV{orig, vunit(dir)}; }

// Viewport::pixel_ray (raytrace.rs:1374-1394), px = (row, col).  The centred ray is the rule of a 1-sample FRAME: a
// pass of one sample of a larger frame (Samp::PASS / LIST) is jittered like every other sample of it.  Samp::VIEWS: (row, col)
// inside the view, whose camera is `cam` (FRAME's rule; width and height are shared by the views).
template <Samp S>
__device__ inline RayV pixel_ray(const DView& v, uint32_t row, uint32_t col, uint64_t seed, uint32_t pixel, uint32_t sample,
                                 const VCam* cam = nullptr) {
    auto v4 = [](float4 a) { return V4{a.x, a.y, a.z, a.w}; };
    float px_x = (float)row, px_y = (float)col;
    V4 vu_delta = vmul(S == Samp::VIEWS ? v4(cam->vu) : v.vu, 1.f / (float)v.width);
    V4 vv_delta = vmul(S == Samp::VIEWS ? v4(cam->vv) : v.vv, 1.f / (float)v.height);
    float u_off = 0.5f, v_off = 0.5f;
    if (S != Samp::FRAME && S != Samp::VIEWS ? (v.sample_key & RTMI_KEY_JITTER) != 0u : v.spp != 1) {  // spp_frame != 1
        uint32_t w[4];
        rng_block(seed, pixel, sample, 0, w);
        u_off = u32_to_unit_f32(w[0]);
        v_off = u32_to_unit_f32(w[1]);
    }
    V4 vu_frac = vmul(vu_delta, px_y + u_off);
    V4 vv_frac = vmul(vv_delta, px_x + v_off);
    V4 px_u = vadd(vadd(S == Samp::VIEWS ? v4(cam->orig) : v.orig, vu_frac), vv_frac);
    return make_ray(px_u, vunit(vsub(px_u, S == Samp::VIEWS ? v4(cam->cam) : v.cam)));
}

// random_vec (raytrace.rs:188-192): k-th call of the path uses RNG block k
__device__ inline V4 random_vec(uint64_t seed, uint32_t pixel, uint32_t sample, uint32_t k) {
    uint32_t w[4];
    rng_block(seed, pixel, sample, k, w);
    return vunit(mk(u32_to_unit_f32(w[0]) - 0.5f, u32_to_unit_f32(w[1]) - 0.5f, u32_to_unit_f32(w[2]) - 0.5f));
}
// random_vec that also hands out word 3 of its block as a unit float: the dielectric's reflect-or-refract draw (include/rtmi.h,
// RTMI_DIELECTRIC).  random_vec never reads that word, so the draw costs no block and moves no other draw.
__device__ inline V4 random_vec_u(uint64_t seed, uint32_t pixel, uint32_t sample, uint32_t k, float& u3) {
    uint32_t w[4];
    rng_block(seed, pixel, sample, k, w);
    u3 = u32_to_unit_f32(w[3]);
    return vunit(mk(u32_to_unit_f32(w[0]) - 0.5f, u32_to_unit_f32(w[1]) - 0.5f, u32_to_unit_f32(w[2]) - 0.5f));
}
// mix_color (raytrace.rs:299-301)
__device__ inline V4 mix_color(V4 c1, V4 c2, float a) { return vadd(vmul(c1, 1.f - a), vmul(c2, a)); }

// The environment of a scene (rtmi_scene_set_environment / rtmi_scene_set_sky, include/rtmi.h): an n x n table of
// one float4 per texel (lane 3 +0) over the octahedral map of the directions, texel (i, j) at tab[j * n + i], and the rows of the
// frame that takes a world direction to map space (lane 3 +0).  An argument of the k_shade*_env kernels only, as ViewTab and the
// pixel list are of theirs: DScene, and with it every other kernel's argument block, stays as it is.
struct EnvTab { const float4* __restrict__ tab; uint32_t n; float fn; float4 r0, r1, r2; };
// the octahedral map's fold of the lower hemisphere (m.z < 0) over the outer triangles of the square, and its own inverse: both
// results from the OLD values
__device__ inline void oct_fold(float& px, float& py) {
    const float ox = px, oy = py;
    px = (1.f - fabsf(oy)) * (ox >= 0.f ? 1.f : -1.f);
    py = (1.f - fabsf(ox)) * (oy >= 0.f ? 1.f : -1.f);
}
// texel (i, j) of the table, i and j in [-1, n], through the octahedral border rule: points x and -x of an outer edge are the
// same direction, so a texel one step outside a column range mirrors its row, and the other way round
__device__ inline uint32_t env_texel(int i, int j, int n) {
    const bool ox = i < 0 || i >= n, oy = j < 0 || j >= n;
    int ic = i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
    int jc = j < 0 ? 0 : (j > n - 1 ? n - 1 : j);
    if (ox) jc = n - 1 - jc;
    if (oy) ic = n - 1 - ic;
    return (uint32_t)jc * (uint32_t)n + (uint32_t)ic;
}
// The colour of the environment in unit direction d, operation by operation as include/rtmi.h lists it: + - * /, fabsf, floorf
// and comparisons in f32, plain loads.  The indices come from the clamped texel coordinates, so that no value of d reads outside
// the table; the weights from the unclamped ones, which the clamp leaves alone unless they are NaN, so that a NaN stays one.
// The four loads do not depend on each other and are requested together.
__device__ inline V4 env_lookup(const EnvTab& e, V4 d) {
    auto v4 = [](float4 a) { return V4{a.x, a.y, a.z, a.w}; };
    const float mx = vdot(v4(e.r0), d), my = vdot(v4(e.r1), d), mz = vdot(v4(e.r2), d);
    const float a = (fabsf(mx) + fabsf(my)) + fabsf(mz);
    float px = mx / a, py = my / a;
    if (mz < 0.f) oct_fold(px, py);
    const float fx = (px * 0.5f + 0.5f) * e.fn - 0.5f, fy = (py * 0.5f + 0.5f) * e.fn - 0.5f;
    const float cx = !(fx >= -1.f) ? -1.f : (fx > e.fn ? e.fn : fx), cy = !(fy >= -1.f) ? -1.f : (fy > e.fn ? e.fn : fy);
    const int ix = (int)floorf(cx), iy = (int)floorf(cy), n = (int)e.n;
    const float tx = fx - floorf(fx), ty = fy - floorf(fy);
    const uint32_t k00 = env_texel(ix, iy, n), k10 = env_texel(ix + 1, iy, n), k01 = env_texel(ix, iy + 1, n), k11 = env_texel(ix + 1, iy + 1, n);
    const float4 c00 = e.tab[k00], c10 = e.tab[k10], c01 = e.tab[k01], c11 = e.tab[k11];
    return mix_color(mix_color(v4(c00), v4(c10), tx), mix_color(v4(c01), v4(c11), tx), ty);
}

// The vertex normals of a scene (rtmi_scene_set_normals, include/rtmi.h "VERTEX NORMALS OF A SCENE"): six float4
// per triangle, (c0, d00) (e1, d01) (e2, d11) (n0, den) (n1, 0) (n2, 0) -- corner 0, the two edges from it, their dot products and
// the three corner normals -- entry 0 the sentinel's, n = ntris.  An argument of the k_shade*_smooth and k_features_smooth kernels
// only, as EnvTab is of its kernels: DScene, and with it every other kernel's argument block, stays as it is.
struct SmoothTab { const float4* __restrict__ tab; uint32_t n; };
// The shading normal at `point` of triangle `tri` (< sm.n), operation by operation as include/rtmi.h lists it: barycentric
// coordinates from the stored dot products, the corner normals interpolated and normalised, * -1.f on a back face.  ng = the
// record's normal, already * -1.f on a back face.  use: the result faces the geometric side that was hit and the incoming ray;
// otherwise (a flat triangle's NaN among the cases) the caller shades with ng.  The six loads do not depend on each other and
// are requested together.
__device__ inline V4 smooth_normal(const SmoothTab& sm, uint32_t tri, uint32_t face, V4 point, V4 rd, V4 ng, bool& use) {
    const float4* __restrict__ r = sm.tab + (size_t)tri * 6u;
    const float4 q0 = r[0], q1 = r[1], q2 = r[2], q3 = r[3], q4 = r[4], q5 = r[5];
    const V4 e1 = mk(q1.x, q1.y, q1.z), e2 = mk(q2.x, q2.y, q2.z);
    const float d00 = q0.w, d01 = q1.w, d11 = q2.w, den = q3.w;
    const V4 w = vsub(point, mk(q0.x, q0.y, q0.z));
    const float d20 = vdot(w, e1), d21 = vdot(w, e2);
    const float b1 = (d11 * d20 - d01 * d21) / den, b2 = (d00 * d21 - d01 * d20) / den, b0 = (1.f - b1) - b2;
    V4 ns = vunit(vadd(vadd(vmul(mk(q3.x, q3.y, q3.z), b0), vmul(mk(q4.x, q4.y, q4.z), b1)), vmul(mk(q5.x, q5.y, q5.z), b2)));
    if (face & 1u) ns = vmul(ns, -1.f);
    use = vdot(ns, ng) > 0.f && vdot(rd, ns) < 0.f;
    return ns;
}
// The shading level of a scene.  Every surface feature came with all earlier ones, so the kernels that shade a path form a ladder
// and not a product: each level knows what the levels below it know, and a table of a lower level that the scene lacks is passed
// empty (n = 0).  GLASS: RTMI_DIELECTRIC; ENV: + the environment; SMOOTH: + vertex normals; TEX: + textures and the colour stack;
// NMAP: + normal maps (shade_hit below says what each adds).  The host picks a scene's level in one place, shade_level()
// (rtmi_device.hip), and launches the level's kernels through launch_shade() and launch_features().
enum class Shade { PLAIN, GLASS, ENV, SMOOTH, TEX, NMAP };

// The bounce of one hit with normal `norm`: shade_hit's three arms (lambertian_ray, reflect_ray, the dielectric of include/rtmi.h)
// statement for statement, for the kernels that may evaluate it twice (SMOOTH).  dir: the direction as passed to make_ray;
// side: -1.f for a refracted ray, +1.f otherwise.
template <Shade L>
__device__ inline RayV bounce_ray(uint32_t kind, float m1x, uint32_t face, V4 point, V4 norm, V4 rd, V4 rv, float u3, V4& dir, float& side) {
    float scat = m1x;
    side = 1.f;
    if constexpr (L >= Shade::GLASS) {
        if (kind == RTMI_DIELECTRIC) {  // m1x = ior
            const float ior = m1x;
            const float ci = fabsf(vdot(rd, norm));
            const float eta = (face & 1u) ? ior : 1.f / ior;
            const float s2 = 1.f - ci * ci;
            const float k = 1.f - (eta * eta) * s2;
            const bool tir = !(k >= 0.f);
            const float ct = sqrtf(k);
            const float cs = (face & 1u) ? ct : ci;
            float r0 = (1.f - ior) / (1.f + ior);
            r0 = r0 * r0;
            const float x = 1.f - cs, x2 = x * x, x5 = (x2 * x2) * x;
            const float R = r0 + (1.f - r0) * x5;
            if (!(tir || u3 < R)) {
                const V4 perp = vmul(vadd(rd, vmul(norm, ci)), eta);
                const V4 par = vmul(norm, -ct);
                const V4 td = vunit(vadd(perp, par));
                dir = td;
                side = -1.f;
                return make_ray(vadd(point, vmul(td, 0.001f)), td);
            }
            scat = 0.f;
        }
    }
    if (kind == RTMI_MATTE) {
        dir = vadd(norm, rv);
        return make_ray(vadd(point, vmul(rv, 0.001f)), dir);
    }
    const float ddot = fabsf(vdot(rd, norm));
    const V4 dir_p = vmul(norm, ddot);
    const V4 dir_o = vadd(rd, dir_p);
    const V4 reflect = vadd(dir_p, dir_o);
    const V4 rvf = vmul(rv, scat);
    const V4 reflect_dir = vunit(vadd(reflect, rvf));
    dir = vunit(vadd(reflect, rvf));
    return make_ray(vadd(point, vmul(reflect_dir, 0.001f)), dir);
}

// The textures of a scene (rtmi_scene_set_textures, include/rtmi.h "TEXTURES OF A SCENE").  tri: five float4 per
// triangle, (c0, d00) (e1, d01) (e2, d11) (u0, u1, u2, den) (v0, v1, v2, bits of tex_of_tri) -- SmoothTab's barycentric data, the
// corner uvs and the texture number (0: none) -- entry 0 the sentinel's, n = ntris.  hdr: per image k = 1..ntex at hdr[k - 1],
// (offset into texels, width, height, 0).  texels: all images in one buffer, one float4 per texel (lane 3 +0), texel (i, j) of an
// image at offset + j * width + i.  An argument of the k_shade*_tex and k_features_tex kernels only, as EnvTab and SmoothTab are
// of theirs: DScene, and with it every other kernel's argument block, stays as it is.
struct TexTab { const float4* __restrict__ tri; const uint4* __restrict__ hdr; const float4* __restrict__ texels; uint32_t n; };
// one wrap step of the repeat: i in [-1, N]
__device__ inline uint32_t tex_wrap(int i, int N) { return (uint32_t)(i < 0 ? i + N : (i >= N ? i - N : i)); }
// tex_colour's statements in three parts, for tex_colour_nmap below, where the colour and the normal map share one (u, v).
// tex_colour itself keeps them written out: calling these parts from it changed the machine code of the k_shade*_tex kernels.
// (u, v) at `point` of a triangle whose record is q0 .. q4: barycentric coordinates by smooth_normal's statements and the corner
// uvs interpolated, as include/rtmi.h lists them.
__device__ inline void tex_uv(float4 q0, float4 q1, float4 q2, float4 q3, float4 q4, V4 point, float& u, float& v) {
    const V4 e1 = mk(q1.x, q1.y, q1.z), e2 = mk(q2.x, q2.y, q2.z);
    const float d00 = q0.w, d01 = q1.w, d11 = q2.w, den = q3.w;
    const V4 w = vsub(point, mk(q0.x, q0.y, q0.z));
    const float d20 = vdot(w, e1), d21 = vdot(w, e2);
    const float b1 = (d11 * d20 - d01 * d21) / den, b2 = (d00 * d21 - d01 * d20) / den, b0 = (1.f - b1) - b2;
    u = (q3.x * b0 + q3.y * b1) + q3.z * b2;
    v = (q4.x * b0 + q4.y * b1) + q4.z * b2;
}
// The four texels and the two weights of the bilinear, repeating lookup of the image with header h at (u, v): indices (relative to
// the image's first texel) from the clamped texel coordinates, weights from the unclamped ones.
struct TexTap { uint32_t i00, i10, i01, i11; float tx, ty; };
__device__ inline TexTap tex_tap(uint4 h, float u, float v) {
    const float fu = u - floorf(u), fv = v - floorf(v);
    const int W = (int)h.y, H = (int)h.z;
    const float fW = (float)h.y, fH = (float)h.z;
    const float fx = fu * fW - 0.5f, fy = fv * fH - 0.5f;
    const float cx = !(fx >= -1.f) ? -1.f : (fx > fW - 1.f ? fW - 1.f : fx), cy = !(fy >= -1.f) ? -1.f : (fy > fH - 1.f ? fH - 1.f : fy);
    const int ix = (int)floorf(cx), iy = (int)floorf(cy);
    const float tx_ = fx - floorf(fx), ty_ = fy - floorf(fy);
    const uint32_t x0 = tex_wrap(ix, W), x1 = tex_wrap(ix + 1, W), y0 = tex_wrap(iy, H) * h.y, y1 = tex_wrap(iy + 1, H) * h.y;
    return TexTap{y0 + x0, y0 + x1, y1 + x0, y1 + x1, tx_, ty_};
}
// the bilinear mix of four loaded texels
__device__ inline V4 tex_mix(float4 c00, float4 c10, float4 c01, float4 c11, float tx_, float ty_) {
    auto v4 = [](float4 a) { return V4{a.x, a.y, a.z, a.w}; };
    return mix_color(mix_color(v4(c00), v4(c10), tx_), mix_color(v4(c01), v4(c11), tx_), ty_);
}
// The colour of a hit at `point` of triangle `tri` (< tx.n) whose material colour is m0, operation by operation as include/rtmi.h
// lists it: barycentric coordinates by smooth_normal's statements, the corner uvs interpolated, the repeat, a bilinear lookup with
// plain loads whose indices come from the clamped texel coordinates (no value reads outside the image) and whose weights come from
// the unclamped ones (a NaN stays one), times the material's colour.  An untextured triangle gives m0's colour unmodified.  The
// five record loads are requested together, and so are the four texel loads.
__device__ inline V4 tex_colour(const TexTab& tx, uint32_t tri, V4 point, float4 m0) {
    const float4* __restrict__ r = tx.tri + (size_t)tri * 5u;
    const float4 q0 = r[0], q1 = r[1], q2 = r[2], q3 = r[3], q4 = r[4];
    const uint32_t k = __float_as_uint(q4.w);
    if (k == 0u) return mk(m0.x, m0.y, m0.z);
    const uint4 h = tx.hdr[k - 1u];
    const V4 e1 = mk(q1.x, q1.y, q1.z), e2 = mk(q2.x, q2.y, q2.z);
    const float d00 = q0.w, d01 = q1.w, d11 = q2.w, den = q3.w;
    const V4 w = vsub(point, mk(q0.x, q0.y, q0.z));
    const float d20 = vdot(w, e1), d21 = vdot(w, e2);
    const float b1 = (d11 * d20 - d01 * d21) / den, b2 = (d00 * d21 - d01 * d20) / den, b0 = (1.f - b1) - b2;
    const float u = (q3.x * b0 + q3.y * b1) + q3.z * b2, v = (q4.x * b0 + q4.y * b1) + q4.z * b2;
    const float fu = u - floorf(u), fv = v - floorf(v);
    const int W = (int)h.y, H = (int)h.z;
    const float fW = (float)h.y, fH = (float)h.z;
    const float fx = fu * fW - 0.5f, fy = fv * fH - 0.5f;
    const float cx = !(fx >= -1.f) ? -1.f : (fx > fW - 1.f ? fW - 1.f : fx), cy = !(fy >= -1.f) ? -1.f : (fy > fH - 1.f ? fH - 1.f : fy);
    const int ix = (int)floorf(cx), iy = (int)floorf(cy);
    const float tx_ = fx - floorf(fx), ty_ = fy - floorf(fy);
    const uint32_t x0 = tex_wrap(ix, W), x1 = tex_wrap(ix + 1, W), y0 = tex_wrap(iy, H) * h.y, y1 = tex_wrap(iy + 1, H) * h.y;
    const float4* __restrict__ img = tx.texels + h.x;
    const float4 c00 = img[y0 + x0], c10 = img[y0 + x1], c01 = img[y1 + x0], c11 = img[y1 + x1];
    auto v4 = [](float4 a) { return V4{a.x, a.y, a.z, a.w}; };
    const V4 tc = mix_color(mix_color(v4(c00), v4(c10), tx_), mix_color(v4(c01), v4(c11), tx_), ty_);
    return mk(m0.x * tc.x, m0.y * tc.y, m0.z * tc.z);
}

// The normal maps of a scene (rtmi_scene_set_normal_maps, include/rtmi.h "NORMAL MAPS OF A SCENE").  tri: one float4
// per triangle, (T.xyz, bits): bits 0-30 the map's image number among TexTab's images (0: none), bit 31 set when hand = -1.f; entry
// 0 the sentinel's, n = ntris.  An argument of the k_shade*_nmap and k_features_nmap kernels only: DScene, and with it every other
// kernel's argument block, stays as it is.
struct NmapTab { const float4* __restrict__ tri; uint32_t n; float strength; };
// tex_colour for the kernels of scenes with normal maps: the colour of the hit and, for a mapped triangle (kmap != 0), the map's
// bilinear lookup M at the same (u, v).  fr: the triangle's NmapTab record.  The two header loads are requested together, and
// after them the eight texel loads; an image number of 0 borrows the other's so that both lookups read valid texels, and its
// result is not used.  A triangle without a colour texture keeps m0's colour bit for bit.
__device__ inline V4 tex_colour_nmap(const TexTab& tx, const NmapTab& nt, uint32_t tri, V4 point, float4 m0, V4& M, float4& fr, uint32_t& kmap) {
    const float4* __restrict__ r = tx.tri + (size_t)tri * 5u;
    const float4 q0 = r[0], q1 = r[1], q2 = r[2], q3 = r[3], q4 = r[4];
    fr = tri < nt.n ? nt.tri[tri] : make_float4(0.f, 0.f, 0.f, 0.f);
    const uint32_t k = __float_as_uint(q4.w);
    kmap = __float_as_uint(fr.w) & 0x7FFFFFFFu;
    M = mk(0.f, 0.f, 0.f);
    if (k == 0u && kmap == 0u) return mk(m0.x, m0.y, m0.z);
    const uint4 hc = tx.hdr[(k ? k : kmap) - 1u], hm = tx.hdr[(kmap ? kmap : k) - 1u];
    float u, v;
    tex_uv(q0, q1, q2, q3, q4, point, u, v);
    const TexTap a = tex_tap(hc, u, v), b = tex_tap(hm, u, v);
    const float4* __restrict__ ic = tx.texels + hc.x;
    const float4* __restrict__ im = tx.texels + hm.x;
    const float4 c00 = ic[a.i00], c10 = ic[a.i10], c01 = ic[a.i01], c11 = ic[a.i11];
    const float4 m00 = im[b.i00], m10 = im[b.i10], m01 = im[b.i01], m11 = im[b.i11];
    const V4 tc = tex_mix(c00, c10, c01, c11, a.tx, a.ty);
    M = tex_mix(m00, m10, m01, m11, b.tx, b.ty);
    return k ? mk(m0.x * tc.x, m0.y * tc.y, m0.z * tc.z) : mk(m0.x, m0.y, m0.z);
}
// The mapped normal of a hit, operation by operation as include/rtmi.h lists it: the texel M decoded and scaled, the stored
// tangent T made orthogonal to the shading normal N (Gram-Schmidt) and normalised, the bitangent from their cross product and the
// stored handedness (negated on a back face, where N is negated, so that t and b are the same world vectors), the sum normalised.
// usem: the result faces the geometric side that was hit (ng) and the incoming ray; otherwise (a NaN among the cases) the caller
// shades with N.
__device__ inline V4 nmap_normal(float4 fr, V4 M, float strength, uint32_t face, V4 N, V4 ng, V4 rd, bool& usem) {
    const V4 T = mk(fr.x, fr.y, fr.z);
    const float hand = (__float_as_uint(fr.w) >> 31) ? -1.f : 1.f;
    const float x = (M.x * 2.f - 1.f) * strength, y = (M.y * 2.f - 1.f) * strength, z = M.z * 2.f - 1.f;
    const V4 t = vunit(vsub(T, vmul(N, vdot(N, T))));
    const V4 c = mk(N.y * t.z - N.z * t.y, N.z * t.x - N.x * t.z, N.x * t.y - N.y * t.x);
    const V4 b = vmul(c, (face & 1u) ? -hand : hand);
    const V4 nm = vunit(vadd(vadd(vmul(t, x), vmul(b, y)), vmul(N, z)));
    usem = vdot(nm, ng) > 0.f && vdot(rd, nm) < 0.f;
    return nm;
}

// color_ray + the tail of project_ray for ONE traced ray of a path.  `pass` = bounces the path has behind it (the ray's
// remaining depth is maxdepth - pass >= 1); tf = hit triangle | face << 30 (0 = miss), t = hit time; (ro, rd) the ray.
// Returns true when the path goes on: its surface has been pushed on the path's stack (mstack[pass][path]) and `nr` is
// the bounce ray (lambertian_ray / reflect_ray with the path's RNG block pass + 1).  Returns false when the path ends
// here: sky, Solid, edge face (Solid black, raytrace.rs:452-457) or depth exhausted (black, raytrace.rs:1261-1263); the
// nested mix_color calls (raytrace.rs:1233-1251) are then evaluated inside-out over the stack and the sample colour is
// written to scol[path].  `mirror` (optional): set to true when the path goes on through a Reflective surface.
// L (Shade, above) adds to that, level by level:
// GLASS: the kernels of scenes with a dielectric (k_shade*_glass, rtmi_device.hip) also know RTMI_DIELECTRIC, operation by
// operation as include/rtmi.h defines it: the level is pushed like Matte's, the bounce ray is the refracted one or, on total
// internal reflection or with Schlick's probability, reflect_ray's with scattering 0.f.  Without it (every other kernel, the
// path kernels among them) the arm is not compiled and the function is the one it was.
// ENV: the kernels of scenes with an environment (k_shade*_env) start a miss's fold at env_lookup(*env, rd) instead of the sky
// constant -- rd must then be the ray's direction for a miss too -- and nothing else moves: no draw, no ray, black at an edge
// face and at exhausted depth.  Without it `env` is never read.
// SMOOTH: the kernels of scenes with vertex normals (k_shade*_smooth) shade a bouncing triangle hit
// with smooth_normal's result where it is usable, and evaluate the bounce again with the geometric normal when the ray it gives
// leaves on the wrong side of the real surface: same rv, same u3, no new draw.  Their `env` may be an empty table (n = 0: the
// scene has normals and no environment), and a miss then starts at the sky constant.  Without it `sm` is never read.
// TEX: the kernels of scenes with textures (k_shade*_tex; their `sm` may be an empty table too)
// give a triangle hit that is no edge face tex_colour's colour: a Solid hit ends with it, every other hit pushes it with the
// material's alpha on the colour stack cstack[pass][path], and the fold reads the level's colour there and not in the material
// table.  Nothing else moves.  Without it `tex` and `cstack` are never read.
// NMAP: the kernels of scenes with normal maps (k_shade*_nmap) look the map up with the
// colour (tex_colour_nmap: one (u, v)) and shade a bouncing hit of a mapped triangle with nmap_normal's result where it is usable;
// the wrong-side rule is SMOOTH's with (use || usem).  The mapped normal is used where it is computed and is not stacked.
// Without it `nm` is never read.
template <Shade L = Shade::PLAIN>
__device__ inline bool shade_hit(const DScene& sc, uint32_t maxdepth, uint64_t seed, uint32_t npaths, uint32_t path, uint32_t pixel,
                                 uint32_t sample, uint32_t pass, uint32_t tf, float t, V4 ro, V4 rd, uint16_t* __restrict__ mstack,
                                 float4* __restrict__ scol, RayV& nr, bool* mirror = nullptr, const EnvTab* env = nullptr,
                                 const SmoothTab* sm = nullptr, const TexTab* tex = nullptr, float4* __restrict__ cstack = nullptr,
                                 const NmapTab* nm = nullptr) {
    constexpr bool GLASS = L >= Shade::GLASS, ENV = L >= Shade::ENV, SMOOTH = L >= Shade::SMOOTH, TEX = L >= Shade::TEX, NMAP = L >= Shade::NMAP;
    const uint32_t tri = tf & 0x3FFFFFFFu, face = tf >> 30;
    V4 c;
    uint32_t npushed = pass;
    if (tri == 0) {
        if constexpr (ENV && SMOOTH) c = env->n ? env_lookup(*env, rd) : mk(128.f / 255.f, 180.f / 255.f, 255.f / 255.f);
        else if constexpr (ENV) c = env_lookup(*env, rd);
        else c = mk(128.f / 255.f, 180.f / 255.f, 255.f / 255.f);  // raytrace.rs:1264
    } else if (face & 2u) {
        c = mk(0.f / 255.f, 0.f / 255.f, 0.f / 255.f);  // edge faces are Solid black, raytrace.rs:452-457
    } else {
        // a triangle's record, or (hit index >= ntris) an analytic sphere's: the sphere's normal needs the hit point and
        // is filled in below
        const bool is_sphere = tri >= sc.ntris;
        const float4 p1 = is_sphere ? sc.spheres[2 * (tri - sc.ntris) + 1] : sc.tplane[2 * tri + 1];
        const uint32_t mat = __float_as_uint(is_sphere ? p1.x : p1.w);
        const float4 m0 = sc.mats[2 * mat], m1 = sc.mats[2 * mat + 1];
        const uint32_t kind = __float_as_uint(m1.y);
        V4 tcol = mk(m0.x, m0.y, m0.z);
        V4 mapM = mk(0.f, 0.f, 0.f);
        float4 mapfr = make_float4(0.f, 0.f, 0.f, 0.f);
        uint32_t kmap = 0u;
        if constexpr (TEX && NMAP) {
            if (!is_sphere && tri < tex->n) tcol = tex_colour_nmap(*tex, *nm, tri, vadd(vmul(rd, t), ro), m0, mapM, mapfr, kmap);
        } else if constexpr (TEX) {
            if (!is_sphere && tri < tex->n) tcol = tex_colour(*tex, tri, vadd(vmul(rd, t), ro), m0);
        }
        if (kind == RTMI_SOLID) {
            if constexpr (TEX) c = tcol;
            else c = mk(m0.x, m0.y, m0.z);
        } else {
            mstack[(size_t)pass * npaths + path] = (uint16_t)mat;
            if constexpr (TEX) cstack[(size_t)pass * npaths + path] = make_float4(tcol.x, tcol.y, tcol.z, m0.w);
            npushed = pass + 1;
            c = mk(0.f / 255.f, 0.f / 255.f, 0.f / 255.f);  // project_ray at depth 0, raytrace.rs:1261-1263
            if (maxdepth - pass - 1u != 0u) {
                const V4 point = vadd(vmul(rd, t), ro);                      // Ray::at, raytrace.rs:227-229
                V4 norm = mk(p1.x, p1.y, p1.z);
                if (is_sphere) {  // (point - center).unit()
                    const float4 sc0 = sc.spheres[2 * (tri - sc.ntris)];
                    norm = vunit(vsub(point, mk(sc0.x, sc0.y, sc0.z)));
                }
                if (face & 1u) norm = vmul(norm, -1.f);                       // raytrace.rs:441-449
                float u3 = 0.f;
                V4 rv;
                if constexpr (GLASS) rv = random_vec_u(seed, pixel, sample, pass + 1u, u3);
                else rv = random_vec(seed, pixel, sample, pass + 1u);
                if constexpr (SMOOTH) {
                    bool use = false;
                    V4 n = norm;
                    if (!is_sphere && tri < sm->n) n = smooth_normal(*sm, tri, face, point, rd, norm, use);
                    if (!use) n = norm;
                    if constexpr (NMAP) {
                        if (kmap != 0u) {
                            bool usem = false;
                            const V4 mn = nmap_normal(mapfr, mapM, nm->strength, face, n, norm, rd, usem);
                            if (usem) { n = mn; use = true; }
                        }
                    }
                    for (;;) {
                        V4 dir;
                        float side;
                        nr = bounce_ray<L>(kind, m1.x, face, point, n, rd, rv, u3, dir, side);
                        if (!use || side * vdot(dir, norm) > 0.f) break;
                        n = norm;  // the ray leaves on the wrong side of the real surface: the whole bounce again with ng
                        use = false;
                    }
                    return true;
                }
                float scat = m1.x;
                if constexpr (GLASS) {
                    if (kind == RTMI_DIELECTRIC) {  // m1.x = ior
                        const float ior = m1.x;
                        const float ci = fabsf(vdot(rd, norm));
                        const float eta = (face & 1u) ? ior : 1.f / ior;
                        const float s2 = 1.f - ci * ci;
                        const float k = 1.f - (eta * eta) * s2;
                        const bool tir = !(k >= 0.f);
                        const float ct = sqrtf(k);
                        const float cs = (face & 1u) ? ct : ci;
                        float r0 = (1.f - ior) / (1.f + ior);
                        r0 = r0 * r0;
                        const float x = 1.f - cs, x2 = x * x, x5 = (x2 * x2) * x;
                        const float R = r0 + (1.f - r0) * x5;
                        if (!(tir || u3 < R)) {
                            const V4 perp = vmul(vadd(rd, vmul(norm, ci)), eta);
                            const V4 par = vmul(norm, -ct);
                            const V4 td = vunit(vadd(perp, par));
                            nr = make_ray(vadd(point, vmul(td, 0.001f)), td);
                            return true;
                        }
                        scat = 0.f;  // reflect_ray below with scattering = 0.f
                    }
                }
                if (kind == RTMI_MATTE) {
                    nr = make_ray(vadd(point, vmul(rv, 0.001f)), vadd(norm, rv));  // lambertian_ray, :292-297
                } else {
                    const float ddot = fabsf(vdot(rd, norm));                 // reflect_ray, :278-290
                    const V4 dir_p = vmul(norm, ddot);
                    const V4 dir_o = vadd(rd, dir_p);
                    const V4 reflect = vadd(dir_p, dir_o);
                    const V4 rvf = vmul(rv, scat);
                    const V4 reflect_dir = vunit(vadd(reflect, rvf));
                    nr = make_ray(vadd(point, vmul(reflect_dir, 0.001f)), vunit(vadd(reflect, rvf)));
                    if (mirror) *mirror = true;
                }
                return true;
            }
        }
    }
    // inside-out evaluation of the nested mix_color calls (raytrace.rs:1233-1251)
    for (int j = (int)npushed - 1; j >= 0; j--) {
        float4 mm;
        if constexpr (TEX) {
            mm = cstack[(size_t)j * npaths + path];
        } else {
            const uint32_t mj = mstack[(size_t)j * npaths + path];
            mm = sc.mats[2 * mj];
        }
        c = mix_color(mk(mm.x, mm.y, mm.z), c, mm.w);
    }
    store_stream(&scol[path], make_float4(c.x, c.y, c.z, c.w));
    return false;
}

// First-hit features of ONE traced primary ray (k_features, rtmi_render_features*): tf = hit triangle | face << 30 (0 = miss),
// t = hit time.  a = (albedo.rgb, coverage), n = (shading normal.xyz, depth).  The gather and the face rules are shade_hit's,
// restated so that shade_hit compiles to the code it had: a miss is the sky with no coverage, no normal and no depth; an edge
// face is Solid black (raytrace.rs:452-457); any other hit shows its surface's colour, whatever its kind; the normal of a hit
// is the triangle's, * (-1.f) on a back face (raytrace.rs:441-449).  Triangles only: the caller refuses analytic spheres.
struct HitFeat { float4 a, n; };
__device__ inline HitFeat hit_features(const DScene& sc, uint32_t tf, float t) {
    const uint32_t tri = tf & 0x3FFFFFFFu, face = tf >> 30;
    const bool hit = tri != 0u;
    float4 p1 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (hit) p1 = sc.tplane[2 * tri + 1];
    float4 m0 = make_float4(0.f / 255.f, 0.f / 255.f, 0.f / 255.f, 0.f);  // an edge face's colour
    if (hit && !(face & 2u)) m0 = sc.mats[2 * __float_as_uint(p1.w)];
    V4 norm = mk(p1.x, p1.y, p1.z);
    if (face & 1u) norm = vmul(norm, -1.f);
    HitFeat f;
    f.a.x = hit ? m0.x : 128.f / 255.f;  // the sky, raytrace.rs:1264
    f.a.y = hit ? m0.y : 180.f / 255.f;
    f.a.z = hit ? m0.z : 255.f / 255.f;
    f.a.w = hit ? 1.f : 0.f;
    f.n.x = hit ? norm.x : 0.f;
    f.n.y = hit ? norm.y : 0.f;
    f.n.z = hit ? norm.z : 0.f;
    f.n.w = hit ? t : 0.f;
    return f;
}
// hit_features for a scene with vertex normals (k_features_smooth): the normal of a triangle hit that is no edge face is the
// shading normal of include/rtmi.h -- smooth_normal at the hit point of the primary ray (ro, rd) where it is usable, the
// geometric one otherwise.  Albedo, coverage and depth are hit_features'.
__device__ inline HitFeat hit_features_smooth(const DScene& sc, const SmoothTab& sm, uint32_t tf, float t, V4 ro, V4 rd) {
    HitFeat f = hit_features(sc, tf, t);
    const uint32_t tri = tf & 0x3FFFFFFFu, face = tf >> 30;
    if (tri != 0u && !(face & 2u) && tri < sm.n) {
        bool use = false;
        const V4 ns = smooth_normal(sm, tri, face, vadd(vmul(rd, t), ro), rd, mk(f.n.x, f.n.y, f.n.z), use);
        if (use) { f.n.x = ns.x; f.n.y = ns.y; f.n.z = ns.z; }
    }
    return f;
}

// hit_features for a scene with textures (k_features_tex): the albedo of a triangle hit that is no edge face is tex_colour's at
// the hit point of the primary ray (ro, rd); the normal is hit_features_smooth's (sm may be empty).  Coverage and depth are
// hit_features'.
__device__ inline HitFeat hit_features_tex(const DScene& sc, const SmoothTab& sm, const TexTab& tx, uint32_t tf, float t, V4 ro, V4 rd) {
    HitFeat f = hit_features_smooth(sc, sm, tf, t, ro, rd);
    const uint32_t tri = tf & 0x3FFFFFFFu, face = tf >> 30;
    if (tri != 0u && !(face & 2u) && tri < tx.n) {
        const V4 c = tex_colour(tx, tri, vadd(vmul(rd, t), ro), f.a);
        f.a.x = c.x; f.a.y = c.y; f.a.z = c.z;
    }
    return f;
}

// hit_features for a scene with normal maps (k_features_nmap): the normal of a hit of a mapped triangle that is no edge face is
// nmap_normal's about hit_features_tex's normal N at the hit point of the primary ray (ro, rd) where it is usable, N otherwise.
// Albedo, coverage and depth are hit_features_tex's.
__device__ inline HitFeat hit_features_nmap(const DScene& sc, const SmoothTab& sm, const TexTab& tx, const NmapTab& nt, uint32_t tf, float t,
                                            V4 ro, V4 rd) {
    HitFeat f = hit_features_tex(sc, sm, tx, tf, t, ro, rd);
    const uint32_t tri = tf & 0x3FFFFFFFu, face = tf >> 30;
    if (tri != 0u && !(face & 2u) && tri < tx.n && tri < nt.n) {
        const float4 p1 = sc.tplane[2 * tri + 1];
        V4 ng = mk(p1.x, p1.y, p1.z);
        if (face & 1u) ng = vmul(ng, -1.f);
        V4 M;
        float4 fr;
        uint32_t kmap;
        (void)tex_colour_nmap(tx, nt, tri, vadd(vmul(rd, t), ro), f.a, M, fr, kmap);
        if (kmap != 0u) {
            bool usem = false;
            const V4 mn = nmap_normal(fr, M, nt.strength, face, mk(f.n.x, f.n.y, f.n.z), ng, rd, usem);
            if (usem) { f.n.x = mn.x; f.n.y = mn.y; f.n.z = mn.z; }
        }
    }
    return f;
}

}  // namespace rtmi
