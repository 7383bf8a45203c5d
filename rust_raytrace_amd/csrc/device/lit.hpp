// lit.hpp — box lights inside the path trace (rtmi_render_lit*, include/rtmi.h "BOX LIGHTS IN THE PATH" defines it operation by
// operation): the two elementwise kernels of the pass, which is rtmi_render_shadowed*'s pass structure with
// rtmi_render_envlight*'s direct stack.  Per pass j:
//   (the scene's closest-hit launch of path queue j)
//   k_lit_rays    up to nlights candidate shadow rays per queue entry that hit a Matte surface that bounces, each built as
//                 k_light_rays builds a candidate, from the light's own RNG block; the live ones compacted into shadow queue j
//                 with their limit and their weight light_color[l] * g_l
//   (the any-hit walk of shadow queue j: launch_occluded with the limit array)
//   k_shade_lit   k_shade_envlight's loop: the weights of the entry's unoccluded candidates summed in l order, pushed on the
//                 direct stack and added in the fold; no balance weight, the environment only where the scene has one
// The rays, the RNG blocks 0 .. maxdepth and the queue order rules are shade_pass's.  Included by rtmi_device.hip after
// envlight.hpp (RTMI_SHADOW_NONE is shadowed.hpp's, env_lookup shade.hpp's).
// The same two kernels for explicit rays (rtmi_render_rays_lit*, rtmi_bake_lit*): k_lit_rays_explicit and
// k_shade_lit_explicit, and the bake's own pair for the lamps' light at an element: k_bake_lit_rays, k_bake_lit_resolve (below).
#pragma once

namespace rtmi {

#define RTMI_LIT_LIGHTS 4
// One light of a lit call as the kernels take it
struct LitLight {
    V4 orig;
    float len2, bias;
    uint32_t unbounded;  // its rays' limit is +inf (rtmi_occluded's rule: the NULL limit)
    float col[3];
};
struct LitArgs {
    uint32_t nlights, inverse_square;
    LitLight li[RTMI_LIT_LIGHTS];
};

// One thread per entry of path queue `pass`: the hit is read and (point, n, the RNG key) made once, then candidate after candidate
// in registers (the loop over lights is unrolled, nlights bounds it for the whole wave).  The candidate's arithmetic is
// k_light_rays' (rtmi.h) with the Philox block 0xC0000000 | l << 16 | pass.  Compaction per block: one ballot per light, the
// lane's place = the wave's live candidates of the lights before l + the live lanes below it in light l, the four wave totals in
// LDS, ONE atomic per block of four waves on sctrl->count[pass + 1]; so consecutive live lanes of a light store consecutive
// entries.  slot[l * npaths + i] = the shadow queue entry of candidate l of path queue entry i, or RTMI_SHADOW_NONE (no candidate,
// or culled).  The caller sizes the shadow queue for npaths * nlights entries: count <= npaths bounds every index.
// The kernel's text is lit_rays_kernel.hpp, compiled once per sampling mode: k_lit_rays with a frame's key (Samp::PASS), and
// k_lit_rays_explicit (rtmi_render_rays_lit*, rtmi_bake_lit*) with rays_key()'s: keys = the batch's RNG keys or null,
// pix0 = the key of its first group.  Nothing else differs.
#define RTMI_LIT_KERNEL k_lit_rays
#define RTMI_LIT_KEYS_PARAM
#define RTMI_LIT_RAYS_KEY                                                         \
    uint32_t row, col;                                                            \
    path_pixel<Samp::PASS>(v, pix0, qpath[i], row, col, sample, nullptr);         \
    pixel = row * v.width + col;
#include "lit_rays_kernel.hpp"
#undef RTMI_LIT_KERNEL
#undef RTMI_LIT_KEYS_PARAM
#undef RTMI_LIT_RAYS_KEY
#define RTMI_LIT_KERNEL k_lit_rays_explicit
#define RTMI_LIT_KEYS_PARAM , const uint32_t* __restrict__ keys
#define RTMI_LIT_RAYS_KEY rays_key(v, pix0, qpath[i], keys, pixel, sample);
#include "lit_rays_kernel.hpp"
#undef RTMI_LIT_KERNEL
#undef RTMI_LIT_KEYS_PARAM
#undef RTMI_LIT_RAYS_KEY

// shade_hit's plain arm (Solid, Matte, Reflective, flat triangles) for ONE traced ray of a lit path: the same rays, stack and
// return value.  `direct` is the level's light (the sum of the weights of its unoccluded candidates, else 0): stored on
// dstack[pass][path] whenever a level is pushed (0 for a Reflective level and at exhausted depth).  A miss is the sky constant, or
// with ENV the plain lookup of the ray's direction.  The fold: c = mix_color(color_j, c + direct_j, alpha_j), inside-out.
template <bool ENV>
__device__ inline bool shade_hit_lit(const DScene& sc, const EnvTab& env, uint32_t maxdepth, uint64_t seed, uint32_t npaths, uint32_t path,
                                     uint32_t pixel, uint32_t sample, uint32_t pass, uint32_t tf, float t, V4 ro, V4 rd, V4 direct,
                                     uint16_t* __restrict__ mstack, float4* __restrict__ dstack, float4* __restrict__ scol, RayV& nr) {
    const uint32_t tri = tf & 0x3FFFFFFFu, face = tf >> 30;
    const V4 black = mk(0.f / 255.f, 0.f / 255.f, 0.f / 255.f);
    V4 c;
    uint32_t npushed = pass;
    if (tri == 0) {
        if (ENV) c = env_lookup(env, rd);
        else c = mk(128.f / 255.f, 180.f / 255.f, 255.f / 255.f);  // raytrace.rs:1264
    } else if (face & 2u) {
        c = black;  // edge faces are Solid black, raytrace.rs:452-457
    } else {
        const float4 p1 = sc.tplane[2 * tri + 1];  // triangles only: the caller refuses analytic spheres
        const uint32_t mat = __float_as_uint(p1.w);
        const float4 m0 = sc.mats[2 * mat], m1 = sc.mats[2 * mat + 1];
        const uint32_t kind = __float_as_uint(m1.y);
        if (kind == RTMI_SOLID) {
            c = mk(m0.x, m0.y, m0.z);
        } else {
            mstack[(size_t)pass * npaths + path] = (uint16_t)mat;
            npushed = pass + 1;
            c = black;  // project_ray at depth 0, raytrace.rs:1261-1263
            if (maxdepth - pass - 1u != 0u) {
                const V4 point = vadd(vmul(rd, t), ro);  // Ray::at, raytrace.rs:227-229
                V4 norm = mk(p1.x, p1.y, p1.z);
                if (face & 1u) norm = vmul(norm, -1.f);  // raytrace.rs:441-449
                const V4 rv = random_vec(seed, pixel, sample, pass + 1u);
                if (kind == RTMI_MATTE) {
                    nr = make_ray(vadd(point, vmul(rv, 0.001f)), vadd(norm, rv));  // lambertian_ray, :292-297
                } else {
                    const float ddot = fabsf(vdot(rd, norm));  // reflect_ray, :278-290
                    const V4 dir_p = vmul(norm, ddot);
                    const V4 dir_o = vadd(rd, dir_p);
                    const V4 reflect = vadd(dir_p, dir_o);
                    const V4 rvf = vmul(rv, m1.x);
                    const V4 reflect_dir = vunit(vadd(reflect, rvf));
                    nr = make_ray(vadd(point, vmul(reflect_dir, 0.001f)), vunit(vadd(reflect, rvf)));
                    direct = V4{0.f, 0.f, 0.f, 0.f};
                }
                store_stream(&dstack[(size_t)pass * npaths + path], make_float4(direct.x, direct.y, direct.z, direct.w));
                return true;
            }
            dstack[(size_t)pass * npaths + path] = make_float4(0.f, 0.f, 0.f, 0.f);  // no sample at exhausted depth
        }
    }
    // inside-out evaluation of the nested mix_color calls (raytrace.rs:1233-1251), each level's inner colour plus its direct light
    for (int j = (int)npushed - 1; j >= 0; j--) {
        const uint32_t mj = mstack[(size_t)j * npaths + path];
        const float4 mm = sc.mats[2 * mj], dj = dstack[(size_t)j * npaths + path];
        c = mix_color(mk(mm.x, mm.y, mm.z), vadd(c, V4{dj.x, dj.y, dj.z, dj.w}), mm.w);
    }
    store_stream(&scol[path], make_float4(c.x, c.y, c.z, c.w));
    return false;
}

// k_shade_envlight's loop with the sum of the entry's unoccluded weights, l ascending from (0, 0, 0, 0), for its direct light
// The kernel's text is lit_shade_kernel.hpp, once per sampling mode as above: k_shade_lit<ENV> and k_shade_lit_explicit<ENV>.  The
// sample colour goes to scol[path]: the caller's `color` buffer when an explicit-ray call asks for it.
#define RTMI_LIT_KERNEL k_shade_lit
#define RTMI_LIT_KEYS_PARAM
#define RTMI_LIT_SHADE_KEY                                                        \
    uint32_t prow, pcol, sample;                                                  \
    path_pixel<Samp::PASS>(v, pix0, path, prow, pcol, sample, nullptr);
#define RTMI_LIT_SHADE_PIXEL prow * v.width + pcol
#define RTMI_LIT_SHADE_HIT shade_hit_lit<ENV>
template <bool ENV>
#include "lit_shade_kernel.hpp"
#undef RTMI_LIT_KERNEL
#undef RTMI_LIT_KEYS_PARAM
#undef RTMI_LIT_SHADE_KEY
#undef RTMI_LIT_SHADE_PIXEL
#define RTMI_LIT_KERNEL k_shade_lit_explicit
#define RTMI_LIT_KEYS_PARAM , const uint32_t* __restrict__ keys
#define RTMI_LIT_SHADE_KEY                                                        \
    uint32_t pixel, sample;                                                       \
    rays_key(v, pix0, path, keys, pixel, sample);
#define RTMI_LIT_SHADE_PIXEL pixel
template <bool ENV>
#include "lit_shade_kernel.hpp"
#undef RTMI_LIT_KERNEL
#undef RTMI_LIT_KEYS_PARAM
#undef RTMI_LIT_SHADE_KEY
#undef RTMI_LIT_SHADE_PIXEL
#undef RTMI_LIT_SHADE_HIT

// ---------------------------------------------------------------- box lights on shaded surfaces (RTMI_LIT_SURFACES; include/rtmi.h
// "BOX LIGHTS ON SHADED SURFACES"): the kernels above for scenes with a dielectric, vertex normals, textures or normal
// maps.  One set at the top of the shading ladder (Shade::NMAP): a table the scene lacks is passed empty (n = 0) and tested at run
// time, cstack is null on a scene without textures.  The shading kernel computes the hit's shading normal again, as shade_hit<NMAP>
// does, and reads no record from the candidate kernel.

// The map's texel of a hit of triangle tri at `point`: tex_colour_nmap's M without the colour's lookup (the same record, header,
// (u, v), taps and mix).  kmap = 0: the triangle has no map and M is not set.
__device__ inline V4 lit_nmap_texel(const TexTab& tx, const NmapTab& nt, uint32_t tri, V4 point, float4& fr, uint32_t& kmap) {
    fr = tri < nt.n ? nt.tri[tri] : make_float4(0.f, 0.f, 0.f, 0.f);
    kmap = __float_as_uint(fr.w) & 0x7FFFFFFFu;
    if (kmap == 0u) return mk(0.f, 0.f, 0.f);
    const float4* __restrict__ r = tx.tri + (size_t)tri * 5u;
    const float4 q0 = r[0], q1 = r[1], q2 = r[2], q3 = r[3], q4 = r[4];
    const uint4 hm = tx.hdr[kmap - 1u];
    float u, v;
    tex_uv(q0, q1, q2, q3, q4, point, u, v);
    const TexTap b = tex_tap(hm, u, v);
    const float4* __restrict__ im = tx.texels + hm.x;
    const float4 m00 = im[b.i00], m10 = im[b.i10], m01 = im[b.i01], m11 = im[b.i11];
    return tex_mix(m00, m10, m01, m11, b.tx, b.ty);
}
// N of a hit: the value n has in shade_hit<Shade::NMAP> before its wrong-side loop.  ng: the record's normal, * -1.f on a back face.
__device__ inline V4 lit_shading_normal(const SmoothTab& sm, const TexTab& tx, const NmapTab& nt, uint32_t tri, uint32_t face, V4 point, V4 rd,
                                        V4 ng) {
    bool use = false;
    V4 n = ng;
    if (tri < sm.n) n = smooth_normal(sm, tri, face, point, rd, ng, use);
    if (!use) n = ng;
    if (tri < tx.n) {
        float4 fr;
        uint32_t kmap;
        const V4 M = lit_nmap_texel(tx, nt, tri, point, fr, kmap);
        if (kmap != 0u) {
            bool usem = false;
            const V4 mn = nmap_normal(fr, M, nt.strength, face, n, ng, rd, usem);
            if (usem) n = mn;
        }
    }
    return n;
}

#define RTMI_LIT_SURFACES_KERNEL
#define RTMI_LIT_KERNEL k_lit_rays_surf
#define RTMI_LIT_KEYS_PARAM , SmoothTab sm, TexTab tex, NmapTab nm
#define RTMI_LIT_RAYS_KEY                                                         \
    uint32_t row, col;                                                            \
    path_pixel<Samp::PASS>(v, pix0, qpath[i], row, col, sample, nullptr);         \
    pixel = row * v.width + col;
#include "lit_rays_kernel.hpp"
#undef RTMI_LIT_KERNEL
#undef RTMI_LIT_KEYS_PARAM
#undef RTMI_LIT_RAYS_KEY
#define RTMI_LIT_KERNEL k_lit_rays_surf_explicit
#define RTMI_LIT_KEYS_PARAM , const uint32_t* __restrict__ keys, SmoothTab sm, TexTab tex, NmapTab nm
#define RTMI_LIT_RAYS_KEY rays_key(v, pix0, qpath[i], keys, pixel, sample);
#include "lit_rays_kernel.hpp"
#undef RTMI_LIT_KERNEL
#undef RTMI_LIT_KEYS_PARAM
#undef RTMI_LIT_RAYS_KEY
#undef RTMI_LIT_SURFACES_KERNEL

// shade_hit<Shade::NMAP> (triangles only: the caller refuses analytic spheres) for ONE traced ray of a lit path: the same rays,
// stacks and return value, the bounce and its wrong-side re-evaluation statement for statement.  `direct` as in shade_hit_lit: it
// is stored for a Matte level that bounces, 0 for a Reflective or Dielectric level and at exhausted depth.  On a textured scene
// (tex.n != 0) a level's colour and alpha are pushed on cstack and the fold reads them there; otherwise it reads the material table.
__device__ inline bool shade_hit_lit_surf(const DScene& sc, const EnvTab& env, uint32_t maxdepth, uint64_t seed, uint32_t npaths, uint32_t path,
                                          uint32_t pixel, uint32_t sample, uint32_t pass, uint32_t tf, float t, V4 ro, V4 rd, V4 direct,
                                          uint16_t* __restrict__ mstack, float4* __restrict__ dstack, float4* __restrict__ scol, RayV& nr,
                                          const SmoothTab& sm, const TexTab& tex, float4* __restrict__ cstack, const NmapTab& nm) {
    const uint32_t tri = tf & 0x3FFFFFFFu, face = tf >> 30;
    const bool textured = tex.n != 0u;
    V4 c;
    uint32_t npushed = pass;
    if (tri == 0) {
        c = env.n ? env_lookup(env, rd) : mk(128.f / 255.f, 180.f / 255.f, 255.f / 255.f);
    } else if (face & 2u) {
        c = mk(0.f / 255.f, 0.f / 255.f, 0.f / 255.f);
    } else {
        const float4 p1 = sc.tplane[2 * tri + 1];
        const uint32_t mat = __float_as_uint(p1.w);
        const float4 m0 = sc.mats[2 * mat], m1 = sc.mats[2 * mat + 1];
        const uint32_t kind = __float_as_uint(m1.y);
        V4 tcol = mk(m0.x, m0.y, m0.z);
        V4 mapM = mk(0.f, 0.f, 0.f);
        float4 mapfr = make_float4(0.f, 0.f, 0.f, 0.f);
        uint32_t kmap = 0u;
        if (tri < tex.n) tcol = tex_colour_nmap(tex, nm, tri, vadd(vmul(rd, t), ro), m0, mapM, mapfr, kmap);
        if (kind == RTMI_SOLID) {
            c = tcol;
        } else {
            mstack[(size_t)pass * npaths + path] = (uint16_t)mat;
            if (textured) cstack[(size_t)pass * npaths + path] = make_float4(tcol.x, tcol.y, tcol.z, m0.w);
            npushed = pass + 1;
            c = mk(0.f / 255.f, 0.f / 255.f, 0.f / 255.f);
            if (maxdepth - pass - 1u != 0u) {
                const V4 point = vadd(vmul(rd, t), ro);
                V4 norm = mk(p1.x, p1.y, p1.z);
                if (face & 1u) norm = vmul(norm, -1.f);
                float u3 = 0.f;
                const V4 rv = random_vec_u(seed, pixel, sample, pass + 1u, u3);
                bool use = false;
                V4 n = norm;
                if (tri < sm.n) n = smooth_normal(sm, tri, face, point, rd, norm, use);
                if (!use) n = norm;
                if (kmap != 0u) {
                    bool usem = false;
                    const V4 mn = nmap_normal(mapfr, mapM, nm.strength, face, n, norm, rd, usem);
                    if (usem) { n = mn; use = true; }
                }
                for (;;) {
                    V4 dir;
                    float side;
                    nr = bounce_ray<Shade::NMAP>(kind, m1.x, face, point, n, rd, rv, u3, dir, side);
                    if (!use || side * vdot(dir, norm) > 0.f) break;
                    n = norm;  // the ray leaves on the wrong side of the real surface: the whole bounce again with ng
                    use = false;
                }
                if (kind != RTMI_MATTE) direct = V4{0.f, 0.f, 0.f, 0.f};
                store_stream(&dstack[(size_t)pass * npaths + path], make_float4(direct.x, direct.y, direct.z, direct.w));
                return true;
            }
            dstack[(size_t)pass * npaths + path] = make_float4(0.f, 0.f, 0.f, 0.f);  // no sample at exhausted depth
        }
    }
    // inside-out evaluation of the nested mix_color calls, each level's inner colour plus its direct light
    for (int j = (int)npushed - 1; j >= 0; j--) {
        float4 mm;
        if (textured) {
            mm = cstack[(size_t)j * npaths + path];
        } else {
            const uint32_t mj = mstack[(size_t)j * npaths + path];
            mm = sc.mats[2 * mj];
        }
        const float4 dj = dstack[(size_t)j * npaths + path];
        c = mix_color(mk(mm.x, mm.y, mm.z), vadd(c, V4{dj.x, dj.y, dj.z, dj.w}), mm.w);
    }
    store_stream(&scol[path], make_float4(c.x, c.y, c.z, c.w));
    return false;
}

// k_shade_lit's slot loop in front of shade_hit_lit_surf: the text is lit_shade_kernel.hpp's, once per sampling mode
#define RTMI_LIT_SHADE_HIT(...) shade_hit_lit_surf(__VA_ARGS__, sm, tex, cstack, nm)
#define RTMI_LIT_KERNEL k_shade_lit_surf
#define RTMI_LIT_KEYS_PARAM , SmoothTab sm, TexTab tex, float4* __restrict__ cstack, NmapTab nm
#define RTMI_LIT_SHADE_KEY                                                        \
    uint32_t prow, pcol, sample;                                                  \
    path_pixel<Samp::PASS>(v, pix0, path, prow, pcol, sample, nullptr);
#define RTMI_LIT_SHADE_PIXEL prow * v.width + pcol
#include "lit_shade_kernel.hpp"
#undef RTMI_LIT_KERNEL
#undef RTMI_LIT_KEYS_PARAM
#undef RTMI_LIT_SHADE_KEY
#undef RTMI_LIT_SHADE_PIXEL
#define RTMI_LIT_KERNEL k_shade_lit_surf_explicit
#define RTMI_LIT_KEYS_PARAM , const uint32_t* __restrict__ keys, SmoothTab sm, TexTab tex, float4* __restrict__ cstack, NmapTab nm
#define RTMI_LIT_SHADE_KEY                                                        \
    uint32_t pixel, sample;                                                       \
    rays_key(v, pix0, path, keys, pixel, sample);
#define RTMI_LIT_SHADE_PIXEL pixel
#include "lit_shade_kernel.hpp"
#undef RTMI_LIT_KERNEL
#undef RTMI_LIT_KEYS_PARAM
#undef RTMI_LIT_SHADE_KEY
#undef RTMI_LIT_SHADE_PIXEL
#undef RTMI_LIT_SHADE_HIT

// ---------------------------------------------------------------- the lamps' light at a bake element (rtmi_bake_lit*: `direct`)
// k_bake_rays' loop (bake.hpp: a block stages `epb` whole elements per step in LDS, thread e of the step's (element h, ray k) pairs, k
// fastest) with k_lit_rays' candidates and compaction where the gather ray is made: the point is gather ray k's (POINTS: the
// element's; TRIANGLES: the same draw of block 0x20000000 and the same fold), n the element's normal on all four lanes as given, the
// key (seed, pix0 + element, k), the candidate of light l from block 0xC000FFFF | l << 16 (level field 0xFFFF: no path level has
// it).  The live candidates go to the shadow queue counted in sctrl->count[q]; slot[l * (nelems * K) + entry] = the queue entry of
// candidate l of ray `entry` = element * K + k, or RTMI_SHADOW_NONE.  The caller sizes the queue for nelems * K * nlights entries.
#define RTMI_BAKE_LIT_LEVEL 0xFFFFu
template <bool TRI>
__global__ void __launch_bounds__(256) k_bake_lit_rays(uint32_t nelems, uint32_t K, FastDiv dK, uint32_t epb, const float4* __restrict__ pos,
                                                       const float4* __restrict__ nrm, uint64_t seed, uint32_t pix0, LitArgs la,
                                                       float4* __restrict__ lq_o, float4* __restrict__ lq_d, float* __restrict__ lq_tmax,
                                                       float4* __restrict__ lw, uint32_t* __restrict__ slot, DCtrl* __restrict__ sctrl, int q) {
    __shared__ float s_pt[TRI ? 12 : 4][RTMI_BAKE_STEP_MAX], s_n[4][RTMI_BAKE_STEP_MAX];  // [lane of the vector][element of the step]
    __shared__ uint32_t s_cnt[4], s_base;
    const uint32_t nsteps = (nelems + epb - 1u) / epb;
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t nl = min(la.nlights, (uint32_t)RTMI_LIT_LIGHTS);
    const size_t nentries = (size_t)nelems * K;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (uint32_t step = blockIdx.x; step < nsteps; step += gridDim.x) {  // uniform per block: the barriers stay converged
        const uint32_t m0 = step * epb, cnt = min(epb, nelems - m0);
        if (threadIdx.x < cnt) {
            const uint32_t j = threadIdx.x, m = m0 + j;
            const float4 n = nrm[m];
            s_n[0][j] = n.x; s_n[1][j] = n.y; s_n[2][j] = n.z; s_n[3][j] = n.w;
            if constexpr (TRI) {
                const float4 a = pos[3u * m], b = pos[3u * m + 1u], c = pos[3u * m + 2u];
                const V4 c0{a.x, a.y, a.z, a.w};
                const V4 e1 = vsub(V4{b.x, b.y, b.z, b.w}, c0), e2 = vsub(V4{c.x, c.y, c.z, c.w}, c0);
                s_pt[0][j] = c0.x; s_pt[1][j] = c0.y; s_pt[2][j] = c0.z; s_pt[3][j] = c0.w;
                s_pt[4][j] = e1.x; s_pt[5][j] = e1.y; s_pt[6][j] = e1.z; s_pt[7][j] = e1.w;
                s_pt[8][j] = e2.x; s_pt[9][j] = e2.y; s_pt[10][j] = e2.z; s_pt[11][j] = e2.w;
            } else {
                const float4 p = pos[m];
                s_pt[0][j] = p.x; s_pt[1][j] = p.y; s_pt[2][j] = p.z; s_pt[3][j] = p.w;
            }
        }
        __syncthreads();
        const uint32_t base = m0 * K, nrays = cnt * K;  // the step's first entry (nelems * K < 2^31)
        for (uint32_t e0 = 0; e0 < nrays; e0 += 256u) {  // whole blocks stay converged for the ballots and the barriers
            const uint32_t e = e0 + threadIdx.x;
            const bool cand = e < nrays;
            V4 point{}, n{};
            uint32_t pixel = 0, k = 0;
            if (cand) {
                const uint32_t h = fdiv(e, dK);
                k = e - h * K;
                pixel = pix0 + m0 + h;
                n = V4{s_n[0][h], s_n[1][h], s_n[2][h], s_n[3][h]};
                point = V4{s_pt[0][h], s_pt[1][h], s_pt[2][h], s_pt[3][h]};
                if constexpr (TRI) {
                    const V4 e1{s_pt[4][h], s_pt[5][h], s_pt[6][h], s_pt[7][h]}, e2{s_pt[8][h], s_pt[9][h], s_pt[10][h], s_pt[11][h]};
                    point = bake_triangle_point(seed, pixel, k, point, e1, e2);
                }
            }
            bool live[RTMI_LIT_LIGHTS];
            V4 o[RTMI_LIT_LIGHTS], dir[RTMI_LIT_LIGHTS];
            float r[RTMI_LIT_LIGHTS], g[RTMI_LIT_LIGHTS];
            uint32_t place[RTMI_LIT_LIGHTS];  // the lane's place among the wave's live candidates
            uint32_t wtotal = 0;
#pragma unroll
            for (uint32_t l = 0; l < RTMI_LIT_LIGHTS; l++) {
                live[l] = false;
                o[l] = V4{}; dir[l] = V4{};
                r[l] = 0.f; g[l] = 0.f;
                place[l] = 0;
                if (l < nl) {
                    if (cand) {
                        const LitLight& L = la.li[l];
                        uint32_t w[4];
                        rng_block(seed, pixel, k, 0xC0000000u | (l << 16) | RTMI_BAKE_LIT_LEVEL, w);
                        const V4 adj{L.orig.x + u32_to_unit_f32(w[0]) * L.len2, L.orig.y + u32_to_unit_f32(w[1]) * L.len2,
                                     L.orig.z + u32_to_unit_f32(w[2]) * L.len2, 0.f};
                        const V4 vv = vsub(adj, point);
                        const float d2 = vdot(vv, vv);
                        r[l] = sqrtf(d2);
                        dir[l] = vmul(vv, 1.f / r[l]);
                        o[l] = vadd(point, vmul(n, L.bias * (u32_to_unit_f32(w[3]) + 1.f)));
                        const float c = vdot(n, dir[l]);
                        live[l] = c > 0.f;  // false for the light behind the element, for a NaN and for the light at the point
                        g[l] = la.inverse_square ? c / d2 : c;
                    }
                    const unsigned long long mask = __ballot(live[l]);
                    place[l] = wtotal + (uint32_t)__popcll(mask & below);
                    wtotal += (uint32_t)__popcll(mask);
                }
            }
            if (lane == 0) s_cnt[wv] = wtotal;
            __syncthreads();
            if (threadIdx.x == 0) {
                const uint32_t total = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
                s_base = total ? atomicAdd(&sctrl->count[q], total) : 0u;
            }
            __syncthreads();
            uint32_t qb = s_base;
            for (uint32_t x = 0; x < wv; x++) qb += s_cnt[x];
#pragma unroll
            for (uint32_t l = 0; l < RTMI_LIT_LIGHTS; l++) {
                if (l < nl) {
                    if (live[l]) {
                        const LitLight& L = la.li[l];
                        const uint32_t qe = qb + place[l];
                        store_stream(&lq_o[qe], make_float4(o[l].x, o[l].y, o[l].z, o[l].w));
                        store_stream(&lq_d[qe], make_float4(dir[l].x, dir[l].y, dir[l].z, dir[l].w));
                        store_stream(&lq_tmax[qe], L.unbounded ? INFINITY : r[l]);
                        store_stream(&lw[qe], make_float4(L.col[0] * g[l], L.col[1] * g[l], L.col[2] * g[l], 0.f));
                        store_stream(&slot[(size_t)l * nentries + base + e], qe);
                    } else if (cand) {
                        store_stream(&slot[(size_t)l * nentries + base + e], RTMI_SHADOW_NONE);
                    }
                }
            }
            __syncthreads();  // s_cnt / s_base are rewritten by the next iteration, the staged elements by the next step
        }
    }
}

// One thread per (element, k): d_k = the weights of the ray's unoccluded candidates summed in l order from (0, 0, 0, 0), as
// k_shade_lit sums a level's.  k_accum then folds an element's K of them to direct[m].
__global__ void __launch_bounds__(256) k_bake_lit_resolve(uint32_t nentries, uint32_t nlights, const uint32_t* __restrict__ slot,
                                                          const uint8_t* __restrict__ occ, const float4* __restrict__ lw,
                                                          float4* __restrict__ dk) {
    const uint32_t stride = gridDim.x * blockDim.x;
    const uint32_t nl = min(nlights, (uint32_t)RTMI_LIT_LIGHTS);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nentries; i += stride) {
        V4 d{0.f, 0.f, 0.f, 0.f};
        for (uint32_t l = 0; l < nl; l++) {
            const uint32_t e = slot[(size_t)l * nentries + i];
            if (e != RTMI_SHADOW_NONE && occ[e] == 0) {
                const float4 l4 = lw[e];
                d = vadd(d, V4{l4.x, l4.y, l4.z, l4.w});
            }
        }
        store_stream(&dk[i], make_float4(d.x, d.y, d.z, d.w));
    }
}

}  // namespace rtmi
