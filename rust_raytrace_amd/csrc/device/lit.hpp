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
__global__ void __launch_bounds__(256) k_lit_rays(DScene sc, DView v, uint64_t seed, uint32_t pix0, uint32_t npaths, int pass, LitArgs la,
                                                  const float4* __restrict__ qo, const float4* __restrict__ qd,
                                                  const uint32_t* __restrict__ qpath, const uint32_t* __restrict__ hit_tf,
                                                  const float* __restrict__ hit_t, const DCtrl* __restrict__ ctrl,
                                                  float4* __restrict__ lq_o, float4* __restrict__ lq_d, float* __restrict__ lq_tmax,
                                                  float4* __restrict__ lw, uint32_t* __restrict__ slot, DCtrl* __restrict__ sctrl) {
    __shared__ uint32_t s_cnt[4], s_base;
    const uint32_t count = min(ctrl->count[pass], npaths);
    const uint32_t stride = gridDim.x * blockDim.x;
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t bound = (count + 255u) & ~255u;  // whole blocks stay converged for the ballots and the barriers
    const uint32_t nl = min(la.nlights, (uint32_t)RTMI_LIT_LIGHTS);
    // (launched for the passes whose Matte hits bounce, maxdepth - pass - 1 != 0: an exhausted level gets no sample)
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < bound; i += stride) {
        bool cand = false;
        V4 point{}, n{};
        uint32_t pixel = 0, sample = 0;
        if (i < count) {
            const uint32_t tf = hit_tf[i], tri = tf & 0x3FFFFFFFu;
            if (tri != 0u && !((tf >> 30) & 2u)) {
                const float4 p1 = sc.tplane[2 * tri + 1];
                const float4 m1 = sc.mats[2 * __float_as_uint(p1.w) + 1];
                if (__float_as_uint(m1.y) == RTMI_MATTE) {
                    cand = true;
                    const float t = hit_t[i];
                    const float4 o4 = qo[i], d4 = qd[i];
                    point = vadd(vmul(V4{d4.x, d4.y, d4.z, d4.w}, t), V4{o4.x, o4.y, o4.z, o4.w});
                    n = mk(p1.x, p1.y, p1.z);
                    if ((tf >> 30) & 1u) n = vmul(n, -1.f);
                    uint32_t row, col;
                    path_pixel<Samp::PASS>(v, pix0, qpath[i], row, col, sample, nullptr);
                    pixel = row * v.width + col;
                }
            }
        }
        bool live[RTMI_LIT_LIGHTS];
        V4 o[RTMI_LIT_LIGHTS], dir[RTMI_LIT_LIGHTS];
        float r[RTMI_LIT_LIGHTS], g[RTMI_LIT_LIGHTS];
        uint32_t place[RTMI_LIT_LIGHTS];  // the lane's place among the wave's live candidates
        uint32_t wtotal = 0;
        const unsigned long long below = (1ull << lane) - 1ull;
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
                    rng_block(seed, pixel, sample, 0xC0000000u | (l << 16) | (uint32_t)pass, w);
                    const V4 adj{L.orig.x + u32_to_unit_f32(w[0]) * L.len2, L.orig.y + u32_to_unit_f32(w[1]) * L.len2,
                                 L.orig.z + u32_to_unit_f32(w[2]) * L.len2, 0.f};
                    const V4 vv = vsub(adj, point);
                    const float d2 = vdot(vv, vv);
                    r[l] = sqrtf(d2);
                    dir[l] = vmul(vv, 1.f / r[l]);
                    o[l] = vadd(point, vmul(n, L.bias * (u32_to_unit_f32(w[3]) + 1.f)));
                    const float c = vdot(n, dir[l]);
                    live[l] = c > 0.f;  // false for the light behind the surface, for a NaN and for the light at the point
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
            s_base = total ? atomicAdd(&sctrl->count[pass + 1], total) : 0u;
        }
        __syncthreads();
        uint32_t base = s_base;
        for (uint32_t k = 0; k < wv; k++) base += s_cnt[k];
#pragma unroll
        for (uint32_t l = 0; l < RTMI_LIT_LIGHTS; l++) {
            if (l < nl) {
                if (live[l]) {
                    const LitLight& L = la.li[l];
                    const uint32_t q = base + place[l];
                    store_stream(&lq_o[q], make_float4(o[l].x, o[l].y, o[l].z, o[l].w));
                    store_stream(&lq_d[q], make_float4(dir[l].x, dir[l].y, dir[l].z, dir[l].w));
                    store_stream(&lq_tmax[q], L.unbounded ? INFINITY : r[l]);
                    store_stream(&lw[q], make_float4(L.col[0] * g[l], L.col[1] * g[l], L.col[2] * g[l], 0.f));
                    store_stream(&slot[(size_t)l * npaths + i], q);
                } else if (i < count) {
                    store_stream(&slot[(size_t)l * npaths + i], RTMI_SHADOW_NONE);
                }
            }
        }
        __syncthreads();  // s_cnt / s_base are rewritten by the next iteration
    }
}

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
template <bool ENV>
__global__ void __launch_bounds__(256) k_shade_lit(DScene sc, DView v, uint64_t seed, uint32_t pix0, uint32_t npaths, int pass, EnvTab env,
                                                   uint32_t nlights, const float4* __restrict__ qo, const float4* __restrict__ qd,
                                                   const uint32_t* __restrict__ qpath, const uint32_t* __restrict__ hit_tf,
                                                   const float* __restrict__ hit_t, const uint32_t* __restrict__ slot,
                                                   const uint8_t* __restrict__ occ, const float4* __restrict__ lw,
                                                   float4* __restrict__ qo_n, float4* __restrict__ qd_n, uint32_t* __restrict__ qpath_n,
                                                   uint16_t* __restrict__ mstack, float4* __restrict__ dstack, float4* __restrict__ scol,
                                                   DCtrl* __restrict__ ctrl) {
    __shared__ uint32_t s_cnt[4], s_base;
    const uint32_t count = min(ctrl->count[pass], npaths);
    const uint32_t stride = gridDim.x * blockDim.x;
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t bound = (count + 255u) & ~255u;  // whole blocks stay converged for the ballot and the queue reservation
    // (the exhausted pass has no candidates: k_lit_rays is not launched for it and the slots are stale)
    const uint32_t nl = v.maxdepth - (uint32_t)pass - 1u != 0u ? min(nlights, (uint32_t)RTMI_LIT_LIGHTS) : 0u;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < bound; i += stride) {
        bool push = false;
        RayV nr;
        uint32_t path = 0;
        if (i < count) {
            path = qpath[i];
            const uint32_t tf = hit_tf[i];
            float t = 0.f;
            const float4 o4 = qo[i], d4 = qd[i];  // (with ENV a miss looks the environment up in its ray's direction)
            V4 direct{0.f, 0.f, 0.f, 0.f};
            if ((tf & 0x3FFFFFFFu) != 0u && !((tf >> 30) & 2u)) {
                t = hit_t[i];
                for (uint32_t l = 0; l < nl; l++) {
                    const uint32_t e = slot[(size_t)l * npaths + i];
                    if (e != RTMI_SHADOW_NONE && occ[e] == 0) {
                        const float4 l4 = lw[e];
                        direct = vadd(direct, V4{l4.x, l4.y, l4.z, l4.w});
                    }
                }
            }
            uint32_t prow, pcol, sample;
            path_pixel<Samp::PASS>(v, pix0, path, prow, pcol, sample, nullptr);
            push = shade_hit_lit<ENV>(sc, env, v.maxdepth, seed, npaths, path, prow * v.width + pcol, sample, (uint32_t)pass, tf, t,
                                      V4{o4.x, o4.y, o4.z, o4.w}, V4{d4.x, d4.y, d4.z, d4.w}, direct, mstack, dstack, scol, nr);
        }
        const unsigned long long mask = __ballot(push);
        if (lane == 0) s_cnt[wv] = (uint32_t)__popcll(mask);
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t total = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
            s_base = total ? atomicAdd(&ctrl->count[pass + 1], total) : 0u;
        }
        __syncthreads();
        {
            uint32_t base = s_base;
            for (uint32_t k = 0; k < wv; k++) base += s_cnt[k];
            if (push) {
                const uint32_t q = base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
                store_stream(&qo_n[q], make_float4(nr.orig.x, nr.orig.y, nr.orig.z, nr.orig.w));
                store_stream(&qd_n[q], make_float4(nr.dir.x, nr.dir.y, nr.dir.z, nr.dir.w));
                store_stream(&qpath_n[q], path);
            }
        }
        __syncthreads();  // s_cnt / s_base are rewritten by the next iteration
    }
}

}  // namespace rtmi
