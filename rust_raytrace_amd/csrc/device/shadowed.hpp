// shadowed.hpp — the two elementwise kernels of the shadowed path-trace (rtmi_render_shadowed*, include/rtmi.h defines it
// operation by operation): a progressive pass of the per-pass pipeline (k_gen_samples, one closest-hit launch
// per bounce pass, k_accum_samples) in which every surface hit of every bounce is tested against one box light, as the
// reference's color_ray spells it out (raytrace.rs:1203-1224, commented out there).  Per pass j of a batch:
//   (the scene's closest-hit launch of path queue j)
//   k_shadow_rays     one candidate shadow ray per queue entry that hit a surface (not a miss, not an edge face), built as
//                     k_light_rays builds candidate k = j; those with c > 0 compacted into shadow queue j, whose counter
//                     lives in the stream's SECOND control block (the path queues own the first one's indices)
//   (the scene's any-hit walk of shadow queue j: launch_occluded on that control block, with hit records of its own where
//    it falls back to the closest-hit launch, so that the path queue's hit records survive it)
//   k_shade_shadowed  shade_pass<Samp::PASS> with the entry's shadow bit: kept in one mask word per path, applied in the fold
// The rays, the RNG blocks 0 .. maxdepth and the queue order rules are shade_pass's: the shadow bit changes colours only.
// Included by rtmi_device.hip.
#pragma once

namespace rtmi {

#define RTMI_SHADOW_NONE 0xFFFFFFFFu    // slot of a queue entry that is not tested: a miss or an edge face (entries are < 2^31)
#define RTMI_SHADOW_CULLED 0xFFFFFFFEu  // slot of a tested entry whose ray is not traced: !(c > 0.f), shadowed

// One thread per entry of path queue `pass`.  The candidate's arithmetic is k_light_rays' (rtmi.h: adj = orig + u * len2 per
// lane, v = adj - point, r = sqrt(ordered dot), dir = v * (1.f / r), o = point + n * (bias * (u_3 + 1.f)), c = ordered
// dot(n, dir); all four lanes) with the one Philox block 0xC0000000 | pass of the path's (pixel, sample).  The live ones are
// compacted per block: ballot + popcount per wave, ONE atomic per block of four waves on sctrl->count[pass + 1] (as
// shade_pass and k_light_rays do, and for their reason), so consecutive live lanes store consecutive queue entries.  Index
// pass + 1 and not pass: launch_occluded reads the count of queue 0 from the host.  tmax: null when the light is unbounded.
__global__ void __launch_bounds__(256) k_shadow_rays(DScene sc, DView v, uint64_t seed, uint32_t pix0, int pass, V4 lorig, float len2,
                                                     float bias, const float4* __restrict__ qo, const float4* __restrict__ qd,
                                                     const uint32_t* __restrict__ qpath, const uint32_t* __restrict__ hit_tf,
                                                     const float* __restrict__ hit_t, const DCtrl* __restrict__ ctrl,
                                                     float4* __restrict__ lq_o, float4* __restrict__ lq_d, float* __restrict__ lq_tmax,
                                                     uint32_t* __restrict__ slot, DCtrl* __restrict__ sctrl) {
    __shared__ uint32_t s_cnt[4], s_base;
    const uint32_t count = ctrl->count[pass];
    const uint32_t stride = gridDim.x * blockDim.x;
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t bound = (count + 255u) & ~255u;  // whole blocks stay converged for the ballots and the barriers
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < bound; i += stride) {
        bool tested = false, live = false;
        V4 o{}, dir{};
        float r = 0.f;
        if (i < count) {
            const uint32_t tf = hit_tf[i];
            tested = (tf & 0x3FFFFFFFu) != 0u && !((tf >> 30) & 2u);
            if (tested) {
                const float t = hit_t[i];
                const float4 o4 = qo[i], d4 = qd[i];
                const V4 point = vadd(vmul(V4{d4.x, d4.y, d4.z, d4.w}, t), V4{o4.x, o4.y, o4.z, o4.w});
                const float4 p1 = sc.tplane[2 * (tf & 0x3FFFFFFFu) + 1];
                V4 n = mk(p1.x, p1.y, p1.z);
                if ((tf >> 30) & 1u) n = vmul(n, -1.f);
                uint32_t row, col, sample;
                path_pixel<Samp::PASS>(v, pix0, qpath[i], row, col, sample, nullptr);
                uint32_t w[4];
                rng_block(seed, row * v.width + col, sample, 0xC0000000u | (uint32_t)pass, w);
                const V4 adj{lorig.x + u32_to_unit_f32(w[0]) * len2, lorig.y + u32_to_unit_f32(w[1]) * len2,
                             lorig.z + u32_to_unit_f32(w[2]) * len2, 0.f};
                const V4 vv = vsub(adj, point);
                r = sqrtf(vdot(vv, vv));
                dir = vmul(vv, 1.f / r);
                o = vadd(point, vmul(n, bias * (u32_to_unit_f32(w[3]) + 1.f)));
                live = vdot(n, dir) > 0.f;  // false for the light behind the surface, for a NaN and for the light at the point
            }
        }
        const unsigned long long mask = __ballot(live);
        if (lane == 0) s_cnt[wv] = (uint32_t)__popcll(mask);
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t total = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
            s_base = total ? atomicAdd(&sctrl->count[pass + 1], total) : 0u;
        }
        __syncthreads();
        if (live) {
            uint32_t q = s_base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
            for (uint32_t k = 0; k < wv; k++) q += s_cnt[k];
            store_stream(&lq_o[q], make_float4(o.x, o.y, o.z, o.w));
            store_stream(&lq_d[q], make_float4(dir.x, dir.y, dir.z, dir.w));
            if (lq_tmax) store_stream(&lq_tmax[q], r);
            store_stream(&slot[i], q);
        } else if (i < count) {
            store_stream(&slot[i], tested ? RTMI_SHADOW_CULLED : RTMI_SHADOW_NONE);
        }
        __syncthreads();  // s_cnt / s_base are rewritten by the next iteration
    }
}

// shade_hit (shade.hpp) for ONE traced ray of a shadowed path: the same rays, stack and return value; `shadowed` is the
// shadow test's answer for this hit (ignored for a miss and an edge face, which are not tested).  smask[path] holds the
// answers of the path's levels, bit j for the hit of its ray j (maxdepth <= 32): read from pass 1 on, written when the path
// goes on.  Where the path ends, a terminal Solid shows shadowed ? black : colour and the fold takes black for the colour
// of every level whose bit is set: c = mix_color(bit_j ? black : color_j, c, alpha_j), inside-out.
__device__ inline bool shade_hit_shadowed(const DScene& sc, uint32_t maxdepth, uint64_t seed, uint32_t npaths, uint32_t path, uint32_t pixel,
                                          uint32_t sample, uint32_t pass, uint32_t tf, float t, V4 ro, V4 rd, bool shadowed,
                                          uint16_t* __restrict__ mstack, uint32_t* __restrict__ smask, float4* __restrict__ scol, RayV& nr) {
    const uint32_t tri = tf & 0x3FFFFFFFu, face = tf >> 30;
    const V4 black = mk(0.f / 255.f, 0.f / 255.f, 0.f / 255.f);
    V4 c;
    uint32_t npushed = pass;
    uint32_t bits = pass ? smask[path] : 0u;
    if (tri == 0) {
        c = mk(128.f / 255.f, 180.f / 255.f, 255.f / 255.f);  // raytrace.rs:1264
    } else if (face & 2u) {
        c = black;  // edge faces are Solid black, raytrace.rs:452-457
    } else {
        const float4 p1 = sc.tplane[2 * tri + 1];  // triangles only: the caller refuses analytic spheres
        const uint32_t mat = __float_as_uint(p1.w);
        const float4 m0 = sc.mats[2 * mat], m1 = sc.mats[2 * mat + 1];
        const uint32_t kind = __float_as_uint(m1.y);
        if (kind == RTMI_SOLID) {
            c = shadowed ? black : mk(m0.x, m0.y, m0.z);  // raytrace.rs:1209-1212
        } else {
            mstack[(size_t)pass * npaths + path] = (uint16_t)mat;
            npushed = pass + 1;
            if (shadowed) bits |= 1u << pass;
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
                }
                smask[path] = bits;
                return true;
            }
        }
    }
    // inside-out evaluation of the nested mix_color calls (raytrace.rs:1233-1251), a shadowed level's colour black
    for (int j = (int)npushed - 1; j >= 0; j--) {
        const uint32_t mj = mstack[(size_t)j * npaths + path];
        const float4 mm = sc.mats[2 * mj];
        c = mix_color((bits >> j) & 1u ? black : mk(mm.x, mm.y, mm.z), c, mm.w);
    }
    store_stream(&scol[path], make_float4(c.x, c.y, c.z, c.w));
    return false;
}

// shade_pass<Samp::PASS> (rtmi_device.hip) for a shadowed path: the same loads, the same compaction into queue pass + 1 of
// the path control block (ballot + prefix sum per wave, ONE atomic per block of four waves), plus the entry's slot and, for
// a live ray, its answer byte.  No slow queue: a bounce ray with a zero direction component is traced in place.
__global__ void __launch_bounds__(256) k_shade_shadowed(DScene sc, DView v, uint64_t seed, uint32_t pix0, uint32_t npaths, int pass,
                                                        const float4* __restrict__ qo, const float4* __restrict__ qd,
                                                        const uint32_t* __restrict__ qpath, const uint32_t* __restrict__ hit_tf,
                                                        const float* __restrict__ hit_t, const uint32_t* __restrict__ slot,
                                                        const uint8_t* __restrict__ occ, float4* __restrict__ qo_n,
                                                        float4* __restrict__ qd_n, uint32_t* __restrict__ qpath_n,
                                                        uint16_t* __restrict__ mstack, uint32_t* __restrict__ smask,
                                                        float4* __restrict__ scol, DCtrl* __restrict__ ctrl) {
    __shared__ uint32_t s_cnt[4], s_base;
    const uint32_t count = ctrl->count[pass];
    const uint32_t stride = gridDim.x * blockDim.x;
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t bound = (count + 255u) & ~255u;  // whole blocks stay converged for the ballot and the queue reservation
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < bound; i += stride) {
        bool push = false;
        RayV nr;
        uint32_t path = 0;
        if (i < count) {
            path = qpath[i];
            const uint32_t tf = hit_tf[i];
            float t = 0.f;
            float4 o4 = make_float4(0.f, 0.f, 0.f, 0.f), d4 = make_float4(0.f, 0.f, 1.f, 0.f);
            bool shadowed = false;
            if ((tf & 0x3FFFFFFFu) != 0u && !((tf >> 30) & 2u)) {
                t = hit_t[i]; o4 = qo[i]; d4 = qd[i];
                const uint32_t e = slot[i];  // CULLED or a shadow queue entry: the hit was tested
                shadowed = e == RTMI_SHADOW_CULLED || occ[e] != 0;
            }
            uint32_t prow, pcol, sample;
            path_pixel<Samp::PASS>(v, pix0, path, prow, pcol, sample, nullptr);
            push = shade_hit_shadowed(sc, v.maxdepth, seed, npaths, path, prow * v.width + pcol, sample, (uint32_t)pass, tf, t,
                                      V4{o4.x, o4.y, o4.z, o4.w}, V4{d4.x, d4.y, d4.z, d4.w}, shadowed, mstack, smask, scol, nr);
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
