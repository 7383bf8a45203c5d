// light.hpp — the two elementwise kernels of the direct-light pass (rtmi_render_light*, include/rtmi.h defines it operation by
// operation).  The pass is a features pass (k_gen_samples, the scene's closest-hit launch) whose hit records
// stay on the device, as for ambient occlusion (ao.hpp), with three differences: a candidate ray whose surface faces away from
// its light sample is never queued (compaction per RAY, not per path), every ray has its own limit (the distance to its light
// sample), and the second output is a float sum whose order of addition is defined.
//   k_light_rays     primary ray + hit record of every path -> K candidate shadow rays per path that HIT; those with c > 0
//                    compacted into queue 1, the count of the any-hit launch is the compaction's own counter (ctrl->count[1])
//   (the scene's any-hit walk of queue 1: k_occluded_oct / k_occluded_linear, or its closest-hit launch + k_ao_occl_from_hits)
//   k_light_resolve  per pixel: visible rays counted in integers -> shadow, their c added in (sample, k) order -> irradiance
// Which queue entry a ray gets depends on the order of the blocks' atomics and is free: slot[path * K + k] names it, and the
// resolve visits the slots in the defined order.  Included by rtmi_device.hip.
#pragma once

namespace rtmi {

#define RTMI_LIGHT_MISS 0xFFFFFFFFu    // slot of every candidate of a path whose primary ray missed (entries are < 2^31)
#define RTMI_LIGHT_CULLED 0xFFFFFFFEu  // slot of a candidate that was not traced: !(c > 0.f)

// One thread per path; a block stages its paths that hit in LDS as k_ao_rays does (hit point, shading normal, RNG key, and
// the path's place in the block) and writes the sentinel of the paths that missed.  All 256 threads then run over the block's
// (hit path j, ray k) pairs, k fastest, 256 at a time: each builds one candidate (rtmi.h: adj = orig + u * len2 per lane,
// v = adj - point, r = sqrt(ordered dot), dir = v * (1.f / r), o = point + n * (bias * (u_3 + 1.f)), c = ordered dot(n, dir);
// all four lanes, one Philox block 0xC0000000 | k per candidate) and tests c > 0.f.  The live ones are compacted per ray:
// ballot + popcount per wave, ONE atomic per block of four waves on ctrl->count[1] (as shade_pass and k_ao_rays do, and for
// their reason), so consecutive live lanes store consecutive queue entries.  tmax: null when the light is unbounded (the
// walk's null tmax), else the ray's r.
__global__ void __launch_bounds__(256) k_light_rays(DScene sc, DView v, uint64_t seed, uint32_t pix0, uint32_t npaths, uint32_t K, FastDiv dK,
                                                    V4 lorig, float len2, float bias, const float4* __restrict__ qo,
                                                    const float4* __restrict__ qd, const uint32_t* __restrict__ hit_tf,
                                                    const float* __restrict__ hit_t, float4* __restrict__ lq_o, float4* __restrict__ lq_d,
                                                    float* __restrict__ lq_tmax, float* __restrict__ lq_c, uint32_t* __restrict__ slot,
                                                    DCtrl* __restrict__ ctrl) {
    __shared__ uint32_t s_cnt[4], s_base;
    __shared__ float s_pt[4][256], s_n[4][256];  // [lane of the vector][compacted path of the block]
    __shared__ uint32_t s_pix[256], s_smp[256];  // the path's RNG key
    __shared__ uint32_t s_path[256];             // the path's index in the block
    __shared__ uint8_t s_hit[256];               // [path of the block]
    const uint32_t stride = gridDim.x * blockDim.x;
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t bound = (npaths + 255u) & ~255u;  // whole blocks stay converged for the ballots and the barriers
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < bound; i += stride) {
        const uint32_t blk0 = i - threadIdx.x, nb = min(256u, npaths - blk0);  // the block's paths: [blk0, blk0 + nb)
        bool hit = false;
        uint32_t tf = 0;
        if (i < npaths) {
            tf = hit_tf[i];
            hit = (tf & 0x3FFFFFFFu) != 0u;
        }
        const unsigned long long hmask = __ballot(hit);
        if (lane == 0) s_cnt[wv] = (uint32_t)__popcll(hmask);
        s_hit[threadIdx.x] = hit ? (uint8_t)1 : (uint8_t)0;
        __syncthreads();
        const uint32_t total = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        uint32_t j = (uint32_t)__popcll(hmask & ((1ull << lane) - 1ull));
        for (uint32_t k = 0; k < wv; k++) j += s_cnt[k];
        if (hit) {
            const float t = hit_t[i];
            const float4 o4 = qo[i], d4 = qd[i];
            const V4 point = vadd(vmul(V4{d4.x, d4.y, d4.z, d4.w}, t), V4{o4.x, o4.y, o4.z, o4.w});
            const float4 p1 = sc.tplane[2 * (tf & 0x3FFFFFFFu) + 1];
            V4 n = mk(p1.x, p1.y, p1.z);
            if ((tf >> 30) & 1u) n = vmul(n, -1.f);
            s_pt[0][j] = point.x; s_pt[1][j] = point.y; s_pt[2][j] = point.z; s_pt[3][j] = point.w;
            s_n[0][j] = n.x; s_n[1][j] = n.y; s_n[2][j] = n.z; s_n[3][j] = n.w;
            uint32_t row, col, sample;
            path_pixel<Samp::PASS>(v, pix0, i, row, col, sample, nullptr);
            s_pix[j] = row * v.width + col;
            s_smp[j] = sample;
            s_path[j] = threadIdx.x;
        }
        __syncthreads();  // (the last read of s_cnt for the paths is behind this barrier: the loop below rewrites it)
        for (uint32_t e = threadIdx.x; e < nb * K; e += 256u)
            if (!s_hit[fdiv(e, dK)]) store_stream(&slot[blk0 * K + e], RTMI_LIGHT_MISS);
        const uint32_t ncand = total * K;  // block-uniform
        for (uint32_t e0 = 0; e0 < ncand; e0 += 256u) {
            const uint32_t e = e0 + threadIdx.x;
            bool live = false;
            V4 o{}, dir{};
            float r = 0.f, c = 0.f;
            uint32_t cand = 0;
            if (e < ncand) {
                const uint32_t h = fdiv(e, dK), k = e - h * K;
                const V4 point{s_pt[0][h], s_pt[1][h], s_pt[2][h], s_pt[3][h]}, n{s_n[0][h], s_n[1][h], s_n[2][h], s_n[3][h]};
                uint32_t w[4];
                rng_block(seed, s_pix[h], s_smp[h], 0xC0000000u | k, w);
                const V4 adj{lorig.x + u32_to_unit_f32(w[0]) * len2, lorig.y + u32_to_unit_f32(w[1]) * len2,
                             lorig.z + u32_to_unit_f32(w[2]) * len2, 0.f};
                const V4 vv = vsub(adj, point);
                r = sqrtf(vdot(vv, vv));
                dir = vmul(vv, 1.f / r);
                o = vadd(point, vmul(n, bias * (u32_to_unit_f32(w[3]) + 1.f)));
                c = vdot(n, dir);
                live = c > 0.f;  // false for the light behind the surface, for a NaN and for the light at the point
                cand = (blk0 + s_path[h]) * K + k;
            }
            const unsigned long long mask = __ballot(live);
            if (lane == 0) s_cnt[wv] = (uint32_t)__popcll(mask);
            __syncthreads();
            if (threadIdx.x == 0) {
                const uint32_t tot = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
                s_base = tot ? atomicAdd(&ctrl->count[1], tot) : 0u;
            }
            uint32_t q = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
            for (uint32_t k = 0; k < wv; k++) q += s_cnt[k];
            __syncthreads();
            if (live) {
                q += s_base;
                store_stream(&lq_o[q], make_float4(o.x, o.y, o.z, o.w));
                store_stream(&lq_d[q], make_float4(dir.x, dir.y, dir.z, dir.w));
                if (lq_tmax) store_stream(&lq_tmax[q], r);
                store_stream(&lq_c[q], c);
                store_stream(&slot[cand], q);
            } else if (e < ncand) {
                store_stream(&slot[cand], RTMI_LIGHT_CULLED);
            }
            __syncthreads();  // s_cnt / s_base are rewritten by the next round
        }
        __syncthreads();  // the staged paths, s_hit and s_cnt are rewritten by the next iteration
    }
}

// Eight lanes per pixel (k_ao_resolve's grouping: a block takes 32 consecutive pixels).  The pixel's nsamples * K slots are
// consecutive (sample order, then k) and are visited eight at a time, lane l reading slot e0 + l, its answer byte and its c.
// visible: a MISS slot, or a live ray whose answer byte is 0; counted in integers, added across the lanes at the end (below
// 2^24: the order is free).  irradiance: acc = acc + c for the visible live rays IN SLOT ORDER: the eight terms of a round are
// passed round the group with __shfl and every lane of the group adds them in lane order, so acc is the same one-lane fold in
// all eight lanes; rounds follow each other in e0 order.  Lane 0 stores (float)visible * inv and acc * inv, inv = 1.f /
// (float)(nsamples * K).  Sub-tile and stripe addressing of the planes (one f32 per pixel of the tile) is k_ao_resolve's.
#define RTMI_LIGHT_PIX 32
__global__ void __launch_bounds__(256) k_light_resolve(uint32_t npixels, uint32_t per, const uint32_t* __restrict__ slot,
                                                       const uint8_t* __restrict__ occ, const float* __restrict__ lq_c,
                                                       float* __restrict__ shadow, float* __restrict__ irradiance, uint32_t pix0, uint32_t W,
                                                       uint32_t nsub, uint32_t sub, FastDiv dW) {
    const uint32_t j = threadIdx.x >> 3, l = threadIdx.x & 7u;
    const float inv = 1.f / (float)per;
    // the bound is rounded up to whole blocks: the shuffles below need all eight lanes of a pixel's group
    for (uint32_t pb = blockIdx.x * RTMI_LIGHT_PIX; pb < npixels; pb += gridDim.x * RTMI_LIGHT_PIX) {
        const uint32_t p = pb + j;
        uint32_t vis = 0;
        float acc = 0.f;
        for (uint32_t e0 = 0; e0 < per; e0 += 8u) {
            const uint32_t e = e0 + l;
            uint32_t lit = 0;  // 1: this slot's ray is live and visible
            float c = 0.f;
            if (p < npixels && e < per) {
                const uint32_t b = slot[(size_t)p * per + e];
                if (b == RTMI_LIGHT_MISS) vis++;
                else if (b != RTMI_LIGHT_CULLED && occ[b] == 0) { vis++; lit = 1u; c = lq_c[b]; }
            }
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const uint32_t lq = __shfl(lit, q, 8);
                const float cq = __shfl(c, q, 8);
                if (lq) acc = acc + cq;
            }
        }
        vis += __shfl_xor(vis, 1, 8);
        vis += __shfl_xor(vis, 2, 8);
        vis += __shfl_xor(vis, 4, 8);
        if (p < npixels && l == 0u) {
            const uint32_t lp = pix0 + p, lr = fdiv(lp, dW), col = lp - lr * W;
            const size_t at = ((size_t)lr * nsub + sub) * W + col;
            if (shadow) store_stream(&shadow[at], (float)vis * inv);
            if (irradiance) store_stream(&irradiance[at], acc * inv);
        }
    }
}

}  // namespace rtmi
