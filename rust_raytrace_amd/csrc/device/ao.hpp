// ao.hpp — the two elementwise kernels of the ambient-occlusion pass (rtmi_render_ao*, include/rtmi.h defines it operation
// by operation) and the two one-thread kernels that keep its ray count on the device.  The pass is a features
// pass (k_gen_samples, the scene's closest-hit launch) whose hit records stay on the device:
//   k_ao_rays     primary ray + hit record of every path -> K hemisphere rays per path that HIT, compacted
//   k_ao_count    ctrl->count[1] = compacted paths * K: the any-hit launch drains queue 1 of the batch's control block
//   (the scene's any-hit walk of queue 1: k_occluded_oct / k_occluded_linear, or its closest-hit launch + k_ao_occl_from_hits)
//   k_ao_resolve  per pixel: visible rays counted in integers -> one f32
// A path that missed gets no slot and costs no walk (80 % of the canonical view's samples; a ray that hits nothing is the one
// kind the any-hit walk cannot retire early).  Which slot a path's rays get depends on the order of the blocks' atomics and is
// free: the result is a count.  Included by rtmi_device.hip.
#pragma once

namespace rtmi {

#define RTMI_AO_MISS 0xFFFFFFFFu  // slot[path] of a path whose primary ray missed (slots are < 2^31)
#define RTMI_AO_HITS 2            // ctrl->count[RTMI_AO_HITS]: paths compacted so far (an AO batch has no pass 2)

// One thread per path; a block compacts its paths that hit (ballot + popcount per wave, ONE atomic per block of four waves,
// as shade_pass does and for its reason), leaves each one's hit point and shading normal in LDS and then writes the block's
// rays with all 256 threads: thread e of the block's (hit path j, ray k) pairs, k fastest, so consecutive lanes store
// consecutive queue entries.  Arithmetic per ray (rtmi.h): point = rd * t + ro, n = norm * (-1.f on a back face),
// rv = random_vec(block 0x80000000 | k), orig = point + n * bias, dir = unit(n + rv); all four lanes, shade.hpp's functions.
// tmax: null when the radius is +inf (the walk's null tmax), else one float per ray.
__global__ void __launch_bounds__(256) k_ao_rays(DScene sc, DView v, uint64_t seed, uint32_t pix0, uint32_t npaths, uint32_t K, FastDiv dK,
                                                 float radius, float bias, const float4* __restrict__ qo, const float4* __restrict__ qd,
                                                 const uint32_t* __restrict__ hit_tf, const float* __restrict__ hit_t,
                                                 float4* __restrict__ ao_o, float4* __restrict__ ao_d, float* __restrict__ ao_tmax,
                                                 uint32_t* __restrict__ slot, DCtrl* __restrict__ ctrl) {
    __shared__ uint32_t s_cnt[4], s_base;
    __shared__ float s_pt[4][256], s_n[4][256];  // [lane of the vector][compacted path of the block]
    __shared__ uint32_t s_pix[256], s_smp[256];  // the path's RNG key
    const uint32_t stride = gridDim.x * blockDim.x;
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t bound = (npaths + 255u) & ~255u;  // whole blocks stay converged for the ballot and the barriers
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < bound; i += stride) {
        bool hit = false;
        uint32_t tf = 0;
        if (i < npaths) {
            tf = hit_tf[i];
            hit = (tf & 0x3FFFFFFFu) != 0u;
        }
        const unsigned long long mask = __ballot(hit);
        if (lane == 0) s_cnt[wv] = (uint32_t)__popcll(mask);
        __syncthreads();
        const uint32_t total = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        if (threadIdx.x == 0) s_base = total ? atomicAdd(&ctrl->count[RTMI_AO_HITS], total) : 0u;
        uint32_t j = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
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
        }
        __syncthreads();
        const uint32_t base = s_base * K;  // the block's first queue entry
        if (i < npaths) slot[i] = hit ? base + j * K : RTMI_AO_MISS;
        for (uint32_t e = threadIdx.x; e < total * K; e += 256u) {
            const uint32_t h = fdiv(e, dK), k = e - h * K;
            const V4 point{s_pt[0][h], s_pt[1][h], s_pt[2][h], s_pt[3][h]}, n{s_n[0][h], s_n[1][h], s_n[2][h], s_n[3][h]};
            const V4 rv = random_vec(seed, s_pix[h], s_smp[h], 0x80000000u | k);
            const V4 orig = vadd(point, vmul(n, bias));
            const V4 dir = vunit(vadd(n, rv));
            store_stream(&ao_o[base + e], make_float4(orig.x, orig.y, orig.z, orig.w));
            store_stream(&ao_d[base + e], make_float4(dir.x, dir.y, dir.z, dir.w));
            if (ao_tmax) store_stream(&ao_tmax[base + e], radius);
        }
        __syncthreads();  // s_cnt / s_base and the staged paths are rewritten by the next iteration
    }
}

// The ray count of the any-hit launch, set where the compaction left it: no host round trip between the two walks
__global__ void k_ao_count(DCtrl* ctrl, uint32_t K) { ctrl->count[1] = ctrl->count[RTMI_AO_HITS] * K; }

// k_occl_from_hits for queue `pass` of the control block (generic tree, RTMI_OPT_GENERIC, RTMI_OPT_BVH): the same rule with the
// count read on the device
__global__ void __launch_bounds__(256) k_ao_occl_from_hits(const DCtrl* __restrict__ ctrl, int pass, const uint32_t* __restrict__ hit_tf,
                                                           const float* __restrict__ hit_t, const float* __restrict__ tmax,
                                                           uint8_t* __restrict__ occ) {
    const uint32_t n = ctrl->count[pass], stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        occ[i] = ((hit_tf[i] & 0x3FFFFFFFu) != 0u && hit_t[i] < (tmax ? tmax[i] : INFINITY)) ? (uint8_t)1 : (uint8_t)0;
}

// Eight lanes per pixel (k_features' grouping: a block takes 32 consecutive pixels).  Lane l counts the visible rays among
// entries l, l + 8, ... of the pixel's nsamples * K (sample, ray) pairs: 1 for every ray of a sample that missed, 1 for a zero
// answer byte otherwise; consecutive lanes read consecutive bytes.  The eight counts are added across the lanes and lane 0
// stores ao = (float)visible * (1.f / (float)(nsamples * K)): integers below 2^24, so the order of the additions is free.
// Sub-tile and stripe addressing of `out` (one f32 per pixel of the tile) is accum_pixels<Samp::PASS>'s.
#define RTMI_AO_PIX 32
__global__ void __launch_bounds__(256) k_ao_resolve(uint32_t npixels, uint32_t nsamples, uint32_t K, FastDiv dK, const uint32_t* __restrict__ slot,
                                                    const uint8_t* __restrict__ occ, float* __restrict__ out, uint32_t pix0, uint32_t W,
                                                    uint32_t nsub, uint32_t sub, FastDiv dW) {
    const uint32_t j = threadIdx.x >> 3, l = threadIdx.x & 7u;
    const uint32_t per = nsamples * K;
    const float inv = 1.f / (float)per;
    // the bound is rounded up to whole blocks: the shuffles below need all eight lanes of a pixel's group
    for (uint32_t pb = blockIdx.x * RTMI_AO_PIX; pb < npixels; pb += gridDim.x * RTMI_AO_PIX) {
        const uint32_t p = pb + j;
        uint32_t vis = 0;
        if (p < npixels) {
            const uint32_t* __restrict__ sl = slot + (size_t)p * nsamples;
            for (uint32_t e = l; e < per; e += 8u) {
                const uint32_t s = fdiv(e, dK), k = e - s * K;
                const uint32_t b = sl[s];
                vis += b == RTMI_AO_MISS ? 1u : (occ[b + k] == 0 ? 1u : 0u);
            }
        }
        vis += __shfl_xor(vis, 1, 8);
        vis += __shfl_xor(vis, 2, 8);
        vis += __shfl_xor(vis, 4, 8);
        if (p < npixels && l == 0u) {
            const uint32_t lp = pix0 + p, lr = fdiv(lp, dW), col = lp - lr * W;
            store_stream(&out[((size_t)lr * nsub + sub) * W + col], (float)vis * inv);
        }
    }
}

}  // namespace rtmi
