// preview.hpp — the two elementwise kernels of the shaded preview (rtmi_render_preview*, include/rtmi.h defines it operation by
// operation).  The pass is a features pass (k_gen_samples, the scene's closest-hit launch, k_features when its
// buffers are asked for) whose hit records stay on the device, followed by what the AO pass (ao.hpp) and one direct-light pass
// per light (light.hpp) do, with the primary rays traced ONCE and every secondary ray in ONE queue and one any-hit walk:
//   k_preview_rays     primary ray + hit record of every path -> the path's albedo; Ka AO rays per path that HIT and, per light,
//                      its K_l candidates with c > 0 compacted into queue 1; the walk's ray count is the compaction's own
//                      counter (ctrl->count[1])
//   (the scene's any-hit walk of queue 1: k_occluded_oct / k_occluded_linear, or its closest-hit launch + k_ao_occl_from_hits)
//   k_preview_resolve  per pixel, sample after sample: the AO count and every light's fold -> the sample's colour -> the pixel's
//                      colour; the per-pixel counts and folds of the layers in the same pass
// Which queue entry a ray gets depends on the order of the blocks' atomics and is free: aslot[path] names a path's first AO
// entry, lslot[npaths * koff_l + path * K_l + k] a candidate's entry (ao.hpp's and light.hpp's slots), and the resolve visits
// them in the defined order.  Included by rtmi_device.hip.
#pragma once

namespace rtmi {

#define RTMI_PV_MAX_LIGHTS 4
// One light of a preview call as the kernels take it
struct PvLight {
    V4 orig;
    float len2, bias;
    uint32_t K, koff;     // koff: the sum of the K of the lights before this one (its slots start at npaths * koff)
    FastDiv dK;
    uint32_t unbounded;   // its rays' limit is +inf (rtmi_occluded's rule: the NULL limit)
    float col[3];
};
struct PvArgs {
    float amb[3];
    uint32_t nlights, Ka;  // Ka == 0: no AO rays, the factor is 1.f
    FastDiv dKa;
    float radius, abias;
    PvLight li[RTMI_PV_MAX_LIGHTS];
};

// The candidates of one light for the block's staged paths: k_light_rays' rounds (256 (hit path, k) pairs at a time, k fastest,
// live ones compacted with ballot + popcount per wave and ONE atomic per block of four waves on ctrl->count[1]).  Every thread
// of the block calls it with the same arguments (it has barriers).
__device__ __forceinline__ void preview_light_rounds(const PvLight& L, uint64_t seed, uint32_t blk0, uint32_t nb, uint32_t total,
                                                     const float (*s_pt)[256], const float (*s_n)[256], const uint32_t* s_pix,
                                                     const uint32_t* s_smp, const uint32_t* s_path, const uint8_t* s_hit,
                                                     uint32_t* s_cnt, uint32_t* s_base, float4* __restrict__ pq_o,
                                                     float4* __restrict__ pq_d, float* __restrict__ pq_tmax, float* __restrict__ pq_c,
                                                     uint32_t* __restrict__ slot, DCtrl* __restrict__ ctrl) {
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t K = L.K;
    for (uint32_t e = threadIdx.x; e < nb * K; e += 256u)
        if (!s_hit[fdiv(e, L.dK)]) store_stream(&slot[blk0 * K + e], RTMI_LIGHT_MISS);
    const uint32_t ncand = total * K;  // block-uniform
    for (uint32_t e0 = 0; e0 < ncand; e0 += 256u) {
        const uint32_t e = e0 + threadIdx.x;
        bool live = false;
        V4 o{}, dir{};
        float r = 0.f, c = 0.f;
        uint32_t cand = 0;
        if (e < ncand) {
            const uint32_t h = fdiv(e, L.dK), k = e - h * K;
            const V4 point{s_pt[0][h], s_pt[1][h], s_pt[2][h], s_pt[3][h]}, n{s_n[0][h], s_n[1][h], s_n[2][h], s_n[3][h]};
            uint32_t w[4];
            rng_block(seed, s_pix[h], s_smp[h], 0xC0000000u | k, w);
            const V4 adj{L.orig.x + u32_to_unit_f32(w[0]) * L.len2, L.orig.y + u32_to_unit_f32(w[1]) * L.len2,
                         L.orig.z + u32_to_unit_f32(w[2]) * L.len2, 0.f};
            const V4 vv = vsub(adj, point);
            r = sqrtf(vdot(vv, vv));
            dir = vmul(vv, 1.f / r);
            o = vadd(point, vmul(n, L.bias * (u32_to_unit_f32(w[3]) + 1.f)));
            c = vdot(n, dir);
            live = c > 0.f;  // false for the light behind the surface, for a NaN and for the light at the point
            cand = (blk0 + s_path[h]) * K + k;
        }
        const unsigned long long mask = __ballot(live);
        if (lane == 0) s_cnt[wv] = (uint32_t)__popcll(mask);
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t tot = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
            *s_base = tot ? atomicAdd(&ctrl->count[1], tot) : 0u;
        }
        uint32_t q = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
        for (uint32_t k = 0; k < wv; k++) q += s_cnt[k];
        __syncthreads();
        if (live) {
            q += *s_base;
            store_stream(&pq_o[q], make_float4(o.x, o.y, o.z, o.w));
            store_stream(&pq_d[q], make_float4(dir.x, dir.y, dir.z, dir.w));
            store_stream(&pq_tmax[q], L.unbounded ? INFINITY : r);
            store_stream(&pq_c[q], c);
            store_stream(&slot[cand], q);
        } else if (e < ncand) {
            store_stream(&slot[cand], RTMI_LIGHT_CULLED);
        }
        __syncthreads();  // s_cnt / s_base are rewritten by the next round
    }
}

// One thread per path; a block stages its paths that hit in LDS ONCE (hit point, shading normal, RNG key, the path's place in
// the block: what k_ao_rays and k_light_rays each stage) and stores every path's albedo (hit_features' a: the sky on a miss, 0
// on an edge face, lane 3 = 1 on a hit), which the resolve reads: the closest-hit fallback of the walk overwrites the hit
// records.  Then, with all 256 threads: the block's Ka AO rays per hit path, k fastest, at total * Ka consecutive entries
// claimed with one atomic (k_ao_rays' arithmetic: orig = point + n * bias, dir = unit(n + random_vec(block 0x80000000 | k)),
// limit = radius); then light after light, preview_light_rounds.
__global__ void __launch_bounds__(256) k_preview_rays(DScene sc, DView v, uint64_t seed, uint32_t pix0, uint32_t npaths, PvArgs pv,
                                                      const float4* __restrict__ qo, const float4* __restrict__ qd,
                                                      const uint32_t* __restrict__ hit_tf, const float* __restrict__ hit_t,
                                                      float4* __restrict__ pq_o, float4* __restrict__ pq_d, float* __restrict__ pq_tmax,
                                                      float* __restrict__ pq_c, uint32_t* __restrict__ aslot, uint32_t* __restrict__ lslot,
                                                      float4* __restrict__ palb, DCtrl* __restrict__ ctrl) {
    __shared__ uint32_t s_cnt[4], s_base;
    __shared__ float s_pt[4][256], s_n[4][256];  // [lane of the vector][compacted path of the block]
    __shared__ uint32_t s_pix[256], s_smp[256];  // the path's RNG key
    __shared__ uint32_t s_path[256];             // the path's index in the block
    __shared__ uint8_t s_hit[256];               // [path of the block]
    const uint32_t stride = gridDim.x * blockDim.x;
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t bound = (npaths + 255u) & ~255u;  // whole blocks stay converged for the ballots and the barriers
    const uint32_t Ka = pv.Ka;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < bound; i += stride) {
        const uint32_t blk0 = i - threadIdx.x, nb = min(256u, npaths - blk0);  // the block's paths: [blk0, blk0 + nb)
        bool hit = false;
        uint32_t tf = 0;
        if (i < npaths) {
            tf = hit_tf[i];
            hit = (tf & 0x3FFFFFFFu) != 0u;
            store_stream(&palb[i], hit_features(sc, tf, 0.f).a);
        }
        const unsigned long long hmask = __ballot(hit);
        if (lane == 0) s_cnt[wv] = (uint32_t)__popcll(hmask);
        s_hit[threadIdx.x] = hit ? (uint8_t)1 : (uint8_t)0;
        __syncthreads();
        const uint32_t total = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        if (threadIdx.x == 0) s_base = (total && Ka) ? atomicAdd(&ctrl->count[1], total * Ka) : 0u;
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
        __syncthreads();  // (the last read of s_cnt for the paths is behind this barrier: the lights' rounds rewrite it)
        if (Ka) {
            const uint32_t base = s_base;  // the block's first AO entry (read before the first round's barrier lets s_base go)
            if (i < npaths) aslot[i] = hit ? base + j * Ka : RTMI_AO_MISS;
            for (uint32_t e = threadIdx.x; e < total * Ka; e += 256u) {
                const uint32_t h = fdiv(e, pv.dKa), k = e - h * Ka;
                const V4 point{s_pt[0][h], s_pt[1][h], s_pt[2][h], s_pt[3][h]}, n{s_n[0][h], s_n[1][h], s_n[2][h], s_n[3][h]};
                const V4 rv = random_vec(seed, s_pix[h], s_smp[h], 0x80000000u | k);
                const V4 orig = vadd(point, vmul(n, pv.abias));
                const V4 dir = vunit(vadd(n, rv));
                store_stream(&pq_o[base + e], make_float4(orig.x, orig.y, orig.z, orig.w));
                store_stream(&pq_d[base + e], make_float4(dir.x, dir.y, dir.z, dir.w));
                store_stream(&pq_tmax[base + e], pv.radius);
            }
            __syncthreads();  // every thread has read s_base
        }
#pragma unroll
        for (uint32_t l = 0; l < RTMI_PV_MAX_LIGHTS; l++)
            if (l < pv.nlights)
                preview_light_rounds(pv.li[l], seed, blk0, nb, total, s_pt, s_n, s_pix, s_smp, s_path, s_hit, s_cnt, &s_base, pq_o, pq_d,
                                     pq_tmax, pq_c, lslot + (size_t)npaths * pv.li[l].koff, ctrl);
        __syncthreads();  // the staged paths, s_hit and s_cnt are rewritten by the next iteration
    }
}

// One thread per pixel: every sum of the definition is one lane's fold in the defined order, whatever Ka and the K_l are.  The
// pixel's samples are visited in order; per sample: its albedo, the integer count v of its visible AO rays (f = (float)v *
// (1.f / (float)Ka)), per light acc = acc + c over the live and visible candidates in k order (g_l = acc * (1.f / (float)K_l)),
// L = amb * f, L = L + col_l * g_l for l ascending, e = a * L (a miss: e = a), and the pixel's sum += e.  The layers in the same
// pass: the AO plane's integer count (a miss counts Ka, as k_ao_resolve has it), per light the integer count of visible rays (a
// miss counts K_l) and the fold of c over (sample, k) from 0.f (k_light_resolve's order).  Sub-tile and stripe addressing of the
// outputs is k_ao_resolve's; plane l of shadow / irradiance starts at l * plane.  A pixel reads Ka + sum K_l slots and bytes per
// sample: 12 of each at the defaults, against the walk that produced them.
__global__ void __launch_bounds__(256) k_preview_resolve(uint32_t npixels, uint32_t nsamples, uint32_t npaths, PvArgs pv,
                                                         const float4* __restrict__ palb, const uint32_t* __restrict__ aslot,
                                                         const uint32_t* __restrict__ lslot, const uint8_t* __restrict__ occ,
                                                         const float* __restrict__ pq_c, float4* __restrict__ color, float* __restrict__ ao,
                                                         float* __restrict__ shadow, float* __restrict__ irradiance, size_t plane,
                                                         uint32_t pix0, uint32_t W, uint32_t nsub, uint32_t sub, FastDiv dW) {
    const uint32_t stride = gridDim.x * blockDim.x;
    const uint32_t Ka = pv.Ka;
    const float inv_ka = 1.f / (float)Ka, inv_s = 1.f / (float)nsamples;
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < npixels; p += stride) {
        float cr = 0.f, cg = 0.f, cb = 0.f;
        uint32_t avis = 0;
        uint32_t lvis[RTMI_PV_MAX_LIGHTS] = {0u, 0u, 0u, 0u};
        float lacc[RTMI_PV_MAX_LIGHTS] = {0.f, 0.f, 0.f, 0.f};
        for (uint32_t s = 0; s < nsamples; s++) {
            const uint32_t path = p * nsamples + s;
            const float4 a = palb[path];
            float er = a.x, eg = a.y, eb = a.z;
            if (a.w != 0.f) {  // a hit
                float f = 1.f;
                if (Ka) {
                    const uint32_t b = aslot[path];
                    uint32_t vv = 0;
                    for (uint32_t k = 0; k < Ka; k++) vv += occ[b + k] == 0 ? 1u : 0u;
                    avis += vv;
                    f = (float)vv * inv_ka;
                }
                float Lr = pv.amb[0] * f, Lg = pv.amb[1] * f, Lb = pv.amb[2] * f;
#pragma unroll
                for (uint32_t l = 0; l < RTMI_PV_MAX_LIGHTS; l++) {
                    if (l < pv.nlights) {
                        const uint32_t K = pv.li[l].K;
                        const uint32_t* __restrict__ sl = lslot + (size_t)npaths * pv.li[l].koff + (size_t)path * K;
                        float acc = 0.f;
                        for (uint32_t k = 0; k < K; k++) {
                            const uint32_t b = sl[k];
                            if (b != RTMI_LIGHT_CULLED && occ[b] == 0) {
                                const float c = pq_c[b];
                                acc = acc + c;
                                lacc[l] = lacc[l] + c;
                                lvis[l]++;
                            }
                        }
                        const float g = acc * (1.f / (float)K);
                        Lr = Lr + pv.li[l].col[0] * g;
                        Lg = Lg + pv.li[l].col[1] * g;
                        Lb = Lb + pv.li[l].col[2] * g;
                    }
                }
                er = a.x * Lr; eg = a.y * Lg; eb = a.z * Lb;
            } else {
                avis += Ka;
#pragma unroll
                for (uint32_t l = 0; l < RTMI_PV_MAX_LIGHTS; l++)
                    if (l < pv.nlights) lvis[l] += pv.li[l].K;
            }
            cr = cr + er; cg = cg + eg; cb = cb + eb;
        }
        const uint32_t lp = pix0 + p, lr = fdiv(lp, dW), col = lp - lr * W;
        const size_t at = ((size_t)lr * nsub + sub) * W + col;
        if (color) store_stream(&color[at], make_float4(cr * inv_s, cg * inv_s, cb * inv_s, 0.f));
        if (ao) store_stream(&ao[at], (float)avis * (1.f / (float)(nsamples * Ka)));
#pragma unroll
        for (uint32_t l = 0; l < RTMI_PV_MAX_LIGHTS; l++) {
            if (l < pv.nlights) {
                const float inv = 1.f / (float)(nsamples * pv.li[l].K);
                if (shadow) store_stream(&shadow[(size_t)l * plane + at], (float)lvis[l] * inv);
                if (irradiance) store_stream(&irradiance[(size_t)l * plane + at], lacc[l] * inv);
            }
        }
    }
}

}  // namespace rtmi
