// bake.hpp — the two elementwise kernels of the light bake (rtmi_bake*, include/rtmi.h defines it operation by operation;
// DESIGN.md 4.21).  A bake is an explicit-ray render (rays.hpp) whose rays are made on the device: K Matte-bounce gather rays
// at each of M surface points, or at a uniformly drawn point of each of M triangles:
//   k_bake_rays   stands where k_rays_begin stands: element m's K rays -> queue entries m K .. m K + K - 1, the identity qpath
//                 and the queue's count
//   (per pass: the scene's closest-hit launch, k_shade_rays; k_accum folds an element's K colours to light[m])
//   k_bake_open   after pass 0: per element, the rays that hit nothing counted in integers -> one f32
// Every element has K rays, so there is no compaction and a ray's queue entry is fixed.  Included by rtmi_device.hip.
#pragma once

namespace rtmi {

#define RTMI_BAKE_STEP_MAX 256   // elements a block stages per step at most
#define RTMI_BAKE_STEP_RAYS 1024 // ... as many whole elements as make about this many rays (four per thread), at least one
inline uint32_t bake_step_elems(uint32_t K) { return std::min<uint32_t>(RTMI_BAKE_STEP_MAX, std::max<uint32_t>(1u, RTMI_BAKE_STEP_RAYS / K)); }

// A block takes `epb` consecutive elements per step (bake_step_elems(K): whole elements, so that what is computed per element
// is computed once).  Thread j stages element j of the step in LDS: its normal and its point (POINTS), or corner c0 and the
// edge vectors vsub(c1, c0), vsub(c2, c0) (TRIANGLES).  Then all 256 threads write the step's rays: thread e of the step's
// (element h, ray k) pairs, k fastest, so consecutive lanes store consecutive queue entries (k_ao_rays' layout).
// Arithmetic per ray (rtmi.h), all four lanes, shade.hpp's functions, key (seed, pix0 + element, k):
//   TRIANGLES: (u, v) = unit floats of words 0, 1 of block 0x20000000; if (u + v > 1.f) { u = 1.f - u; v = 1.f - v; }
//              point = (c0 + e1 * u) + e2 * v
//   rv = random_vec(block 0), orig = point + n * bias, dir = unit(n + rv)
// pos / nrm: the batch's elements (3 float4 per element when TRI); qo / qd: the batch's queue entries; pix0: the key of the
// batch's first element.
#define RTMI_BAKE_BLOCK_POINT 0x20000000u
template <bool TRI>
__global__ void __launch_bounds__(256) k_bake_rays(uint32_t nelems, uint32_t K, FastDiv dK, uint32_t epb, const float4* __restrict__ pos,
                                                   const float4* __restrict__ nrm, uint64_t seed, uint32_t pix0, float bias,
                                                   float4* __restrict__ qo, float4* __restrict__ qd, uint32_t* __restrict__ qpath,
                                                   DCtrl* __restrict__ ctrl) {
    __shared__ float s_pt[TRI ? 12 : 4][RTMI_BAKE_STEP_MAX], s_n[4][RTMI_BAKE_STEP_MAX];  // [lane of the vector][element of the step]
    const uint32_t nsteps = (nelems + epb - 1u) / epb;
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
        const uint32_t base = m0 * K, nrays = cnt * K;  // the step's first queue entry (nelems * K < 2^31)
        for (uint32_t e = threadIdx.x; e < nrays; e += 256u) {
            const uint32_t h = fdiv(e, dK), k = e - h * K;
            const uint32_t pixel = pix0 + m0 + h;
            const V4 n{s_n[0][h], s_n[1][h], s_n[2][h], s_n[3][h]};
            V4 point{s_pt[0][h], s_pt[1][h], s_pt[2][h], s_pt[3][h]};
            if constexpr (TRI) {
                uint32_t w[4];
                rng_block(seed, pixel, k, RTMI_BAKE_BLOCK_POINT, w);
                float u = u32_to_unit_f32(w[0]), v = u32_to_unit_f32(w[1]);
                if (u + v > 1.f) { u = 1.f - u; v = 1.f - v; }  // the fold of the unit square onto the triangle: area-preserving
                const V4 e1{s_pt[4][h], s_pt[5][h], s_pt[6][h], s_pt[7][h]}, e2{s_pt[8][h], s_pt[9][h], s_pt[10][h], s_pt[11][h]};
                point = vadd(vadd(point, vmul(e1, u)), vmul(e2, v));
            }
            const V4 rv = random_vec(seed, pixel, k, 0u);
            const V4 orig = vadd(point, vmul(n, bias));
            const V4 dir = vunit(vadd(n, rv));
            store_stream(&qo[base + e], make_float4(orig.x, orig.y, orig.z, orig.w));
            store_stream(&qd[base + e], make_float4(dir.x, dir.y, dir.z, dir.w));
            qpath[base + e] = base + e;
        }
        __syncthreads();  // the staged elements are rewritten by the next step
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) ctrl->count[0] = nelems * K;
}

// The point gather ray k of a TRIANGLES element starts from, for what else is computed there (lit.hpp's k_bake_lit_rays: the lamps'
// candidates at the element): k_bake_rays' draw and fold above, operation for operation.  c0, e1, e2 as k_bake_rays stages them.
__device__ inline V4 bake_triangle_point(uint64_t seed, uint32_t pixel, uint32_t k, V4 c0, V4 e1, V4 e2) {
    uint32_t w[4];
    rng_block(seed, pixel, k, RTMI_BAKE_BLOCK_POINT, w);
    float u = u32_to_unit_f32(w[0]), v = u32_to_unit_f32(w[1]);
    if (u + v > 1.f) { u = 1.f - u; v = 1.f - v; }
    return vadd(vadd(c0, vmul(e1, u)), vmul(e2, v));
}

// Eight lanes per element (k_ao_resolve's grouping: a block takes 32 consecutive elements).  Lane l counts the misses (tri == 0)
// among entries l, l + 8, ... of the element's K hit records of pass 0; consecutive lanes read consecutive words.  The eight
// counts are added across the lanes and lane 0 stores open = (float)misses * (1.f / (float)K): integers, so the order is free.
#define RTMI_BAKE_OPEN_ELEMS 32
__global__ void __launch_bounds__(256) k_bake_open(uint32_t nelems, uint32_t K, const uint32_t* __restrict__ hit_tf, float* __restrict__ open) {
    const uint32_t j = threadIdx.x >> 3, l = threadIdx.x & 7u;
    const float inv = 1.f / (float)K;
    // the bound is rounded up to whole blocks: the shuffles below need all eight lanes of an element's group
    for (uint32_t mb = blockIdx.x * RTMI_BAKE_OPEN_ELEMS; mb < nelems; mb += gridDim.x * RTMI_BAKE_OPEN_ELEMS) {
        const uint32_t m = mb + j;
        uint32_t misses = 0;
        if (m < nelems) {
            const uint32_t* __restrict__ tf = hit_tf + (size_t)m * K;
            for (uint32_t e = l; e < K; e += 8u) misses += (tf[e] & 0x3FFFFFFFu) == 0u ? 1u : 0u;
        }
        misses += __shfl_xor(misses, 1, 8);
        misses += __shfl_xor(misses, 2, 8);
        misses += __shfl_xor(misses, 4, 8);
        if (m < nelems && l == 0u) store_stream(&open[m], (float)misses * inv);
    }
}

}  // namespace rtmi
