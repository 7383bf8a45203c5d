// lit_shade_kernel.hpp -- the text of lit.hpp's shading kernel (after `template <bool ENV>`), included there once per sampling mode
// (no include guard) with RTMI_LIT_KERNEL and RTMI_LIT_KEYS_PARAM as in lit_rays_kernel.hpp and
//   RTMI_LIT_SHADE_KEY    the statements that declare `sample` and what RTMI_LIT_SHADE_PIXEL names, the RNG key of `path`
//   RTMI_LIT_SHADE_PIXEL  the key's pixel
//   RTMI_LIT_SHADE_HIT    the shading function: shade_hit_lit<ENV>, or for the kernels of scenes with surface features (no template
//                         line; RTMI_LIT_KEYS_PARAM then ends with the tables and the colour stack) a macro that appends them
__global__ void __launch_bounds__(256) RTMI_LIT_KERNEL(DScene sc, DView v, uint64_t seed, uint32_t pix0, uint32_t npaths, int pass, EnvTab env,
                                                   uint32_t nlights, const float4* __restrict__ qo, const float4* __restrict__ qd,
                                                   const uint32_t* __restrict__ qpath, const uint32_t* __restrict__ hit_tf,
                                                   const float* __restrict__ hit_t, const uint32_t* __restrict__ slot,
                                                   const uint8_t* __restrict__ occ, const float4* __restrict__ lw,
                                                   float4* __restrict__ qo_n, float4* __restrict__ qd_n, uint32_t* __restrict__ qpath_n,
                                                   uint16_t* __restrict__ mstack, float4* __restrict__ dstack, float4* __restrict__ scol,
                                                   DCtrl* __restrict__ ctrl RTMI_LIT_KEYS_PARAM) {
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
            RTMI_LIT_SHADE_KEY
            push = RTMI_LIT_SHADE_HIT(sc, env, v.maxdepth, seed, npaths, path, RTMI_LIT_SHADE_PIXEL, sample, (uint32_t)pass, tf, t,
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
