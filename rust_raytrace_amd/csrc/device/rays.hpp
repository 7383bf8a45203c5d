// rays.hpp — the two elementwise kernels of the explicit-ray calls (rtmi_render_rays*, rtmi_trace_device; include/rtmi.h
// defines them).  An explicit-ray render is the per-pass pipeline with the caller's rays where k_gen's would be:
//   k_rays_begin   stands where k_gen stands: queue 0 is the rays themselves, so only the identity qpath and the queue's count
//                  are written; with RTMI_RAYS_MAKE_RAY it also writes make_ray's unit directions to the workspace queue
//   (per pass: the scene's closest-hit launch, k_shade_rays = shade_pass<Samp::RAYS>; after pass 0 k_features for the guides)
//   (k_accum folds a batch's sample colours to the groups' means: a "tile" one pixel-row long)
//   k_unpack_hits  rtmi_trace_device: the workspace's hit records -> the caller's tri / t / face
// Included by rtmi_device.hip.
#pragma once

namespace rtmi {

// dir_in == null: the directions are used as given and qd is not touched.  Otherwise qd[i] = vunit(dir_in[i]): the ordered
// four-lane dot and v * (1.f / sqrt(.)) of make_ray (raytrace.rs:201-210, :93-96).  dir_in and qd may be the same buffer (the
// host variant normalises its staged copy in place): every thread reads its own element before it writes it.
__global__ void __launch_bounds__(256) k_rays_begin(uint32_t n, const float4* dir_in, float4* qd, uint32_t* __restrict__ qpath,
                                                    DCtrl* __restrict__ ctrl) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        if (dir_in) {
            const float4 d = dir_in[i];
            const V4 u = vunit(V4{d.x, d.y, d.z, d.w});
            qd[i] = make_float4(u.x, u.y, u.z, u.w);
        }
        qpath[i] = i;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) ctrl->count[0] = n;
}

// tri = hit_tf & 0x3FFFFFFF (0 = miss), face = hit_tf >> 30 (0 front, 1 back, 2 edge front, 3 edge back), t as traced: what
// rtmi_trace does on the host after its copy.
__global__ void __launch_bounds__(256) k_unpack_hits(uint32_t n, const uint32_t* __restrict__ hit_tf, const float* __restrict__ hit_t,
                                                     uint32_t* __restrict__ tri, float* __restrict__ t, uint32_t* __restrict__ face) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t tf = hit_tf[i];
        tri[i] = tf & 0x3FFFFFFFu;
        face[i] = tf >> 30;
        t[i] = hit_t[i];
    }
}

}  // namespace rtmi
