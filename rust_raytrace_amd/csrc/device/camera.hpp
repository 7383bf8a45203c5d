// camera.hpp — the built-in camera models of rtmi_render_camera* (include/rtmi.h states every operation):
// the pinhole (Viewport::pixel_ray itself), an orthographic camera and a thin lens, generated on the device.
//   k_gen_camera   a Samp::PASS generator: it stands where k_gen_samples stands in a progressive pass of the per-pass pipeline
//   (everything after it is that pass's own: the scene's closest-hit launch and k_shade_samples per pass, k_accum_samples;
//   k_features after pass 0 for the guides)
// The RNG key of a path stays (pixel, sample): its bounces draw blocks 1.. as ever; the lens draws blocks 0x40000000 | k.
// Included by rtmi_device.hip.
#pragma once

namespace rtmi {

// rtmi_camera_t as the kernel takes it (an argument of k_gen_camera alone: DView, which every kernel takes, is unchanged)
struct DCam { uint32_t model; float lens_radius, focus; };

#define RTMI_LENS_BLOCK 0x40000000u

// The lens sample of (pixel, sample): the first of four candidates in [-1, 1)^2 that lies in the unit disc, else (0, 0).
// Candidate 2 k + j comes from words 2 j and 2 j + 1 of block RTMI_LENS_BLOCK | k.
__device__ inline void lens_sample(uint64_t seed, uint32_t pixel, uint32_t sample, float& x, float& y) {
    x = 0.f; y = 0.f;
    for (uint32_t k = 0; k < 2u; k++) {
        uint32_t w[4];
        rng_block(seed, pixel, sample, RTMI_LENS_BLOCK | k, w);
        for (uint32_t j = 0; j < 2u; j++) {
            const float cx = 2.f * u32_to_unit_f32(w[2u * j]) - 1.f, cy = 2.f * u32_to_unit_f32(w[2u * j + 1u]) - 1.f;
            if ((cx * cx) + (cy * cy) <= 1.f) { x = cx; y = cy; return; }
        }
    }
}

// The ray of (row, col, sample).  p is pixel_ray's image-plane point (make_ray keeps the origin as given), so the pinhole is
// pixel_ray's own ray.
__device__ inline RayV camera_ray(const DView& v, const DCam& cam, uint32_t row, uint32_t col, uint64_t seed, uint32_t pixel,
                                  uint32_t sample) {
    const RayV pin = pixel_ray<Samp::PASS>(v, row, col, seed, pixel, sample);
    if (cam.model == RTMI_CAMERA_PINHOLE) return pin;
    const V4 p = pin.orig;
    if (cam.model == RTMI_CAMERA_ORTHO) {
        const V4 c = vadd(vadd(v.orig, vmul(v.vu, 0.5f)), vmul(v.vv, 0.5f));
        return make_ray(p, vunit(vsub(c, v.cam)));
    }
    const V4 eu = vunit(v.vu), ev = vunit(v.vv);
    float x, y;
    lens_sample(seed, pixel, sample, x, y);
    const V4 o = vadd(vmul(eu, x * cam.lens_radius), vmul(ev, y * cam.lens_radius));
    const V4 e = vsub(p, v.cam);
    const V4 F = vadd(v.cam, vmul(e, cam.focus));
    const V4 O = vadd(p, vmul(o, 1.f - 1.f / cam.focus));
    return make_ray(O, vunit(vsub(F, vadd(v.cam, o))));
}

// gen_paths<Samp::PASS> with camera_ray for pixel_ray
__global__ void __launch_bounds__(256) k_gen_camera(DView v, DCam cam, RTMI_GEN_PARAMS) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t path = blockIdx.x * blockDim.x + threadIdx.x; path < npaths; path += stride) {
        uint32_t row, col, sample;
        path_pixel<Samp::PASS>(v, pix0, path, row, col, sample, nullptr);
        const RayV r = camera_ray(v, cam, row, col, seed, row * v.width + col, sample);
        qo[path] = make_float4(r.orig.x, r.orig.y, r.orig.z, r.orig.w);
        qd[path] = make_float4(r.dir.x, r.dir.y, r.dir.z, r.dir.w);
        qpath[path] = path;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) ctrl->count[0] = npaths;
}

}  // namespace rtmi
