// ray_walk.h -- the per-ray stage's arithmetic, stated once for the kernels that walk a ray's slots 0..SR-1 (its
// selected samples, then the zero-position padding slots of sample_loc_tensor, worldcoords.py:835): composite.hip's
// k_composite, k_ray_march_dense and k_early_stop_tier, loss.hip's ray_forward and k_loss_bwd.  Replaces
//   ray_dist        neural_points_volumetric_model.py:569-577 (cummax of pers z, last interval vsize[2],
//                   raydist_mode_unit replacement, * ray_valid)
//   ray_march       diff_ray_marching.py:509-555 with alpha_blend / radiance_render (diff_render_func.py:36-49):
//                   o = 1 - exp(-sigma*dist), T = exclusive cumprod(1 - o + 1e-10)
// Built with -ffp-contract=off, every caller gets the same bits: the early-stop bound and "the training step's
// colour is the renderer's" rest on that.  What differs between the callers on purpose: DESIGN.md §1.7.
#pragma once

#include <hip/hip_runtime.h>

namespace sgn {

// camera-space depth of a world position: ((x - c0) r2 + (y - c1) r5) + (z - c2) r8, every operation rounded
__device__ __forceinline__ float pers_z(const float *campos, const float *rot, float x, float y, float z) {
    const float sx = __fsub_rn(x, campos[0]), sy = __fsub_rn(y, campos[1]), sz = __fsub_rn(z, campos[2]);
    return __fadd_rn(__fadd_rn(__fmul_rn(sx, rot[2]), __fmul_rn(sy, rot[5])), __fmul_rn(sz, rot[8]));
}

// sample id's depth
__device__ __forceinline__ float sample_z(const float *campos, const float *rot, const float *samp_locw, int64_t id) {
    return pers_z(campos, rot, samp_locw[id * 3], samp_locw[id * 3 + 1], samp_locw[id * 3 + 2]);
}

// The running cummax at slot s (depth z): returns the new cummax, raw = its step from the previous one -- the
// raw interval of slot s - 1.  Slot 0 takes its own z (its raw is not an interval).
__device__ __forceinline__ float cummax_step(int s, float prev_cm, float z, float &raw) {
    const float cm = s == 0 ? z : fmaxf(prev_cm, z);
    raw = cm - prev_cm;
    return cm;
}

struct SlotClose {
    float dist, e, o;  // the slot's distance, exp(-sigma dist), opacity
};

// o = 1 - exp(-sigma dist)
__device__ __forceinline__ SlotClose opacity(float sigma, float dist) {
    const float e = expf(-sigma * dist);
    return {dist, e, 1.f - e};
}

// A slot closes with the raw interval to the next slot's cummax (a full ray's last slot: vz): the distance
// replacement (below 1e-8, or in unit mode above 2 vz: vz), then distance and sigma times the slot's validity.
__device__ __forceinline__ SlotClose close_slot(float dist, bool slot_valid, float sigma, float vz, int unit) {
    const bool mask = dist < 1e-8f || (unit && dist > 2.f * vz);
    dist = mask ? vz : dist;
    const float valid = slot_valid ? 1.f : 0.f;
    dist = dist * valid;
    sigma = sigma * valid;
    return opacity(sigma, dist);
}

// the transmittance factor of a slot of opacity o, and T after it
__device__ __forceinline__ float trans_factor(float o) { return 1.f - o + 1e-10f; }
__device__ __forceinline__ float trans_step(float T, float o) { return T * trans_factor(o); }

}  // namespace sgn
