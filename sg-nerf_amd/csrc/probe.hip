// probe.hip -- per-ray hole-probing maps (opt.prob = 1).
//
// Replaces, for one ray r, the probe branch of NeuralPointsRayMarching.forward
// (models/neural_points_volumetric_model.py:633-668) and its unmask / fill_invalid expansion (:192-203):
//   ray_max_shading_opacity, ray_max_sample_loc_w, ray_max_far_dist   the ray's most opaque shading slot, its
//                   position and its distance to the nearest of its K neighbour slots
//   shading_avg_color / _dir / _conf / _embedding                    that slot's neighbours' point features,
//                   blended by weight * conf_coefficient (the aggregator's out_blend)
// The reference takes them from the dense [1, R, SR, K, C] gathers; here they come from the sample-major
// query output and the point tables, one packed 48-float record per ray (include/sgn_hip.h).
//
// 8 lanes per ray, 8 rays per wave.  The 8 lanes split the ray's SR opacities and combine (value, slot)
// over DPP; lane c then owns embedding channels 4c .. 4c + 3, so each neighbour's 128-B embedding row is
// one 16-B load per lane, and lanes 0 / 2 / 3 also carry conf / colour / dir.  Every sum is per lane, k
// ascending: no cross-lane sum, no LDS, coalesced 16-B stores.
#include "sgn_common.h"

namespace sgn {
namespace {

struct ProbeArgs {
    const int32_t *ray_ns, *ray_soff, *pidx;
    const float *samp_locw;
    const float *xyz, *emb, *color, *dir, *conf;
    int64_t n_points;
    const float *opacity, *blend;
    const int8_t *mask;
    int64_t R;
    int SR, K, vec;   // vec: the opacity rows take 16-B loads (SR % 4 == 0, aligned base)
    float *out;
};

constexpr int PROBE_TPB = 256, PROBE_LANES = 8, PROBE_RAYS = PROBE_TPB / PROBE_LANES, PROBE_REC = 48;

// lane exchanges inside a group of 8: xor 1, xor 2 (quad_perm) and i <-> 7 - i (row_half_mirror); every
// source lane lies in the reader's own group, and the callers keep all 64 lanes active
constexpr int DPP_XOR1 = 0xB1, DPP_XOR2 = 0x4E, DPP_HALF_MIRROR = 0x141;
template <int CTRL>
__device__ __forceinline__ int dpp_i(int v) {
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, false);
}
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
    return __int_as_float(dpp_i<CTRL>(__float_as_int(v)));
}

// (value, slot) of the larger value, the lower slot on a tie: a total order, so the 8 lanes agree
template <int CTRL>
__device__ __forceinline__ void argmax_step(float &v, int &i) {
    const float ov = dpp_f<CTRL>(v);
    const int oi = dpp_i<CTRL>(i);
    const bool take = ov > v || (ov == v && oi < i);
    v = take ? ov : v;
    i = take ? oi : i;
}

__global__ __launch_bounds__(PROBE_TPB) void k_probe(ProbeArgs a) {
    const int sub = threadIdx.x & (PROBE_LANES - 1);
    const int64_t r = (int64_t)blockIdx.x * PROBE_RAYS + (threadIdx.x >> 3);
    const bool live = r < a.R;
    const int SR = a.SR, K = a.K;
    const int ns = live ? a.ray_ns[r] : 0;
    // a ray of the mask always has a sample (slot 0); one without is treated as masked out, so that no
    // index below depends on the caller's mask
    const bool valid = live && a.mask[r] != 0 && ns > 0;

    // ---- the first slot holding the row maximum.  Each lane scans its slots upwards with a strict >
    // (the first of equal values stays), the combine prefers the lower slot: numpy.argmax's and CPU
    // torch.max's choice (the reference's CUDA torch.max leaves the index among tied slots unspecified).
    // A NaN ranks lowest.
    float best = -INFINITY;
    int bi = sub;   // lane 0's is slot 0: the all -inf row selects it
    if (valid) {
        const float *row = a.opacity + r * SR;
        auto see = [&](float v, int slot) {
            v = v == v ? v : -INFINITY;
            if (v > best) { best = v; bi = slot; }
        };
        if (a.vec) {
            for (int s0 = 4 * sub; s0 < SR; s0 += 4 * PROBE_LANES) {
                const float4 v = *(const float4 *)(row + s0);
                see(v.x, s0); see(v.y, s0 + 1); see(v.z, s0 + 2); see(v.w, s0 + 3);
            }
        } else {
            for (int s0 = sub; s0 < SR; s0 += PROBE_LANES) see(row[s0], s0);
        }
    }
    argmax_step<DPP_XOR1>(best, bi);
    argmax_step<DPP_XOR2>(best, bi);
    argmax_step<DPP_HALF_MIRROR>(best, bi);

    float4 head = make_float4(0.f, 0.f, 0.f, 0.f), e = make_float4(0.f, 0.f, 0.f, 0.f);
    float far = INFINITY;   // lane k: the distance of neighbour slot k (lanes K .. 7: +inf)
    if (valid) {
        // slot 0 is a selected sample and every positive opacity belongs to one, so bi < ns on a
        // composite's output; the clamp keeps the sample id inside the ray for any other input
        const int j = bi < ns ? bi : ns - 1;
        const int64_t s = (int64_t)a.ray_soff[r] + j;
        const float lx = a.samp_locw[s * 3], ly = a.samp_locw[s * 3 + 1], lz = a.samp_locw[s * 3 + 2];
        // lanes 0 / 2 / 3 also blend conf / colour / dir (n floats per point)
        const float *tab = sub == 0 ? a.conf : sub == 2 ? a.color : a.dir;
        const int n = sub == 0 ? 1 : (sub == 2 || sub == 3) ? 3 : 0;
        float t0 = 0.f, t1 = 0.f, t2 = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (k < K) {
                const int pk = a.pidx[s * K + k];
                // an empty slot (-1) reads point 0 (neural_points.py:958-959) and carries blend 0
                const float w = pk >= 0 ? a.blend[s * K + k] : 0.f;
                int64_t p = pk > 0 ? pk : 0;
                p = p < a.n_points ? p : a.n_points - 1;   // never past the tables
                const float4 ev = *(const float4 *)(a.emb + p * 32 + 4 * sub);
                e.x = __fadd_rn(e.x, __fmul_rn(w, ev.x));
                e.y = __fadd_rn(e.y, __fmul_rn(w, ev.y));
                e.z = __fadd_rn(e.z, __fmul_rn(w, ev.z));
                e.w = __fadd_rn(e.w, __fmul_rn(w, ev.w));
                if (n >= 1) t0 = __fadd_rn(t0, __fmul_rn(w, tab[p * n]));
                if (n == 3) {
                    t1 = __fadd_rn(t1, __fmul_rn(w, tab[p * 3 + 1]));
                    t2 = __fadd_rn(t2, __fmul_rn(w, tab[p * 3 + 2]));
                }
                if (sub == k) {
                    const float dx = __fsub_rn(a.xyz[p * 3], lx), dy = __fsub_rn(a.xyz[p * 3 + 1], ly),
                                dz = __fsub_rn(a.xyz[p * 3 + 2], lz);
                    far = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz)));
                }
            }
        }
        head = sub == 0 ? make_float4(a.opacity[r * SR + j], 0.f, t0, 0.f)
             : sub == 1 ? make_float4(lx, ly, lz, 0.f)
                        : make_float4(t0, t1, t2, 0.f);
    }
    // min over the K slots (outside the branch: the DPP reads need every lane active)
    far = fminf(far, dpp_f<DPP_XOR1>(far));
    far = fminf(far, dpp_f<DPP_XOR2>(far));
    far = fminf(far, dpp_f<DPP_HALF_MIRROR>(far));
    if (valid && sub == 0) head.y = far;
    if (live) {
        float4 *rec = (float4 *)(a.out + r * PROBE_REC);
        if (sub < 4) rec[sub] = head;
        rec[4 + sub] = e;
    }
}

}  // namespace
}  // namespace sgn

extern "C" int sgn_probe(const sgn_point_tables *pt, const sgn_query_out *q, const float *d_opacity,
                         const float *d_blend, const int8_t *d_mask, int64_t R, int32_t SR, int32_t K,
                         float *d_out, sgn_stream_t stream) {
    using namespace sgn;
    SGN_REQUIRE(pt && q && d_opacity && d_blend && d_mask && d_out, "null argument");
    SGN_REQUIRE(q->ray_ns && q->ray_soff && q->samp_locw && q->pidx, "null query output (ray_ns, ray_soff, samp_locw, pidx)");
    SGN_REQUIRE(pt->xyz && pt->embedding && pt->color && pt->dir && pt->conf, "null point table");
    SGN_REQUIRE(pt->n_points >= 1, "the probe reads point 0 for empty neighbour slots: n_points >= 1");
    SGN_REQUIRE(K >= 1 && K <= 8, "the probe takes K = 1 .. 8 neighbours per sample");
    SGN_REQUIRE(SR > 0, "SR must be positive");
    SGN_REQUIRE(R >= 0 && R <= ((int64_t)1 << 31), "R out of range");
    SGN_REQUIRE(((uintptr_t)d_out & 15) == 0 && ((uintptr_t)pt->embedding & 15) == 0,
                "16-byte alignment required (d_out, embedding)");
    if (R == 0) return 0;
    ProbeArgs a;
    a.ray_ns = q->ray_ns; a.ray_soff = q->ray_soff; a.pidx = q->pidx; a.samp_locw = q->samp_locw;
    a.xyz = pt->xyz; a.emb = pt->embedding; a.color = pt->color; a.dir = pt->dir; a.conf = pt->conf;
    a.n_points = pt->n_points;
    a.opacity = d_opacity; a.blend = d_blend; a.mask = d_mask;
    a.R = R; a.SR = SR; a.K = K;
    a.vec = (SR & 3) == 0 && ((uintptr_t)d_opacity & 15) == 0;
    a.out = d_out;
    hipLaunchKernelGGL(k_probe, dim3((unsigned)((R + PROBE_RAYS - 1) / PROBE_RAYS)), dim3(PROBE_TPB), 0,
                       as_stream(stream), a);
    SGN_CHECK_HIP(hipGetLastError());
    return 0;
}
