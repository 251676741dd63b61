// loss.hip -- the training step's per-ray loss stage, forward and backward, on the device:
// ray_dist + ray_march (ray_walk.h's slot walk, as k_composite: the colour is the renderer's, bit for bit) +
// fill_invalid (as composite.hip), the masked colour MSE and the zero-one
// loss on the neighbours' confidence, and their gradients w.r.t. the per-sample features
// (alpha, r, g, b) and the points' conf.  Replaces the torch autograd of:
//   ray_dist          neural_points_volumetric_model.py:569-577
//   ray_march         diff_ray_marching.py:509-555 (alpha_blend, radiance_render,
//                     diff_render_func.py:36-49)
//   losses            base_rendering_model.py:534-664 (ray_masked_coarse_raycolor: MSE over the
//                     valid rays; ray_miss_coarse_raycolor / coarse_raycolor weight 0, logged),
//                     mvs_points_volumetric_model.py:607-614 (zero_one_loss on conf_coefficient over
//                     the dense [R'', SR, K] neighbour tensor of point_aggregators.py:951-958, empty
//                     entries reading conf at the clamped index 0, neural_points.py:956-967)
// Three launches, no host synchronisation (graph-capturable):
//   k_loss_fwd     8 lanes per ray: composite, per-slot (T, e, dist) kept in the workspace,
//                  block partial sums of the loss terms (fixed order)
//   k_loss_reduce  one workgroup: the partials in block order -> the four losses and the
//                  gradient scales (the valid-ray count is only known here)
//   k_loss_bwd     8 lanes per ray: reverse pass over the slots -> d feat per sample;
//                  zero-one gradients added into d conf (atomics; a ray's empty entries as one add)
// Depth supervision (sgn_loss_train_depth) runs the DEPTH = true instantiations of the same three kernels:
// per ray W = sum w_s, A = sum w_s z_s (w_s = o_s T_s, z_s the raw pers z the cummax reads),
// D = A / (W + 1e-6) (neural_points_volumetric_model.py:620-624), 0 for a ray without a valid sample;
// L_depth = mean over all R rays of (m (D - gt_depth))^2 (base_rendering_model.py:611-618) goes to the
// loss vector's slot 7, and the reverse pass carries one more "colour channel" with the per-slot value
// q_s = (z_s - D) / (W + 1e-6) and the weight d total / d D (no background term).  The DEPTH = false
// instantiations are the stock kernels (they are passed a plain LossArgs).
// The driver's loss options (sgn_loss_train_opts; opt.color_loss_items / color_loss_weights, zero_one_loss_weights,
// zero_epsilon, sparse_loss_weight of base_rendering_model.py:534-664):
//   colour weights  total holds w_masked L_masked + w_miss L_miss + w_all L_all.  A valid ray's d total / d rgb
//                   is (w_masked 2 / (3 n_valid) + w_all 2 / (3 R)) (c - gt): one scale, made in k_loss_reduce where
//                   n_valid becomes known.  A missed ray's colour is its background (no gradient), so w_miss moves
//                   only the reported total: no kernel reads it.  (1, 0, 0) gives the stock scale's bits
//                   (1 * x + 0 * y = x).
//   sparse loss     SPARSE = true instantiations (sparse_loss_weight > 0, :652-662):
//                   L = sum(wn |1 - exp(-2 cc)|) / (sum(wn) + 1e-6) over every (sample, k) entry of the valid rays,
//                   wn the aggregator's normalised neighbour weight (detached there; 0 on empty entries), cc the
//                   straight-through clamp of the gathered conf.  k_loss_nbw restates wn (the linear distance
//                   kernel, point_aggregators.py:494-502, :946-947) from pidx, the points' xyz and samp_locw into
//                   the workspace; the forward adds the two sums to the block partials, k_loss_reduce writes L to
//                   slot 8 and sparse_w / (sum(wn) + 1e-6) to slot 9, the reverse pass adds
//                   slot 9 * wn * 2 exp(-2 cc) into d conf with the zero-one term's atomic (the straight-through
//                   clamp passes the gradient everywhere).  Nothing goes to d feat.  SPARSE = false are the
//                   stock instantiations.
#include <type_traits>

#include "ray_walk.h"
#include "sgn_common.h"

namespace sgn {
namespace {

constexpr int LOSS_TPB = 256;
constexpr int LPR = 8;  // lanes per ray: the slot walk runs on all 8 (same values), the SR x K zero-one
                        // entries are split over them by neighbour k
constexpr int LOSS_NSUM = 5;  // masked se, missed se, all se, zero-one sum, valid rays

struct LossArgs {
    const float *campos, *rot;
    const int32_t *ray_ns, *ray_soff, *samp_nnb, *pidx;
    const float *samp_locw, *feat, *gt, *conf;
    int64_t R;
    int SR, K, unit;
    float vz, bg0, bg1, bg2, zo_w, zo_eps;
    float w_masked, w_all;  // colour weights of ray_masked_coarse_raycolor / coarse_raycolor (stock: 1, 0)
    const float *bg_ray;  // [R][3] per-ray background (ABI 16, inputs['bg_ray']) or null: (bg0, bg1, bg2)
    float *slot_ws;   // [R][SR][3]: T (transmittance before the slot), e = exp(-sigma dist), dist
    float *partial;   // [blocks][LOSS_NSUM]
    float *sums;      // [8]: l_col, l_zo, l_miss, l_all, 2 / max(3 n, 1), zo_w / max(n SR K, 1), n
    float *out_rgb;   // [R][3]
    int8_t *out_mask; // [R]
    float *dfeat;     // [S][4]
    float *dconf;     // [N]
};

// sgn_loss_train_depth's arguments: the stock block first
struct LossDepthArgs : LossArgs {
    const float *gt_depth;  // [R]
    const float *gt_mask;   // [R] float mask or null: gt_depth > 0
    float depth_w;          // depth_loss_weights[i]: scales the depth term's gradient only
    float *out_depth;       // [R] D
    float *ray_w;           // [R] W (workspace), read by the reverse pass
};
// the sparse loss's arguments: the depth block (unused without DEPTH) first
struct LossSparseArgs : LossDepthArgs {
    const float *xyz;  // [N][3] point positions
    float sparse_w;    // sparse_loss_weight
    float *nbw;        // [R][SR][K] (workspace) normalised neighbour weight of the rays' (slot, k) entries
};
template <bool DEPTH, bool SPARSE>
using loss_args_t = std::conditional_t<SPARSE, LossSparseArgs, std::conditional_t<DEPTH, LossDepthArgs, LossArgs>>;
// + the depth term's squared error (index LOSS_NSUM), + the sparse loss's two sums (the last two)
template <bool DEPTH, bool SPARSE>
constexpr int loss_nsum = LOSS_NSUM + (DEPTH ? 1 : 0) + (SPARSE ? 2 : 0);

__device__ __forceinline__ float depth_mask(const LossDepthArgs &a, int64_t r, float g) {
    return a.gt_mask ? a.gt_mask[r] : (g > 0.f ? 1.f : 0.f);
}

// the ray's background colour: inputs['bg_ray'] when given (fill_invalid blends T_bg * bg_ray,
// neural_points_volumetric_model.py:175-177), else the constant bg
__device__ __forceinline__ void ray_bg(const LossArgs &a, int64_t r, float (&bg)[3]) {
    if (a.bg_ray) {
        bg[0] = a.bg_ray[r * 3]; bg[1] = a.bg_ray[r * 3 + 1]; bg[2] = a.bg_ray[r * 3 + 2];
    } else {
        bg[0] = a.bg0; bg[1] = a.bg1; bg[2] = a.bg2;
    }
}

// zero-one term of one (slot, k) entry and its derivative w.r.t. the gathered conf (the straight-
// through clamp passes the gradient unchanged, point_aggregators.py:863-865)
__device__ __forceinline__ float clamped_conf(float cd) {
    const float cl = fminf(fmaxf(cd, 1e-4f), 1.f);
    return __fsub_rn(cd, __fsub_rn(cd, cl));
}

__device__ __forceinline__ void zero_one(float cd, float eps, float &term, float &dterm) {
    const float cc = clamped_conf(cd);
    const float val = fminf(fmaxf(cc, eps), 1.f - eps);
    term = logf(val) + logf(1.f - val);
    dterm = (cc >= eps && cc <= 1.f - eps) ? 1.f / val - 1.f / (1.f - val) : 0.f;
}

// Per ray forward: slot s of the ray (s < ns: sample soff + s; later slots are padding at the
// origin's depth) closes slot s - 1's interval (running cummax of pers z).
// DEPTH: also dW = sum w_s and dA = sum w_s z_s over the slots in ascending order.
template <bool STORE, bool DEPTH>
__device__ void ray_forward(const LossArgs &a, int64_t r, bool store, float (&col)[3], float &T, bool &any_valid,
                            float &dW, float &dA) {
    const int ns = a.ray_ns[r], off = a.ray_soff[r], SR = a.SR;
    const float z0 = pers_z(a.campos, a.rot, 0.f, 0.f, 0.f);
    float *ws = a.slot_ws + r * (int64_t)SR * 3;
    T = 1.f;
    col[0] = col[1] = col[2] = 0.f;
    any_valid = false;
    float prev_cm = 0.f;
    bool pv = false;
    float4 pf = make_float4(0.f, 0.f, 0.f, 0.f);
    float pz = 0.f;  // DEPTH: slot s - 1's z
    if constexpr (DEPTH) dW = dA = 0.f;
    auto process = [&](int slot, float raw) {  // every sample's feat is loaded (zeros without neighbours)
        const SlotClose c = close_slot(raw, pv, pf.x, a.vz, a.unit);
        const float wgt = c.o * T;
        col[0] += pf.y * wgt;
        col[1] += pf.z * wgt;
        col[2] += pf.w * wgt;
        if constexpr (DEPTH) {
            dW += wgt;
            dA += wgt * pz;
        }
        if (STORE && store) {
            ws[3 * slot + 0] = T;
            ws[3 * slot + 1] = c.e;
            ws[3 * slot + 2] = c.dist;
        }
        T = trans_step(T, c.o);
    };
    const int last = ns < SR ? ns : SR - 1;
    for (int s = 0; s <= last; ++s) {
        float z = z0;
        bool v = false;
        float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
        if (s < ns) {
            const int64_t id = off + s;
            z = sample_z(a.campos, a.rot, a.samp_locw, id);
            v = a.samp_nnb[id] > 0;
            f = *(const float4 *)(a.feat + id * 4);  // zero features for samples without neighbours
        }
        float raw;
        const float cm = cummax_step(s, prev_cm, z, raw);
        if (s > 0) process(s - 1, raw);
        prev_cm = cm;
        pv = v;
        pf = f;
        if constexpr (DEPTH) pz = z;
        any_valid |= v;
    }
    if (ns >= SR) process(SR - 1, a.vz);
}

__device__ __forceinline__ float block_sum(float v, float *red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();
    if (lane == 0) red[w] = v;
    __syncthreads();
    float t = 0.f;
    for (int i = 0; i < LOSS_TPB / 64; ++i) t += red[i];  // fixed order
    return t;
}

// The aggregator's normalised neighbour weights of slot s of ray r, one thread per (ray, slot):
// 1 / max(|xyz_p - x_s|, 1e-6) over the slot's neighbours (0 on empty entries), divided by max(their sum, 1e-8),
// k ascending (point_aggregators.py:494-502 linear, :946-947; train.aggregate).  Slots past the ray's samples
// are neither written here nor read later.
__global__ __launch_bounds__(LOSS_TPB) void k_loss_nbw(LossSparseArgs a) {
    const int64_t i = (int64_t)blockIdx.x * LOSS_TPB + threadIdx.x;
    if (i >= a.R * a.SR) return;
    const int64_t r = i / a.SR;
    const int s = (int)(i - r * a.SR);
    if (s >= a.ray_ns[r]) return;
    const int64_t id = (int64_t)a.ray_soff[r] + s;
    const float x = a.samp_locw[id * 3], y = a.samp_locw[id * 3 + 1], z = a.samp_locw[id * 3 + 2];
    float *w = a.nbw + i * a.K;
    float sum = 0.f;
    for (int k = 0; k < a.K; ++k) {
        const int p = a.pidx[id * a.K + k];
        float v = 0.f;
        if (p >= 0) {
            const float dx = a.xyz[(int64_t)p * 3] - x, dy = a.xyz[(int64_t)p * 3 + 1] - y,
                        dz = a.xyz[(int64_t)p * 3 + 2] - z;
            v = 1.f / fmaxf(sqrtf(dx * dx + dy * dy + dz * dz), 1e-6f);
        }
        w[k] = v;
        sum += v;
    }
    const float den = fmaxf(sum, 1e-8f);
    for (int k = 0; k < a.K; ++k) w[k] = w[k] / den;
}

template <bool DEPTH, bool SPARSE>
__global__ __launch_bounds__(LOSS_TPB) void k_loss_fwd(loss_args_t<DEPTH, SPARSE> a) {
    constexpr int NSUM = loss_nsum<DEPTH, SPARSE>;
    __shared__ float red[LOSS_TPB / 64];
    const int64_t r = ((int64_t)blockIdx.x * LOSS_TPB + threadIdx.x) / LPR;
    const int sub = threadIdx.x % LPR;
    float v[NSUM] = {};
    if (r < a.R) {
        float col[3], T, dW, dA;
        bool any;
        ray_forward<true, DEPTH>(a, r, sub == 0, col, T, any, dW, dA);
        float bg[3];
        ray_bg(a, r, bg);
        float se = 0.f;
        for (int c = 0; c < 3; ++c) {
            const float full = any ? col[c] + bg[c] * T : bg[c];
            if (sub == 0) a.out_rgb[r * 3 + c] = full;
            const float d = full - a.gt[r * 3 + c];
            se += d * d;
        }
        if (sub == 0) {
            a.out_mask[r] = any ? 1 : 0;
            v[0] = any ? se : 0.f;
            v[1] = any ? 0.f : se;
            v[2] = se;
            v[4] = any ? 1.f : 0.f;
            if constexpr (DEPTH) {  // every ray counts: a ray without a valid sample has D = 0
                const float D = any ? dA / (dW + 1e-6f) : 0.f;
                a.out_depth[r] = D;
                a.ray_w[r] = dW;
                const float g = a.gt_depth[r];
                const float md = depth_mask(a, r, g) * (D - g);
                v[LOSS_NSUM] = md * md;
            }
        }
        if (any) {  // zero-one terms over the ray's SR x K entries, neighbour k = sub, sub + 8, ..
            const int ns = a.ray_ns[r], off = a.ray_soff[r];
            const int nv = ns < a.SR ? ns : a.SR;
            float t0, d0;
            zero_one(a.conf[0], a.zo_eps, t0, d0);
            float zs = 0.f;
            float sl = 0.f, sw = 0.f;  // SPARSE: sum wn |1 - exp(-2 cc)|, sum wn (empty entries weigh 0)
            int n_empty = 0;
            for (int k = sub; k < a.K; k += LPR) {
                n_empty += a.SR - nv;
                for (int s2 = 0; s2 < nv; ++s2) {
                    const int p = a.pidx[(int64_t)(off + s2) * a.K + k];
                    if (p < 0) {
                        ++n_empty;
                        continue;
                    }
                    float t, d;
                    zero_one(a.conf[p], a.zo_eps, t, d);
                    zs += t;
                    if constexpr (SPARSE) {
                        const float wn = a.nbw[(r * a.SR + s2) * a.K + k];
                        sl += wn * fabsf(1.f - expf(-2.f * clamped_conf(a.conf[p])));
                        sw += wn;
                    }
                }
            }
            v[3] = zs + (float)n_empty * t0;
            if constexpr (SPARSE) {
                v[NSUM - 2] = sl;
                v[NSUM - 1] = sw;
            }
        }
    }
    for (int i = 0; i < NSUM; ++i) {
        const float t = block_sum(v[i], red);
        if (threadIdx.x == 0) a.partial[(int64_t)blockIdx.x * NSUM + i] = t;
    }
}

template <bool DEPTH, bool SPARSE>
__global__ __launch_bounds__(LOSS_TPB) void k_loss_reduce(loss_args_t<DEPTH, SPARSE> a, int nblocks) {
    constexpr int NSUM = loss_nsum<DEPTH, SPARSE>;
    __shared__ float red[LOSS_TPB / 64];
    float t[NSUM];
    for (int i = 0; i < NSUM; ++i) {
        float v = 0.f;
        for (int b = threadIdx.x; b < nblocks; b += LOSS_TPB) v += a.partial[(int64_t)b * NSUM + i];
        t[i] = block_sum(v, red);
    }
    if (threadIdx.x == 0) {
        const float n = t[4];
        const float den_c = fmaxf(3.f * n, 1.f), den_z = fmaxf(n * (float)(a.SR * a.K), 1.f);
        a.sums[0] = t[0] / den_c;
        a.sums[1] = t[3] / den_z;
        a.sums[2] = t[1] / 3.f;
        a.sums[3] = t[2] / (3.f * (float)a.R);
        // d total / d rgb of a valid ray over (c - gt); w_masked = 1, w_all = 0: 2 / den_c, bit for bit
        a.sums[4] = a.w_masked * (2.f / den_c) + a.w_all * (2.f / (3.f * (float)a.R));
        a.sums[5] = a.zo_w / den_z;
        a.sums[6] = n;
        if constexpr (DEPTH)
            a.sums[7] = t[LOSS_NSUM] / (float)a.R;  // L_depth: MSELoss over all R rays
        else
            a.sums[7] = 0.f;
        if constexpr (SPARSE) {  // the loss vector of sgn_loss_train_opts has 12 slots
            const float den_s = t[NSUM - 1] + 1e-6f;
            a.sums[8] = t[NSUM - 2] / den_s;
            a.sums[9] = a.sparse_w / den_s;
            a.sums[10] = t[NSUM - 1];
        }
    }
}

// CONF: points_conf is trained (dconf non-NULL); frozen, the zero-one term is still in the loss
// (k_loss_fwd) and only its gradient -- the loop below, point 0's empty-slot term included -- goes
template <bool CONF, bool DEPTH, bool SPARSE>
__global__ __launch_bounds__(LOSS_TPB) void k_loss_bwd(loss_args_t<DEPTH, SPARSE> a) {
    const int64_t r = ((int64_t)blockIdx.x * LOSS_TPB + threadIdx.x) / LPR;
    const int sub = threadIdx.x % LPR;
    if (r >= a.R) return;
    const int ns = a.ray_ns[r], off = a.ray_soff[r], SR = a.SR;
    const int nv = ns < SR ? ns : SR;
    if (!a.out_mask[r]) {  // fill_invalid: the background colour carries no gradient
        for (int s = sub; s < nv; s += LPR)
            *(float4 *)(a.dfeat + (int64_t)(off + s) * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    if (sub == 0) {  // reverse pass over the slots (one lane of the ray)
        const float gs = a.sums[4];
        float g[3];
        for (int c = 0; c < 3; ++c) g[c] = gs * (a.out_rgb[r * 3 + c] - a.gt[r * 3 + c]);
        const float *ws = a.slot_ws + r * (int64_t)SR * 3;
        // T after every slot (the padding slots' factors are exactly 1): from the last slot
        float Tend = 1.f;
        if (nv > 0) Tend = trans_step(ws[3 * (nv - 1)], 1.f - ws[3 * (nv - 1) + 1]);
        // U = sum over later slots of g . c_i o_i T_i + g . bg T_end (d L / d a_s times a_s), from the end
        float bg[3];
        ray_bg(a, r, bg);
        float U = (g[0] * bg[0] + g[1] * bg[1] + g[2] * bg[2]) * Tend;
        // DEPTH: gD = d total / d D of the ray, q_s = (z_s - D) / Wd; a zero gD leaves every bit as stock
        float gD = 0.f, Dr = 0.f, Wd = 1.f;
        if constexpr (DEPTH) {
            const float gt_d = a.gt_depth[r], m = depth_mask(a, r, gt_d);
            Dr = a.out_depth[r];
            Wd = a.ray_w[r] + 1e-6f;
            gD = a.depth_w * 2.f * (m * m) * (Dr - gt_d) / (float)a.R;
        }
        for (int s = nv - 1; s >= 0; --s) {
            const int64_t id = off + s;
            const float T = ws[3 * s], e = ws[3 * s + 1], dist = ws[3 * s + 2];
            const float4 f = *(const float4 *)(a.feat + id * 4);
            const float o = 1.f - e;
            float gc = g[0] * f.y + g[1] * f.z + g[2] * f.w;
            if constexpr (DEPTH) {
                if (gD != 0.f) {
                    gc += gD * ((sample_z(a.campos, a.rot, a.samp_locw, id) - Dr) / Wd);
                }
            }
            const float dO = gc * T - U / trans_factor(o);  // d L / d o_s
            const bool v = a.samp_nnb[id] > 0;
            const float dsig = dO * e * dist;              // o = 1 - exp(-sigma dist)
            const float w = o * T;
            *(float4 *)(a.dfeat + id * 4) = make_float4(v ? dsig : 0.f, g[0] * w, g[1] * w, g[2] * w);
            U += gc * w;
        }
    }
    if constexpr (!CONF) return;
    // zero-one gradients, neighbour k = sub, sub + 8, ..; the empty entries all read conf[0]
    // SPARSE: each entry's sparse gradient rides the same add (its weight is 0 on the empty entries)
    const float gz = a.sums[5];
    if constexpr (!SPARSE) {
        if (gz == 0.f) return;  // zero-one weight 0: nothing to add
    }
    float gsp = 0.f;
    if constexpr (SPARSE) gsp = a.sums[9];
    float t0, d0;
    zero_one(a.conf[0], a.zo_eps, t0, d0);
    int n_empty = 0;
    for (int k = sub; k < a.K; k += LPR) {
        n_empty += SR - nv;
        for (int s = 0; s < nv; ++s) {
            const int p = a.pidx[(int64_t)(off + s) * a.K + k];
            if (p < 0) {
                ++n_empty;
                continue;
            }
            float t, d;
            zero_one(a.conf[p], a.zo_eps, t, d);
            if constexpr (SPARSE) {
                const float wn = a.nbw[(r * SR + s) * a.K + k];
                const float g = gz * d + gsp * wn * (2.f * expf(-2.f * clamped_conf(a.conf[p])));
                if (g != 0.f) atomicAdd(a.dconf + p, g);
            } else {
                if (d != 0.f) atomicAdd(a.dconf + p, gz * d);
            }
        }
    }
    if (n_empty > 0 && d0 != 0.f && gz != 0.f) atomicAdd(a.dconf, gz * d0 * (float)n_empty);
}

}  // namespace
}  // namespace sgn

// the three launches (after k_loss_nbw with SPARSE) of one instantiation; `a` is cut down to its argument block
template <bool DEPTH, bool SPARSE>
static void loss_kernels(const sgn::LossSparseArgs &a, int64_t nb, bool conf, hipStream_t st) {
    using namespace sgn;
    const dim3 grid((unsigned)nb), one(1), tpb(LOSS_TPB);
    const loss_args_t<DEPTH, SPARSE> &b = a;
    if constexpr (SPARSE) {
        const dim3 gw((unsigned)((a.R * a.SR + LOSS_TPB - 1) / LOSS_TPB));
        hipLaunchKernelGGL(k_loss_nbw, gw, tpb, 0, st, a);
    }
    hipLaunchKernelGGL((k_loss_fwd<DEPTH, SPARSE>), grid, tpb, 0, st, b);
    hipLaunchKernelGGL((k_loss_reduce<DEPTH, SPARSE>), one, tpb, 0, st, b, (int)nb);
    hipLaunchKernelGGL((conf ? k_loss_bwd<true, DEPTH, SPARSE> : k_loss_bwd<false, DEPTH, SPARSE>), grid, tpb, 0, st, b);
}

extern "C" {

size_t sgn_loss_workspace_bytes(int64_t R, int32_t SR) {
    if (R < 0 || SR <= 0) return 0;
    const int64_t nb = (R * sgn::LPR + sgn::LOSS_TPB - 1) / sgn::LOSS_TPB;
    return (size_t)(R * SR * 3 * 4 + (nb + 1) * sgn::LOSS_NSUM * 4 + 64);
}

static int loss_launch(const sgn_loss_params *lp, const sgn_loss_opts *op, const sgn_loss_depth *dp,
                       const float *d_campos, const float *d_camrotc2w, int64_t R, const sgn_query_out *q,
                       const float *d_feat, const float *d_gt, const float *d_conf, float *d_out_rgb,
                       int8_t *d_out_mask, float *d_losses, float *d_dfeat, float *d_dconf, void *d_workspace,
                       size_t workspace_bytes, bool depth, sgn_stream_t stream) {
    using namespace sgn;
    SGN_REQUIRE(lp && q && d_campos && d_camrotc2w && d_feat && d_gt && d_conf && d_out_rgb && d_out_mask &&
                    d_losses && d_dfeat && d_workspace,
                "null argument");
    SGN_REQUIRE(!depth || (dp && dp->gt_depth && dp->out_depth), "null argument");
    SGN_REQUIRE(lp->SR > 0 && lp->K > 0, "SR and K must be positive");
    SGN_REQUIRE(R >= 0, "R must be non-negative");
    const bool sparse = op && op->sparse_weight > 0.f;
    if (op) {
        SGN_REQUIRE(op->w_masked >= 0.f && op->w_miss >= 0.f && op->w_all >= 0.f && op->sparse_weight >= 0.f,
                    "loss weights must be non-negative");
        SGN_REQUIRE(!sparse || op->xyz, "the sparse loss needs the points' xyz");
    }
    SGN_REQUIRE(workspace_bytes >= (op      ? sgn_loss_opts_workspace_bytes(R, lp->SR, lp->K)
                                    : depth ? sgn_loss_depth_workspace_bytes(R, lp->SR)
                                            : sgn_loss_workspace_bytes(R, lp->SR)),
                "loss workspace too small");
    SGN_REQUIRE(((uintptr_t)d_feat & 15) == 0 && ((uintptr_t)d_dfeat & 15) == 0 && ((uintptr_t)d_workspace & 15) == 0,
                "16-byte alignment required");
    hipStream_t st = as_stream(stream);
    const int64_t nb = (R * LPR + LOSS_TPB - 1) / LOSS_TPB;
    LossSparseArgs a{};
    a.campos = d_campos; a.rot = d_camrotc2w;
    a.ray_ns = q->ray_ns; a.ray_soff = q->ray_soff; a.samp_nnb = q->samp_nnb; a.pidx = q->pidx;
    a.samp_locw = q->samp_locw; a.feat = d_feat; a.gt = d_gt; a.conf = d_conf;
    a.R = R; a.SR = lp->SR; a.K = lp->K; a.unit = lp->raydist_mode_unit; a.vz = lp->vsize_z;
    a.bg0 = lp->bg[0]; a.bg1 = lp->bg[1]; a.bg2 = lp->bg[2];
    a.bg_ray = lp->bg_ray;
    a.zo_w = lp->zero_one_weight; a.zo_eps = lp->zero_one_eps;
    a.w_masked = op ? op->w_masked : 1.f; a.w_all = op ? op->w_all : 0.f;
    a.slot_ws = (float *)d_workspace;
    a.partial = a.slot_ws + R * lp->SR * 3;
    a.sums = d_losses;
    a.out_rgb = d_out_rgb; a.out_mask = d_out_mask; a.dfeat = d_dfeat; a.dconf = d_dconf;
    if (sparse) {  // workspace: slots, the entries' weights, (W per ray,) partials
        a.xyz = op->xyz; a.sparse_w = op->sparse_weight;
        a.nbw = a.partial;
        a.partial = a.nbw + R * lp->SR * lp->K;
    }
    if (depth) {  // workspace: slots, W per ray, partials
        a.gt_depth = dp->gt_depth; a.gt_mask = dp->gt_mask; a.depth_w = dp->weight; a.out_depth = dp->out_depth;
        a.ray_w = a.partial;
        a.partial = a.ray_w + R;
    }
    if (op)  // the loss vector's slots 8..11: L_sparse, its gradient scale, sum(wn), spare (0 without the sparse loss)
        SGN_CHECK_HIP(hipMemsetAsync(d_losses + 8, 0, 4 * sizeof(float), st));
    if (R == 0) {
        SGN_CHECK_HIP(hipMemsetAsync(d_losses, 0, 8 * sizeof(float), st));
        return 0;
    }
    if (sparse) {
        if (depth) loss_kernels<true, true>(a, nb, d_dconf != nullptr, st);
        else loss_kernels<false, true>(a, nb, d_dconf != nullptr, st);
    } else {
        if (depth) loss_kernels<true, false>(a, nb, d_dconf != nullptr, st);
        else loss_kernels<false, false>(a, nb, d_dconf != nullptr, st);
    }
    SGN_CHECK_HIP(hipGetLastError());
    return 0;
}

size_t sgn_loss_depth_workspace_bytes(int64_t R, int32_t SR) {
    if (R < 0 || SR <= 0) return 0;
    const int64_t nb = (R * sgn::LPR + sgn::LOSS_TPB - 1) / sgn::LOSS_TPB;
    return (size_t)(R * SR * 3 * 4 + R * 4 + (nb + 1) * (sgn::LOSS_NSUM + 1) * 4 + 64);
}

int sgn_loss_train(const sgn_loss_params *lp, const float *d_campos, const float *d_camrotc2w, int64_t R,
                   const sgn_query_out *q, const float *d_feat, const float *d_gt, const float *d_conf,
                   float *d_out_rgb, int8_t *d_out_mask, float *d_losses, float *d_dfeat, float *d_dconf,
                   void *d_workspace, size_t workspace_bytes, sgn_stream_t stream) {
    return loss_launch(lp, nullptr, nullptr, d_campos, d_camrotc2w, R, q, d_feat, d_gt, d_conf, d_out_rgb, d_out_mask,
                       d_losses, d_dfeat, d_dconf, d_workspace, workspace_bytes, false, stream);
}

int sgn_loss_train_depth(const sgn_loss_params *lp, const sgn_loss_depth *dp, const float *d_campos,
                         const float *d_camrotc2w, int64_t R, const sgn_query_out *q, const float *d_feat,
                         const float *d_gt, const float *d_conf, float *d_out_rgb, int8_t *d_out_mask,
                         float *d_losses, float *d_dfeat, float *d_dconf, void *d_workspace, size_t workspace_bytes,
                         sgn_stream_t stream) {
    return loss_launch(lp, nullptr, dp, d_campos, d_camrotc2w, R, q, d_feat, d_gt, d_conf, d_out_rgb, d_out_mask,
                       d_losses, d_dfeat, d_dconf, d_workspace, workspace_bytes, true, stream);
}

size_t sgn_loss_opts_workspace_bytes(int64_t R, int32_t SR, int32_t K) {
    if (R < 0 || SR <= 0 || K <= 0) return 0;
    const int64_t nb = (R * sgn::LPR + sgn::LOSS_TPB - 1) / sgn::LOSS_TPB;
    return (size_t)(R * SR * 3 * 4 + R * SR * K * 4 + R * 4 + (nb + 1) * (sgn::LOSS_NSUM + 3) * 4 + 64);
}

int sgn_loss_train_opts(const sgn_loss_params *lp, const sgn_loss_opts *op, const sgn_loss_depth *dp,
                        const float *d_campos, const float *d_camrotc2w, int64_t R, const sgn_query_out *q,
                        const float *d_feat, const float *d_gt, const float *d_conf, float *d_out_rgb,
                        int8_t *d_out_mask, float *d_losses, float *d_dfeat, float *d_dconf, void *d_workspace,
                        size_t workspace_bytes, sgn_stream_t stream) {
    SGN_REQUIRE(op, "null argument");
    return loss_launch(lp, op, dp, d_campos, d_camrotc2w, R, q, d_feat, d_gt, d_conf, d_out_rgb, d_out_mask, d_losses,
                       d_dfeat, d_dconf, d_workspace, workspace_bytes, dp != nullptr, stream);
}

}  // extern "C"
