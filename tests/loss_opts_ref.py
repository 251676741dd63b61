"""Float64 restatement of compute_losses under the driver's loss options (base_rendering_model.py:534-664) and of
its gradients, in explicit loops over rays, slots and neighbours, on the scenes of tests/ray_stage_ref.py -- the
reference of sgn_loss_train_opts (csrc/loss.hip) in tests/test_loss_opts_gpu.py.  tests/test_loss_opts_ref_cpu.py
pins it to train.composite_losses under torch float64 autograd.

  colour items   L_masked = sum over the valid rays of |c - gt|^2 / (3 n_valid)   (0 without a valid ray)
                 L_miss   = sum over the missed rays of |c - gt|^2 / 3
                 L_all    = sum over every ray of |c - gt|^2 / (3 R)
                 each listed item adds weight * L + 1e-6; weights follow the item order (one weight serves all)
  zero-one       L_zo = mean over every (slot, k) of the valid rays of log(val) + log(1 - val),
                 val = clamp(cc, eps, 1 - eps), cc the straight-through clamp of the gathered conf to [1e-4, 1]
                 (empty entries read conf[0]); an empty item list drops the term from the total
  sparse         L_sp = sum(wn |1 - exp(-2 cc)|) / (sum(wn) + 1e-6) over the valid rays' entries with a neighbour,
                 wn = (1 / max(|xyz_p - x_s|, 1e-6)) / max(sum over the sample's neighbours, 1e-8), a constant
  depth          L_d = mean over all R rays of (m (D - g))^2,  D = sum w z / (sum w + 1e-6), 0 on a missed ray
  total          = sum_i (w_i L_i + 1e-6) + w_zo L_zo + w_sp L_sp + w_d L_d

A valid ray's d total / d rgb is (w_masked 2 / (3 n_valid) + w_all 2 / (3 R)) (c - gt); a missed ray's colour is its
background, so w_miss moves the total alone.  The reverse pass over a ray's slots is written out by hand
(d total / d o_s = T_s G_s - (sum_{j > s} G_j w_j + g . bg T_end) / (1 - o_s + 1e-10), G_s = g . c_s + gD q_s,
q_s = (z_s - D) / (W + 1e-6)).  d total / d conf sums, per entry, w_zo / (n SR K) (1 / val - 1 / (1 - val)) where cc
lies inside [eps, 1 - eps] and w_sp wn 2 exp(-2 cc) / (sum(wn) + 1e-6) (the straight-through clamp passes the
gradient everywhere).

As in ray_stage_ref, every branch (the cummax, the distance tests, the clamps) is decided on fp32 values as the
kernels decide them (rs.ray_dist_fp32, the fp32 comparisons below, depth_ref.z_fp32); float64 starts after them."""
import numpy as np
import torch

import depth_ref as dr
import ray_stage_ref as rs

COLOR_ITEMS = ("ray_masked_coarse_raycolor", "ray_miss_coarse_raycolor", "coarse_raycolor")
F32 = np.float32
EPS_SP = float(F32(1e-6))


def item_weight(items, weights, name):
    if name not in items:
        return 0.0
    return float(weights[0] if len(weights) == 1 else weights[list(items).index(name)])


def neighbour_weights(scene):
    """wn [S, K] float64 from the fp32 positions: the linear distance kernel, normalised per sample."""
    S, K = scene["S"], scene["K"]
    xyz, loc, pidx = scene["xyz"].double().numpy(), scene["samp_locw"].double().numpy(), scene["pidx"].numpy()
    wn = np.zeros((S, K))
    for s in range(S):
        for k in range(K):
            p = pidx[s, k]
            if p >= 0:
                wn[s, k] = 1.0 / max(float(np.sqrt(((xyz[p] - loc[s]) ** 2).sum())), 1e-6)
        wn[s] /= max(wn[s].sum(), 1e-8)
    return wn


def reference(scene, unit, use_bg_ray, color_items=COLOR_ITEMS, color_weights=(1.0, 0.0, 0.0),
              zero_one_items=("conf_coefficient",), zero_one_weights=(1e-4,), zero_eps=1e-3, sparse_weight=0.0,
              depth=None, bg=(1.0, 1.0, 1.0)):
    """depth: None or (gt_depth [R] fp32, gt_mask [R] fp32 or None, weight).  Returns a dict: total, parts (by the
    reported names: the three colour items, conf_coefficient, sparse when on, coarse_depth with depth), dfeat
    [S_cap, 4] and dconf [N] (float64 tensors), full [R, 3], mask [R], n."""
    R, SR, K, S = scene["R"], scene["SR"], scene["K"], scene["S"]
    w_masked, w_miss, w_all = (item_weight(color_items, color_weights, n) for n in COLOR_ITEMS)
    w_zo = item_weight(zero_one_items, zero_one_weights, "conf_coefficient")
    dist_t, valid_t, _ = rs.ray_dist_fp32(scene, unit)
    dist, valid = dist_t.double().numpy(), valid_t.numpy()
    feat = scene["feat"].double().numpy()
    gt = scene["gt"].double().numpy()
    conf32 = scene["conf"].numpy().astype(F32)
    conf = conf32.astype(np.float64)
    pidx = scene["pidx"].numpy()
    ns, soff = scene["ray_ns"].numpy(), scene["ray_soff"].numpy()
    bgv = (scene["bg_ray"].double().numpy() if use_bg_ray else np.tile(np.array(bg, dtype=F32).astype(np.float64), (R, 1)))
    z = dr.z_fp32(scene).double().numpy()
    if depth is not None:
        gt_d = depth[0].double().numpy()
        m_d = (depth[0] > 0).double().numpy() if depth[1] is None else depth[1].double().numpy()
        w_d = float(depth[2])
    # ---- forward, ray by ray
    T = np.ones((R, SR + 1))
    o = np.zeros((R, SR))
    e = np.ones((R, SR))
    full = np.zeros((R, 3))
    mask = np.zeros(R, dtype=bool)
    D = np.zeros(R)
    W = np.zeros(R)
    for r in range(R):
        col = np.zeros(3)
        A = 0.0
        for s in range(SR):
            f = feat[soff[r] + s] if s < ns[r] else np.zeros(4)
            sigma = f[0] if valid[r, s] else 0.0
            e[r, s] = np.exp(-sigma * dist[r, s])
            o[r, s] = 1.0 - e[r, s]
            w = o[r, s] * T[r, s]
            col += f[1:4] * w
            W[r] += w
            A += w * z[r, s]
            T[r, s + 1] = T[r, s] * (1.0 - o[r, s] + rs.EPS_T)
        mask[r] = valid[r].any()
        full[r] = col + bgv[r] * T[r, SR] if mask[r] else bgv[r]
        D[r] = A / (W[r] + dr.EPS_D) if mask[r] else 0.0
    n = int(mask.sum())
    se = ((full - gt) ** 2).sum(1)
    parts = {"ray_masked_coarse_raycolor": se[mask].sum() / max(3 * n, 1), "ray_miss_coarse_raycolor": se[~mask].sum() / 3,
             "coarse_raycolor": se.sum() / (3 * R)}
    # ---- the conf terms: per point, decided in fp32 as zero_one() decides
    e32 = F32(zero_eps)
    hi32 = F32(1.0) - e32
    cl32 = np.minimum(np.maximum(conf32, F32(1e-4)), F32(1.0))
    cc32 = conf32 - (conf32 - cl32)
    inside = (cc32 >= e32) & (cc32 <= hi32)
    val = np.where(inside, conf, np.where(cc32 < e32, float(e32), float(hi32)))
    zo_term = np.log(val) + np.log(1.0 - val)
    zo_d = np.where(inside, 1.0 / val - 1.0 / (1.0 - val), 0.0)
    cc = np.where(cc32 == conf32, conf, cc32.astype(np.float64))   # the clamp's value as fp32 rounds it
    wn = neighbour_weights(scene) if sparse_weight > 0 else None
    zo_sum = sp_num = sp_den = 0.0
    for r in range(R):
        if not mask[r]:
            continue
        for s in range(SR):
            for k in range(K):
                p = pidx[soff[r] + s, k] if s < ns[r] else -1
                zo_sum += zo_term[max(p, 0)]
                if p >= 0 and wn is not None:
                    sp_num += wn[soff[r] + s, k] * abs(1.0 - np.exp(-2.0 * cc[p]))
                    sp_den += wn[soff[r] + s, k]
    den_z = max(n * SR * K, 1)
    parts["conf_coefficient"] = zo_sum / den_z
    total = sum(item_weight(color_items, color_weights, name) * parts[name] + 1e-6 for name in color_items)
    total += w_zo * parts["conf_coefficient"]
    if sparse_weight > 0:
        parts["sparse"] = sp_num / (sp_den + EPS_SP)
        total += sparse_weight * parts["sparse"]
    if depth is not None:
        parts["coarse_depth"] = ((m_d * (D - gt_d)) ** 2).sum() / R
        total += w_d * parts["coarse_depth"]
    # ---- d total / d conf
    dconf = np.zeros(conf.shape[0])
    for r in range(R):
        if not mask[r]:
            continue
        for s in range(SR):
            for k in range(K):
                p = pidx[soff[r] + s, k] if s < ns[r] else -1
                dconf[max(p, 0)] += w_zo / den_z * zo_d[max(p, 0)]
                if p >= 0 and wn is not None:
                    dconf[p] += sparse_weight * wn[soff[r] + s, k] * 2.0 * np.exp(-2.0 * cc[p]) / (sp_den + EPS_SP)
    # ---- d total / d feat: the reverse pass over each valid ray's slots
    dfeat = np.zeros((scene["S_cap"], 4))
    gs = w_masked * 2.0 / max(3 * n, 1) + w_all * 2.0 / (3 * R)
    for r in range(R):
        if not mask[r]:
            continue
        g = gs * (full[r] - gt[r])
        gD, Wd = 0.0, W[r] + dr.EPS_D
        if depth is not None:
            gD = w_d * 2.0 * m_d[r] ** 2 * (D[r] - gt_d[r]) / R
        U = float(g @ bgv[r]) * T[r, SR]      # sum over the later slots of G_j w_j, plus g . bg T_end
        for s in reversed(range(min(int(ns[r]), SR))):
            i = soff[r] + s
            G = float(g @ feat[i, 1:4]) + gD * (z[r, s] - D[r]) / Wd
            av = 1.0 - o[r, s] + rs.EPS_T
            dO = G * T[r, s] - U / av
            w = o[r, s] * T[r, s]
            dfeat[i, 0] = dO * e[r, s] * dist[r, s] if valid[r, s] else 0.0
            dfeat[i, 1:4] = g * w
            U += G * w
    t = torch.from_numpy
    return dict(total=float(total), parts={k: float(v) for k, v in parts.items()}, dfeat=t(dfeat), dconf=t(dconf),
                full=t(full), mask=t(mask), n=n, D=t(D))


def small_scene(R, SR, K, seed, camera=0, n_points=50):
    """rs.ray_scene with its neighbours folded onto `n_points` points (several entries then share a d conf row; the
    21 planted conf values at points 1 .. 21 stay named), two more conf values inside 0.05 of either end (points 22,
    23: for zero_epsilon = 0.05), and the point tables cut to n_points."""
    sc = dict(rs.ray_scene(R, SR, K, seed, camera=camera))
    first = 1 + rs.conf_plantings().numel()
    p = sc["pidx"].clone()
    fold = first + (p - first) % (n_points - first)
    sc["pidx"] = torch.where(p >= first, fold, p).to(torch.int32).contiguous()
    conf = sc["conf"][:n_points].clone()
    conf[first], conf[first + 1] = 0.03, 0.97
    sc["conf"] = conf.contiguous()
    sc["xyz"] = sc["xyz"][:n_points].contiguous()
    sc["n_points"] = n_points
    return sc
