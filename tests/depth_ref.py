"""Float64 reference of the depth map and the depth loss (csrc/composite.hip: k_composite<true>; csrc/loss.hip:
the DEPTH instantiations of k_loss_fwd / k_loss_reduce / k_loss_bwd) on the scenes of tests/ray_stage_ref.py,
which this module builds on and does not change.

  W_r = sum_s w_s,  A_r = sum_s w_s z_s,  D_r = A_r / (W_r + 1e-6f)   (0 on rays without a valid sample)
  L_depth = (1 / R) sum_r (m_r (D_r - g_r))^2,   m = gt_mask, or g > 0 without one
  total = losses[0] (+ the terms without a gradient in feat) + w_d L_depth

w_s is march_ref's blend weight.  z_s is the sample's camera-space depth in fp32, computed exactly as pers_z
computes it (and as ray_dist_fp32 computes it for the cummax; padding slots sit at the world origin and carry
w = 0): the float64 arithmetic starts after it, so reference and kernel hold the same z.  tests/test_depth_ref_cpu.py
pins this module to train.composite_losses and to finite differences."""
import torch

import ray_stage_ref as rs

F32 = torch.float32
EPS_D = float(torch.tensor(1e-6, dtype=F32))   # the denominator's 1e-6f


def z_fp32(scene):
    """[R, SR] fp32: ((x - c0) r2 + (y - c1) r5) + (z - c2) r8, every operation rounded to fp32 (pers_z)."""
    c, r = scene["campos"], scene["rot"].reshape(-1)
    p = rs.densify(scene, scene["samp_locw"])
    z = ((p[..., 0] - c[0]) * r[2] + (p[..., 1] - c[1]) * r[5]) + (p[..., 2] - c[2]) * r[8]
    assert z.dtype == F32
    return z


def depth_of(w, z, mask):
    """(D, W, A) [R] float64 from blend weights w [R, SR] (float64), z [R, SR] and the ray mask."""
    W = w.sum(dim=1)
    A = (w * z.double()).sum(dim=1)
    return torch.where(mask, A / (W + EPS_D), torch.zeros_like(A)), W, A


def depth_loss(D, gt_depth, gt_mask):
    """L_depth in float64 from fp32 targets: the mean over all rays of (m (D - g))^2."""
    g = gt_depth.double()
    m = (gt_depth > 0).double() if gt_mask is None else gt_mask.double()
    return ((m * (D - g)) ** 2).mean() if D.numel() else D.sum()


def targets(scene, D, seed):
    """gt_depth = D + U(-0.05, 0.05) with every fifth ray at 0 (fp32), and an explicit mask over {0, 0.5, 1}."""
    g = torch.Generator().manual_seed(1000 + seed)
    R = scene["R"]
    gt = (D + 0.1 * (torch.rand(R, generator=g, dtype=torch.float64) - 0.5)).to(F32)
    gt[torch.arange(R) % 5 == 4] = 0.0
    mask = (torch.randint(0, 3, (R,), generator=g).double() * 0.5).to(F32)
    return gt, mask


def depth_map(scene, unit):
    """The forward alone: dict of D, W, A [R] (float64), mask [R], z [R, SR] fp32 and march_ref's tensors."""
    dist, valid, _ = rs.ray_dist_fp32(scene, unit)
    m = rs.march_ref(dist, valid, rs.densify(scene, scene["feat"].double()))
    mask = valid.any(dim=-1)
    z = z_fp32(scene)
    D, W, A = depth_of(m["w"], z, mask)
    return dict(m, D=D, W=W, A=A, mask=mask, z=z, dist=dist, valid=valid)


def reference(scene, unit, use_bg_ray, gt_depth, gt_mask, w_d, bg=(1.0, 1.0, 1.0), zero_one_weight=1e-4):
    """rs.reference's dict (the stock stage: losses [4], dfeat = d losses[0] / d feat, dconf, full, mask ..) plus
    D, W, A [R], z [R, SR], l_depth and dfeat_depth [S_cap, 4] = d (losses[0] + w_d L_depth) / d feat, by float64
    autograd."""
    base = rs.reference(scene, unit, use_bg_ray, bg=bg, zero_one_weight=zero_one_weight)
    feat = scene["feat"].double().requires_grad_(True)
    conf = scene["conf"].double()
    bgv = base["bg"]
    m = rs.march_ref(base["dist"], base["valid"], rs.densify(scene, feat), bgv)
    full, mask, _ = rs.fill_invalid(m["rgb"], m["bgT"], base["valid"], bgv)
    losses, _ = rs.loss_ref(full, mask, scene["gt"], conf, scene["conf"], base["pd"])
    z = z_fp32(scene)
    D, W, A = depth_of(m["w"], z, mask)
    l_depth = depth_loss(D, gt_depth, gt_mask)
    g = torch.autograd.grad(losses[0] + w_d * l_depth, feat, allow_unused=True)[0]
    g = torch.zeros_like(feat) if g is None else g
    return dict(base, D=D.detach(), W=W.detach(), A=A.detach(), z=z, l_depth=l_depth.detach(), dfeat_depth=g.detach())
