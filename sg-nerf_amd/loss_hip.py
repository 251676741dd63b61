"""The training losses on the HIP loss stage (csrc/loss.hip, sgn_loss_train).

`LossStage(...)` has the signature and results of train.composite_losses (ray_dist +
ray_march + fill_invalid + ray_masked_coarse_raycolor + zero_one_loss on conf_coefficient, with
ray_miss / coarse colour logged; neural_points_volumetric_model.py:569-631,
diff_ray_marching.py:509-555, base_rendering_model.py:534-664, mvs_points_volumetric_model.py:607-614)
but runs as three HIP launches that compute the losses AND their gradients w.r.t. the per-sample
features and the points' conf in one pass, with no host synchronisation (graph-capturable).
Autograd sees one node: its backward scales the kernel's gradients by the incoming ones.

The objective follows the options' colour items and weights, zero-one weight and epsilon and sparse_loss_weight
(base_rendering_model.py:534-664).  The ScanNet colour weights without a sparse loss run the stock entries as
before; anything else runs sgn_loss_train_opts with the real weights, whose gradients are d total / d feat and
d total / d conf as they stand.

This module owns the stage's call path for every HIP step (train_f32.ColourStage, F32Runner, train_f16.F16Step):
the argument structs, the workspace size, the entry choice (loss_train) and the loss vector's names (loss_parts).
"""
import ctypes

import torch

from . import _lib
from .opts import HotPathOpts


def loss_params(opts: HotPathOpts, bg=(1.0, 1.0, 1.0), bg_ray=None, zero_one_weight=None, zero_eps=None):
    """sgn_loss_params from the options.  bg_ray: the rays' background [R, 3] (device fp32, contiguous; replaces bg).
    zero_one_weight / zero_eps: None reads opts.zero_one_weight / zero_epsilon (train_ft: weight 1e-4, epsilon 1e-3)."""
    lp = _lib.LossParams()
    lp.SR, lp.K = opts.SR, opts.K
    lp.vsize_z, lp.raydist_mode_unit = float(opts.vsize[2]), int(opts.raydist_mode_unit)
    lp.bg = (_lib.c_f32 * 3)(*bg)
    lp.zero_one_weight = float(opts.zero_one_weight if zero_one_weight is None else zero_one_weight)
    lp.zero_one_eps = float(opts.zero_epsilon if zero_eps is None else zero_eps)
    if bg_ray is not None:
        lp.bg_ray = bg_ray.data_ptr()
    return lp


def loss_opts(opts: HotPathOpts, points):
    """sgn_loss_opts (the colour weights, the sparse loss and the points' xyz its neighbour weights are restated
    from), or None: the ScanNet objective on the stock entries."""
    if opts.stock_loss:
        return None
    return _lib.LossOpts(*opts.color_weights, float(opts.sparse_loss_weight), points.xyz.data_ptr())


def loss_depth(depth, out_depth):
    """sgn_loss_depth of a train.DepthTarget writing the depth map into out_depth [R], or None without one."""
    if depth is None:
        return None
    return _lib.LossDepth(depth.gt.data_ptr(), None if depth.mask is None else depth.mask.data_ptr(), depth.weight,
                          out_depth.data_ptr())


def loss_len(lo):   # the loss vector: 8 floats, 12 of sgn_loss_train_opts (+ L_sparse, its scale, sum of weights, spare)
    return 8 if lo is None else 12


def workspace_bytes(R, SR, K, stock, depth):
    """Bytes of the loss stage's workspace for the entry these settings select."""
    L = _lib.lib()
    return max(int(L.sgn_loss_depth_workspace_bytes(R, SR) if depth else L.sgn_loss_workspace_bytes(R, SR)),
               0 if stock else int(L.sgn_loss_opts_workspace_bytes(R, SR, K)), 16)


def loss_train(lp, lo, dp, *args):
    """The loss stage's launch: sgn_loss_train_opts under loss options (lo), else sgn_loss_train_depth with depth
    supervision (dp), else sgn_loss_train.  args: the entries' common tail, campos .. stream."""
    L = _lib.lib()
    if lo is not None:
        _lib.check(L.sgn_loss_train_opts(ctypes.byref(lp), ctypes.byref(lo), None if dp is None else ctypes.byref(dp),
                                         *args), "sgn_loss_train_opts")
    elif dp is not None:
        _lib.check(L.sgn_loss_train_depth(ctypes.byref(lp), ctypes.byref(dp), *args), "sgn_loss_train_depth")
    else:
        _lib.check(L.sgn_loss_train(ctypes.byref(lp), *args), "sgn_loss_train")


def loss_parts(opts: HotPathOpts, losses, depth):
    """The reported parts by name from the loss vector (any indexable of scalars); depth: the stage ran with one."""
    parts = {"ray_masked_coarse_raycolor": losses[0], "ray_miss_coarse_raycolor": losses[2],
             "coarse_raycolor": losses[3], "conf_coefficient": losses[1]}
    if opts.sparse_loss_weight > 0:
        parts["sparse"] = losses[8]
    if depth:
        parts["coarse_depth"] = losses[7]
    return parts


class _HipLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, conf, run, weighted=False):
        losses, full, mask, dfeat, dconf = run(feat, conf)
        ctx.save_for_backward(dfeat, dconf)
        ctx.weighted = weighted
        ctx.mark_non_differentiable(full, mask)
        return losses, full, mask

    @staticmethod
    def backward(ctx, g_losses, g_full, g_mask):
        dfeat, dconf = ctx.saved_tensors
        # losses[0] = ray_masked_coarse_raycolor (d/d feat in dfeat), losses[1] = zero-one (d/d conf in dconf)
        # (dconf None: points_conf is frozen, the kernel skipped its zero-one gradients)
        # weighted (sgn_loss_train_opts ran with every weight): both are d total already, total's handle is losses[0]
        g_conf = g_losses[0] if ctx.weighted else g_losses[1]
        return dfeat * g_losses[0], None if dconf is None else dconf * g_conf, None, None


class LossStage:
    """The loss stage with its reusable workspace."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.ws = None

    def __call__(self, points, q_abi, feat, campos, rot, gt, opts: HotPathOpts, R, bg=(1.0, 1.0, 1.0),
                 zero_one_weight=None, zero_eps=None, bg_ray=None, depth=None):
        """feat [S_cap, 4] fp32 per sample (alpha, r, g, b; zeros for samples without neighbours),
        q_abi: the query's sgn_query_out; bg_ray: the rays' background [R, 3] (device, replaces bg).
        zero_one_weight / zero_eps: None reads opts.zero_one_weight / opts.zero_epsilon.
        depth: a train.DepthTarget -- depth supervision on sgn_loss_train_depth, whose d feat carries the
        depth term's gradient already scaled by depth.weight (backward scales it with losses[0]'s incoming
        gradient, as the colour term's).
        Returns (total, parts, full [R, 3], ray_mask [R] bool) and, with depth, the depth map [R], as
        train.composite_losses."""
        dev = self.device
        conf = points.points_conf
        n_points = conf.shape[0]
        feat = feat.contiguous()
        if feat.shape[0] == 0:   # a batch without samples: one zero row keeps the pointers valid
            feat = torch.cat([feat, feat.new_zeros(1, 4)])
        lo = loss_opts(opts, points)
        stock = lo is None
        zero_one_weight = opts.zero_one_weight if zero_one_weight is None else zero_one_weight
        need = workspace_bytes(R, opts.SR, opts.K, stock, depth is not None)
        if self.ws is None or self.ws.numel() < need:   # the workspace grows, never moves to a smaller one
            self.ws = torch.empty(need, dtype=torch.uint8, device=dev)
        campos = campos.reshape(3).to(dev, torch.float32).contiguous()
        rot = rot.reshape(3, 3).to(dev, torch.float32).contiguous()
        gt = gt.reshape(-1, 3).to(dev, torch.float32).contiguous()
        if bg_ray is not None:
            bg_ray = bg_ray.reshape(R, 3).to(dev, torch.float32).contiguous()
        # stock: dconf = d zero-one / d conf, weighted by autograd; else the kernel weighs every term
        lp = loss_params(opts, bg, bg_ray, 1.0 if stock else zero_one_weight, zero_eps)
        dmap = None if depth is None else torch.empty(R, dtype=torch.float32, device=dev)
        dp = loss_depth(depth, dmap)

        def run(feat_t, conf_t):
            losses = torch.empty(loss_len(lo), dtype=torch.float32, device=dev)
            full = torch.empty(R, 3, dtype=torch.float32, device=dev)
            mask = torch.empty(R, dtype=torch.int8, device=dev)
            dfeat = torch.zeros_like(feat_t)   # entries past the rays' samples (capacity padding) stay 0
            dconf = torch.zeros(n_points, dtype=torch.float32, device=dev) if conf_t.requires_grad else None
            args = (_lib.ptr(campos), _lib.ptr(rot), R, ctypes.byref(q_abi), _lib.ptr(feat_t.detach()), _lib.ptr(gt),
                    _lib.ptr(conf_t.detach()), _lib.ptr(full), _lib.ptr(mask), _lib.ptr(losses), _lib.ptr(dfeat),
                    _lib.ptr(dconf), _lib.ptr(self.ws), self.ws.numel(), _lib.stream_handle())
            loss_train(lp, lo, dp, *args)
            return losses, full, mask, dfeat, None if dconf is None else dconf.view(conf_t.shape)

        losses, full, mask = _HipLoss.apply(feat, conf, run, not stock)
        l_col, l_zo = losses[0], losses[1]
        parts = loss_parts(opts, losses.detach(), depth is not None)   # coarse_depth's gradient is in d feat already
        if stock:
            total = opts.total_loss({**parts, "ray_masked_coarse_raycolor": l_col, "conf_coefficient": l_zo},
                                    zero_one_weight=zero_one_weight)
            if depth is not None:
                total = total + depth.weight * parts["coarse_depth"]
        else:   # the value of the weighted sum on the node's one differentiable handle
            value = opts.total_loss(parts, None if depth is None else depth.weight, zero_one_weight=zero_one_weight)
            total = l_col + (value - l_col.detach())
        if depth is None:
            return total, parts, full, mask.bool()
        return total, parts, full, mask.bool(), dmap
