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
"""
import ctypes

import torch

from . import _lib
from .opts import HotPathOpts

_N_LOSS = 8
_N_LOSS_OPTS = 12   # sgn_loss_train_opts: + L_sparse, its gradient scale, sum of the weights, spare


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
        self._key = None

    def _buffers(self, R, SR, depth=False, K=0):
        """The workspace grows, never moves to a smaller one (a captured graph keeps the pointer it
        was captured with: HipTrainer gives every captured loss stage its own LossStage)."""
        L = _lib.lib()
        need = max(int(L.sgn_loss_depth_workspace_bytes(R, SR) if depth else L.sgn_loss_workspace_bytes(R, SR)), 16)
        if K:   # sgn_loss_train_opts
            need = max(need, int(L.sgn_loss_opts_workspace_bytes(R, SR, K)))
        if self._key is None or self.ws.numel() < need:
            self.ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            self._key = (R, SR)
        return self.ws

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
        stock = opts.stock_loss
        zero_one_weight = opts.zero_one_weight if zero_one_weight is None else zero_one_weight
        zero_eps = opts.zero_epsilon if zero_eps is None else zero_eps
        ws = self._buffers(R, opts.SR, depth is not None, 0 if stock else opts.K)
        campos = campos.reshape(3).to(dev, torch.float32).contiguous()
        rot = rot.reshape(3, 3).to(dev, torch.float32).contiguous()
        gt = gt.reshape(-1, 3).to(dev, torch.float32).contiguous()
        lp = _lib.LossParams()
        lp.SR, lp.K = opts.SR, opts.K
        lp.vsize_z, lp.raydist_mode_unit = float(opts.vsize[2]), int(opts.raydist_mode_unit)
        for i in range(3):
            lp.bg[i] = float(bg[i])
        # stock: dconf = d zero-one / d conf, weighted by autograd; else the kernel weighs every term
        lp.zero_one_weight, lp.zero_one_eps = 1.0 if stock else float(zero_one_weight), float(zero_eps)
        lo = None if stock else _lib.LossOpts(*opts.color_weights, float(opts.sparse_loss_weight),
                                              points.xyz.data_ptr())
        if bg_ray is not None:
            bg_ray = bg_ray.reshape(R, 3).to(dev, torch.float32).contiguous()
            lp.bg_ray = bg_ray.data_ptr()
        dmap = None
        if depth is not None:
            dmap = torch.empty(R, dtype=torch.float32, device=dev)
            dp = _lib.LossDepth(depth.gt.data_ptr(), None if depth.mask is None else depth.mask.data_ptr(),
                                depth.weight, dmap.data_ptr())

        def run(feat_t, conf_t):
            losses = torch.empty(_N_LOSS if stock else _N_LOSS_OPTS, dtype=torch.float32, device=dev)
            full = torch.empty(R, 3, dtype=torch.float32, device=dev)
            mask = torch.empty(R, dtype=torch.int8, device=dev)
            dfeat = torch.zeros_like(feat_t)   # entries past the rays' samples (capacity padding) stay 0
            dconf = torch.zeros(n_points, dtype=torch.float32, device=dev) if conf_t.requires_grad else None
            args = (_lib.ptr(campos), _lib.ptr(rot), R, ctypes.byref(q_abi), _lib.ptr(feat_t.detach()), _lib.ptr(gt),
                    _lib.ptr(conf_t.detach()), _lib.ptr(full), _lib.ptr(mask), _lib.ptr(losses), _lib.ptr(dfeat),
                    _lib.ptr(dconf), _lib.ptr(ws), ws.numel(), _lib.stream_handle())
            if not stock:
                _lib.check(_lib.lib().sgn_loss_train_opts(ctypes.byref(lp), ctypes.byref(lo),
                                                          None if depth is None else ctypes.byref(dp), *args),
                           "sgn_loss_train_opts")
            elif depth is None:
                _lib.check(_lib.lib().sgn_loss_train(ctypes.byref(lp), *args), "sgn_loss_train")
            else:
                _lib.check(_lib.lib().sgn_loss_train_depth(ctypes.byref(lp), ctypes.byref(dp), *args),
                           "sgn_loss_train_depth")
            return losses, full, mask, dfeat, None if dconf is None else dconf.view(conf_t.shape)

        losses, full, mask = _HipLoss.apply(feat, conf, run, not stock)
        l_col, l_zo = losses[0], losses[1]
        parts = {"ray_masked_coarse_raycolor": l_col.detach(), "ray_miss_coarse_raycolor": losses[2].detach(),
                 "coarse_raycolor": losses[3].detach(), "conf_coefficient": l_zo.detach()}
        if opts.sparse_loss_weight > 0:
            parts["sparse"] = losses[8].detach()
        if depth is not None:
            parts["coarse_depth"] = losses[7].detach()   # its gradient is in d feat already
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
