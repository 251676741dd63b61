"""Hot-path subset of the reference's option namespace.

The reference spreads these over argparse hooks
(models/neural_points/neural_points.py:80-309,
models/aggregators/point_aggregators.py:14-253,
models/neural_points_volumetric_model.py:63-124).  Defaults below are the
ScanNet values of dev_scripts/w_scannet_etf/scene241.sh:11-106 and
pointnerf/run/checkpoints/scannet/scene0710_00640480/opt.txt.
"""
import math
import numbers
from dataclasses import dataclass, field, fields, replace
from typing import Tuple

COLOR_LOSS_ITEMS = ("ray_masked_coarse_raycolor", "ray_miss_coarse_raycolor", "coarse_raycolor")


@dataclass(frozen=True)
class HotPathOpts:
    # querier (query_point_indices_worldcoords.py)
    vsize: Tuple[float, float, float] = (0.008, 0.008, 0.008)
    vscale: Tuple[int, int, int] = (2, 2, 2)
    kernel_size: Tuple[int, int, int] = (3, 3, 3)
    query_size: Tuple[int, int, int] = (3, 3, 3)
    ranges: Tuple[float, ...] = (-10.0, -10.0, -10.0, 10.0, 10.0, 10.0)
    radius_limit_scale: float = 4.0
    depth_limit_scale: float = 0.0
    z_depth_dim: int = 400
    max_o: int = 610000
    SR: int = 24
    K: int = 8
    P: int = 26
    NN: int = 2
    inverse: int = 0
    wcoord_query: int = 1
    semantic_guidance: int = 0
    predict_semantic: int = 0  # 1: BPNet embedding (96) feeds block2_bpnet (point_aggregators.py:346)
    near_plane: float = 0.1
    far_plane: float = 8.0
    # aggregator (point_aggregators.py)
    point_features_dim: int = 32
    shading_feature_num: int = 256
    shading_feature_mlp_layer1: int = 2
    shading_feature_mlp_layer2: int = 0
    shading_feature_mlp_layer2_bpnet: int = 0
    shading_feature_mlp_layer3: int = 2
    shading_alpha_mlp_layer: int = 1
    shading_color_mlp_layer: int = 4
    shading_color_channel_num: int = 3
    num_feat_freqs: int = 3
    dist_xyz_freq: int = 5
    num_viewdir_freqs: int = 4
    num_pos_freqs: int = 10
    view_ori: int = 0
    agg_dist_pers: int = 20
    agg_distance_kernel: str = "linear"
    agg_intrp_order: int = 2
    agg_weight_norm: int = 1
    agg_axis_weight: Tuple[float, float, float] = (1.0, 1.0, 1.0)
    agg_feat_xyz_mode: str = "None"
    agg_alpha_xyz_mode: str = "None"
    agg_color_xyz_mode: str = "None"
    apply_pnt_mask: int = 1
    act_type: str = "LeakyReLU"
    act_super: int = 1
    dist_xyz_deno: float = 0.0
    point_color_mode: str = "1"
    point_dir_mode: str = "1"
    point_conf_mode: str = "1"
    # which neural-point tensors train (neural_points.py:410-416, again after prune / grow :527-536,
    # :553-560): any non-zero value means trained (the reference tests `> 0`), a frozen tensor gets no
    # gradient and no Adam moments.  The defaults are scene241.sh:13-16 (all four trained), not the
    # reference's argparse default dir_grad 0: a driver's opt always carries the real value (from_opt).
    feat_grad: int = 1
    color_grad: int = 1
    dir_grad: int = 1
    conf_grad: int = 1
    xyz_grad: int = 0          # positions feed the grid and the query, which carry no gradient here
    # ray marching (neural_points_volumetric_model.py)
    raydist_mode_unit: int = 1
    which_tonemap_func: str = "off"
    which_render_func: str = "radiance"
    which_blend_func: str = "alpha"
    bg_color: str = "white"
    # depth (neural_points_volumetric_model.py:211, 620-624; base_rendering_model.py:611-618): compute_depth
    # adds coarse_depth to the outputs, depth_loss_items = ("coarse_depth",) trains against inputs['gt_depth']
    compute_depth: int = 0
    depth_loss_items: Tuple[str, ...] = ()
    depth_loss_weights: Tuple[float, ...] = (1.0,)
    # the training objective (base_rendering_model.py:534-664).  Colour items in any order or a subset, one weight
    # per item (or one for all), each listed item adding weight * loss + 1e-6; the zero-one loss on
    # conf_coefficient (an empty item list drops it); sparse_loss_weight > 0 adds the sparse loss on conf
    # (:652-662, reported as "sparse").  The defaults are the ScanNet opt.txt.  bg / l2_size items are refused.
    color_loss_items: Tuple[str, ...] = COLOR_LOSS_ITEMS
    color_loss_weights: Tuple[float, ...] = (1.0, 0.0, 0.0)
    zero_one_loss_items: Tuple[str, ...] = ("conf_coefficient",)
    zero_one_loss_weights: Tuple[float, ...] = (1e-4,)
    zero_epsilon: float = 1e-3
    sparse_loss_weight: float = 0.0
    bg_loss_items: Tuple[str, ...] = ()
    l2_size_loss_items: Tuple[str, ...] = ()
    # knobs of this implementation (no reference counterpart)
    # aggregator arithmetic: "f32" = the reference's fp32 products, each carried as three fp16 MFMA
    # products with fp32 accumulation (mlp_x3.hip); "f16" = fp16 MFMA operands (mlp.hip, faster)
    precision: str = "f32"
    fix_occ0: int = 0          # 1: do not reproduce the `voxel_idx > 0` bug (worldcoords.py:395)
    reservoir_seed: int = 0    # replaces the reference's wall-clock curand seed (:314, :402)
    # early ray termination of HipRenderer.render (render.py): a ray whose transmittance has fallen to
    # early_stop or below at a slot boundary of early_stop_slots skips its remaining samples; a colour
    # channel moves by at most 1.001 * early_stop.  0 = off (every valid sample is aggregated).
    early_stop: float = 0.0
    early_stop_slots: Tuple[int, ...] = (4, 8, 16)   # strictly increasing; boundaries >= SR are ignored
    # 1: HipRenderer renders the viewmlp without block3 (shading_feature_mlp_layer3 = 0) on the split-fp16 row
    # GEMMs (sgn_x3_gemm over item windows, render.py) instead of the plain-fp32 kernels.  0 = off.
    rows_gemm: int = 0
    # 1: HipRenderer renders that network on the fused split-fp16 row kernel (k_rows16 without block3,
    # sgn_aggregate_f32_nb3): the stock f32 path's frame with two of its row layers.  0 = off.
    rows_fused: int = 0
    # 1: HipTrainer trains the viewmlp without block3 (shading_feature_mlp_layer3 = 0) with the fp32 step on the
    # split-fp16 row GEMMs (train_f32.F32StepNb3).  0 = off: training that network stays refused.
    train_rows: int = 0
    is_train: int = 0

    @property
    def bpnet_variant(self):
        """(bpnet_layers, bpnet_dim) of the aggregator (SG block2_bpnet, point_aggregators.py:345-354)."""
        if self.shading_feature_mlp_layer2_bpnet == 0:
            return 0, 0
        return 1, (96 if self.predict_semantic == 1 else 0)

    @property
    def block3_layers(self):
        """block3's layer count: 2, or 0 for the viewmlp without block3 (point_aggregators.py:356-368), which
        the plain-fp32 kernels render (sgn_aggregate_exact_nb3)."""
        return int(self.shading_feature_mlp_layer3)

    @property
    def _train_rows_on(self):
        """train_rows is the integer 1 (True, 1.0 and "1" are refused, not taken for it)."""
        tr = self.train_rows
        return not isinstance(tr, bool) and isinstance(tr, numbers.Integral) and tr == 1

    @property
    def trained_points(self):
        """The trained point tensors' names, in the point Adam group's order.  Without block3 the points' colour
        and dir are outside the network's graph (point_aggregators.py:356-368): frozen whatever their switches say."""
        nb3 = not self.block3_layers
        sw = (("points_embeding", self.feat_grad), ("points_color", 0 if nb3 else self.color_grad),
              ("points_dir", 0 if nb3 else self.dir_grad), ("points_conf", self.conf_grad))
        return tuple(name for name, v in sw if v)

    @property
    def want_depth(self):
        """Whether the outputs carry coarse_depth."""
        return bool(self.compute_depth) or bool(self.depth_loss_items)

    @property
    def depth_loss_weight(self):
        """The weight of the coarse_depth loss item, or None without depth supervision."""
        if "coarse_depth" not in self.depth_loss_items:
            return None
        w = self.depth_loss_weights
        return float(w[0] if len(w) == 1 else w[self.depth_loss_items.index("coarse_depth")])

    @staticmethod
    def _item_weight(items, weights, name):
        """weights[i] of `name` in items (one weight serves every item), 0.0 when it is not listed."""
        if name not in items:
            return 0.0
        return float(weights[0] if len(weights) == 1 else weights[items.index(name)])

    @property
    def color_weights(self):
        """(w_masked, w_miss, w_all): the weights of the three colour items, 0 for one that is not listed."""
        return tuple(self._item_weight(self.color_loss_items, self.color_loss_weights, n) for n in COLOR_LOSS_ITEMS)

    @property
    def zero_one_weight(self):
        """The weight of the zero-one loss on conf_coefficient, 0 when it is not listed."""
        return self._item_weight(self.zero_one_loss_items, self.zero_one_loss_weights, "conf_coefficient")

    @property
    def stock_loss(self):
        """Whether the loss stage runs its stock entries: the ScanNet colour weights and no sparse loss (the
        zero-one weight and epsilon travel in the stock parameters)."""
        return self.color_weights == (1.0, 0.0, 0.0) and not self.sparse_loss_weight > 0

    def total_loss(self, parts, depth_weight=None, zero_one_weight=None):
        """loss_total from the reported parts (a mapping of the items' names, "conf_coefficient", "sparse" and
        "coarse_depth" to scalars), as compute_losses adds it up: weight * loss + 1e-6 per listed colour item,
        then the zero-one, sparse and depth terms.  Items of weight 0 only leave their 1e-6 (the defaults give
        ray_masked + 3e-6 + 1e-4 * conf_coefficient, in this order).  zero_one_weight: a caller's override."""
        zw = self.zero_one_weight if zero_one_weight is None else zero_one_weight
        total = None
        for name, w in zip(COLOR_LOSS_ITEMS, self.color_weights):
            if w != 0.0:
                t = parts[name] if w == 1.0 else w * parts[name]
                total = t if total is None else total + t
        eps = len(self.color_loss_items) / 1e6
        total = eps if total is None else total + eps
        if zw != 0.0:
            total = total + zw * parts["conf_coefficient"]
        if self.sparse_loss_weight > 0:
            total = total + self.sparse_loss_weight * parts["sparse"]
        if depth_weight is not None:
            total = total + depth_weight * parts["coarse_depth"]
        return total

    @property
    def early_stop_tiers(self):
        """The slot ranges [lo, hi) a frame is aggregated in with early_stop > 0: [0, b0), [b0, b1), ...,
        [b_last, SR) over the boundaries of early_stop_slots below SR."""
        b = [0] + [int(x) for x in self.early_stop_slots if x < self.SR] + [int(self.SR)]
        return tuple(zip(b[:-1], b[1:]))

    @classmethod
    def from_opt(cls, opt, **overrides):
        """Take every known field from a reference-style Namespace."""
        kw = {}
        for f in fields(cls):
            if hasattr(opt, f.name):
                v = getattr(opt, f.name)
                if isinstance(v, list):
                    v = tuple(v)
                if f.name in ("depth_loss_items", "depth_loss_weights", "color_loss_items", "color_loss_weights",
                              "zero_one_loss_items", "zero_one_loss_weights", "bg_loss_items",
                              "l2_size_loss_items"):   # unset (None) or one bare value
                    if v is None:
                        continue
                    v = v if isinstance(v, tuple) else (v,)
                if f.name == "early_stop_slots":   # unset (None), "4,8,16" or one bare value
                    if v is None:
                        continue
                    if isinstance(v, str):
                        v = tuple(int(x) for x in v.replace(",", " ").split())
                    v = v if isinstance(v, tuple) else (int(v),)
                if f.name in ("early_stop", "zero_epsilon", "sparse_loss_weight", "rows_gemm", "rows_fused",
                              "train_rows") and v is None:
                    continue
                kw[f.name] = v
        # argparse's lone default weight beside unset items (color_loss_items None, color_loss_weights [1.0]):
        # the ScanNet items keep their ScanNet weights
        for items, weights in (("color_loss_items", "color_loss_weights"), ("zero_one_loss_items", "zero_one_loss_weights")):
            if items not in kw and len(kw.get(weights, ())) == 1:
                del kw[weights]
        kw.update(overrides)
        o = cls(**kw)
        if o.query_size[0] == 0:  # neural_points.py:425
            o = replace(o, query_size=o.kernel_size)
        return o

    def check_supported(self):
        """The HIP path implements the ScanNet viewmlp layout; refuse others loudly."""
        bad = []
        if self.wcoord_query != 1:
            bad.append("wcoord_query must be 1 (perspective querier is out of scope)")
        if self.agg_dist_pers != 20 or self.agg_distance_kernel != "linear" or self.agg_intrp_order != 2:
            bad.append("aggregator must be agg_dist_pers=20, linear kernel, agg_intrp_order=2")
        if (self.point_features_dim, self.shading_feature_num, self.num_feat_freqs, self.dist_xyz_freq,
                self.num_viewdir_freqs) != (32, 256, 3, 5, 4):
            bad.append("MLP widths/frequencies must match the ScanNet viewmlp (32/256/3/5/4)")
        if (self.shading_feature_mlp_layer1, self.shading_feature_mlp_layer2, self.shading_feature_mlp_layer3,
                self.shading_alpha_mlp_layer, self.shading_color_mlp_layer) not in ((2, 0, 2, 1, 4), (2, 0, 0, 1, 4)):
            bad.append("viewmlp layer counts must be (2, 0, 2, 1, 4), or (2, 0, 0, 1, 4) without block3")
        elif self.shading_feature_mlp_layer3 == 0:
            # the viewmlp without block3 (point_aggregators.py:356-368) renders on the plain-fp32 kernels only
            if self.precision == "f16":
                bad.append("shading_feature_mlp_layer3 = 0 is rendered in plain fp32 only: precision must be 'f32', not 'f16'")
            if self.is_train and not self._train_rows_on:
                bad.append("shading_feature_mlp_layer3 = 0 renders only: training (is_train) is not implemented")
        if self.shading_feature_mlp_layer2_bpnet not in (0, 1):
            bad.append("block2_bpnet: at most one layer (shading_feature_mlp_layer2_bpnet 0 or 1)")
        elif self.shading_feature_mlp_layer2_bpnet == 1 and bool(self.predict_semantic) != bool(self.semantic_guidance):
            # the reference concatenates the gathered embedding iff semantic_guidance (neural_points.py:971,
            # point_aggregators.py:631-635) but sizes the layer by predict_semantic (:346): other pairs crash there
            bad.append("block2_bpnet needs predict_semantic == semantic_guidance")
        if self.shading_feature_mlp_layer2_bpnet == 0 and self.predict_semantic not in (0, 1):
            bad.append("predict_semantic must be 0 or 1")
        if self.act_type != "LeakyReLU" or self.act_super != 1 or self.view_ori != 0:
            bad.append("activations must be LeakyReLU + act_super=1, view_ori=0")
        if self.agg_feat_xyz_mode != "None" or self.agg_alpha_xyz_mode != "None" or self.agg_color_xyz_mode != "None":
            bad.append("agg_*_xyz_mode must be None")
        if self.dist_xyz_deno != 0.0 or self.apply_pnt_mask != 1 or self.agg_weight_norm != 1:
            bad.append("dist_xyz_deno=0, apply_pnt_mask=1, agg_weight_norm=1 required")
        if self.which_render_func != "radiance" or self.which_blend_func != "alpha":
            bad.append("radiance render + alpha blend required")
        if self.precision not in ("f32", "f16"):
            bad.append("precision must be 'f32' (reference arithmetic) or 'f16'")
        if self.inverse != 0:
            bad.append("inverse (disparity) ray generation is not implemented")
        if self.xyz_grad:
            bad.append("xyz_grad must be 0 (point positions feed the grid and the query, which carry no gradient)")
        other = [i for i in self.depth_loss_items if i != "coarse_depth"]
        if other:
            bad.append(f"depth_loss_items: only coarse_depth is produced, not {', '.join(map(str, other))}")
        if self.depth_loss_items and len(self.depth_loss_weights) not in (1, len(self.depth_loss_items)):
            bad.append("depth_loss_weights must hold one weight or one per depth_loss_items entry")
        def weights_ok(w):
            return all(not isinstance(x, bool) and isinstance(x, numbers.Real) and math.isfinite(x) and x >= 0 for x in w)
        other = [i for i in self.color_loss_items if i not in COLOR_LOSS_ITEMS]
        if other:
            bad.append(f"color_loss_items: only {', '.join(COLOR_LOSS_ITEMS)} are produced, not "
                       f"{', '.join(map(str, other))}")
        if len(set(self.color_loss_items)) != len(self.color_loss_items):
            bad.append("color_loss_items must not repeat an item")
        if self.color_loss_items and len(self.color_loss_weights) not in (1, len(self.color_loss_items)):
            bad.append("color_loss_weights must hold one weight or one per color_loss_items entry")
        if not weights_ok(self.color_loss_weights):
            bad.append("color_loss_weights must be finite and non-negative")
        other = [i for i in self.zero_one_loss_items if i != "conf_coefficient"]
        if other:
            bad.append(f"zero_one_loss_items: only conf_coefficient is produced, not {', '.join(map(str, other))}")
        if len(self.zero_one_loss_items) > 1:
            bad.append("zero_one_loss_items must not repeat an item")
        if self.zero_one_loss_items and len(self.zero_one_loss_weights) not in (1, len(self.zero_one_loss_items)):
            bad.append("zero_one_loss_weights must hold one weight or one per zero_one_loss_items entry")
        if not weights_ok(self.zero_one_loss_weights):
            bad.append("zero_one_loss_weights must be finite and non-negative")
        ze = self.zero_epsilon
        if isinstance(ze, bool) or not isinstance(ze, numbers.Real) or not 0.0 < ze < 0.5:   # NaN fails too
            bad.append("zero_epsilon must satisfy 0 < zero_epsilon < 0.5")
        if not weights_ok((self.sparse_loss_weight,)):
            bad.append("sparse_loss_weight must be finite and non-negative")
        if self.bg_loss_items:
            bad.append("bg_loss_items must be empty (the background loss is not implemented)")
        if self.l2_size_loss_items:
            bad.append("l2_size_loss_items must be empty (the l2 size loss is not implemented)")
        es = self.early_stop
        if isinstance(es, bool) or not isinstance(es, numbers.Real) or not 0.0 <= es < 1.0:   # NaN fails too
            bad.append("early_stop (transmittance threshold) must satisfy 0 <= early_stop < 1")
        sl = self.early_stop_slots
        if (not isinstance(sl, tuple) or any(isinstance(x, bool) or not isinstance(x, numbers.Integral) or x <= 0 for x in sl)
                or any(b <= a for a, b in zip(sl, sl[1:]))):
            bad.append("early_stop_slots must be a tuple of strictly increasing positive slot boundaries")
        rg = self.rows_gemm
        if isinstance(rg, bool) or not isinstance(rg, numbers.Integral) or rg not in (0, 1):
            bad.append("rows_gemm must be 0 or 1")
        elif rg == 1:
            if self.shading_feature_mlp_layer3 != 0:
                bad.append("rows_gemm = 1 renders the viewmlp without block3 only (shading_feature_mlp_layer3 = 0)")
            if self.precision != "f32":
                bad.append("rows_gemm = 1 is the split-fp16 fp32-faithful path: precision must be 'f32'")
            if self.is_train:
                bad.append("rows_gemm = 1 renders only: not with is_train")
        rf = self.rows_fused
        if isinstance(rf, bool) or not isinstance(rf, numbers.Integral) or rf not in (0, 1):
            bad.append("rows_fused must be 0 or 1")
        elif rf == 1:
            if self.shading_feature_mlp_layer3 != 0:
                bad.append("rows_fused = 1 renders the viewmlp without block3 only (shading_feature_mlp_layer3 = 0)")
            if self.precision != "f32":
                bad.append("rows_fused = 1 is the split-fp16 fp32-faithful path: precision must be 'f32'")
            if self.is_train:
                bad.append("rows_fused = 1 renders only: not with is_train")
            if not isinstance(rg, bool) and isinstance(rg, numbers.Integral) and rg == 1:
                bad.append("rows_fused = 1 and rows_gemm = 1 are two paths for the same frames: set one of them")
        tr = self.train_rows
        if isinstance(tr, bool) or not isinstance(tr, numbers.Integral) or tr not in (0, 1):
            bad.append("train_rows must be 0 or 1")
        elif tr == 1:
            if self.shading_feature_mlp_layer3 != 0:
                bad.append("train_rows = 1 trains the viewmlp without block3 only (shading_feature_mlp_layer3 = 0): the "
                           "stock network trains on its own step")
            if self.precision != "f32":
                bad.append("train_rows = 1 is the fp32 step on the split-fp16 row GEMMs: precision must be 'f32'")
        if bad:
            raise NotImplementedError("; ".join(bad))
        return self


SCANNET = HotPathOpts()
