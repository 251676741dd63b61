"""Fused frame renderer: query -> MFMA aggregator -> composite, all on one stream,
no host synchronisation and no [R, SR, K, C] intermediates.

This is the product path behind NeuralPointsRayMarching.forward (ray_marching.py)
and bench.py.  Buffers are sized once per (R, SR) and reused.
"""
import ctypes
from dataclasses import dataclass, replace

import torch

from . import _lib
from .opts import HotPathOpts
from .querier import LightningFastQuerier
from .rows_gemm import RowsGemmNb3
from .weights import block3_layers, mlp_variant, pack_mlp, strip_prefix


@dataclass
class RenderOut:
    rgb: torch.Tensor        # [R,3] fill_invalid'ed colour (bg for invalid rays)
    ray_mask: torch.Tensor   # [R] int8, reference ray_mask after masked_valid_ray
    bg_transmission: torch.Tensor  # [R] coarse_is_background (1 for invalid rays)
    opacity: torch.Tensor    # [R,SR] coarse_point_opacity (0 for invalid rays / empty slots)
    query: object            # QueryResult (sample-major, device)
    feat: torch.Tensor       # [S_cap,4] per-sample (alpha, r, g, b)
    blend: torch.Tensor      # [S_cap,8] weight * conf_coefficient (when want_blend)
    wnorm: torch.Tensor = None    # [S_cap,8] normalised weight (when want_weights)
    blendw: torch.Tensor = None   # [R,SR] alpha-blend weight o*T (when want_weights)
    probe: torch.Tensor = None    # [R,48] packed hole-probing records (sgn_probe; when want_probe)
    depth: torch.Tensor = None    # [R] coarse_depth, 0 for invalid rays (sgn_composite_depth; when want_depth)
    # early ray termination (opts.early_stop > 0 and the frame was aggregated tier by tier; else None)
    stop_slot: torch.Tensor = None   # [R] int32: the slot boundary at which the ray was found finished, SR if never
    skipped: torch.Tensor = None     # int32 scalar (device): valid samples that were not aggregated
    tiers: torch.Tensor = None       # [n_tiers, 4] int32 (device): sgn_early_stop_tier's counters of each tier


class PointTables:
    """Device-resident neural point cloud (contiguous fp32 tables).

    `rot`: the reference's Rw2c (neural_points.py:967), [N,3,3] per point or one [3,3] for every
    point -> the [N,9] table the rotated kernels read.  A table that is exactly identity is kept as
    None: such clouds run the stock kernels, bit for bit.

    `color` / `dir` may be None for the viewmlp without block3 (shading_feature_mlp_layer3 = 0), which reads
    neither; every other consumer (the stock aggregators, the hole probe) refuses such tables."""

    def __init__(self, xyz, embedding, color, dir, conf, device, bpnet=None, rot=None):
        def t(x, cols):
            x = torch.as_tensor(x).reshape(-1, cols)
            return x.to(device=device, dtype=torch.float32).contiguous()
        self.xyz = t(xyz, 3)
        self.embedding = t(embedding, 32)
        self.color = None if color is None else t(color, 3)
        self.dir = None if dir is None else t(dir, 3)
        self.conf = t(conf, 1)
        self.n = self.xyz.shape[0]
        self.bpnet16 = None
        self.bpnet32 = None
        if bpnet is not None:
            self.set_bpnet(bpnet)
        self.rot = self._rot_table(rot, device)

    def _rot_table(self, rot, device):
        if rot is None:
            return None
        r = torch.as_tensor(rot).detach().to(dtype=torch.float32)
        if r.numel() == 9:
            r = r.reshape(1, 3, 3)
        elif r.numel() == 9 * self.n and r.dim() >= 2:
            r = r.reshape(self.n, 3, 3)
        else:
            raise ValueError(f"Rw2c has shape {tuple(r.shape)}: expected [3,3] or [{self.n},3,3]")
        if torch.equal(r, torch.eye(3, dtype=torch.float32, device=r.device).expand_as(r)):
            return None
        return r.expand(self.n, 3, 3).reshape(self.n, 9).to(device=device).contiguous()

    def set_bpnet(self, bpnet):
        """SG: bpnet_points_embedding [N, 96] (neural_points.py:653-665, detached there too)
        -> the fp16 table the aggregator gathers (sgn_bpnet_pack)."""
        b = torch.as_tensor(bpnet).reshape(-1, 96).to(device=self.xyz.device, dtype=torch.float32).contiguous()
        if b.shape[0] != self.n:
            raise ValueError(f"bpnet embedding has {b.shape[0]} rows for {self.n} points")
        self.bpnet32 = b  # fp32 table of the fp32-faithful aggregator
        self.bpnet16 = torch.empty(self.n, 96, dtype=torch.float16, device=self.xyz.device)
        with torch.cuda.device(self.xyz.device):
            _lib.check(_lib.lib().sgn_bpnet_pack(_lib.ptr(b), self.n, 96, _lib.ptr(self.bpnet16),
                                                 _lib.stream_handle()), "sgn_bpnet_pack")

    @classmethod
    def from_cloud(cls, pc, device):
        return cls(pc.xyz, pc.embedding, pc.color, pc.dir, pc.conf, device, getattr(pc, "bpnet", None),
                   getattr(pc, "rot", None))


class HipRenderer:
    def __init__(self, points: PointTables, mlp_state, opts: HotPathOpts, device, rows_gemm=None, rows_ci=None,
                 rows_fused=None):
        """rows_gemm (0 / 1): overrides opts.rows_gemm -- the viewmlp without block3 on the split-fp16 row GEMMs
        (rows_gemm.RowsGemmNb3).  rows_ci: that path's window size in work items (default: CI K <= 1 M rows).
        rows_fused (0 / 1): overrides opts.rows_fused -- that network on the fused split-fp16 row kernel
        (sgn_aggregate_f32_nb3)."""
        self.device = torch.device(device)
        if rows_gemm is not None:
            opts = replace(opts, rows_gemm=rows_gemm)
        if rows_fused is not None:
            opts = replace(opts, rows_fused=rows_fused)
        self.opts = opts.check_supported()
        if self.opts.rows_gemm and self.opts.K > 8:
            raise NotImplementedError(f"rows_gemm = 1 holds a sample's rows in one wave: K <= 8, not {self.opts.K}")
        if self.opts.rows_fused and self.opts.K > 8:
            raise NotImplementedError(f"rows_fused = 1 holds a sample's rows in one 8-row half: K <= 8, not {self.opts.K}")
        self.fused = bool(self.opts.rows_fused)   # rows_fused = 1: the viewmlp without block3 on the fused row kernel
        self._fused_frame = False                 # the last frame was aggregated on it
        self._rows_ci = rows_ci
        self.rows = None           # rows_gemm = 1: the row-GEMM path's weights, window buffers and launch arguments
        self._rows_frame = False   # the last frame was aggregated on it
        self.points = points
        self.querier = LightningFastQuerier(self.device, opts)
        self.set_mlp(mlp_state)
        self._cap = None
        self._proj = None
        self._fp = None        # sgn_frame_points buffers (marks, list, counts) for the projection subset
        self._pending = []   # deferred fp16-range checks: (pinned flag copy, event)
        self._flag_host = None
        self._tiered = False   # the last frame was aggregated tier by tier (early ray termination)

    def set_mlp(self, mlp_state):
        nb3 = block3_layers(mlp_state)
        if nb3 != self.opts.block3_layers:
            raise ValueError(f"aggregator weights hold {nb3} block3 layers, options say "
                             f"shading_feature_mlp_layer3 = {self.opts.block3_layers}")
        self.block3 = nb3
        self.mlp_state = {k: torch.as_tensor(v).detach().to("cpu", torch.float32)
                          for k, v in strip_prefix(mlp_state, block3_layers=nb3).items()}
        self.variant = mlp_variant(self.mlp_state)
        if self.variant != self.opts.bpnet_variant:
            raise ValueError(f"aggregator weights are block2_bpnet variant {self.variant}, options say "
                             f"{self.opts.bpnet_variant} (shading_feature_mlp_layer2_bpnet / predict_semantic)")
        self.f32 = self.opts.precision == "f32"
        if not self.block3:
            # the viewmlp without block3 lives on the plain-fp32 path (sgn_aggregate_exact_nb3): no split-fp16
            # blob, no point projection, no fp16-range check, and (as on that path, _tiers) no early-stop tiers
            self.packed = None
            self.packed_exact = pack_mlp(self.mlp_state, self.device, "exact", block3_layers=0)
            self.exact = True
            if self.opts.rows_gemm:
                # ... or, opted in, on the split-fp16 row GEMMs, with the plain-fp32 path as the range fallback
                # (`exact` turns on once a frame's activations left fp16 range) and for rotated points / tiers
                self.rows = RowsGemmNb3(self.mlp_state, self.variant, self.opts.K, self._rows_ci, self.device)
                self.exact = False
            if self.fused:
                # ... or on the fused split-fp16 row kernel: the stock f32 path's frame (frame point list,
                # projection, paired rows, colour, workspace range flag) on its own blob, with the plain-fp32 path
                # as the range fallback and for rotated points
                self.packed = pack_mlp(self.mlp_state, self.device, "fused", block3_layers=0)
                self.exact = False
            return
        self.packed = pack_mlp(self.mlp_state, self.device, self.opts.precision)
        # f32 mode's range fallback: plain fp32 weights for sgn_aggregate_exact, packed on first use; `exact`
        # turns on (for these weights) once a frame's activations left fp16 range
        self.packed_exact = None
        self.exact = False

    def _buffers(self, R):
        SR = self.opts.SR
        if self._cap is None or self._cap[0] < R:
            cap = max(R * SR, 1)
            dev = self.device
            self.feat = torch.empty(cap, 4, dtype=torch.float32, device=dev)
            self.blend = torch.empty(cap, self.opts.K, dtype=torch.float32, device=dev)
            L = _lib.lib()
            nb = int(L.sgn_aggregate_workspace_bytes_f32(cap) if self.f32 else L.sgn_aggregate_workspace_bytes(cap))
            self.agg_ws = torch.empty(nb, dtype=torch.uint8, device=dev)
            self.rgb = torch.empty(max(R, 1), 3, dtype=torch.float32, device=dev)
            self.mask = torch.empty(max(R, 1), dtype=torch.int8, device=dev)
            self.bgT = torch.empty(max(R, 1), dtype=torch.float32, device=dev)
            self.opacity = torch.empty(max(R, 1), SR, dtype=torch.float32, device=dev)
            self.wnorm = None
            self.blendw = None
            self.probe = None
            self.depth = None
            self.viewdir = None   # [cap,3] rotated view direction per sample (rotated points only)
            self.es = None        # early ray termination: (tier work list, tier counters, stop_slot, range flag)
            self._cap = (R, cap)
        if self.points.rot is not None and self.viewdir is None:
            self.viewdir = torch.zeros(self._cap[1], 3, dtype=torch.float32, device=self.device)

    def _es_buffers(self):
        """Early ray termination: the tier work list [cap], one counters row per tier, stop_slot [R] and the
        fp16-range flag accumulated over a frame's tiers (f32 mode)."""
        if self.es is None:
            i32 = dict(dtype=torch.int32, device=self.device)
            self.es = (torch.empty(self._cap[1], **i32), torch.zeros(len(self.opts.early_stop_tiers), 4, **i32),
                       torch.empty(max(self._cap[0], 1), **i32), torch.zeros(1, **i32))
        return self.es

    def _ws_flag(self):
        off = int(_lib.lib().sgn_aggregate_flag_offset_f32(self.agg_ws.numel()))
        return self.agg_ws[off:off + 4].view(torch.int32)

    def _flag(self):
        """The fp16-range flag of the last frame: the workspace word of its colour stage, or, for a frame
        aggregated tier by tier (every tier's colour stage clears that word), the OR over its tiers."""
        if self._rows_frame:   # the row-GEMM path: its launches' amax words folded into one
            return self.rows.flag()
        return self.es[3] if self._tiered else self._ws_flag()

    def _range_check(self, mode, redo):
        """f32 mode: the colour stage flags samples whose decoded features are not finite (an
        activation outside fp16 range, mlp_x3.hip header).  "sync": check now (one stream sync) and,
        when flagged, re-run the frame's aggregation and composite on the plain-fp32 path (`redo`,
        sgn_aggregate_exact), which later frames then take directly; "deferred": copy the flag to
        pinned memory and check it after the NEXT frame has been enqueued (or at finish()), so frames
        stay pipelined -- a flagged frame raises there (its output was handed out already) and switches
        the renderer to the plain-fp32 path; False: no check."""
        if not self.f32 or not mode or self.exact:
            return
        if self.rows is not None and not self._rows_frame:
            return   # rows_gemm = 1, but this frame ran on the plain-fp32 path (rotated points, early-stop tiers)
        if self.fused and not self._fused_frame:
            return   # rows_fused = 1, but this frame ran on the plain-fp32 path (rotated points)
        if mode == "sync":
            flag = self._flag()
            if int(flag.item()) != 0:
                self.exact = True
                flag.zero_()
                redo()
            return
        if self._flag_host is None:
            self._flag_host = [torch.zeros(1, dtype=torch.int32, pin_memory=True) for _ in range(2)]
        prev = self._pending.pop(0) if self._pending else None   # at most one frame is pending
        buf = self._flag_host[1] if prev is not None and prev[0] is self._flag_host[0] else self._flag_host[0]
        buf.copy_(self._flag(), non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._pending.append((buf, ev))
        if prev is not None:
            self._raise_if_flagged(*prev)

    def _raise_if_flagged(self, buf, ev):
        ev.synchronize()
        if int(buf.item()) != 0:
            self.exact = True   # every later frame on the plain-fp32 path
            self._flag().zero_()
            raise _lib.SgnError("sgn_aggregate_f32: fp16 range exceeded -- an aggregator activation or point "
                                "feature reached |x| >= 65504, so the decoded features of a frame rendered with "
                                "check_range='deferred' are not finite; the renderer now uses the plain-fp32 path "
                                "(sgn_aggregate_exact): render that frame again")

    def _tiers(self, want_probe=False, want_weights=False, want_blend=False):
        """The slot ranges of a frame aggregated tier by tier (opts.early_stop_tiers), or () for a frame
        rendered in full: early_stop = 0, training options, per-slot outputs wanted (the aggregate
        entries zero blend / wnorm on every call, and the hole probe must see every sample), or the
        plain-fp32 range fallback."""
        o = self.opts
        if not o.early_stop > 0 or o.is_train or want_probe or want_weights or want_blend or self.exact or o.rows_fused:
            return ()
        return o.early_stop_tiers

    def finish(self):
        """Wait for the deferred range checks of the frames rendered so far (raises if one failed)."""
        while self._pending:
            self._raise_if_flagged(*self._pending.pop(0))

    def render(self, campos, camrotc2w, raydir, near, far, want_opacity=True, want_blend=False, marks=None,
               bg=None, want_weights=False, point_labels=None, ray_labels=None, seconds=None,
               count_traffic=False, check_range="sync", want_probe=False, query_size=None, want_depth=False):
        """One frame.  `marks(name)` (optional) is called between stages on the host thread
        (bench.py records HIP events on the current stream there).  `bg`: 3 floats
        overriding opts.bg_color.  `want_weights`: also produce the normalised neighbour
        weights and the per-slot alpha-blend weights (reference `weight`, `blend_weight`).
        `point_labels` [N] / `ray_labels` [R] int32 (+ `seconds`): the SG semantic-guided kNN
        (semantic_guidance = 1, worldcoords.py:839-938).  `check_range`: the f32 mode's fp16-range
        guard ("sync" default: a frame whose activations leave fp16 range is re-rendered on the
        plain-fp32 path, sgn_aggregate_exact; "deferred" for pipelined frame loops + finish(), False).
        The viewmlp without block3 with rows_fused = 1 takes the stock protocol as it is (the workspace flag of
        sgn_aggregate_f32_nb3, fallback sgn_aggregate_exact_nb3) and renders frames of rotated points on the
        plain-fp32 path and every frame in full (no early-stop tiers).
        The viewmlp without block3 with rows_gemm = 1 follows the same protocol on its own amax words
        (rows_gemm.RowsGemmNb3.flag, fallback sgn_aggregate_exact_nb3); that path reads the frame's item count
        on the host once per frame (one small copy and stream sync, whatever check_range says), and renders
        frames of rotated points and frames the stock network would aggregate tier by tier on the plain-fp32 path.
        `want_probe`: also the per-ray hole-probing records (opt.prob = 1; sgn_probe, RenderOut.probe
        [R, 48]); implies want_opacity and want_blend.  `query_size`: overrides opts.query_size for this
        call (probe_hole's prob_kernel_size); the cached grid is kept.  `want_depth`: also the depth map
        (RenderOut.depth [R]: sum w z / (sum w + 1e-6) over the blend weights and the samples' camera-space z,
        0 for rays without a valid sample; sgn_composite_depth in place of sgn_composite).

        Early ray termination (opts.early_stop = eps > 0, no reference counterpart): the frame is aggregated
        tier by tier over the slot ranges of opts.early_stop_tiers.  Before each tier sgn_early_stop_tier
        recomputes every ray's transmittance T over the slots done so far; a ray with T <= eps is finished --
        its remaining valid samples are not aggregated and get feat (0, 0, 0, 0), so the composite (run once
        over the full query, unchanged) gives them opacity exactly 0.  A colour channel moves by at most
        1.001 eps and bg_transmission rises by at most eps against the full render; ray_mask does not move.
        RenderOut.stop_slot / skipped / tiers report what was skipped.  want_depth works (a skipped sample
        has weight 0).  The option is ignored, and the frame rendered in full (those three fields None), with
        want_probe, want_weights or want_blend (the aggregate entries zero the per-slot outputs on every call,
        and the hole probe must see every sample), with opts.is_train, and on the plain-fp32 range fallback
        (a frame whose tiers flag the fp16 range is re-rendered there in full)."""
        o = self.opts
        if want_probe:
            want_opacity = want_blend = True
        mark = marks or (lambda name: None)
        campos = campos.reshape(3).to(self.device, torch.float32).contiguous()
        rot = camrotc2w.reshape(3, 3).to(self.device, torch.float32).contiguous()
        raydir = raydir.reshape(-1, 3).to(self.device, torch.float32).contiguous()
        R = raydir.shape[0]
        self._buffers(R)
        if want_weights and self.wnorm is None:
            self.wnorm = torch.empty(self._cap[1], o.K, dtype=torch.float32, device=self.device)
            self.blendw = torch.empty(max(self._cap[0], 1), o.SR, dtype=torch.float32, device=self.device)
        if want_weights:
            self.wnorm.zero_()
        if want_probe and self.probe is None:
            self.probe = torch.empty(max(self._cap[0], 1), _lib.PROBE_RECORD, dtype=torch.float32, device=self.device)
        if want_depth and self.depth is None:
            self.depth = torch.empty(max(self._cap[0], 1), dtype=torch.float32, device=self.device)
        mark("query")
        if o.semantic_guidance == 1 and (point_labels is None or ray_labels is None):
            raise ValueError("semantic_guidance = 1 needs point_labels and ray_labels")
        q = self.querier.query_samples(self.points.xyz, campos, raydir, near, far, point_labels, ray_labels, seconds,
                                       count_traffic, query_size)
        L = _lib.lib()
        st = _lib.stream_handle()
        pt = _lib.PointTables()
        pts = self.points
        if self.block3 and (pts.color is None or pts.dir is None):
            raise ValueError("point tables without colour / dir: block3 reads both (only the viewmlp without block3, "
                             "shading_feature_mlp_layer3 = 0, renders without them)")
        if want_probe and (pts.color is None or pts.dir is None):
            raise ValueError("the hole probe (want_probe) averages the points' colour and dir: the point tables hold none")
        pt.xyz, pt.embedding, pt.conf, pt.n_points = pts.xyz.data_ptr(), pts.embedding.data_ptr(), pts.conf.data_ptr(), pts.n
        pt.color = None if pts.color is None else pts.color.data_ptr()
        pt.dir = None if pts.dir is None else pts.dir.data_ptr()
        pt.campos, pt.camrotc2w, pt.raydir = campos.data_ptr(), rot.data_ptr(), raydir.data_ptr()
        qo = q.abi()
        cap = R * o.SR
        nl, dim = self.variant
        if self.points.rot is not None:
            # rotated points (per-point Rw2c): the samples' rotated view directions, once per frame
            if nl:
                raise NotImplementedError("a non-identity Rw2c is built for the base viewmlp only, not block2_bpnet (SG)")
            pt.rot = self.points.rot.data_ptr()
            _lib.check(L.sgn_sample_viewdirs(ctypes.byref(pt), ctypes.byref(qo), cap, o.K, _lib.ptr(self.viewdir), st),
                       "sgn_sample_viewdirs")
            pt.samp_viewdir = self.viewdir.data_ptr()
        if dim and self.points.bpnet16 is None:
            raise ValueError("block2_bpnet with predict_semantic = 1 needs the points' BPNet embedding (set_bpnet)")
        bp = (_lib.ptr(self.points.bpnet32) if self.f32 else _lib.ptr(self.points.bpnet16)) if dim else None
        def aggregate_exact():
            # the f32 mode's range fallback: the whole aggregator and colour MLP in plain fp32
            if self.packed_exact is None:
                self.packed_exact = pack_mlp(self.mlp_state, self.device, "exact")
            entry, name = ((L.sgn_aggregate_exact, "sgn_aggregate_exact") if self.block3 else
                           (L.sgn_aggregate_exact_nb3, "sgn_aggregate_exact_nb3"))
            _lib.check(entry(nl, dim, bp, ctypes.byref(pt), ctypes.byref(qo), cap, o.K,
                             _lib.ptr(self.packed_exact), _lib.ptr(self.feat),
                             _lib.ptr(self.blend) if want_blend else None,
                             _lib.ptr(self.wnorm) if want_weights else None, _lib.ptr(self.agg_ws),
                             self.agg_ws.numel(), _lib.stream_handle()), name)

        # split block1.0: P[point] = W0a [feat | PE(feat)] + b0, once per frame, for the points the
        # frame's samples name only (sgn_frame_points: ~19 % of a config-2 frame's)
        mark("proj")
        # rows_fused = 1: the frame on the fused row kernel, unless the plain-fp32 path has to take it (after a range
        # fallback, with rotated points)
        self._fused_frame = self.fused and not self.exact and self.points.rot is None
        split = self.block3 or self.fused   # the paths that read a point projection
        nproj = 0 if not split else int(L.sgn_point_proj_bytes_f32(self.points.n) if self.f32 else
                                        L.sgn_point_proj_bytes(self.points.n))
        if split and (self._proj is None or self._proj.numel() < nproj):
            self._proj = torch.empty(max(nproj, 16), dtype=torch.uint8, device=self.device)
        if not self.exact and (self.block3 or self._fused_frame):
            n = self.points.n
            if self._fp is None or self._fp[0] != n:
                self._fp = (n, torch.zeros(int(L.sgn_frame_points_mark_bytes(n)), dtype=torch.uint8, device=self.device),
                            torch.empty(n, dtype=torch.int32, device=self.device),
                            torch.zeros(2, dtype=torch.int64, device=self.device))
            _, marks, plist, pcount = self._fp
            _lib.check(L.sgn_frame_points(_lib.ptr(q.pidx), _lib.ptr(q.counters), q.pidx.numel() // o.K, o.K, n,
                                          _lib.ptr(marks), _lib.ptr(plist), _lib.ptr(pcount), st), "sgn_frame_points")
            project = (L.sgn_point_project_f32_nb3 if self.fused else
                       L.sgn_point_project_f32 if self.f32 else L.sgn_point_project)   # different arithmetic
            _lib.check(project(ctypes.byref(pt), _lib.ptr(self.packed), _lib.ptr(plist), _lib.ptr(pcount),
                               _lib.ptr(self._proj), st), "point projection (frame list)")
        cp = _lib.CompositeParams()
        cp.SR, cp.vsize_z, cp.raydist_mode_unit = o.SR, float(o.vsize[2]), o.raydist_mode_unit
        if bg is None:
            bg = (1.0, 1.0, 1.0) if o.bg_color == "white" else (0.0, 0.0, 0.0)
        for i in range(3):
            cp.bg[i] = bg[i]

        def aggregate(stage, qa):
            blend = _lib.ptr(self.blend) if want_blend else None
            wnorm = _lib.ptr(self.wnorm) if want_weights and stage == 1 else None
            if self.fused:
                _lib.check(L.sgn_aggregate_f32_nb3(nl, dim, bp, _lib.ptr(self._proj), ctypes.byref(pt), ctypes.byref(qa),
                                                   cap, o.K, _lib.ptr(self.packed), _lib.ptr(self.feat), blend, wnorm,
                                                   _lib.ptr(self.agg_ws), self.agg_ws.numel(), stage, st),
                           "sgn_aggregate_f32_nb3")
            elif self.f32:
                _lib.check(L.sgn_aggregate_f32(nl, dim, bp, _lib.ptr(self._proj), ctypes.byref(pt), ctypes.byref(qa), cap, o.K,
                                               _lib.ptr(self.packed), _lib.ptr(self.feat), blend, wnorm,
                                               _lib.ptr(self.agg_ws), self.agg_ws.numel(), stage, st), "sgn_aggregate_f32")
            else:
                _lib.check(L.sgn_aggregate(nl, dim, bp, _lib.ptr(self._proj), ctypes.byref(pt), ctypes.byref(qa), cap,
                                           o.K, _lib.ptr(self.packed), _lib.ptr(self.feat), blend, wnorm,
                                           _lib.ptr(self.agg_ws), self.agg_ws.numel(), stage, st), "sgn_aggregate")

        tiers = self._tiers(want_probe, want_weights, want_blend)
        if self.rows is not None:
            # rows_gemm = 1: the frame on the row GEMMs, unless the plain-fp32 path has to take it: after a range
            # fallback, with rotated points, and where the stock network would aggregate tier by tier
            self._rows_frame = not self.exact and self.points.rot is None and not tiers
            tiers = ()
        self._tiered = bool(tiers)
        if tiers:
            # early ray termination: tier by tier, every launch enqueued without a host sync.  Each tier's
            # work list is built on the device from the transmittance over the slots already aggregated
            # (sgn_early_stop_tier); the aggregators run on a copy of the query naming that list.
            work, counters, stop_slot, flag = self._es_buffers()
            stop_slot.fill_(o.SR)
            flag.zero_()
            qt = q.abi()
            qt.work = work.data_ptr()
            for t, (lo, hi) in enumerate(tiers):
                mark("agg_tier" if t else "agg_rows")
                qt.counters = counters[t].data_ptr()
                _lib.check(L.sgn_early_stop_tier(ctypes.byref(cp), _lib.ptr(campos), _lib.ptr(rot), R, ctypes.byref(qo),
                                                 _lib.ptr(self.feat), lo, hi, float(o.early_stop), cap, _lib.ptr(work),
                                                 _lib.ptr(counters[t]), _lib.ptr(counters[t - 1]) if t else None,
                                                 _lib.ptr(stop_slot), st), "sgn_early_stop_tier")
                aggregate(1, qt)
                aggregate(2, qt)
                if self.f32:
                    flag.bitwise_or_(self._ws_flag())
        else:
            for stage, name in ((1, "agg_rows"), (2, "agg_color")):
                mark(name)
                if self._rows_frame:
                    if stage == 1:
                        self.rows.run(pt, qo, q, cap, bp, self.feat, self.blend if want_blend else None,
                                      self.wnorm if want_weights else None)
                elif self.exact or self.rows is not None or (self.fused and not self._fused_frame):
                    if stage == 1:
                        aggregate_exact()
                else:
                    aggregate(stage, qo)
        mark("composite")

        def composite():
            args = (ctypes.byref(cp), _lib.ptr(campos), _lib.ptr(rot), _lib.ptr(raydir), R, _lib.ptr(q.t_table),
                    q.per_ray_t, q.t_table.shape[-1], ctypes.byref(qo), _lib.ptr(self.feat), _lib.ptr(self.rgb),
                    _lib.ptr(self.mask), _lib.ptr(self.bgT), _lib.ptr(self.opacity) if want_opacity else None,
                    _lib.ptr(self.blendw) if want_weights else None)
            if want_depth:
                _lib.check(L.sgn_composite_depth(*args, _lib.ptr(self.depth), _lib.stream_handle()),
                           "sgn_composite_depth")
            else:
                _lib.check(L.sgn_composite(*args, _lib.stream_handle()), "sgn_composite")

        def probe():
            # after the composite: reads its opacity and mask, and the aggregator's blend
            if want_probe:
                _lib.check(L.sgn_probe(ctypes.byref(pt), ctypes.byref(qo), _lib.ptr(self.opacity), _lib.ptr(self.blend),
                                       _lib.ptr(self.mask), R, o.SR, o.K, _lib.ptr(self.probe), _lib.stream_handle()),
                           "sgn_probe")
        composite()
        if want_probe:
            mark("probe")
            probe()
        mark("end")
        self._range_check(check_range, lambda: (aggregate_exact(), composite(), probe()))
        if self.exact:
            tiers = ()   # the range fallback re-rendered the frame in full
        return RenderOut(self.rgb[:R], self.mask[:R], self.bgT[:R], self.opacity[:R], q, self.feat, self.blend,
                         self.wnorm if want_weights else None, self.blendw[:R] if want_weights else None,
                         self.probe[:R] if want_probe else None, self.depth[:R] if want_depth else None,
                         *((self.es[2][:R], self.es[1][-1, 2], self.es[1]) if tiers else ()))

    def points_projected(self):
        """The last frame's projected point count and the neighbour indices >= n_points met so far
        (host sync), or None before any frame (or on the plain-fp32 fallback path only)."""
        if self._fp is None:
            return None
        c, bad = (int(x) for x in self._fp[3].tolist())
        return c, bad

    def grid_info(self):
        return self.querier.grid_for(self.points.xyz).info()
