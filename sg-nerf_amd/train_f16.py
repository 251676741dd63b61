"""The f16 training step (precision "f16"): fp16-operand MFMA, fp32 accumulation.

`F16Step` is what `train_hip.HipTrainer` runs between its shared prologue (inputs, query) and
epilogue (all-reduce, point-row exchange):

  begin        the query's counts start their copy to pinned memory, the point Adam's launch
               (HipTrainer._adam_rows on the query's table), the MFMA blobs re-packed
  run          the step's one host sync (sample / work-item counts; under DP they ride the touched-row
               counts' sync), then
    forward      sgn_aggregate_train_fwd (k_agg_rows save mode): f_s (fp16) and alpha per sample, the
                 row layers' inputs saved
    colour+loss  one captured HIP graph per capacity bucket (sgn_colour_inputs, train_f32.ColourStage
                 with one fp16 product per backward multiply-add, its sgn_reduce_partials,
                 sgn_pow2_scale; the results out through ColourStage.results_out), or the same stage eagerly (HipTrainer.use_graph = False) through
                 loss_hip.LossStage and torch autograd of the colour MLP -- the graph's parity
                 reference in the tests
    backward     sgn_aggregate_backward (k_agg_bwd): deltas of the 4 row layers, d alpha-logit, point
                 gradients, under a power-of-two loss scale; dW = delta^T x per row layer on k_f16dw
                 (sgn_f16_weight_grad, split-K fp32 partials) and the alpha branch's weighted column
                 sums, all added into the flat gradient by one sgn_grad_accumulate
"""
import ctypes
import gc
import os

import torch
import torch.nn.functional as F

from . import _lib
from .flat_mlp import _colmap
from .loss_hip import LossStage, loss_parts
from .train import DepthTarget, _pe, gather_counts, touched_rows
from .train_f32 import ColourStage, _attach_bpack
from .weights import BPNET

# loss-stage graphs: capacity bucket (items / samples) and how many captured graphs are kept
GRAPH_BUCKET = int(os.environ.get("SGN_GRAPH_BUCKET", "8192"))
GRAPH_CACHE = 8

# rows per split-K batch of the colour layers' fp32 weight gradients
DW_CHUNK_COLOUR = int(os.environ.get("SGN_DW_CHUNK_COLOUR", "4096"))

_COLOUR = ("color_branch.0", "color_branch.2", "color_branch.4", "color_branch.6")


def _grad_into(g, dst, parts, tail=None, scale=None):
    """g[dst[j]] += (sum of the partials [nb, n] (+ tail)) (/ scale): one sgn_grad_accumulate launch."""
    n = dst.numel()
    seg = _lib.GradSegment(parts.data_ptr(), tail.data_ptr() if tail is not None else None, dst.data_ptr(), n, n,
                           parts.numel() // n, 0)
    _lib.check(_lib.lib().sgn_grad_accumulate(1, ctypes.byref(seg), _lib.ptr(scale), _lib.ptr(g),
                                              _lib.stream_handle()), "sgn_grad_accumulate")


class _LinearInto(torch.autograd.Function):
    """F.linear (fp32) of a weight / bias held in the flat parameter whose gradients the backward
    ADDS into the flat gradient (split-K weight partials through sgn_grad_accumulate, the bias sum
    in place) instead of returning them through autograd -- which would zero-fill a full-size
    gradient per parameter view, copy the slice in and add it back: six launches per layer."""

    @staticmethod
    def forward(ctx, x, w, b, g, dst_w, off_b):
        ctx.save_for_backward(x, w)
        ctx.g, ctx.dst_w, ctx.off_b = g, dst_w, off_b
        return F.linear(x, w, b)

    @staticmethod
    def backward(ctx, gz):
        x, w = ctx.saved_tensors
        gz = gz.contiguous()
        parts, tail = _fp32_rows_parts(gz, x, DW_CHUNK_COLOUR)
        _grad_into(ctx.g, ctx.dst_w, parts, tail)
        ctx.g[ctx.off_b:ctx.off_b + w.shape[0]].add_(gz.sum(0))
        return (gz @ w if ctx.needs_input_grad[0] else None), None, None, None, None, None


def _fp32_rows_parts(gz, x, chunk):
    """gz^T x (fp32) over the rows as split-K partials ([nb, M, N], tail [M, N] or None)."""
    rows = gz.shape[0]
    nb = rows // chunk if chunk > 0 else 0
    if nb <= 1:
        return (gz.t() @ x)[None].contiguous(), None
    body = nb * chunk
    parts = torch.bmm(gz[:body].view(nb, chunk, gz.shape[1]).transpose(1, 2), x[:body].reshape(nb, chunk, x.shape[1]))
    tail = (gz[body:].t() @ x[body:]).contiguous() if body < rows else None
    return parts.contiguous(), tail


def _inverse(m, n):
    inv = torch.full((n,), -1, dtype=torch.long, device=m.device)
    ok = m >= 0
    inv[m[ok]] = torch.nonzero(ok).reshape(-1)
    assert bool((inv >= 0).all())
    return inv


class F16Step:
    """The f16 step's buffers, column maps and captured loss-stage graphs, bound to one trainer."""

    def __init__(self, trainer):
        L = _lib.lib()
        self.tr = trainer
        dev = self.device = trainer.device
        # stored column p -> reference index; inverses: reference index -> stored column
        self.map_chain = _colmap(0, 256, dev)
        self.map_x0 = _colmap(1, 288, dev)
        self.map_h2 = _colmap(2, 272, dev)
        self.inv_chain = _inverse(self.map_chain, 256)
        self.inv_x0 = _inverse(self.map_x0, 284)
        self.inv_h2 = _inverse(self.map_h2, 263)
        self._flat_maps = {}     # layer -> int32 maps from its gradient's storage order to the flat gradient
        # the colour MLP, losses and their backward (train_f32.ColourStage on the HIP loss stage) as one
        # replayed HIP graph; trainer.use_graph = False runs the same stage eagerly (torch autograd of the
        # colour MLP into the HIP loss stage)
        self.loss_stage = LossStage(dev)
        self._graphs = {}        # (capacity bucket, buffers) -> captured loss stage, LRU order
        self.graph_captures = 0
        # per-sample features / per-item and per-row buffers: allocated at the first step, grown on demand
        self._scap = self._cap = 0
        self.feat = self.fs = None
        self.x0 = self.h1 = self.h2 = self.h3 = self.h4 = self.h2b = None   # the row layers' inputs
        self.d = self.db = self.dza = None                                  # their deltas (d1..d4), d alpha-logit
        self._dw_bufs = {}       # layer -> its split-K weight / bias gradient partials
        self._scale_ws = torch.empty(int(L.sgn_pow2_scale_workspace_bytes()), dtype=torch.uint8, device=dev)
        self._cs_ws = torch.empty(int(L.sgn_colsum_workspace_bytes(1)) // 4, dtype=torch.float32, device=dev)
        # the query's counts leave for pinned memory right after the query (one GPU)
        self._cnt_host = torch.zeros(2, dtype=torch.int32, pin_memory=dev.type == "cuda")
        self._cnt_event = torch.cuda.Event() if dev.type == "cuda" else None
        self._blobs = None       # this step's forward and transposed MFMA blobs (begin)
        self._dp_rows = None     # under DP: this rank's touched rows and every rank's count (run)

    # -- buffers -----------------------------------------------------------------------
    def _buffers(self, n_items, S_cap):
        dev = self.device
        if S_cap > self._scap:
            self.feat = torch.zeros(S_cap, 4, dtype=torch.float32, device=dev)
            self._scap = S_cap
        if n_items > self._cap or self.x0 is None:   # a first step without hits allocates too
            cap = max(128, ((n_items + 127) // 128) * 128)   # rows (8 per item) a multiple of 1024
            rows = cap * 8
            h = dict(dtype=torch.float16, device=dev)
            self.fs = torch.empty(cap, 256, **h)
            self.x0 = torch.empty(rows, 288, **h)
            self.h1 = torch.empty(rows, 256, **h)
            self.h2 = torch.empty(rows, 272, **h)
            self.h3 = torch.empty(rows, 256, **h)
            self.d = [torch.empty(rows, 256, **h) for _ in range(4)]  # d1..d4
            self.h4 = torch.empty(rows, 256, **h)
            if self.tr.sg:  # block2_bpnet inputs h and deltas
                self.h2b = torch.empty(rows, 256, **h)
                self.db = torch.empty(rows, 256, **h)
            self.dza = torch.empty(rows, dtype=torch.float32, device=dev)
            self._cap = cap

    def _colour(self, fs, v):
        """colour MLP (point_aggregators.py color_branch) on the flat parameter's weights (detached),
        the weight / bias gradients added straight into the flat gradient (_LinearInto)."""
        m = self.tr.mlp
        g = m.flat.grad
        vpe = _pe(v, 4, ori=True)[..., 3:]
        c = torch.cat([fs, vpe], dim=-1)
        for name in _COLOUR:
            dst = self._flat_maps.get(("colour", name))
            off, o, i = m.slices[name]
            if dst is None:
                dst = self._flat_maps[("colour", name)] = (off + torch.arange(o * i, device=self.device)).to(torch.int32)
            c = _LinearInto.apply(c, m.w(name).detach(), m.b(name).detach(), g, dst, off + o * i)
            if name != "color_branch.6":
                c = F.leaky_relu(c, 0.01)
        return torch.sigmoid(c) * (1 + 2 * 0.001) - 0.001

    def _loss_scale(self, dfs, dal):
        """2^-floor(log2(max |d|)) of the per-row deltas' inputs, on the device (sgn_pow2_scale)."""
        scale = torch.empty(1, dtype=torch.float32, device=self.device)
        _lib.check(_lib.lib().sgn_pow2_scale(_lib.ptr(dfs), dfs.numel(), _lib.ptr(dal), dal.numel(),
                                             _lib.ptr(self._scale_ws), _lib.ptr(scale), _lib.stream_handle()),
                   "sgn_pow2_scale")
        return scale

    # -- one step ------------------------------------------------------------------------
    def begin(self, b):
        """What the step queues before the gradients are made ready: the counts' copy (right after the
        query: the host then waits for the query only), the point Adam's launch and the blobs."""
        tr, q = self.tr, b.q
        if not b.dp:
            self._cnt_host.copy_(q.counters[:2], non_blocking=True)
            self._cnt_event.record()
        if tr._adam_rows(q.pidx, q.counters, False, tr.opts.K) is None and not tr.point_params:
            tr.touched_points(q)   # every point tensor frozen: no Adam launch, the OOB watch still sees the step
        # work that does not depend on the counts is queued before the step's one host sync, so the
        # GPU runs it while the host waits, and still has it queued when the host issues the rest
        self._blobs = tr.packer.pack(tr.mlp.flat)

    def run(self, b):
        """Forward + backward of the batch into the (ready) gradients.  Returns (loss parts, rendered
        colour [R, 3], ray_mask [R])."""
        tr, dev = self.tr, self.device
        o, q, R = tr.opts, b.q, b.R
        campos, rot, raydir = b.campos, b.rot, b.raydir
        blob, tblob = self._blobs
        if b.dp:   # the point rows this rank's step can touch, and every rank's count, ride the same sync
            t_idx, t_cnt = touched_rows(q.pidx, q.counters[0], o.K, tr.points.xyz.shape[0])
            sync = torch.cat([q.counters[:2].to(torch.int64), gather_counts(t_cnt)])
            S, n, *t_counts = (int(x) for x in sync.tolist())  # one host sync per step
            self._dp_rows = (t_idx, t_counts)
        else:
            self._cnt_event.synchronize()   # one host sync per step, on the query's counts
            S, n = (int(x) for x in self._cnt_host.tolist())
        graph = tr.use_graph and dev.type == "cuda"
        if graph:
            self._buffers(R * o.SR, R * o.SR)   # static shapes: every buffer at the batch's capacity
        else:
            self._buffers(n, max(S, 1))
        L = _lib.lib()
        st = _lib.stream_handle()
        pt = tr._tables(campos, rot, raydir)
        qo = q.abi()
        if graph:
            tr.packer32.pack(tr.mlp.flat)   # the colour GEMMs' weight shifts
            self.feat.zero_()               # samples without neighbours keep zero features
        saved = _lib.AggSaved(self.x0.data_ptr(), self.h1.data_ptr(), self.h2.data_ptr(), self.h3.data_ptr())
        if n > 0:   # h2b / db (block2_bpnet's input and delta) exist for SG trainers only
            _lib.check(L.sgn_aggregate_train_fwd(*tr.variant, _lib.ptr(tr.bpnet16), ctypes.byref(pt), ctypes.byref(qo),
                                                 n, o.K, _lib.ptr(blob), _lib.ptr(self.feat), _lib.ptr(self.fs),
                                                 ctypes.byref(saved), _lib.ptr(self.h2b), st),
                       "sgn_aggregate_train_fwd")
        # ---- colour MLP + composite + losses ------------------------------------------------
        if graph:
            out = self._graph_losses(b, S, n)
            b.depth_map = out.get("depth")
            total, parts, full, ray_mask = out["total"], dict(out["parts"]), out["full"], out["ray_mask"]
            dfs, dal, scale = out["dfs"], out["dal"], out["scale"]
        else:   # torch autograd, per sample / per ray
            samp = q.work[:n]   # int32 indices throughout (no widening copies)
            fs_t = self.fs[:n].float().requires_grad_(True)
            alpha_t = self.feat[samp, 0].clone().requires_grad_(True)
            v = raydir[q.samp_ray[samp]]
            feat_s = torch.cat([alpha_t[:, None], self._colour(fs_t, v)], dim=-1)
            featS = torch.zeros(S, 4, device=dev).index_put((samp,), feat_s)
            total, parts, full, ray_mask, *dmap = self.loss_stage(tr.points, qo, featS, campos, rot, b.gt, o, R,
                                                                  bg_ray=b.bg_ray, depth=b.depth)
            if dmap:
                b.depth_map = dmap[0]
            total.backward()
            if n > 0:
                dfs = fs_t.grad.contiguous()
                dal = alpha_t.grad.contiguous()
                scale = self._loss_scale(dfs, dal)
        # ---- HIP backward of the per-row part -----------------------------------------------
        if n > 0:
            deltas = _lib.AggDeltas(self.d[3].data_ptr(), self.d[2].data_ptr(), self.d[1].data_ptr(),
                                    self.d[0].data_ptr(), self.h4.data_ptr(), self.dza.data_ptr())
            grads = tr.point_grads()   # NULL members: frozen tensors
            _lib.check(L.sgn_aggregate_backward(*tr.variant, ctypes.byref(pt), ctypes.byref(qo), n, o.K,
                                                _lib.ptr(blob), _lib.ptr(tblob), ctypes.byref(saved),
                                                _lib.ptr(self.h2b), _lib.ptr(dfs), _lib.ptr(dal), _lib.ptr(scale),
                                                ctypes.byref(deltas), _lib.ptr(self.db), ctypes.byref(grads), st),
                       "sgn_aggregate_backward")
            self._weight_grads(n * 8, scale, q)
        parts["total"] = total.detach()
        return parts, full.detach(), ray_mask

    def dp_rows(self):
        """Under DP: this rank's touched rows and every rank's count (read in the step's sync)."""
        return self._dp_rows

    # -- graph-captured loss stage -----------------------------------------------------------
    def _loss_body(self, st):
        """Colour MLP + composite + losses + their backward on the hand-written kernels over the batch's
        full sample capacity (R * SR entries, static shapes, no host sync): items past the device count
        n and samples past S are padding, zeroed on input and routed to sentinel rows, so the gradients
        equal the eager path's.  Runs inside a HIP graph capture (and its warm-up)."""
        L = _lib.lib()
        stream = _lib.stream_handle()
        Sc, Nc = st["Sc"], st["Nc"]             # sample / item capacity of this graph
        q, col = st["q"], st["col"]
        fs32, al32, v, samp = st["fs32"], st["al32"], st["v"], st["samp"]
        # one launch: items past the device count n are padding (zeros, ray 0, sentinel sample Sc)
        _lib.check(L.sgn_colour_inputs(_lib.ptr(q.counters), _lib.ptr(q.work), _lib.ptr(q.samp_ray), Nc, Sc,
                                       _lib.ptr(self.fs), _lib.ptr(self.feat), _lib.ptr(st["raydir"]),
                                       _lib.ptr(fs32), _lib.ptr(al32), _lib.ptr(v), _lib.ptr(samp),
                                       _lib.ptr(col.vpe), stream), "sgn_colour_inputs")
        # hand-written colour MLP, losses and backward (train_f32.ColourStage), its weight gradients reduced
        st["amax"].zero_()
        col.forward_and_loss(st["campos"], st["rot"], st["gt"], st["bg_ray"], stream, st["depth"])
        col.backward(stream)
        _lib.check(L.sgn_reduce_partials(len(st["segs"]), st["segs"], stream), "sgn_reduce_partials")
        dfs = col.dfs
        dal = col.dfeat[samp.long(), 0]      # per item (padding: the zero row Sc)
        scale = self._loss_scale(dfs, dal)
        parts = loss_parts(self.tr.opts, col.losses, st["depth"] is not None)
        total = self.tr.opts.total_loss(parts, None if st["depth"] is None else st["depth"].weight)
        return {"scalars": torch.stack([total] + list(parts.values())), "names": list(parts),
                "dfs": dfs, "dal": dal, "scale": scale}

    def _graph_losses(self, b, S, n):
        """Replay the captured loss stage for this step's capacity bucket (item / sample counts
        rounded up to GRAPH_BUCKET); captured on first use and again when a buffer it reads
        moved.  At most GRAPH_CACHE graphs are kept.  A step with a per-ray background (bg_ray)
        replays a graph of its own whose static bg_ray buffer the step's colours are copied into; so does a
        step with depth supervision (static gt_depth / gt_mask buffers; the weight and the mask's presence
        are part of the key: the captured launch holds them)."""
        tr, dev = self.tr, self.device
        q, R, campos, rot, raydir, gt, bg_ray, depth = b.q, b.R, b.campos, b.rot, b.raydir, b.gt, b.bg_ray, b.depth
        P, fl = tr.points, tr.mlp.flat
        cap = R * tr.opts.SR
        Sc = min(cap, -(-max(S, 1) // GRAPH_BUCKET) * GRAPH_BUCKET)
        Nc = min(Sc, -(-max(n, 1) // GRAPH_BUCKET) * GRAPH_BUCKET)
        key = (R, Sc, Nc, q.work.data_ptr(), q.counters.data_ptr(), self.fs.data_ptr(), self.feat.data_ptr(),
               fl.data_ptr(), fl.grad.data_ptr(), P.points_conf.data_ptr(),
               None if P.points_conf.grad is None else P.points_conf.grad.data_ptr(), bg_ray is not None,
               None if depth is None else (depth.mask is not None, depth.weight))
        st = self._graphs.pop(key, None)
        if st is not None:
            self._graphs[key] = st              # most recently used goes last (LRU eviction order)
        else:
            self.graph_captures += 1
            if len(self._graphs) >= GRAPH_CACHE:
                self._graphs.pop(next(iter(self._graphs)))
            f32 = dict(dtype=torch.float32, device=dev)
            st = {"key": key, "R": R, "Sc": Sc, "Nc": Nc, "q": q,
                  "raydir": raydir.clone(), "gt": gt.clone(), "campos": campos.clone(), "rot": rot.clone(),
                  "bg_ray": None if bg_ray is None else bg_ray.clone(),
                  "depth": None if depth is None else DepthTarget(
                      depth.gt.clone(), None if depth.mask is None else depth.mask.clone(), depth.weight),
                  "fs32": torch.zeros(Nc, 256, **f32), "al32": torch.zeros(Nc, **f32),
                  "v": torch.zeros(Nc, 3, **f32), "samp": torch.zeros(Nc, dtype=torch.int32, device=dev),
                  "amax": torch.zeros(4, dtype=torch.int32, device=dev)}
            # items are the query's work-list positions (k_agg_rows' f_s rows), their device count at
            # q.counters[1]; PE(viewdir) | 1 | 0 arrives from sgn_colour_inputs; d feat has the padding
            # items' zero row; d f_s of the padding items stays 0 (the loss scale is the max over all rows);
            # the backward GEMMs take one fp16 product per multiply-add, the step's delta precision
            col = st["col"] = ColourStage(tr, q.abi(), R, Nc, q.counters[1:2].data_ptr(), st["fs32"], None, self.feat,
                                          torch.zeros(self.feat.shape[0] + 1, 4, **f32), st["amax"], products=1,
                                          zero_dfs=True)
            if depth is not None:
                col.depth = torch.empty(max(R, 1), **f32)
            st["segs"] = (_lib.PartialSegment * len(col.segments))(*col.segments)
            st["bpack"] = _attach_bpack(col.gemms, dev)
            cg = P.points_conf.grad   # None: conf is frozen, the stage writes no d conf
            keep = [fl.grad.clone(), None if cg is None else cg.clone()]   # warm-up accumulates into them
            side = torch.cuda.Stream(dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                for _ in range(2):
                    self._loss_body(st)
            torch.cuda.current_stream(dev).wait_stream(side)
            g = torch.cuda.CUDAGraph()
            # a garbage collection inside the capture would destroy dead objects that hold HIP resources (an
            # earlier trainer's graphs, streams, events), which invalidates a global-mode capture: keep the
            # collector off until the capture ends (no gc.collect() first: a full collection costs tens of ms
            # per capture, +0.3..0.9 ms per step over a 100-step run with one capture in it)
            gc_on = gc.isenabled()
            gc.disable()
            try:
                with torch.cuda.graph(g):
                    st["out"] = self._loss_body(st)
            finally:
                if gc_on:
                    gc.enable()
            fl.grad.copy_(keep[0])
            if cg is not None:
                cg.copy_(keep[1])
            st["graph"] = g
            self._graphs[key] = st
        # the step's inputs into the graph's static buffers: one launch
        _lib.copy_segments([(raydir, st["raydir"]), (gt, st["gt"]), (campos, st["campos"]), (rot, st["rot"])] +
                           ([] if bg_ray is None else [(bg_ray, st["bg_ray"])]) +
                           ([] if depth is None else [(depth.gt, st["depth"].gt)]) +
                           ([] if depth is None or depth.mask is None else [(depth.mask, st["depth"].mask)]))
        st["graph"].replay()
        out = st["out"]
        # the loss, its parts, the rendered colour and the ray mask out of the graph's buffers (the caller may
        # keep them across steps)
        sc, full, ray_mask, dmap = st["col"].results_out(out["scalars"], depth is not None)
        return {"total": sc[0], "parts": {k: sc[1 + i] for i, k in enumerate(out["names"])},
                "full": full, "ray_mask": ray_mask.view(torch.bool), "depth": dmap,
                "dfs": out["dfs"], "dal": out["dal"], "scale": out["scale"]}

    # -- weight gradients of the row layers ---------------------------------------------------
    def _dst_maps(self, name, x_cols, ix):
        """int32 maps from the MFMA storage order to the flat parameter for layer `name`: weight
        [256 stored units][x_cols stored columns] (-1: padding column) and bias [256 stored]."""
        maps = self._flat_maps.get(name)
        if maps is None:
            m, iu = self.tr.mlp, self.inv_chain
            off, o, i = m.slices[name]
            fi = (iu[:, None] * x_cols + ix[None, :]).reshape(-1)   # stored index of each reference weight
            dw = torch.full((o * x_cols,), -1, dtype=torch.int32, device=self.device)
            dw[fi] = (off + torch.arange(o * i, device=self.device)).to(torch.int32)
            db = torch.full((o,), -1, dtype=torch.int32, device=self.device)
            db[iu] = (off + o * i + torch.arange(o, device=self.device)).to(torch.int32)
            maps = self._flat_maps[name] = (dw, db)
        return maps

    def _dw_parts(self, name, d, x, rows):
        """dW = d^T x and db = sum_r d[r] over the first `rows` rows (fp16 operands, fp32 accumulation) as
        split-K partials ([splits, 256, C], [splits, 256]) from sgn_f16_weight_grad (rows past `rows` are
        never read).  One pair of buffers per layer: the step's single sgn_grad_accumulate reads them all."""
        C = x.shape[1]
        bufs = self._dw_bufs.get(name)
        if bufs is None or bufs[0].shape[2] != C:
            splits = max(1, 256 // -(-C // 128))   # about one workgroup per CU
            bufs = self._dw_bufs[name] = (torch.empty(splits, 256, C, dtype=torch.float32, device=self.device),
                                          torch.empty(splits, 256, dtype=torch.float32, device=self.device))
        parts, pb = bufs
        _lib.check(_lib.lib().sgn_f16_weight_grad(_lib.ptr(d), d.stride(0), _lib.ptr(x), x.stride(0), C, rows,
                                                  parts.shape[0], _lib.ptr(parts), _lib.ptr(pb), _lib.stream_handle()),
                   "sgn_f16_weight_grad")
        return parts, pb

    def _weight_grads(self, rows, scale, q=None):
        """dW_l = delta_l^T x_l (sgn_f16_weight_grad: fp16 operands, fp32 split-K partials), db_l = sum
        delta_l; the partials summed, unscaled and unpermuted into the flat gradient by one
        sgn_grad_accumulate launch."""
        tr = self.tr
        m = tr.mlp
        g = m.flat.grad
        L = _lib.lib()
        st = _lib.stream_handle()
        rp = ((rows + 1023) // 1024) * 1024   # rows padded (the SG embedding gather's view)
        # the alpha branch's dWa = dza^T h4 and dba = sum dza as row-slab partials (one launch; the final sums
        # happen in the step's sgn_grad_accumulate); the row layers' bias gradients come with their weight
        # gradients (sgn_f16_weight_grad's column sums)
        _lib.check(L.sgn_colsum_f16_weighted_parts(1, (ctypes.c_void_p * 1)(self.h4.data_ptr()),
                                                   (ctypes.c_void_p * 1)(self.dza.data_ptr()), rows, 256,
                                                   _lib.ptr(self._cs_ws), st), "sgn_colsum_f16_weighted_parts")
        ns = _lib.COLSUM_SLABS
        segs, keep = [], []

        def add(src, tail, dst):
            keep.append((src, tail))
            n = dst.numel()
            segs.append(_lib.GradSegment(src.data_ptr(), tail.data_ptr() if tail is not None else None,
                                         dst.data_ptr(), n, n, src.numel() // n, 0))
        if tr.sg:
            # block2_bpnet.0: x = [h (chain order) | the row's BPNet embedding (natural order)]
            x = self.h2b[:rp]
            if tr.variant[1]:
                # row r = item * 8 + k: rows k < K read pidx index s * K + k, rows k >= K are empty
                K = tr.opts.K
                r = torch.arange(rp, device=self.device)
                item, k = r // 8, r % 8
                ok = (item < rows // 8) & (k < K)
                s_of = q.work[torch.where(ok, item, 0)].long()
                pid = torch.where(ok, q.pidx[s_of * K + torch.clamp(k, max=K - 1)].long(), -1)
                bp = tr.bpnet16[torch.clamp(pid, min=0)]
                bp = torch.where((ok & (pid >= 0))[:, None], bp, torch.zeros((), dtype=bp.dtype, device=bp.device))
                x = torch.cat([x, bp], dim=1)
            ix = torch.cat([self.inv_chain, 256 + torch.arange(tr.variant[1], device=self.device)])
            dw, db = self._dst_maps(BPNET, x.shape[1], ix)
            parts, pb = self._dw_parts(BPNET, self.db, x, rows)
            add(parts, None, dw)
            add(pb, None, db)
        for name, d, x, ix in (("block3.2", self.d[3], self.h3, self.inv_chain),
                               ("block3.0", self.d[2], self.h2, self.inv_h2),
                               ("block1.2", self.d[1], self.h1, self.inv_chain),
                               ("block1.0", self.d[0], self.x0, self.inv_x0)):
            dw, db = self._dst_maps(name, x.shape[1], ix)
            parts, pb = self._dw_parts(name, d, x, rows)
            add(parts, None, dw)    # [256 stored][C stored]
            add(pb, None, db)
        # alpha branch: dWa = dza^T h4, dba = sum dza
        amaps = self._flat_maps.get("alpha_branch.0")
        if amaps is None:
            off, o, i = m.slices["alpha_branch.0"]
            dwa = torch.empty(256, dtype=torch.int32, device=self.device)
            dwa[self.inv_chain] = (off + torch.arange(256, device=self.device)).to(torch.int32)
            amaps = self._flat_maps["alpha_branch.0"] = (dwa, torch.full((1,), off + i, dtype=torch.int32,
                                                                        device=self.device))
        add(self._cs_ws[:ns * 256], None, amaps[0])         # [slabs][256] -> 256
        add(self._cs_ws[ns * 256:ns * 257], None, amaps[1])  # [slabs] -> 1
        _lib.check(L.sgn_grad_accumulate(len(segs), (_lib.GradSegment * len(segs))(*segs), _lib.ptr(scale),
                                         _lib.ptr(g), st), "sgn_grad_accumulate")
