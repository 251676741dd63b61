"""Training step on the HIP kernels.

The reference trains through torch autograd (`optimize_parameters`,
models/base_rendering_model.py:534-664; models/mvs_points_volumetric_model.py:47-141).  Here the
whole step -- the NeuralPoints gather, the per-row MLP + alpha + K-blend of PointAggregator
(point_aggregators.py:868-959, :561-786), the colour MLP, ray_dist / ray_march and the losses,
and all their gradients -- runs as hand-written HIP launches; torch only allocates buffers and
all-reduces gradients.

`HipTrainer` holds what every step shares: the parameters (the points, the MLP as one flat fp32
parameter: flat_mlp.FlatMLP, its MFMA blobs re-packed on the device every step), the two Adam
groups (point_adam.PointAdam), the query, and `backward`:

  prologue   inputs normalised, sgn_query (jittered depths, is_train)
  step       the precision's step object: `begin` (the point Adam's launch -- sgn_adam_rows: the
             previous step's deferred update, this step's rows brought forward, their distinct
             list -- and the step's blobs), the gradients made ready, `run` (forward + backward)
  epilogue   bucketed all-reduce (RCCL) of the flat MLP gradient and, under DP, a sparse all-gather
             of the touched point rows

Two arithmetic modes, as the renderer has: precision "f32" (the reference's fp32 arithmetic,
train_f32.F32Runner / F32Step: no host synchronisation on one GPU) and "f16" (fp16-operand MFMA,
fp32 accumulation, train_f16.F16Step: one host sync per step, the loss stage as a captured graph).

`apply` steps the two Adam groups (lr 5e-4 / plr 2e-3, iter_exponential_decay): the MLP's on
sgn_adam_step_multi, the points' on the row-sparse exact sgn_adam_rows (PointAdam(rows=True):
bit-identical to the dense update, applied at the next step's launch or at a flush).  The plane
background model's per-ray colour (inputs['bg_ray']) enters the loss stage as T_bg * bg_ray.  Depth
supervision (`depth=`, a train.DepthTarget) switches the loss stage to sgn_loss_train_depth on every path;
without it the stock entry runs as before.  The objective follows opts.color_loss_items / color_loss_weights,
zero_one_loss_items / zero_one_loss_weights, zero_epsilon and sparse_loss_weight (base_rendering_model.py:534-664):
anything but the ScanNet colour weights without a sparse loss runs sgn_loss_train_opts.

Which point tensors train follows opts.feat_grad / color_grad / dir_grad / conf_grad (neural_points.py:410-416):
a frozen tensor's gradient pointer is NULL at the C ABI (no kernel computes it), it is in no point-Adam group
and the data-parallel row exchange does not carry it.

The viewmlp without block3 (shading_feature_mlp_layer3 = 0) trains with opts.train_rows = 1 at precision "f32"
(train_f32.F32RunnerNb3 / F32StepNb3): the points' colour and dir are outside that network's graph,
so they may be missing (None) and are treated as frozen tensors whatever their switches say.
"""
from types import SimpleNamespace

import torch
import torch.distributed as dist

from . import _lib
from .flat_mlp import FlatMLP, _Packer, _PackerF32  # noqa: F401  (re-exported)
from .opts import HotPathOpts
from .point_adam import NoPointAdam, PointAdam
from .train import PointParams, _allreduce_buckets, _allreduce_point_rows, depth_target
from .weights import layers_for


POINT_TENSORS = ("points_embeding", "points_color", "points_dir", "points_conf")


class _Watch:
    """A device word (int64 [1]) on its way to pinned host memory without a sync: `post` queues the asynchronous
    copy, `check` reads a copy that has landed (wait: any pending one) and raises RuntimeError(message, formatted
    with n = the word) when it is not 0.  `post` first looks at the previous copy without waiting and then reuses the
    one pinned word, so a word whose copy has not landed by the next `post` is replaced unread.  accumulate: the
    posted words are first folded (max) into a running device word, which is what travels, so a non-zero word is
    still in every later copy until a `check` has raised it (the running word is cleared then)."""

    def __init__(self, device, message, accumulate=False):
        cuda = device.type == "cuda"
        self.message = message
        self._host = torch.zeros(1, dtype=torch.int64, pin_memory=cuda)
        self._event = torch.cuda.Event() if cuda else None
        self._pending = False
        self._acc = torch.zeros(1, dtype=torch.int64, device=device) if accumulate else None

    def post(self, word):
        self.check()
        word = word.reshape(1)
        if self._acc is not None:
            torch.maximum(self._acc, word, out=self._acc)
            word = self._acc
        self._host.copy_(word, non_blocking=True)
        self._event.record()
        self._pending = True

    def check(self, wait=False):
        if not self._pending:
            return
        if not self._event.query():   # the copy has not landed yet
            if not wait:
                return
            self._event.synchronize()
        self._pending = False
        n = int(self._host[0])
        if n:
            if self._acc is not None:
                self._acc.zero_()
            raise RuntimeError(self.message.format(n=n))


class HipTrainer:
    """One data-parallel training step per call on the HIP path (config 5)."""

    def __init__(self, points: PointParams, mlp_state, opts: HotPathOpts, device, lr=5e-4, plr=2e-3,
                 lr_decay_exp=0.1, lr_decay_iters=1_000_000, bucket_mb=64, querier=None, bpnet=None,
                 precision="f16"):
        """bpnet: the SG variant's BPNet point embedding [N, 96] (fp32, detached: it is an input,
        neural_points.py:662), needed when opts select block2_bpnet with predict_semantic = 1.
        precision "f16": the fp16-operand HIP forward + backward (k_agg_rows save mode, k_agg_bwd);
        "f32" (base viewmlp and SG): the reference's fp32 arithmetic -- the HIP fp32-faithful row
        kernel (k_rows16, 3 fp16 MFMA products per fp32 product) saves the row MLP's pre-activations
        and the backward runs through them on the same split-fp16 GEMMs (train_f32.F32Step)."""
        self.device = torch.device(device)
        self.opts = opts.check_supported()
        if not opts.block3_layers and not opts.train_rows:
            raise NotImplementedError("shading_feature_mlp_layer3 = 0 renders only: training this network is not "
                                      "implemented (it runs on the plain-fp32 kernels, which have no backward)")
        self.nb3 = not opts.block3_layers   # the viewmlp without block3 on the fp32 row-GEMM step (train_rows = 1)
        if self.nb3 and precision != "f32":
            raise NotImplementedError("train_rows = 1 trains the viewmlp without block3 with the fp32 step only: "
                                      f"precision must be 'f32', not {precision!r}")
        self.variant = tuple(opts.bpnet_variant)
        self.sg = self.variant != (0, 0)
        if precision not in ("f16", "f32"):
            raise ValueError("precision: 'f16' or 'f32'")
        self.precision = precision
        self.points = points
        self.mlp = FlatMLP(mlp_state, self.device, layers_for(*self.variant, block3_layers=opts.block3_layers))
        self.bpnet16 = self.bpnet32 = None
        if self.variant[1]:
            if bpnet is None:
                raise ValueError("block2_bpnet with predict_semantic = 1 needs the BPNet point embedding")
            e = torch.as_tensor(bpnet).detach().to(self.device, torch.float32).reshape(-1, self.variant[1]).contiguous()
            self.bpnet16 = torch.empty(e.shape, dtype=torch.float16, device=self.device)
            _lib.check(_lib.lib().sgn_bpnet_pack(_lib.ptr(e), e.shape[0], e.shape[1], _lib.ptr(self.bpnet16),
                                                 _lib.stream_handle()), "sgn_bpnet_pack")
            if precision == "f32":   # the fp32 kernels read the embedding as it is
                self.bpnet32 = e
        # opt.feat_grad / color_grad / dir_grad / conf_grad (neural_points.py:410-416): a frozen tensor takes
        # no gradient (its kernels' outputs are NULL), has no Adam moments and never changes;
        # point_params are the trained ones, in the point group's order
        # (without block3 colour and dir may be missing -- None -- and are never trained: opts.trained_points)
        every = {k: getattr(points, k) for k in POINT_TENSORS if getattr(points, k) is not None}
        self.trained = self.opts.trained_points
        for k, p in every.items():
            p.requires_grad_(k in self.trained)
            if k not in self.trained:
                p.grad = None
        self.point_params = [every[k] for k in self.trained]
        # the reference's two Adam groups (mvs_points_volumetric_model.py:100-108); fused: one
        # kernel per group (sgn_adam_step, which also clears the gradient for the next step) instead
        # of the foreach chain; the MLP group's flat 0.35 M elements the same way
        cuda = self.device.type == "cuda"
        if cuda:
            self.opt_net = PointAdam([self.mlp.flat], lr=lr, betas=(0.9, 0.999))
            # row-sparse exact mode: a step updates the ~50 k rows it touches (each first replaying the
            # zero-gradient steps it missed) instead of streaming all 47 M elements; flushed before
            # anything else reads the points (sync_points)
            # (row 0 is brought forward with every step only while conf trains: empty slots read its conf)
            self.opt_pts = (PointAdam(self.point_params, lr=plr, betas=(0.9, 0.999), rows=True, names=self.trained,
                                      row0="points_conf" in self.trained)
                            if self.point_params else NoPointAdam(plr))
        else:   # the reference's way: every tensor listed, the frozen ones without a gradient
            self.opt_net = torch.optim.Adam([self.mlp.flat], lr=lr, betas=(0.9, 0.999))
            self.opt_pts = torch.optim.Adam(list(every.values()), lr=plr, betas=(0.9, 0.999))
        self._grads_clean = False  # the optimizers left every gradient zeroed
        self.base_lr = (lr, plr)
        self.decay = (lr_decay_exp, lr_decay_iters)
        self.step_count = 0
        self.bucket_elems = bucket_mb * (1 << 20) // 4
        self.querier = querier
        self._last_q = None
        # (without block3 there is neither MFMA blob: the packer writes the shifts alone)
        self.packer = None if self.nb3 else _Packer(self.device, self.variant)
        # the fp32-faithful blob (f32 step) and, for both precisions, the per-layer weight shifts the
        # split-fp16 GEMMs of the colour MLP read
        self.packer32 = _PackerF32(self.device, self.mlp, self.variant, shifts_only=self.nb3)
        # the OOB watch: the out-of-range neighbour count of a step, on its way to pinned host memory
        self._oob = _Watch(self.device, "training step: {n} neighbour indices >= n_points (query and point tables "
                                        "disagree)")
        # without a row-sparse Adam launch the OOB count comes from sgn_touched_points' stamp table
        self._stamp = self._tlist = self._tcount = None
        self._stamp_n, self._tstep = -1, 0
        # f16: the loss stage replays as a captured HIP graph; False runs the same stage eagerly (torch
        # autograd of the colour MLP into the HIP loss stage), the graph's parity reference in the tests
        self.use_graph = True
        if self.nb3:
            from .train_f32 import F32RunnerNb3
            # the fp16-range watch: a step whose row forward left fp16 range is reported at the next step whose
            # `begin` finds the copy landed (or in check_touched()); the flags are folded into a running device
            # word, so one whose copy was replaced before it was read is reported with the following step's
            self._range_watch = _Watch(self.device, "training step (train_rows): the row MLP's forward left fp16 range "
                                                    "(|activation| >= 65504 or not finite): the split-fp16 row GEMMs "
                                                    "cannot carry these weights, the step's gradients are not to be "
                                                    "trusted", accumulate=True)
            self.stepper = F32RunnerNb3(self)
        elif precision == "f32":
            from .train_f32 import F32Runner
            self.stepper = F32Runner(self)
        else:
            from .train_f16 import F16Step
            self.stepper = F16Step(self)

    @property
    def graph_captures(self):
        """Loss-stage graph captures so far (f16; 0 at f32)."""
        return self.stepper.graph_captures

    def _query(self, campos, raydir, near, far, labels=None):
        if self.querier is None:
            from .querier import LightningFastQuerier
            self.querier = LightningFastQuerier(self.device, self.opts)
        if self.opts.semantic_guidance:
            if labels is None:
                raise ValueError("semantic_guidance = 1: pass labels=(point_labels [N], ray_labels [R], seconds)")
            pl, rl, sec = labels
            return self.querier.query_samples(self.points.xyz, campos, raydir, near, far,
                                              torch.as_tensor(pl).to(self.device, torch.int32).reshape(-1).contiguous(),
                                              torch.as_tensor(rl).to(self.device, torch.int32).reshape(-1).contiguous(),
                                              sec)
        return self.querier.query_samples(self.points.xyz, campos, raydir, near, far)

    def _tables(self, campos, rot, raydir):
        pt = _lib.PointTables()
        P = self.points
        addr = lambda t: None if t is None else t.data_ptr()  # noqa: E731  (NULL: no colour / dir, without block3)
        pt.xyz, pt.embedding, pt.color = P.xyz.data_ptr(), P.points_embeding.data_ptr(), addr(P.points_color)
        pt.dir, pt.conf, pt.n_points = addr(P.points_dir), P.points_conf.data_ptr(), P.xyz.shape[0]
        pt.campos, pt.camrotc2w, pt.raydir = campos.data_ptr(), rot.data_ptr(), raydir.data_ptr()
        return pt

    # -- the OOB watch ----------------------------------------------------------------------
    def _watch_oob(self, count):
        """The out-of-range neighbour count (a device int64) goes to pinned host memory without a sync;
        the next step (or check_touched()) reads it once the copy has landed and fails loudly on a
        query / point table mismatch (those points would never be projected or updated)."""
        self._oob.post(count)

    def _check_oob(self, wait=False):
        """Raise if an earlier step's query named a point index >= n_points (sgn_touched_points'
        counter d_count2[2]); without wait only a copy that has already landed is read."""
        self._oob.check(wait)

    def check_touched(self):
        """Wait for and check the last step's out-of-range neighbour counter (see _check_oob) and, without
        block3, its fp16-range word."""
        self._check_oob(wait=True)
        if self.nb3:
            self._range_watch.check(wait=True)

    def touched_points(self, q):
        """The step's touched points (sgn_touched_points: an int32 list in no particular order and its
        device count) where no row-sparse Adam launch lists them -- the dense Adam, or every point tensor
        frozen; no host sync, one launch.  Its out-of-range count goes to the OOB watch."""
        dev, npts = self.device, self.points.xyz.shape[0]
        if self._stamp_n != npts:
            self._stamp = torch.full((npts,), -1, dtype=torch.int32, device=dev)
            self._tlist = torch.empty(npts, dtype=torch.int32, device=dev)
            self._tcount = torch.zeros(3, dtype=torch.int64, device=dev)   # [2]: out-of-range ids met
            self._stamp_n, self._tstep = npts, 0
        step = self._tstep
        self._tstep = (step + 1) & 0x7fffffff
        if self._tstep == 0:   # the stamp table outlived 2^31 steps: start it again
            self._stamp_n = -1
        K = self.opts.K
        self._check_oob()
        _lib.check(_lib.lib().sgn_touched_points(_lib.ptr(q.pidx), _lib.ptr(q.counters), q.pidx.numel() // K, K, npts,
                                                 step, _lib.ptr(self._stamp), _lib.ptr(self._tlist),
                                                 _lib.ptr(self._tcount), _lib.stream_handle()), "sgn_touched_points")
        self._watch_oob(self._tcount[2:3])
        return self._tlist, self._tcount[step & 1]

    def point_grads(self):
        """The point gradients as the kernels take them (sgn_point_grads): NULL for a frozen or missing tensor."""
        g = [getattr(getattr(self.points, k), "grad", None) for k in POINT_TENSORS]
        return _lib.PointGrads(*[None if t is None else t.data_ptr() for t in g])

    # -- row-sparse point Adam --------------------------------------------------------------
    def _rows_adam(self):
        return isinstance(self.opt_pts, PointAdam) and self.opt_pts.rows_mode

    def _adam_rows(self, rows, count, count_is64, count_mul):
        """The step's point rows (a device list and count) to the row-sparse Adam: the deferred previous
        step applied and these rows brought to the current step before the forward reads them.  Returns
        the step's distinct rows (int32 list, int64 device count) or None (dense Adam); a list id >=
        n_points is reported at the next step (_watch_oob)."""
        if not self._rows_adam():
            return None
        pb = self.opt_pts.set_rows(rows, count, count_is64, count_mul)
        self._watch_oob(pb[8:16].view(torch.int64))
        return pb[16:].view(torch.int32), pb[:8].view(torch.int64)

    def _adam_union(self, all_idx):
        """Under DP the exchanged gradient covers every rank's rows: the update takes all of them."""
        if all_idx is not None and self._rows_adam():
            self.opt_pts.set_update_rows(all_idx.to(torch.int32))

    def sync_points(self):
        """Bring every point row to the optimizer's current step (the row-sparse Adam updates a row
        when a step touches it): call before reading the point tensors outside a step."""
        if isinstance(self.opt_pts, PointAdam):
            self.opt_pts.flush()

    # -- one step ------------------------------------------------------------------------
    def _bg_ray(self, bg_ray, R):
        """inputs['bg_ray'] (the plane background model's per-ray colour, [1, R, 3]) as a contiguous
        device [R, 3] fp32 tensor, or None (the constant white background)."""
        if bg_ray is None:
            return None
        bg_ray = torch.as_tensor(bg_ray).to(self.device, torch.float32).reshape(-1, 3).contiguous()
        if bg_ray.shape[0] != R:
            raise ValueError(f"bg_ray has {bg_ray.shape[0]} rays, the batch {R}")
        return bg_ray

    def backward(self, campos, rot, raydir, near, far, gt, labels=None, bg_ray=None, depth=None):
        """Forward + backward + gradient all-reduce (no parameter update).  labels: (point_labels,
        ray_labels, seconds) for the semantic-guided query (semantic_guidance = 1).  bg_ray: the
        rays' background [1, R, 3] of the plane background model (inputs['bg_ray']): the composite
        and its gradient use T_bg * bg_ray per ray (neural_points_volumetric_model.py:175-177).
        depth: a train.DepthTarget (depth_loss_items = coarse_depth): the loss stage runs sgn_loss_train_depth,
        parts carry coarse_depth and its weighted term is in total.
        Returns (loss parts, rendered colour [R,3], ray_mask [R]) and, with depth, the depth map [R]."""
        dev = self.device
        campos = campos.reshape(3).to(dev, torch.float32).contiguous()
        rot = rot.reshape(3, 3).to(dev, torch.float32).contiguous()
        raydir = raydir.reshape(-1, 3).to(dev, torch.float32).contiguous()
        gt = gt.reshape(-1, 3).to(dev, torch.float32).contiguous()
        R = raydir.shape[0]
        bg_ray = self._bg_ray(bg_ray, R)
        q = self._last_q = self._query(campos, raydir, near, far, labels)
        dp = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
        if depth is not None:
            depth = depth_target(depth.gt, depth.mask, depth.weight, R, dev)
        b = SimpleNamespace(campos=campos, rot=rot, raydir=raydir, gt=gt, R=R, bg_ray=bg_ray, q=q, dp=dp, depth=depth,
                            depth_map=None)
        step = self.stepper
        step.begin(b)
        # the gradients are made ready after the point Adam's launch: it applies a deferred step, which
        # reads that step's gradient
        for p in self.point_params + [self.mlp.flat]:
            if p.grad is None:
                p.grad = torch.zeros_like(p)
            elif not self._grads_clean:
                p.grad.zero_()
        self._grads_clean = False
        parts, full, ray_mask = step.run(b)
        self.allreduce_grads([self.mlp.flat])
        if dp and self.point_params:   # the sparse row exchange carries the trained tensors only
            self._adam_union(_allreduce_point_rows([p.grad for p in self.point_params], *step.dp_rows()))
        if depth is not None:
            return parts, full, ray_mask.bool(), b.depth_map
        return parts, full, ray_mask.bool()

    @property
    def last_query(self):
        """The last step's sample-major query as a dict (ray_ns, ray_soff, samp_ray, samp_locw,
        pidx): tests rerun fp32 autograd on the very samples the step used.  Reads S (host sync)."""
        q, o = self._last_q, self.opts
        R, S = q.R, int(q.counters[0].item())
        return {"ray_ns": q.ray_ns[:R], "ray_soff": q.ray_soff[:R], "samp_ray": q.samp_ray[:S],
                "samp_locw": q.samp_locw[:S * 3].view(S, 3), "pidx": q.pidx[:S * o.K].view(S, o.K)}

    def allreduce_grads(self, params):
        _allreduce_buckets([p.grad for p in params if p.grad is not None], self.bucket_elems)

    def _set_lr(self):
        exp, iters = self.decay
        f = exp ** (self.step_count / iters)  # iter_exponential_decay
        for opt, base in ((self.opt_net, self.base_lr[0]), (self.opt_pts, self.base_lr[1])):
            for gr in opt.param_groups:
                gr["lr"] = base * f

    def apply(self):
        self._set_lr()
        self.opt_net.step()
        self.opt_pts.step()
        self._grads_clean = all(isinstance(o, (PointAdam, NoPointAdam)) and o.zero_grad_in_step
                                for o in (self.opt_net, self.opt_pts))
        self.step_count += 1

    def step(self, campos, rot, raydir, near, far, gt, labels=None, bg_ray=None, depth=None):
        out = self.backward(campos, rot, raydir, near, far, gt, labels, bg_ray, depth)
        self.apply()
        return out

    def mlp_state(self):
        return self.mlp.state()


def grads_named(trainer: HipTrainer):
    """Gradients under the reference names (for parity tests): MLP layers + point params."""
    m = trainer.mlp
    g = m.flat.grad
    out = {}
    for name, *_ in m.layers:
        out[name + ".weight"] = m.w(name, g).detach().clone()
        out[name + ".bias"] = m.b(name, g).detach().clone()
    P = trainer.points
    for k in POINT_TENSORS:   # a frozen (or missing) tensor has none
        g = getattr(getattr(P, k), "grad", None)
        out[k] = None if g is None else g.detach().clone()
    return out
