"""The fp32 training step on hand-written kernels (precision "f32").

The reference's step (`optimize_parameters`, models/base_rendering_model.py:534-664;
models/mvs_points_volumetric_model.py:47-141) runs the aggregator, colour MLP, ray march and
losses forward in fp32 and differentiates them with torch autograd.  `F32Step` runs the same
arithmetic as a fixed sequence of HIP launches (csrc/train_x3.hip, csrc/mlp_x3.hip, csrc/loss.hip)
with every count kept on the device -- no host synchronisation, so the whole step can be replayed
as one captured graph:

  sgn_train_lists            deterministic work list + compact row offsets (prefix sums)
  sgn_aggregate_train_fwd_f32  k_pair_slots + k_rows16 (save mode): alpha_s, f_s, z1 / z2 / z3 rows
                             (SG: + block2_bpnet.0's zb)
  sgn_train_row_inputs       x0 = [emb | PE(emb) | PE(dists) | 1], extra channels, blend weights,
                             PE(viewdir); SG: sgn_train_row_gather, the rows' BPNet embedding
  colour forward             3 x sgn_x3_gemm (x W^T + b, LeakyReLU) + sgn_train_colour_head (rgb)
  sgn_loss_train             ray_dist + ray_march + losses and d feat, d conf (zero-one); loss_hip.loss_train's entry
  colour backward            sgn_train_colour_head_bwd, 3 x dy W (masked), 3 x dy^T x (split-K)
  row backward               z4 = LReLU(z3) W3^T + b3; sgn_train_row_head (alpha, K-blend, delta4,
                             d conf); 4 x delta W (masked; SG 5); sgn_train_row_tail (d emb /
                             colour / dir); 4 x delta^T x (split-K; SG 5)
  sgn_reduce_partials        every weight / bias gradient into the flat gradient, fixed order

Rows r are the valid (sample, neighbour) pairs, sample-major (sample s owns rows
row_off[s] .. row_off[s] + samp_nnb[s]); items are the samples with a neighbour, ascending.

`ColourStage` is the colour forward, the losses and the colour backward of that sequence; the f16
step's captured graph (train_f16.F16Step) runs the same stage on its own items.  `F32Runner` is what
train_hip.HipTrainer drives: it keeps the F32Step of the current batch capacity, the projection
buffer and the step's touched-point list.

`F32StepNb3` / `F32RunnerNb3` are the step of the viewmlp without block3 (shading_feature_mlp_layer3 = 0,
opts.train_rows = 1): the row MLP's forward runs on the rows-mode GEMMs the renderer's rows_gemm path uses
(`row_forward_gemms`, shared with rows_gemm.RowsGemmNb3), the head, the backward chain and the weight
gradients on the launches above with block3 left out.
"""
import ctypes
import os

import torch

from . import _lib, loss_hip
from .train import gather_counts, touched_rows
from .weights import BPNET

# split-K partials of the weight-gradient GEMMs (rows / items cut into this many 32-aligned runs;
# 84 x 3 column blocks = one workgroup per CU for the row layers).  SGN_SPLITS_ROWS / _ITEMS
# override them for sweeps (tools/splits_sweep.sh).
SPLITS_ROWS = int(os.environ.get("SGN_SPLITS_ROWS", "84"))
SPLITS_ITEMS = int(os.environ.get("SGN_SPLITS_ITEMS", "128"))


def _addr(t, elem_off=0):
    return t.data_ptr() + elem_off * t.element_size()


def _operand(p, ld, ncols, kmajor, p2=None, ld2=0, csplit=None, ones_col=-1, act=0, amax=None, shift=None):
    o = _lib.X3Operand()
    o.p, o.p2 = p, p2
    o.ld, o.ld2 = int(ld), int(ld2)
    o.csplit = int(ncols if csplit is None else csplit)
    o.ncols, o.ones_col, o.act, o.kmajor = int(ncols), int(ones_col), int(act), int(kmajor)
    o.amax, o.shift = amax, shift
    return o


def _rows_gemm(a, b, M, N, K, rows, out, ldo, bias=None, act=0, mask=None, ldm=0, out_cols=None, out2=None, ldo2=0,
               amax_out=None, amax_out2=None):
    g = _lib.X3GemmArgs()
    g.a, g.b = a, b
    g.mode, g.M, g.N, g.K = 0, int(M), int(N), int(K)
    g.d_rows, g.bias, g.act, g.mask, g.ldm = rows, bias, int(act), mask, int(ldm)
    g.out, g.ldo = out, int(ldo)
    g.out_cols = int(N if out_cols is None else out_cols)
    g.out2, g.ldo2, g.amax_out, g.amax_out2 = out2, int(ldo2), amax_out, amax_out2
    return g


def _splitk_gemm(a, b, M, N, K, rows, part, splits):
    g = _lib.X3GemmArgs()
    g.a, g.b = a, b
    g.mode, g.M, g.N, g.K = 1, int(M), int(N), int(K)
    g.d_rows, g.part, g.splits = rows, part, int(splits)
    g.out_cols = int(N)
    return g


def _attach_bpack(gemms, device):
    """One workspace for the rows-mode launches' weight images (sgn_x3_gemm's bpack: the weight blocks are
    split once per call by a small launch, then DMA'd into every workgroup's LDS).  The launches run in
    stream order, so they share it.  Returns the buffer (keep it alive with the arguments)."""
    L = _lib.lib()
    rows = [g for g in gemms if g.mode == 0]
    n = max([int(L.sgn_x3_gemm_bpack_bytes(ctypes.byref(g))) for g in rows] + [16])
    buf = torch.empty(n, dtype=torch.uint8, device=device)
    for g in rows:
        g.bpack = buf.data_ptr()
    return buf


X0_LD = 288                      # block1.0's input row (284 inputs, the ones column, padding)
GEMM_BYTES_LIMIT = 0x7fffffff    # sgn_x3_gemm mode 0: 32-bit buffer offsets, every operand below 2 GiB
FP16_RANGE_BITS = 0x477FE000     # 65504.0f: an amax word at or above it has left fp16 range


def row_forward_gemms(W, B, S, variant, rows, n_rows, x0, z1, z2, zb, bprows, amax):
    """The rows-mode forward launches of the row MLP without block3 over compact rows, for the renderer's windows
    (rows_gemm.RowsGemmNb3) and the training step (F32StepNb3) alike:
        z1 = x0 W10^T + b10;  z2 = LReLU(z1) W12^T + b12;  block2_bpnet.0: zb = LReLU(z2) Wb[:, :256]^T + bb
    and, with the BPNet columns, the sgn_x3_gemm_accumulate launch zb += bprows Wb[:, 256:]^T.
    W / B / S: name -> (weight address, out, in) / bias address / shift address; rows: the buffers' row capacity,
    n_rows: the address of the device row count; x0 [rows, 288], z1, z2, zb [rows, 256], bprows [rows, dim]:
    addresses (zb / bprows unused without their layer); amax: the addresses of z1's, z2's and zb's amax words.
    Returns (the two or three launches in order, the accumulate launch or None)."""
    a_z1, a_z2, a_zb = amax
    w10, o, i = W("block1.0")
    G = [_rows_gemm(_operand(x0, X0_LD, X0_LD, 0), _operand(w10, i, i, 0, shift=S("block1.0")), rows, o, i, n_rows,
                    z1, 256, bias=B("block1.0"), amax_out=a_z1)]
    w12, o, i = W("block1.2")
    G.append(_rows_gemm(_operand(z1, 256, 256, 0, act=1), _operand(w12, i, i, 0, shift=S("block1.2")), rows, o, i,
                        n_rows, z2, 256, bias=B("block1.2"), amax_out=a_z2))
    acc = None
    if variant[0]:
        wb, o, i = W(BPNET)
        G.append(_rows_gemm(_operand(z2, 256, 256, 0, act=1), _operand(wb, i, 256, 0, shift=S(BPNET)), rows, o, 256,
                            n_rows, zb, 256, bias=B(BPNET), amax_out=a_zb))
        if variant[1]:
            d = variant[1]
            acc = _rows_gemm(_operand(bprows, d, d, 0), _operand(wb + 256 * 4, i, d, 0, shift=S(BPNET)),
                             rows, o, d, n_rows, zb, 256, amax_out=a_zb)
    return G, acc


class _FlatAddr:
    """Device addresses inside a trainer's flat parameter, its gradient and the per-layer weight shifts."""

    def __init__(self, trainer):
        m = self.mlp = trainer.mlp
        self.flat, self.grad, self.shift = m.flat, m.flat.grad, trainer.packer32.shift
        self.layer_ix = {name: i for i, (name, *_) in enumerate(m.layers)}

    def W(self, name):
        off, o, i = self.mlp.slices[name]
        return _addr(self.flat, off), o, i

    def B(self, name):
        off, o, i = self.mlp.slices[name]
        return _addr(self.flat, off + o * i)

    def S(self, name):
        return _addr(self.shift, self.layer_ix[name])

    def segment(self, part, splits, M, N, name, n_in, bias_col):
        """A layer's split-K partials [splits, M, N] (its bias gradient in column bias_col) -> flat gradient."""
        off, o_, i_ = self.mlp.slices[name]
        s = _lib.PartialSegment()
        s.part, s.splits, s.M, s.N, s.n_in, s.bias_col, s.ldw = part, splits, M, N, n_in, bias_col, i_
        s.dst_w, s.dst_b = _addr(self.grad, off), _addr(self.grad, off + o_ * i_)
        return s


class ColourStage:
    """The colour MLP, the losses and the colour backward of one batch capacity on sgn_x3_gemm, for both
    precisions (precision "f16" only changes the row MLP).  Items are the samples with a neighbour, `cap`
    of them at most, their device count at `n_items`.

      forward_and_loss   3 x sgn_x3_gemm forward (3 fp16 products per fp32 product) + sgn_train_colour_head
                         (rgb into feat[.].yzw), sgn_loss_train (d feat; the zero-one gradients into
                         points_conf.grad)
      backward           sgn_train_colour_head_bwd, 2 masked dy W, d f_s = dy1 W0[:, :256], the three weight
                         gradients as split-K partials

    The owner reduces `segments` (its own after them) into the flat gradient with one sgn_reduce_partials,
    attaches one bpack workspace to `gemms` and its own, and clears the amax tensor once per step."""

    # amax words (max |x| of a delta tensor, written by its producer, read by its consumers): the first
    # three of the owner's amax tensor
    A_DY3, A_DY2, A_DY1 = range(3)

    def __init__(self, trainer, qo, R, cap, n_items, fs, vpe, feat, dfeat, amax, products=3, zero_dfs=False):
        """n_items: the address of the device item count (int32).  fs [cap, 256] fp32: the items' blended
        features; vpe [cap, 32]: PE(viewdir) | 1 | 0 (None: allocated here, zeroed); feat [S, 4]: the
        per-sample features the colour goes into; dfeat: their gradient.  products: of the backward GEMMs,
        1 (the f16 step's delta precision: one fp16 product per multiply-add) or 3 (split-fp16 at fp32
        accuracy); the forward keeps 3, so the rendered colour and the losses are the fp32 colour MLP's.
        zero_dfs: clear d f_s before the backward writes the counted items' rows (padding items then
        read as 0)."""
        L = _lib.lib()
        dev = trainer.device
        f32 = dict(dtype=torch.float32, device=dev)
        self.points, self.qo, self.R = trainer.points, qo, R
        self.n_items = ctypes.c_void_p(n_items)
        self.fs, self.feat, self.dfeat, self.amax, self.zero_dfs = fs, feat, dfeat, amax, zero_dfs
        self.vpe = torch.zeros(cap, 32, **f32) if vpe is None else vpe
        self.h = [torch.empty(cap, 128, **f32) for _ in range(3)]       # colour h1, h2, h3
        self.dy = [torch.empty(cap, 128, **f32) for _ in range(3)]      # colour dy1, dy2, dy3
        self.dfs = torch.empty(cap, 256, **f32)
        # the loss stage's options (None: the ScanNet objective on the stock entries) and its loss vector
        o = self.opts = trainer.opts
        self.lo = loss_hip.loss_opts(o, trainer.points)
        self.losses = torch.zeros(loss_hip.loss_len(self.lo), **f32)
        self.full = torch.empty(max(R, 1), 3, **f32)
        self.mask = torch.empty(max(R, 1), dtype=torch.int8, device=dev)
        # sized for the depth-supervised stage too (R floats and a few partial sums more)
        self.loss_ws = torch.empty(loss_hip.workspace_bytes(R, o.SR, o.K, self.lo is None, True), dtype=torch.uint8,
                                   device=dev)
        self.depth = None   # [R] the depth map, allocated by the first depth-supervised step
        self.part_col = [torch.empty(SPLITS_ITEMS, 128, n, **f32) for n in (129, 129, 281)]
        self.part_c6 = torch.empty(int(L.sgn_train_head_partial_floats(0)), **f32)
        # ---- the launch arguments (pointers of persistent buffers: built once) ------------------
        A = _FlatAddr(trainer)
        W, S = A.W, A.S
        am = [_addr(amax, i) for i in range(3)]
        h1, h2, h3 = (_addr(t) for t in self.h)
        dy1, dy2, dy3 = (_addr(t) for t in self.dy)
        fsa, vpa = _addr(fs), _addr(self.vpe)
        # colour forward: h = LReLU(x W^T + b)
        w, o_, i_ = W("color_branch.0")
        G = [_rows_gemm(_operand(fsa, 256, 280, 0, p2=vpa, ld2=32, csplit=256),
                        _operand(w, i_, i_, 0, shift=S("color_branch.0")), cap, o_, i_, n_items, h1, 128,
                        bias=A.B("color_branch.0"), act=1)]
        for name, x, y in (("color_branch.2", h1, h2), ("color_branch.4", h2, h3)):
            w, o_, i_ = W(name)
            G.append(_rows_gemm(_operand(x, 128, 128, 0), _operand(w, i_, i_, 0, shift=S(name)), cap, o_, i_, n_items,
                                y, 128, bias=A.B(name), act=1))
        self.g_fwd = G
        # colour backward: dy_prev = (dy W) * LReLU'(h_prev); d f_s = dy1 W0[:, :256]
        G = []
        for name, dyi, mk, dyo, ai, ao in (("color_branch.4", dy3, h2, dy2, self.A_DY3, self.A_DY2),
                                           ("color_branch.2", dy2, h1, dy1, self.A_DY2, self.A_DY1)):
            w, o_, i_ = W(name)
            G.append(_rows_gemm(_operand(dyi, 128, 128, 0, amax=am[ai]), _operand(w, i_, i_, 1, shift=S(name)),
                                cap, i_, o_, n_items, dyo, 128, mask=mk, ldm=128, amax_out=am[ao]))
        w, o_, i_ = W("color_branch.0")
        G.append(_rows_gemm(_operand(dy1, 128, 128, 0, amax=am[self.A_DY1]),
                            _operand(w, i_, 256, 1, shift=S("color_branch.0")), cap, 256, o_, n_items,
                            _addr(self.dfs), 256))
        # colour weight gradients (split-K over the items)
        pc = [_addr(t) for t in self.part_col]
        G.append(_splitk_gemm(_operand(dy3, 128, 128, 1, amax=am[self.A_DY3]), _operand(h2, 128, 128, 1, ones_col=128),
                              128, 129, cap, n_items, pc[0], SPLITS_ITEMS))
        G.append(_splitk_gemm(_operand(dy2, 128, 128, 1, amax=am[self.A_DY2]), _operand(h1, 128, 128, 1, ones_col=128),
                              128, 129, cap, n_items, pc[1], SPLITS_ITEMS))
        G.append(_splitk_gemm(_operand(dy1, 128, 128, 1, amax=am[self.A_DY1]),
                              _operand(fsa, 256, 281, 1, p2=vpa, ld2=32, csplit=256), 128, 281, cap, n_items, pc[2],
                              SPLITS_ITEMS))
        for gs in G:
            gs.products = products
        self.g_bwd = G
        self.gemms = self.g_fwd + self.g_bwd
        self.segments = [A.segment(pc[0], SPLITS_ITEMS, 128, 129, "color_branch.4", 128, 128),
                         A.segment(pc[1], SPLITS_ITEMS, 128, 129, "color_branch.2", 128, 128),
                         A.segment(pc[2], SPLITS_ITEMS, 128, 281, "color_branch.0", 280, 280),
                         A.segment(_addr(self.part_c6), self.part_c6.numel() // (3 * 129), 3, 129, "color_branch.6",
                                   128, 128)]
        self.w6, self.b6 = W("color_branch.6")[0], A.B("color_branch.6")

    def forward_and_loss(self, campos, rot, gt, bg_ray, st, depth=None):
        """Colour forward into feat[.].yzw, then the losses (loss_hip.loss_train: the entry the loss options
        and depth select), on stream st: the loss vector, full [R, 3] and mask [R] (int8) land in self.losses /
        full / mask, d feat in self.dfeat.  bg_ray: the rays' background [R, 3] or None (white).  depth (a
        train.DepthTarget): L_depth in losses[7], the depth map in self.depth, d feat with the depth term."""
        L = _lib.lib()
        ck, p = _lib.check, _lib.ptr
        P = self.points
        for gs in self.g_fwd:
            ck(L.sgn_x3_gemm(ctypes.byref(gs), st), "sgn_x3_gemm")
        ck(L.sgn_train_colour_head(ctypes.byref(self.qo), self.n_items, p(self.h[2]), self.w6, self.b6, p(self.feat),
                                   st), "sgn_train_colour_head")
        if depth is not None and self.depth is None:
            self.depth = torch.empty(max(self.R, 1), dtype=torch.float32, device=self.full.device)
        loss_hip.loss_train(loss_hip.loss_params(self.opts, bg_ray=bg_ray), self.lo,
                            loss_hip.loss_depth(depth, self.depth), p(campos), p(rot), self.R, ctypes.byref(self.qo), p(self.feat), p(gt), p(P.points_conf),
                            p(self.full), p(self.mask), p(self.losses), p(self.dfeat), p(P.points_conf.grad),
                            p(self.loss_ws), self.loss_ws.numel(), st)

    def results_out(self, scalars, depth):
        """The next step reuses the stage's buffers: scalars (the loss vector, or what was made of it), colour, mask
        and, with depth, the depth map out into one fresh allocation by one sgn_copy_segments launch, returned."""
        R = self.R
        ns = scalars.numel()
        o_full = 8 * (-(-ns // 8))
        nm = -(-R // 4)
        buf = torch.empty(o_full + 3 * R + nm + (R if depth else 0), dtype=torch.float32, device=scalars.device)
        sc, full = buf[:ns], buf[o_full:o_full + 3 * R].view(R, 3)
        mask = buf[o_full + 3 * R:o_full + 3 * R + nm].view(torch.int8)[:R]
        dmap = buf[o_full + 3 * R + nm:] if depth else None
        _lib.copy_segments([(scalars, sc), (self.full[:R], full), (self.mask[:R], mask)] +
                           ([(self.depth[:R], dmap)] if depth else []))
        return sc, full, mask, dmap

    def backward(self, st):
        """d feat -> d f_s (self.dfs) and the colour layers' weight-gradient partials, on stream st."""
        L = _lib.lib()
        ck, p = _lib.check, _lib.ptr
        if self.zero_dfs:
            self.dfs.zero_()
        ck(L.sgn_train_colour_head_bwd(ctypes.byref(self.qo), self.n_items, p(self.h[2]), self.w6, self.b6,
                                       p(self.dfeat), p(self.dy[2]), ctypes.c_void_p(_addr(self.amax, self.A_DY3)),
                                       p(self.part_c6), st), "sgn_train_colour_head_bwd")
        for gs in self.g_bwd:
            ck(L.sgn_x3_gemm(ctypes.byref(gs), st), "sgn_x3_gemm")


class F32Step:
    """Device buffers and pre-built launch arguments of the fp32 step for one batch capacity
    (R rays x SR samples x K neighbours), bound to one trainer's parameters and one query
    workspace.  `run` issues the step's launches on the current stream."""

    # amax words after the colour stage's three
    A_D4, A_D3, A_D2, A_D1, A_DB = range(3, 8)

    def __init__(self, trainer, q, R):
        L = _lib.lib()
        o = trainer.opts
        self.trainer, self.R, self.K = trainer, R, o.K
        # SG-NeRF's block2_bpnet.0 between block1.2 and block3.0 (point_aggregators.py:345-354)
        self.sg, self.D = trainer.sg, trainer.variant[1]
        dev = trainer.device
        self.cap = cap = max(R * o.SR, 1)
        self.rows_cap = rows = cap * o.K
        self.q = q
        self.qo = q.abi()
        f32 = dict(dtype=torch.float32, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        self.row_off = torch.zeros(cap, **i32)
        self.counts = torch.zeros(4, **i32)
        self.lists_ws = torch.empty(int(L.sgn_train_lists_workspace_bytes(cap)), dtype=torch.uint8, device=dev)
        self.feat = torch.zeros(cap, 4, **f32)
        self.z = [torch.empty(rows, 256, **f32) for _ in range(4)]     # z1, z2, z3, z4 -> delta4
        self.zb = self.db = self.bprow = None
        if self.sg:   # block2_bpnet.0's pre-activation and delta, the rows' BPNet embedding
            self.zb = torch.empty(rows, 256, **f32)
            self.db = torch.empty(rows, 256, **f32)
            self.bprow = torch.empty(rows, self.D, **f32) if self.D else None
        self.ws32 = torch.empty(int(L.sgn_aggregate_workspace_bytes_f32(cap)), dtype=torch.uint8, device=dev)
        # k_rows16's blended features: fp32 [cap][256] inside the workspace (the ABI names where)
        fs_off = int(L.sgn_aggregate_fs_offset_f32(self.ws32.numel(), cap))
        assert fs_off >= 0, "the aggregate workspace must hold every item's f_s row"
        self.fs = self.ws32[fs_off:fs_off + cap * 256 * 4].view(torch.float32).view(cap, 256)
        self.x0 = torch.empty(rows, 288, **f32)
        self.ext = torch.empty(rows, 8, **f32)
        self.rw = torch.empty(rows, 2, **f32)
        self.vpe = torch.empty(cap, 32, **f32)
        self.d = [torch.empty(rows, 256, **f32) for _ in range(3)]      # delta1, delta2, delta3
        self.dext = torch.empty(rows, 8, **f32)
        # block1.0's input gradient feeds d points_embeding alone: frozen, neither the buffer nor its GEMM exists
        self.dx0 = torch.empty(rows, 224, **f32) if "points_embeding" in trainer.trained else None
        self.amax = torch.zeros(16, dtype=torch.int32, device=dev)
        self.dfeat = torch.empty(cap, 4, **f32)
        # the colour MLP and the losses over the items (their count at counts[0]), all products split-fp16
        self.colour = ColourStage(trainer, self.qo, R, cap, _addr(self.counts, 0), self.fs, self.vpe, self.feat,
                                  self.dfeat, self.amax)
        self.part_rows = [torch.empty(SPLITS_ROWS, 256, n, **f32)
                          for n in (257, 264, 257, 285) + ((257 + self.D,) if self.sg else ())]
        self.part_a = torch.empty(int(L.sgn_train_head_partial_floats(1)), **f32)
        self._build()

    # -- the launch arguments (pointers of persistent buffers: built once) ----------------------
    def _build(self):
        A = _FlatAddr(self.trainer)
        W, Bv, S = A.W, A.B, A.S
        amax = [_addr(self.amax, i) for i in range(16)]
        n_rows = _addr(self.counts, 1)
        rc = self.rows_cap
        z1, z2, z3, z4 = (_addr(t) for t in self.z)
        d1, d2, d3 = (_addr(t) for t in self.d)
        # ---- block3.2 forward again: z4 = LReLU(z3) W3^T + b3 -----------------------------------
        w, o_, i_ = W("block3.2")
        self.g_z4 = _rows_gemm(_operand(z3, 256, 256, 0, act=1), _operand(w, i_, i_, 0, shift=S("block3.2")), rc, o_, i_,
                               n_rows, z4, 256, bias=Bv("block3.2"))
        # ---- row backward chain ----------------------------------------------------------------
        G = []
        w, o_, i_ = W("block3.2")
        G.append(("d3", _rows_gemm(_operand(z4, 256, 256, 0, amax=amax[self.A_D4]), _operand(w, i_, i_, 1, shift=S("block3.2")),
                                   rc, 256, 256, n_rows, d3, 256, mask=z3, ldm=256, amax_out=amax[self.A_D3])))
        w, o_, i_ = W("block3.0")
        if self.sg:   # block3.0's input is block2_bpnet.0's output: its delta, then block1.2's
            db, zb = _addr(self.db), _addr(self.zb)
            G.append(("db", _rows_gemm(_operand(d3, 256, 256, 0, amax=amax[self.A_D3]),
                                       _operand(w, i_, i_, 1, shift=S("block3.0")), rc, 263, 256, n_rows, db, 256, mask=zb,
                                       ldm=256, out_cols=256, out2=_addr(self.dext), ldo2=8, amax_out=amax[self.A_DB])))
            w, o_, i_ = W("block2_bpnet.0")
            G.append(("d2", _rows_gemm(_operand(db, 256, 256, 0, amax=amax[self.A_DB]),
                                       _operand(w, i_, 256, 1, shift=S("block2_bpnet.0")), rc, 256, 256, n_rows, d2, 256,
                                       mask=z2, ldm=256, amax_out=amax[self.A_D2])))
        else:
            G.append(("d2", _rows_gemm(_operand(d3, 256, 256, 0, amax=amax[self.A_D3]),
                                       _operand(w, i_, i_, 1, shift=S("block3.0")), rc, 263, 256, n_rows, d2, 256, mask=z2,
                                       ldm=256, out_cols=256, out2=_addr(self.dext), ldo2=8, amax_out=amax[self.A_D2])))
        w, o_, i_ = W("block1.2")
        G.append(("d1", _rows_gemm(_operand(d2, 256, 256, 0, amax=amax[self.A_D2]), _operand(w, i_, i_, 1, shift=S("block1.2")),
                                   rc, 256, 256, n_rows, d1, 256, mask=z1, ldm=256, amax_out=amax[self.A_D1])))
        w, o_, i_ = W("block1.0")
        if self.dx0 is not None:
            G.append(("dx0", _rows_gemm(_operand(d1, 256, 256, 0, amax=amax[self.A_D1]),
                                        _operand(w, i_, 224, 1, shift=S("block1.0")), rc, 224, 256, n_rows,
                                        _addr(self.dx0), 224)))
        self.g_row_bwd = G
        # ---- row weight gradients: delta^T [x | 1] ---------------------------------------------
        pr = self.part_rows
        self.g_row_dw = [
            _splitk_gemm(_operand(z4, 256, 256, 1, amax=amax[self.A_D4]), _operand(z3, 256, 256, 1, ones_col=256, act=1),
                         256, 257, rc, n_rows, _addr(pr[0]), SPLITS_ROWS),
            _splitk_gemm(_operand(d3, 256, 256, 1, amax=amax[self.A_D3]),
                         _operand(_addr(self.zb) if self.sg else z2, 256, 264, 1, p2=_addr(self.ext), ld2=8, csplit=256,
                                  act=1), 256, 264, rc, n_rows, _addr(pr[1]), SPLITS_ROWS),
            _splitk_gemm(_operand(d2, 256, 256, 1, amax=amax[self.A_D2]), _operand(z1, 256, 256, 1, ones_col=256, act=1),
                         256, 257, rc, n_rows, _addr(pr[2]), SPLITS_ROWS),
            _splitk_gemm(_operand(d1, 256, 256, 1, amax=amax[self.A_D1]), _operand(_addr(self.x0), 288, 285, 1),
                         256, 285, rc, n_rows, _addr(pr[3]), SPLITS_ROWS)]
        if self.sg:   # block2_bpnet.0: delta_b^T [LReLU(z2) | BPNet embedding | 1]
            D = self.D
            xb = (_operand(z2, 256, 256 + D, 1, p2=_addr(self.bprow), ld2=D, csplit=256, ones_col=256 + D, act=1) if D
                  else _operand(z2, 256, 256, 1, ones_col=256, act=1))
            self.g_row_dw.append(_splitk_gemm(_operand(_addr(self.db), 256, 256, 1, amax=amax[self.A_DB]), xb, 256, 257 + D,
                                              rc, n_rows, _addr(pr[4]), SPLITS_ROWS))
        # ---- partials -> flat gradient: the colour stage's segments, then the rows' ----------------
        segs = self.colour.segments + [
            A.segment(_addr(self.part_a), self.part_a.numel() // 257, 1, 257, "alpha_branch.0", 256, 256),
            A.segment(_addr(pr[0]), SPLITS_ROWS, 256, 257, "block3.2", 256, 256),
            A.segment(_addr(pr[1]), SPLITS_ROWS, 256, 264, "block3.0", 263, 263),
            A.segment(_addr(pr[2]), SPLITS_ROWS, 256, 257, "block1.2", 256, 256),
            A.segment(_addr(pr[3]), SPLITS_ROWS, 256, 285, "block1.0", 284, 284)]
        if self.sg:
            segs.append(A.segment(_addr(pr[4]), SPLITS_ROWS, 256, 257 + self.D, "block2_bpnet.0", 256 + self.D,
                                  256 + self.D))
        self.segs = (_lib.PartialSegment * len(segs))(*segs)
        self.n_seg = len(segs)
        self.wa, self.ba = W("alpha_branch.0")[0], Bv("alpha_branch.0")
        self.bpack = _attach_bpack(self.colour.gemms + [gs for _, gs in self.g_row_bwd] + [self.g_z4] + self.g_row_dw,
                                   A.flat.device)

    # -- one step ------------------------------------------------------------------------------
    def run(self, pt, proj, blob, campos, rot, gt, bg_ray, depth=None):
        """Forward + backward of one batch after the query (gradients added into flat.grad and the
        point gradients; those must be zero / as the caller wants them).  Returns fresh copies of the loss
        vector, the rendered colour [R, 3], the ray mask [R] (int8) and, with depth (a train.DepthTarget), the
        depth map (ColourStage.results_out)."""
        L = _lib.lib()
        st = _lib.stream_handle()
        tr, K, qo, col = self.trainer, self.K, self.qo, self.colour
        P = tr.points
        ck = _lib.check
        cap, p = self.cap, _lib.ptr

        def gemm(gs):
            ck(L.sgn_x3_gemm(ctypes.byref(gs), st), "sgn_x3_gemm")

        self.amax.zero_()
        ck(L.sgn_train_lists(p(self.q.counters), p(self.q.samp_nnb), cap, p(self.q.work), p(self.row_off), p(self.feat),
                             p(self.counts), p(self.lists_ws), st), "sgn_train_lists")
        ck(L.sgn_aggregate_train_fwd_f32(*tr.variant, p(tr.bpnet32), p(proj), ctypes.byref(pt), ctypes.byref(qo), cap, K,
                                         p(blob), p(self.feat), p(self.z[0]), p(self.z[1]), p(self.zb), p(self.z[2]),
                                         p(self.row_off), p(self.ws32), self.ws32.numel(), st),
           "sgn_aggregate_train_fwd_f32")
        ck(L.sgn_train_row_inputs(ctypes.byref(pt), ctypes.byref(qo), K, p(self.row_off), p(self.counts), p(self.x0),
                                  p(self.ext), p(self.rw), p(self.vpe), st), "sgn_train_row_inputs")
        if self.D:
            ck(L.sgn_train_row_gather(ctypes.byref(qo), K, p(self.row_off), p(self.counts), p(tr.bpnet32), self.D,
                                      p(self.bprow), st), "sgn_train_row_gather")
        col.forward_and_loss(campos, rot, gt, bg_ray, st, depth)
        col.backward(st)
        gemm(self.g_z4)
        ck(L.sgn_train_row_head(ctypes.byref(pt), ctypes.byref(qo), K, p(self.row_off), p(self.counts), p(self.z[3]),
                                p(col.dfs), p(self.dfeat), p(self.rw), self.wa, self.ba, p(P.points_conf.grad),
                                ctypes.c_void_p(_addr(self.amax, self.A_D4)), p(self.part_a), st), "sgn_train_row_head")
        for _, gs in self.g_row_bwd:
            gemm(gs)
        grads = tr.point_grads()   # NULL members: frozen tensors (all of embedding / colour / dir: no launch)
        ck(L.sgn_train_row_tail(ctypes.byref(pt), ctypes.byref(qo), K, p(self.row_off), p(self.counts), p(self.dx0),
                                p(self.dext), ctypes.byref(grads), st), "sgn_train_row_tail")
        for gs in self.g_row_dw:
            gemm(gs)
        ck(L.sgn_reduce_partials(self.n_seg, self.segs, st), "sgn_reduce_partials")
        return col.results_out(col.losses, depth is not None)


class F32Runner:
    """What `train_hip.HipTrainer` runs at precision "f32" between its shared prologue (inputs, query)
    and epilogue (all-reduce, point-row exchange): the reference's fp32 step as HIP launches with the
    counts on the device -- no host sync on one GPU; under DP one for the touched-row counts.

      begin   the fp32-faithful blob re-packed, the point Adam's launch (HipTrainer._adam_rows: on the
              query's table, whose distinct-row list is then the step's touched list; under DP on the
              rank's touched rows, which ride the point-row exchange)
      run     sgn_point_project_f32 on a list (block1.0's per-point part for the touched points only: ~50 k
              of 1.2 M for a 4096-ray batch -- the rows read no other point, and the weights change
              every step), F32Step.run, the results out into one fresh allocation (ColourStage.results_out)"""

    graph_captures = 0   # no captured graphs at this precision

    def __init__(self, trainer):
        self.tr = trainer
        self.step = None         # the F32Step of the last batch's capacity and buffers (`key`)
        self.key = None
        self.proj = None         # block1.0's per-point projection, grown on demand
        self._blob = None        # this step's fp32-faithful blob (begin)
        self._rows = None        # this step's touched points: (int32 list, device count)
        self._t_idx = self._t_cnt = None   # under DP: touched_rows' list and count

    def begin(self, b):
        """What the step queues before the gradients are made ready: the blob and the point Adam's launch."""
        tr, q = self.tr, b.q
        K, npts = tr.opts.K, tr.points.xyz.shape[0]
        self._blob = tr.packer32.pack(tr.mlp.flat)
        if b.dp:   # every rank's touched rows ride the step's one sync (the point-row exchange)
            self._t_idx, self._t_cnt = touched_rows(q.pidx, q.counters[0], K, npts)
            self._rows = (self._t_idx.to(torch.int32), self._t_cnt)
            if tr._adam_rows(*self._rows, True, 1) is None and not tr.point_params:
                tr.touched_points(q)   # every point tensor frozen: the OOB watch still sees the step
        else:      # the Adam's distinct-row list is the step's touched list (row 0 included)
            self._rows = tr._adam_rows(q.pidx, q.counters, False, K) or tr.touched_points(q)

    def run(self, b):
        """Forward + backward of the batch into the (ready) gradients.  Returns (loss parts, rendered
        colour [R, 3], ray_mask [R] int8)."""
        tr, dev = self.tr, self.tr.device
        q, R = b.q, b.R
        L = _lib.lib()
        pt = tr._tables(b.campos, b.rot, b.raydir)
        nproj = int(L.sgn_point_proj_bytes_f32(tr.points.xyz.shape[0]))
        if self.proj is None or self.proj.numel() < nproj:
            self.proj = torch.empty(max(nproj, 16), dtype=torch.uint8, device=dev)
        idx32, cnt = self._rows
        _lib.check(L.sgn_point_project_f32(ctypes.byref(pt), _lib.ptr(self._blob), _lib.ptr(idx32), _lib.ptr(cnt),
                                           _lib.ptr(self.proj), _lib.stream_handle()), "sgn_point_project_f32")
        fl = tr.mlp.flat
        key = (R, q.work.data_ptr(), q.pidx.data_ptr(), fl.data_ptr(), fl.grad.data_ptr())
        if self.key != key:
            self.step, self.key = F32Step(tr, q, R), key
        lo, full, mask, b.depth_map = self.step.run(pt, self.proj, self._blob, b.campos, b.rot, b.gt, b.bg_ray, b.depth)
        return self._parts(b, lo), full, mask

    def _parts(self, b, lo):
        """The reported loss parts and their total from the step's loss vector."""
        opts = self.tr.opts
        parts = loss_hip.loss_parts(opts, lo, b.depth is not None)
        parts["total"] = opts.total_loss(parts, None if b.depth is None else b.depth.weight)
        return parts

    def dp_rows(self):
        """Under DP: this rank's touched rows and every rank's count (gathered and read here: the
        step's one host sync, after the flat gradient's all-reduce is queued)."""
        return self._t_idx, [int(x) for x in gather_counts(self._t_cnt).tolist()]


class F32StepNb3:
    """F32Step for the viewmlp without block3 (shading_feature_mlp_layer3 = 0; point_aggregators.py:356-368,
    :638-653): device buffers and pre-built launch arguments for one batch capacity.  No point projection and no
    blob: the row MLP's forward is the renderer's rows_gemm sequence (row_forward_gemms) over ONE window holding
    the whole work list, so the window's two device words are the launches' counts and nothing is sized by a host
    read.  z1, z2 and zb keep a buffer each (the backward reads all of them); the head (sgn_train_row_head) runs on
    the last of z2 / zb and leaves its delta there.

      lists          sgn_train_lists, sgn_rows_windows (ci = cap, one window)
      row inputs     sgn_rows_inputs_nb3 -> x0, rw, vpe; 352-input block2_bpnet.0: sgn_rows_gather_nb3 -> bprow
      row forward    z1, z2 (, zb; sgn_x3_gemm_accumulate on the BPNet columns), sgn_rows_blend_nb3 -> alpha_s, f_s
      colour         ColourStage.forward_and_loss, ColourStage.backward
      head           sgn_train_row_head in place on z2 / zb -> delta, d conf, alpha_branch.0's partials
      row backward   (d2 = delta_b Wb[:, :256] masked by z2,) d1 = d2 W12 masked by z1, dx0 = d1 W10[:, :224]
      point grads    sgn_train_row_tail (embedding only: colour and dir are outside this network's graph)
      weight grads   d2^T [LReLU(z1) | 1], d1^T x0 (, delta_b^T [LReLU(z2) | bprow | 1]), one sgn_reduce_partials
    """

    # amax words after the colour stage's three: the deltas', then the forward's (max |z|, the blend's flag)
    A_D2, A_D1, A_DB, A_Z1, A_Z2, A_ZB, A_HEAD = range(3, 10)

    def __init__(self, trainer, q, R):
        L = _lib.lib()
        o = trainer.opts
        self.trainer, self.R, self.K = trainer, R, o.K
        self.sg, self.D = trainer.sg, trainer.variant[1]
        dev = trainer.device
        self.cap = cap = max(R * o.SR, 1)
        self.rows_cap = rows = cap * o.K
        if rows * X0_LD * 4 + X0_LD * 4 >= GEMM_BYTES_LIMIT:
            raise ValueError(f"a batch of {R} rays x {o.SR} samples x K = {o.K} holds {rows} rows: the row GEMMs' "
                             f"operands stay below 2 GiB ({(GEMM_BYTES_LIMIT - 1) // (X0_LD * 4) - 1} rows)")
        self.q = q
        self.qo = q.abi()
        f32 = dict(dtype=torch.float32, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        self.row_off = torch.zeros(cap, **i32)
        self.counts = torch.zeros(4, **i32)
        self.win = torch.zeros(2, **i32)           # the one window's (items, rows)
        self.lists_ws = torch.empty(int(L.sgn_train_lists_workspace_bytes(cap)), dtype=torch.uint8, device=dev)
        self.feat = torch.zeros(cap, 4, **f32)
        self.x0 = torch.empty(rows, X0_LD, **f32)
        self.rw = torch.empty(rows, 2, **f32)
        self.vpe = torch.empty(cap, 32, **f32)
        self.fs = torch.empty(cap, 256, **f32)
        self.z1 = torch.empty(rows, 256, **f32)
        self.z2 = torch.empty(rows, 256, **f32)    # base: the head leaves delta2 here
        self.zb = self.d2 = self.bprow = None
        if self.sg:   # block2_bpnet.0's pre-activation (the head leaves delta_b here), block1.2's delta
            self.zb = torch.empty(rows, 256, **f32)
            self.d2 = torch.empty(rows, 256, **f32)
            self.bprow = torch.empty(rows, self.D, **f32) if self.D else None
        self.zlast = self.zb if self.sg else self.z2
        self.d1 = torch.empty(rows, 256, **f32)
        # block1.0's input gradient feeds d points_embeding alone: frozen, neither the buffer nor its GEMM exists
        self.dx0 = torch.empty(rows, 224, **f32) if "points_embeding" in trainer.trained else None
        self.amax = torch.zeros(16, dtype=torch.int32, device=dev)
        self.dfeat = torch.empty(cap, 4, **f32)
        self.colour = ColourStage(trainer, self.qo, R, cap, _addr(self.counts, 0), self.fs, self.vpe, self.feat,
                                  self.dfeat, self.amax)
        self.part_rows = [torch.empty(SPLITS_ROWS, 256, n, **f32)
                          for n in (257, 285) + ((257 + self.D,) if self.sg else ())]
        self.part_a = torch.empty(int(L.sgn_train_head_partial_floats(1)), **f32)
        self.range_word = None   # after run: int64 [1], non-zero when the forward left fp16 range
        self._build()

    # -- the launch arguments (pointers of persistent buffers: built once) ----------------------
    def _build(self):
        A = _FlatAddr(self.trainer)
        W, Bv, S = A.W, A.B, A.S
        amax = [_addr(self.amax, i) for i in range(16)]
        n_rows = _addr(self.win, 1)
        rc = self.rows_cap
        z1, z2, d1 = _addr(self.z1), _addr(self.z2), _addr(self.d1)
        # ---- row forward: the renderer's launches, every pre-activation in its own buffer ---------
        self.g_fwd, self.g_acc = row_forward_gemms(W, Bv, S, self.trainer.variant, rc, n_rows, _addr(self.x0), z1, z2,
                                                   _addr(self.zb) if self.sg else None,
                                                   _addr(self.bprow) if self.D else None,
                                                   (amax[self.A_Z1], amax[self.A_Z2], amax[self.A_ZB]))
        # ---- row backward chain -------------------------------------------------------------------
        G = []
        if self.sg:   # the head's delta is block2_bpnet.0's: block1.2's through Wb's first 256 columns
            db, d2 = _addr(self.zb), _addr(self.d2)
            self.a_head = self.A_DB
            w, o_, i_ = W(BPNET)
            G.append(("d2", _rows_gemm(_operand(db, 256, 256, 0, amax=amax[self.A_DB]),
                                       _operand(w, i_, 256, 1, shift=S(BPNET)), rc, 256, 256, n_rows, d2, 256,
                                       mask=z2, ldm=256, amax_out=amax[self.A_D2])))
        else:         # the head left block1.2's delta in z2's buffer
            d2 = z2
            self.a_head = self.A_D2
        w, o_, i_ = W("block1.2")
        G.append(("d1", _rows_gemm(_operand(d2, 256, 256, 0, amax=amax[self.A_D2]), _operand(w, i_, i_, 1, shift=S("block1.2")),
                                   rc, 256, 256, n_rows, d1, 256, mask=z1, ldm=256, amax_out=amax[self.A_D1])))
        w, o_, i_ = W("block1.0")
        if self.dx0 is not None:
            G.append(("dx0", _rows_gemm(_operand(d1, 256, 256, 0, amax=amax[self.A_D1]),
                                        _operand(w, i_, 224, 1, shift=S("block1.0")), rc, 224, 256, n_rows,
                                        _addr(self.dx0), 224)))
        self.g_row_bwd = G
        # ---- row weight gradients: delta^T [x | 1] ---------------------------------------------
        pr = self.part_rows
        self.g_row_dw = [
            _splitk_gemm(_operand(d2, 256, 256, 1, amax=amax[self.A_D2]), _operand(z1, 256, 256, 1, ones_col=256, act=1),
                         256, 257, rc, n_rows, _addr(pr[0]), SPLITS_ROWS),
            _splitk_gemm(_operand(d1, 256, 256, 1, amax=amax[self.A_D1]), _operand(_addr(self.x0), X0_LD, 285, 1),
                         256, 285, rc, n_rows, _addr(pr[1]), SPLITS_ROWS)]
        if self.sg:   # block2_bpnet.0: delta_b^T [LReLU(z2) | BPNet embedding | 1]
            D = self.D
            xb = (_operand(z2, 256, 256 + D, 1, p2=_addr(self.bprow), ld2=D, csplit=256, ones_col=256 + D, act=1) if D
                  else _operand(z2, 256, 256, 1, ones_col=256, act=1))
            self.g_row_dw.append(_splitk_gemm(_operand(_addr(self.zb), 256, 256, 1, amax=amax[self.A_DB]), xb, 256, 257 + D,
                                              rc, n_rows, _addr(pr[2]), SPLITS_ROWS))
        # ---- partials -> flat gradient: the colour stage's segments, then the rows' ----------------
        segs = self.colour.segments + [
            A.segment(_addr(self.part_a), self.part_a.numel() // 257, 1, 257, "alpha_branch.0", 256, 256),
            A.segment(_addr(pr[0]), SPLITS_ROWS, 256, 257, "block1.2", 256, 256),
            A.segment(_addr(pr[1]), SPLITS_ROWS, 256, 285, "block1.0", 284, 284)]
        if self.sg:
            segs.append(A.segment(_addr(pr[2]), SPLITS_ROWS, 256, 257 + self.D, BPNET, 256 + self.D, 256 + self.D))
        self.segs = (_lib.PartialSegment * len(segs))(*segs)
        self.n_seg = len(segs)
        self.wa, self.ba = W("alpha_branch.0")[0], Bv("alpha_branch.0")
        every = (self.colour.gemms + self.g_fwd + ([self.g_acc] if self.g_acc is not None else []) +
                 [gs for _, gs in self.g_row_bwd] + self.g_row_dw)
        self.bpack = _attach_bpack(every, A.flat.device)

    # -- one step ------------------------------------------------------------------------------
    def run(self, pt, campos, rot, gt, bg_ray, depth=None):
        """F32Step.run for this network: forward + backward of one batch after the query into flat.grad and the
        point gradients; returns ColourStage.results_out's copies.  self.range_word is the step's fp16-range word."""
        L = _lib.lib()
        st = _lib.stream_handle()
        tr, K, qo, col = self.trainer, self.K, self.qo, self.colour
        P = tr.points
        ck = _lib.check
        cap, p = self.cap, _lib.ptr
        Q, PT = ctypes.byref(qo), ctypes.byref(pt)

        def gemm(gs):
            ck(L.sgn_x3_gemm(ctypes.byref(gs), st), "sgn_x3_gemm")

        self.amax.zero_()
        ck(L.sgn_train_lists(p(self.q.counters), p(self.q.samp_nnb), cap, p(self.q.work), p(self.row_off), p(self.feat),
                             p(self.counts), p(self.lists_ws), st), "sgn_train_lists")
        ck(L.sgn_rows_windows(Q, K, p(self.row_off), p(self.counts), cap, 1, p(self.win), st), "sgn_rows_windows")
        win = p(self.win)
        ck(L.sgn_rows_inputs_nb3(PT, Q, K, p(self.row_off), win, 0, cap, p(self.x0), p(self.rw), p(self.vpe), st),
           "sgn_rows_inputs_nb3")
        if self.D:
            ck(L.sgn_rows_gather_nb3(Q, K, p(self.row_off), win, 0, cap, p(tr.bpnet32), self.D, p(self.bprow), st),
               "sgn_rows_gather_nb3")
        for gs in self.g_fwd:
            gemm(gs)
        if self.g_acc is not None:
            ck(L.sgn_x3_gemm_accumulate(ctypes.byref(self.g_acc), st), "sgn_x3_gemm_accumulate")
        ck(L.sgn_rows_blend_nb3(Q, K, p(self.row_off), win, 0, cap, p(self.zlast), p(self.rw), self.wa, self.ba,
                                p(self.feat), p(self.fs), None, None, ctypes.c_void_p(_addr(self.amax, self.A_HEAD)), st),
           "sgn_rows_blend_nb3")
        col.forward_and_loss(campos, rot, gt, bg_ray, st, depth)
        col.backward(st)
        ck(L.sgn_train_row_head(PT, Q, K, p(self.row_off), p(self.counts), p(self.zlast), p(col.dfs), p(self.dfeat),
                                p(self.rw), self.wa, self.ba, p(P.points_conf.grad),
                                ctypes.c_void_p(_addr(self.amax, self.a_head)), p(self.part_a), st), "sgn_train_row_head")
        for _, gs in self.g_row_bwd:
            gemm(gs)
        grads = tr.point_grads()   # the embedding's gradient or NULL: colour and dir are never trained here
        ck(L.sgn_train_row_tail(PT, Q, K, p(self.row_off), p(self.counts), p(self.dx0), None, ctypes.byref(grads), st),
           "sgn_train_row_tail")
        for gs in self.g_row_dw:
            gemm(gs)
        ck(L.sgn_reduce_partials(self.n_seg, self.segs, st), "sgn_reduce_partials")
        # max |z1|, |z2|, |zb| and the blend's flag folded into one word, on the device
        self.range_word = (self.amax[self.A_Z1:self.A_HEAD + 1].max() >= FP16_RANGE_BITS).to(torch.int64).reshape(1)
        return col.results_out(col.losses, depth is not None)


class F32RunnerNb3(F32Runner):
    """F32Runner for the viewmlp without block3 (opts.train_rows = 1).  `begin` is F32Runner's (the per-layer
    shifts recomputed on the device -- the packer is shifts-only, there is no blob -- and the point Adam's launch)
    after a look, without waiting, at the last step's fp16-range word (train_hip._Watch: a word whose copy has not
    landed yet is reported a step later); `run` is F32StepNb3.run, with no projection."""

    def begin(self, b):
        self.tr._range_watch.check()
        super().begin(b)

    def run(self, b):
        tr = self.tr
        q, R = b.q, b.R
        pt = tr._tables(b.campos, b.rot, b.raydir)
        fl = tr.mlp.flat
        key = (R, q.work.data_ptr(), q.pidx.data_ptr(), fl.data_ptr(), fl.grad.data_ptr())
        if self.key != key:
            self.step, self.key = F32StepNb3(tr, q, R), key
        lo, full, mask, b.depth_map = self.step.run(pt, b.campos, b.rot, b.gt, b.bg_ray, b.depth)
        tr._range_watch.post(self.step.range_word)
        return self._parts(b, lo), full, mask
