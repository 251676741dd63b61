"""The viewmlp without block3 (shading_feature_mlp_layer3 = 0) on the split-fp16 row GEMMs (opts.rows_gemm = 1).

Without block3 the row MLP is block1.0, block1.2 (and block2_bpnet.0) followed by the alpha dot and the K-blend
(point_aggregators.py:356-368, :638-653, :743-770), so a frame is a composition of sgn_x3_gemm launches (rows
mode: three fp16 MFMA products per fp32 product, the weight block in LDS) over COMPACT rows, the training
step's lists, between two small kernels -- window by window of the frame's ascending work list, so that every
buffer is sized for one window and every rows-mode operand stays below the GEMM's 2 GiB limit:

  sgn_train_lists       ascending work list, compact row offsets, feat cleared        (once per frame)
  sgn_rows_windows      every window's (items, rows) as device words                  (once per frame)
  per window of CI items:
    sgn_rows_inputs_nb3   x0 [rows, 288] = [emb | PE(emb) | PE(dists) | 1], rw [rows, 2], vpe [items, 32]
    sgn_x3_gemm           z1 = x0 W10^T + b10;  z2 = LReLU(z1) W12^T + b12
    block2_bpnet.0        zb = LReLU(z2) Wb[:, :256]^T + bb; with the BPNet columns sgn_rows_gather_nb3 and
                          sgn_x3_gemm_accumulate: zb += bpnet rows Wb[:, 256:]^T
    sgn_rows_blend_nb3    h = LReLU(z last); alpha_s -> feat[s].x, f_s -> fs [items, 256], blend / wnorm
    colour MLP            3 x sgn_x3_gemm on [f_s | vpe], sgn_train_colour_head -> feat[s].yzw

Every GEMM writes max |out| into an amax word and the blend kernel flags a blended value that is not finite or
has left fp16 range; `flag()` folds them into the renderer's fp16-range protocol (render.HipRenderer._range_check).
"""
import ctypes

import torch

from . import _lib
from .train_f32 import FP16_RANGE_BITS, GEMM_BYTES_LIMIT, X0_LD, _addr, _operand, _rows_gemm, row_forward_gemms
from .weights import layers_for

ROWS_DEFAULT = 1 << 20           # rows of a default window (CI K <= 1 M rows: x0 1.2 GB, z1 / z2 1 GB each)


def max_window_rows(ld=X0_LD):
    """The largest M of a rows-mode launch whose widest operand has `ld` floats per row (M ld 4 < 2 GiB)."""
    return (GEMM_BYTES_LIMIT - 1) // (ld * 4)


def default_ci(K, rows=ROWS_DEFAULT):
    """Items per window so that a window holds at most `rows` rows (every item has up to K)."""
    return max(1, min(rows, max_window_rows()) // max(int(K), 1))


def check_ci(ci, K):
    ci = int(ci)
    if ci < 1 or ci * int(K) > max_window_rows():
        raise ValueError(f"rows_gemm window of {ci} items x K = {K}: 1 <= CI and CI K <= {max_window_rows()} rows "
                         "(every rows-mode GEMM operand below 2 GiB)")
    return ci


def plan_windows(n_items, ci):
    """The windows of a frame with n_items work items: [(item0, items)], items <= ci, in list order."""
    n_items, ci = int(n_items), int(ci)
    if ci < 1:
        raise ValueError("window size must be at least one item")
    return [(i0, min(ci, n_items - i0)) for i0 in range(0, max(n_items, 0), ci)]


def row_layers(variant):
    """The network's layers in flat order (weights.layers_for without block3)."""
    return layers_for(variant[0], variant[1], block3_layers=0)


class RowsGemmNb3:
    """Weights (flat fp32 + per-layer shifts), window buffers and launch arguments of the path for one renderer."""

    A_Z1, A_Z2, A_ZB, A_H1, A_H2, A_H3, A_HEAD, N_AMAX = range(8)

    def __init__(self, mlp_state, variant, K, ci, device):
        self.device = torch.device(device)
        self.variant, self.K = variant, int(K)
        self.ci = check_ci(default_ci(K) if ci is None else ci, K)
        self.rows = self.ci * self.K
        self._set_weights(mlp_state)
        self._cap = None       # sample capacity the per-frame lists are sized for
        self._win_args = {}    # window index -> its launches' arguments
        self.bpack = None
        dev, f32 = self.device, dict(dtype=torch.float32, device=self.device)
        ci_, rows = self.ci, self.rows
        self.x0 = torch.empty(rows, X0_LD, **f32)
        self.rw = torch.empty(rows, 2, **f32)
        self.z = [torch.empty(rows, 256, **f32) for _ in range(2)]
        self.bprows = torch.empty(rows, variant[1], **f32) if variant[1] else None
        self.vpe = torch.empty(ci_, 32, **f32)
        self.fs = torch.empty(ci_, 256, **f32)
        self.h = [torch.empty(ci_, 128, **f32) for _ in range(3)]
        self.amax = torch.zeros(self.N_AMAX, dtype=torch.int32, device=dev)

    # ---- weights: static while rendering, so flattened and shifted once ------------------------------
    def _set_weights(self, state):
        layers = row_layers(self.variant)
        off, self.slices = 0, {}
        for name, o, i, _ in layers:
            self.slices[name] = (off, o, i)
            off += -(-(o * i + o) // 4) * 4        # every layer 16-B aligned
        flat = torch.zeros(off, dtype=torch.float32)
        for name, o, i, _ in layers:
            a = self.slices[name][0]
            flat[a:a + o * i] = torch.as_tensor(state[name + ".weight"]).detach().float().reshape(-1)
            flat[a + o * i:a + o * i + o] = torch.as_tensor(state[name + ".bias"]).detach().float().reshape(-1)
        self.flat = flat.to(self.device)
        self.layer_ix = {name: j for j, (name, *_) in enumerate(layers)}
        n = len(layers)
        self.shift = torch.zeros(n, dtype=torch.int32, device=self.device)
        w_off = (_lib.c_i64 * n)(*[self.slices[name][0] for name, *_ in layers])
        w_len = (_lib.c_i64 * n)(*[o * i for _, o, i, _ in layers])
        with torch.cuda.device(self.device):   # a shifts-only call: no fp16 / fp32 section
            _lib.check(_lib.lib().sgn_pack_scaled_f32(_lib.ptr(self.flat), self.flat.numel(), n, w_off, w_len, None, 0, None,
                                                      0, _lib.ptr(self.shift), None, None, _lib.stream_handle()),
                       "sgn_pack_scaled_f32 (shifts)")

    def W(self, name):
        off, o, i = self.slices[name]
        return _addr(self.flat, off), o, i

    def B(self, name):
        off, o, i = self.slices[name]
        return _addr(self.flat, off + o * i)

    def S(self, name):
        return _addr(self.shift, self.layer_ix[name])

    # ---- per-frame lists -------------------------------------------------------------------------------
    def _lists(self, cap):
        if self._cap is None or self._cap < cap:
            dev = self.device
            self.row_off = torch.zeros(cap, dtype=torch.int32, device=dev)
            self.counts = torch.zeros(4, dtype=torch.int32, device=dev)
            self.lists_ws = torch.empty(int(_lib.lib().sgn_train_lists_workspace_bytes(cap)), dtype=torch.uint8, device=dev)
            self.win = torch.zeros(2 * (-(-cap // self.ci)), dtype=torch.int32, device=dev)
            self._cap = cap
            self._win_args = {}

    def _window(self, w):
        """Window w's GEMM arguments (pointers of persistent buffers and of its two count words: built once)."""
        if w in self._win_args:
            return self._win_args[w]
        n_rows, n_items = _addr(self.win, 2 * w + 1), _addr(self.win, 2 * w)
        am = [_addr(self.amax, j) for j in range(self.N_AMAX)]
        rows, ci = self.rows, self.ci
        x0, z1, z2 = _addr(self.x0), _addr(self.z[0]), _addr(self.z[1])
        W, S, B = self.W, self.S, self.B
        # block2_bpnet.0's pre-activation reuses z1's buffer: a rendered frame reads z1 no more
        G, acc = row_forward_gemms(W, B, S, self.variant, rows, n_rows, x0, z1, z2, z1,
                                   _addr(self.bprows) if self.variant[1] else None,
                                   (am[self.A_Z1], am[self.A_Z2], am[self.A_ZB]))
        fsa, vpa = _addr(self.fs), _addr(self.vpe)
        h1, h2, h3 = (_addr(t) for t in self.h)
        wc, o, i = W("color_branch.0")
        C = [_rows_gemm(_operand(fsa, 256, 280, 0, p2=vpa, ld2=32, csplit=256), _operand(wc, i, i, 0, shift=S("color_branch.0")),
                        ci, o, i, n_items, h1, 128, bias=B("color_branch.0"), act=1, amax_out=am[self.A_H1])]
        for name, x, y, a in (("color_branch.2", h1, h2, self.A_H2), ("color_branch.4", h2, h3, self.A_H3)):
            wc, o, i = W(name)
            C.append(_rows_gemm(_operand(x, 128, 128, 0), _operand(wc, i, i, 0, shift=S(name)), ci, o, i, n_items, y, 128,
                                bias=B(name), act=1, amax_out=am[a]))
        every = G + ([acc] if acc is not None else []) + C
        if self.bpack is None:   # one weight-image workspace for every window launch (they run in stream order)
            L = _lib.lib()
            n = max(int(L.sgn_x3_gemm_bpack_bytes(ctypes.byref(g))) for g in every)
            self.bpack = torch.empty(max(n, 16), dtype=torch.uint8, device=self.device)
        for g in every:
            g.bpack = self.bpack.data_ptr()
        self._win_args[w] = (G, acc, C)
        return self._win_args[w]

    def flag(self):
        """int32 [1], non-zero when an activation of the last frame reached fp16 range or was not finite."""
        return (self.amax.max() >= FP16_RANGE_BITS).to(torch.int32).reshape(1)

    def run(self, pt, qo, q, cap, bpnet32, feat, blend, wnorm):
        """The frame's aggregation and colour MLP into feat [S, 4] (and blend / wnorm [S, K] when given) on the
        current stream.  One host read per frame: the item count, which sets the number of windows.  Returns it."""
        L = _lib.lib()
        ck, p = _lib.check, _lib.ptr
        st = _lib.stream_handle()
        K = self.K
        self._lists(cap)
        ck(L.sgn_train_lists(p(q.counters), p(q.samp_nnb), cap, p(q.work), p(self.row_off), p(feat), p(self.counts),
                             p(self.lists_ws), st), "sgn_train_lists")
        self.amax.zero_()
        if blend is not None:
            blend.zero_()
        if wnorm is not None:
            wnorm.zero_()
        n = int(self.counts[0].item())
        wins = plan_windows(n, self.ci)
        if not wins:
            return 0
        ck(L.sgn_rows_windows(ctypes.byref(qo), K, p(self.row_off), p(self.counts), self.ci, len(wins), p(self.win), st),
           "sgn_rows_windows")
        wa, ba = self.W("alpha_branch.0")[0], self.B("alpha_branch.0")
        w6, b6 = self.W("color_branch.6")[0], self.B("color_branch.6")
        zlast = self.z[0] if self.variant[0] else self.z[1]
        qw = type(qo)()
        ctypes.pointer(qw)[0] = qo
        for w, (item0, _) in enumerate(wins):
            G, acc, C = self._window(w)
            dwin = ctypes.c_void_p(_addr(self.win, 2 * w))
            ck(L.sgn_rows_inputs_nb3(ctypes.byref(pt), ctypes.byref(qo), K, p(self.row_off), dwin, item0, self.ci,
                                     p(self.x0), p(self.rw), p(self.vpe), st), "sgn_rows_inputs_nb3")
            for g in G:
                ck(L.sgn_x3_gemm(ctypes.byref(g), st), "sgn_x3_gemm")
            if acc is not None:
                ck(L.sgn_rows_gather_nb3(ctypes.byref(qo), K, p(self.row_off), dwin, item0, self.ci, bpnet32,
                                         self.variant[1], p(self.bprows), st), "sgn_rows_gather_nb3")
                ck(L.sgn_x3_gemm_accumulate(ctypes.byref(acc), st), "sgn_x3_gemm_accumulate")
            ck(L.sgn_rows_blend_nb3(ctypes.byref(qo), K, p(self.row_off), dwin, item0, self.ci, p(zlast), p(self.rw), wa, ba,
                                    p(feat), p(self.fs), p(blend), p(wnorm), ctypes.c_void_p(_addr(self.amax, self.A_HEAD)),
                                    st), "sgn_rows_blend_nb3")
            for g in C:
                ck(L.sgn_x3_gemm(ctypes.byref(g), st), "sgn_x3_gemm")
            qw.work = _addr(q.work, item0)
            ck(L.sgn_train_colour_head(ctypes.byref(qw), dwin, p(self.h[2]), w6, b6, p(feat), st), "sgn_train_colour_head")
        return n
