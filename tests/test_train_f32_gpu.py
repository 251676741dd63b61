"""GPU unit tests of the fp32 training step's kernels (csrc/train_x3.hip) through the C ABI:
sgn_x3_gemm in both modes against float64 torch on the same fp32 operands, the deterministic
work list / compact row offsets of sgn_train_lists, and the fixed-order partial reduction."""
import ctypes

import pytest
import torch

import sgnerf_amd  # noqa: F401
from sgnerf_amd import _lib
from sgnerf_amd.train_f32 import _operand, _rows_gemm, _splitk_gemm

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
# the 3-product split carries 22 significant bits per factor with fp32 accumulation: every output
# within a few fp32 ulps of sum |a b| (relative to the output's scale), the bar the f32 mode holds
REL = 2e-6


def _gemm(g):
    _lib.check(_lib.lib().sgn_x3_gemm(ctypes.byref(g), _lib.stream_handle()), "sgn_x3_gemm")


def _gemm_both(g, outs, amax=None):
    """sgn_x3_gemm in rows mode with the in-workgroup weight conversion, then with the weight images
    (bpack, ABI 13) into re-filled outputs: bit-identical results (the same split of the same values)."""
    _gemm(g)
    first = [o.clone() for o in outs]
    am = amax.clone() if amax is not None else None
    nb = int(_lib.lib().sgn_x3_gemm_bpack_bytes(ctypes.byref(g)))
    assert nb > 0
    ws = torch.full((nb // 4 + 4,), float("nan"), device=DEV)
    g2 = type(g).from_buffer_copy(g)
    g2.bpack = ws.data_ptr()
    for o in outs:
        o.fill_(-5.0)
    if amax is not None:
        amax.zero_()
    _gemm(g2)
    torch.cuda.synchronize()
    for a, b in zip(first, outs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    if amax is not None:
        assert torch.equal(am, amax)


def _rel(x, ref):
    return float((x.double() - ref).abs().max() / ref.abs().max().clamp(min=1e-30))


def _lrelu(x):
    return torch.where(x > 0, x, x * 0.01)


@pytest.mark.parametrize("scale", [1.0, 1e-7, 3e3])
def test_x3_gemm_rows_mode_matches_float64(scale):
    """Y = (dY W) * LReLU'(mask) with a bias / column split, and X W^T + b with LeakyReLU on the
    operand and the output: rows beyond the device count untouched, the amax word written."""
    g = torch.Generator().manual_seed(1)
    rows_cap, rows, K, N = 700, 613, 256, 263
    dy = (torch.randn(rows_cap, K, generator=g) * scale).to(DEV)
    W = (torch.randn(K, N, generator=g) * 0.06).to(DEV)          # [K][N] row-major: the NN (kmajor) form
    mask = torch.randn(rows_cap, 256, generator=g).to(DEV)
    shift = torch.tensor([14 - int(torch.frexp(W.abs().max().cpu())[1])], dtype=torch.int32, device=DEV)
    amax_in = torch.tensor([dy[:rows].abs().max().item()], dtype=torch.float32, device=DEV).view(torch.int32)
    nrows = torch.tensor([rows], dtype=torch.int32, device=DEV)
    out = torch.full((rows_cap, 256), -5.0, device=DEV)
    out2 = torch.full((rows_cap, 8), -5.0, device=DEV)
    amax = torch.zeros(2, dtype=torch.int32, device=DEV)
    a = _operand(dy.data_ptr(), K, K, 0, amax=amax_in.data_ptr())
    b = _operand(W.data_ptr(), N, N, 1, shift=shift.data_ptr())
    _gemm_both(_rows_gemm(a, b, rows_cap, N, K, nrows.data_ptr(), out.data_ptr(), 256, mask=mask.data_ptr(), ldm=256,
                          out_cols=256, out2=out2.data_ptr(), ldo2=8, amax_out=amax.data_ptr(),
                          amax_out2=amax[1:].data_ptr()), [out, out2], amax)
    torch.cuda.synchronize()
    ref = dy[:rows].double() @ W.double()
    ref1 = torch.where(mask[:rows] > 0, ref[:, :256], ref[:, :256] * 0.01)
    assert _rel(out[:rows], ref1) < REL
    assert _rel(out2[:rows, :7], ref[:, 256:263]) < REL
    assert bool((out[rows:] == -5.0).all()) and bool((out2[:, 7:] == -5.0).all())
    assert abs(amax[:1].view(torch.float32).item() - out[:rows].abs().max().item()) == 0.0
    # forward form: LReLU(LReLU(x) W^T + b), x with a second source past column 256
    Wf = (torch.randn(128, 280, generator=g) * 0.05).to(DEV)
    bf = torch.randn(128, generator=g).to(DEV)
    x1 = (torch.randn(rows_cap, 256, generator=g) * scale).to(DEV)
    x2 = torch.randn(rows_cap, 32, generator=g).to(DEV)
    sf = torch.tensor([14 - int(torch.frexp(Wf.abs().max().cpu())[1])], dtype=torch.int32, device=DEV)
    y = torch.full((rows_cap, 128), -5.0, device=DEV)
    _gemm_both(_rows_gemm(_operand(x1.data_ptr(), 256, 280, 0, p2=x2.data_ptr(), ld2=32, csplit=256, act=1),
                          _operand(Wf.data_ptr(), 280, 280, 0, shift=sf.data_ptr()), rows_cap, 128, 280, nrows.data_ptr(),
                          y.data_ptr(), 128, bias=bf.data_ptr(), act=1), [y])
    torch.cuda.synchronize()
    xin = torch.cat([_lrelu(x1[:rows].double()), x2[:rows, :24].double()], 1)
    reff = _lrelu(xin @ Wf.double().t() + bf.double())
    assert _rel(y[:rows], reff) < REL
    assert bool((y[rows:] == -5.0).all())


@pytest.mark.parametrize("rows,splits", [(0, 8), (31, 8), (5000, 64), (20011, 128)])
def test_x3_gemm_splitk_mode_matches_float64(rows, splits):
    """dW = dY^T [LReLU(z) | ext | 1] as split-K partials, reduced in order into a flat gradient
    (sgn_reduce_partials): weights, the bias through the ones column, nothing else touched."""
    g = torch.Generator().manual_seed(2)
    cap, M = 20480, 256
    dy = (torch.randn(cap, M, generator=g) * 1e-5).to(DEV)
    z = torch.randn(cap, 256, generator=g).to(DEV)
    ext = torch.randn(cap, 8, generator=g).to(DEV)
    ext[:, 7] = 1.0
    nrows = torch.tensor([rows], dtype=torch.int32, device=DEV)
    amax_in = torch.tensor([max(dy[:rows].abs().max().item(), 1e-30) if rows else 0.0], device=DEV).view(torch.int32)
    N = 264
    part = torch.full((splits, M, N), float("nan"), device=DEV)
    _gemm(_splitk_gemm(_operand(dy.data_ptr(), 256, 256, 1, amax=amax_in.data_ptr()),
                       _operand(z.data_ptr(), 256, 264, 1, p2=ext.data_ptr(), ld2=8, csplit=256, act=1),
                       M, N, cap, nrows.data_ptr(), part.data_ptr(), splits))
    flat = torch.zeros(M * 263 + M + 5, device=DEV)
    seg = _lib.PartialSegment()
    seg.part, seg.splits, seg.M, seg.N, seg.n_in, seg.bias_col, seg.ldw = part.data_ptr(), splits, M, N, 263, 263, 263
    seg.dst_w, seg.dst_b = flat.data_ptr(), flat.data_ptr() + 4 * M * 263
    _lib.check(_lib.lib().sgn_reduce_partials(1, ctypes.byref(seg), _lib.stream_handle()), "sgn_reduce_partials")
    torch.cuda.synchronize()
    x = torch.cat([_lrelu(z[:rows].double()), ext[:rows, :7].double()], 1)
    refw = dy[:rows].double().t() @ x
    refb = dy[:rows].double().sum(0)
    if rows == 0:
        assert bool((flat == 0).all())
        return
    assert _rel(flat[:M * 263].view(M, 263), refw) < REL
    assert _rel(flat[M * 263:M * 264], refb) < REL
    assert bool((flat[M * 264:] == 0).all())


def test_train_lists_deterministic_order():
    """sgn_train_lists: the samples with neighbours in ascending order, compact row offsets = the
    exclusive prefix sum of samp_nnb, totals, feat cleared for s < S (over several blocks)."""
    g = torch.Generator().manual_seed(3)
    cap, S = 5000, 4321
    nnb = torch.randint(0, 9, (cap,), generator=g, dtype=torch.int32)
    nnb[torch.rand(cap, generator=g) < 0.3] = 0
    counters = torch.tensor([S, int((nnb[:S] > 0).sum()), 0, 0], dtype=torch.int32, device=DEV)
    work = torch.full((cap,), -1, dtype=torch.int32, device=DEV)
    row_off = torch.full((cap,), -1, dtype=torch.int32, device=DEV)
    feat = torch.full((cap, 4), 3.0, device=DEV)
    counts = torch.zeros(4, dtype=torch.int32, device=DEV)
    L = _lib.lib()
    ws = torch.empty(int(L.sgn_train_lists_workspace_bytes(cap)), dtype=torch.uint8, device=DEV)
    nd = nnb.to(DEV)
    _lib.check(L.sgn_train_lists(_lib.ptr(counters), _lib.ptr(nd), cap, _lib.ptr(work), _lib.ptr(row_off),
                                 _lib.ptr(feat), _lib.ptr(counts), _lib.ptr(ws), _lib.stream_handle()), "sgn_train_lists")
    torch.cuda.synchronize()
    items = torch.nonzero(nnb[:S] > 0).reshape(-1).to(torch.int32)
    assert int(counts[0]) == items.numel() and int(counts[1]) == int(nnb[:S].sum())
    assert torch.equal(work[:items.numel()].cpu(), items)
    exp_off = torch.cumsum(nnb[:S], 0) - nnb[:S]
    assert torch.equal(row_off[:S].cpu(), exp_off.to(torch.int32))
    assert bool((feat[:S] == 0).all()) and bool((feat[S:] == 3.0).all())


# ---- the whole call table of sgn_x3_gemm ---------------------------------------------------------
# Every distinct call shape train_f32.py builds (ColourStage.__init__, F32Step._build, SG variant included)
# and the shapes that reach the remaining instantiations, each against float64 on the same fp32 operands.
# Operand rows past the counted ones, and weight columns between ncols and ld, hold NaN: a kernel that
# read them would show it.  Outputs are pre-filled and have guard rows after M.

U = 2.0 ** -24
NAN = float("nan")
GUARD = 5


def _weight(g, rows, ld, scale, unaligned):
    """A [rows][ld] fp32 weight matrix as a view of a larger tensor: at element offset 1 (not 16-B aligned: every
    layer after alpha_branch.0's 257 floats in the flat parameter) or 4."""
    store = torch.full((rows * ld + 8,), NAN)
    off = 1 if unaligned else 4
    w = store[off:off + rows * ld].view(rows, ld)
    w.copy_(torch.randn(rows, ld, generator=g) * scale)
    sd = store.to(DEV)
    wd = sd[off:off + rows * ld].view(rows, ld)
    assert (wd.data_ptr() % 16 != 0) == unaligned
    return w, wd, sd


def _shift_of(w):
    m = float(w[~torch.isnan(w)].abs().max())
    return torch.tensor([14 - int(torch.frexp(torch.tensor(m))[1])], dtype=torch.int32, device=DEV)


def _amax_word(x):
    m = float(x.abs().max()) if x.numel() else 0.0
    return torch.tensor([m], dtype=torch.float32, device=DEV).view(torch.int32)


# name: (N, K, A: (ld, csplit, ld2, act), B: (kmajor, ld, ncols), unaligned weight, bias, act, mask, out_cols / out2,
#        delta operand (amax scale), products) -> <KS, WN, P1> and the (HASP2, ACT, O2) flags of k_x3rows.
# Every (KS, WN, P1) the host can choose is reached, and each of the eight (HASP2, ACT, O2) combinations once
# (not their product with the six tile shapes).  As in the step, the mask is as wide as the output (ldm = 128 for
# the colour layers) and amax_out goes with the masked (delta-producing) calls only; amax2: amax_out2 as well.
ROWS_TABLE = {
    # --- production (ColourStage.__init__)
    "colour0_fwd": dict(N=128, K=280, a=(256, 256, 32, 0), b=(0, 280, 280), unal=True, bias=True, act=1),      # <18,W4> HASP2
    "colour2_fwd": dict(N=128, K=128, a=(128, None, 0, 0), b=(0, 128, 128), unal=True, bias=True, act=1),      # <8,W4>
    "colour4_bwd": dict(N=128, K=128, a=(128, None, 0, 0), b=(1, 128, 128), unal=True, mask=True, delta=True),  # <8,W4>
    "colour4_bwd_p1": dict(N=128, K=128, a=(128, None, 0, 0), b=(1, 128, 128), unal=True, mask=True, delta=True,
                           products=1),                                                                        # <8,W4,P1>
    "dfs": dict(N=256, K=128, a=(128, None, 0, 0), b=(1, 280, 256), unal=True, delta=True),                    # <8,W4> ld > ncols
    "dfs_p1": dict(N=256, K=128, a=(128, None, 0, 0), b=(1, 280, 256), unal=True, delta=True, products=1),     # <8,W4,P1>
    # --- production (F32Step._build)
    "z4_fwd": dict(N=256, K=256, a=(256, None, 0, 1), b=(0, 256, 256), unal=True, bias=True),                  # <16,W4> ACT
    "d3": dict(N=256, K=256, a=(256, None, 0, 0), b=(1, 256, 256), unal=True, mask=True, delta=True),           # <16,W4>
    "d2_ext": dict(N=263, K=256, a=(256, None, 0, 0), b=(1, 263, 263), unal=True, mask=True, delta=True, out_cols=256,
                   ldo2=8),                                                                                    # <16,W3> O2
    "sg_d2": dict(N=256, K=256, a=(256, None, 0, 0), b=(1, 352, 256), unal=True, mask=True, delta=True),        # <16,W4> ld > n
    "dx0": dict(N=224, K=256, a=(256, None, 0, 0), b=(1, 284, 224), unal=False, delta=True),                   # <16,W4> ld > n
    # --- the remaining instantiations
    "n96_k64": dict(N=96, K=64, a=(64, None, 0, 0), b=(0, 64, 64), unal=True, bias=True),                      # <8,W3>
    "n263_k288": dict(N=263, K=288, a=(256, 256, 32, 1), b=(0, 288, 288), unal=False, bias=True, act=1, out_cols=256,
                      ldo2=8),                                                                       # <18,W3> HASP2 ACT O2
    "n128_k280_p1": dict(N=128, K=280, a=(280, None, 0, 0), b=(1, 128, 128), unal=True, delta=True, products=1),  # <18,W4,P1>
    # --- the (HASP2, ACT, O2) combinations no call above has
    "p2_act": dict(N=128, K=280, a=(256, 256, 32, 1), b=(0, 280, 280), unal=True, bias=True, act=1),           # <18,W4> HASP2 ACT
    "p2_o2": dict(N=263, K=288, a=(256, 256, 32, 0), b=(0, 288, 288), unal=True, bias=True, out_cols=256, ldo2=8,
                  amax2=True),                                                                     # <18,W3> HASP2 O2
    "act_o2": dict(N=263, K=256, a=(256, None, 0, 1), b=(1, 263, 263), unal=False, mask=True, delta=True, out_cols=256,
                   ldo2=8, amax2=True),                                                            # <16,W3> ACT O2
}


def _run_rows(name, M, d_rows, zero=False, seed=11):
    """One rows-mode call of ROWS_TABLE on M rows of capacity with the device row count d_rows (None: NULL)."""
    t = ROWS_TABLE[name]
    N, K = t["N"], t["K"]
    lda, csplit, ld2, a_act = t["a"]
    kmajor, ldb, b_ncols = t["b"]
    products = t.get("products", 3)
    g = torch.Generator().manual_seed(seed)
    rows = M if d_rows is None else min(d_rows, M)
    scale = 1e-5 if t.get("delta") else 1.0
    # operand a: [M + GUARD][lda] (+ [..][ld2] past csplit); rows past the counted ones are NaN
    a1 = torch.randn(M + GUARD, lda, generator=g) * scale
    a2 = torch.randn(M + GUARD, max(ld2, 1), generator=g) if ld2 else None
    if zero:
        a1.zero_()
    a1[rows:] = NAN
    if a2 is not None:
        a2[rows:] = NAN
        a2[:, K - csplit:] = NAN   # columns past ncols
    k1 = K if csplit is None else csplit
    A = a1[:rows, :k1].double()
    if a_act:
        A = torch.where(A > 0, A, A * 0.01)
    if csplit is not None:
        A = torch.cat([A, a2[:rows, :K - csplit].double()], 1)
    # operand b: the weight, kmajor 0 [N][ld] (columns = k) or kmajor 1 [K][ld] (columns = n); NaN between ncols and ld
    brows = K if kmajor else N
    w, wd, keep = _weight(g, brows, ldb, 0.06, t["unal"])
    w[:, b_ncols:] = NAN
    wd[:, b_ncols:] = NAN
    Wm = w[:, :N].double() if kmajor else w[:, :K].double().t()       # [K][N]
    a1d, a2d = a1.to(DEV), (a2.to(DEV) if a2 is not None else None)
    bias = torch.randn(N, generator=g) if t.get("bias") else None
    ldm = 128 if N == 128 else 256
    mask = torch.randn(M + GUARD, ldm, generator=g) if t.get("mask") else None
    if mask is not None:
        mask[:, ::5] = 0.0    # LeakyReLU'(0) = 0.01
    out_cols = t.get("out_cols", N)
    ldo, ldo2 = out_cols, t.get("ldo2", 0)
    out = torch.full((M + GUARD, ldo), -5.0, device=DEV)
    out2 = torch.full((M + GUARD, ldo2), -5.0, device=DEV) if ldo2 else None
    amax = torch.zeros(2, dtype=torch.int32, device=DEV) if t.get("mask") or t.get("amax2") else None
    amax2 = amax is not None and out2 is not None and t.get("amax2")
    nrows = None if d_rows is None else torch.tensor([d_rows], dtype=torch.int32, device=DEV)
    am_in = _amax_word(a1[:rows]) if t.get("delta") else None
    shift = _shift_of(w)
    biasd = bias.to(DEV) if bias is not None else None
    maskd = mask.to(DEV) if mask is not None else None
    ga = _rows_gemm(_operand(a1d.data_ptr(), lda, K, 0, p2=(a2d.data_ptr() if a2d is not None else None), ld2=ld2,
                             csplit=csplit, act=a_act, amax=(am_in.data_ptr() if am_in is not None else None)),
                    _operand(wd.data_ptr(), ldb, b_ncols, kmajor, shift=shift.data_ptr()), M, N, K,
                    nrows.data_ptr() if nrows is not None else None, out.data_ptr(), ldo,
                    bias=(biasd.data_ptr() if bias is not None else None), act=t.get("act", 0),
                    mask=(maskd.data_ptr() if mask is not None else None), ldm=ldm if mask is not None else 0,
                    out_cols=out_cols, out2=(out2.data_ptr() if out2 is not None else None), ldo2=ldo2,
                    amax_out=(amax.data_ptr() if amax is not None else None),
                    amax_out2=(amax[1:].data_ptr() if amax2 else None))
    ga.products = products
    outs = [out] + ([out2] if out2 is not None else [])
    if M == 0:
        _gemm(ga)
    else:
        _gemm_both(ga, outs, amax)
    torch.cuda.synchronize()
    o, o2 = out.cpu(), (out2.cpu() if out2 is not None else None)
    # exactly `rows` rows written, the guard rows (and out2's columns past N) as they were
    assert bool((o[rows:] == -5.0).all())
    if o2 is not None:
        assert bool((o2[rows:] == -5.0).all()) and bool((o2[:, N - out_cols:] == -5.0).all())
    ref = A @ Wm
    absum = A.abs() @ Wm.abs()
    if bias is not None:
        ref = ref + bias.double()
        absum = absum + bias.double().abs()
    r1 = ref[:, :out_cols]
    if mask is not None:
        r1 = torch.where(mask[:rows, :out_cols] > 0, r1, r1 * 0.01)
    if t.get("act"):
        r1 = torch.where(r1 > 0, r1, r1 * 0.01)
    if amax is not None:
        assert float(amax[:1].view(torch.float32).item()) == (float(o[:rows].abs().max()) if rows else 0.0)
    if amax2:
        assert float(amax[1:].view(torch.float32).item()) == (float(o2[:rows, :N - out_cols].abs().max()) if rows else 0.0)
    if rows == 0:
        return
    if zero:
        assert bool((o[:rows] == 0).all()) and amax is not None and int(amax[0]) == 0
        return
    if products == 1:
        # each operand rounded once to fp16 (relative error <= 2^-11 each: 2^-10 per product, the operands are
        # randn under a power-of-two scale, none underflows), fp32 accumulation of K terms; LReLU' <= 1 after
        bound = (2.0 ** -10 + K * U) * absum[:, :out_cols]
        err = (o[:rows].double() - r1).abs()
        worst = float((err / bound).max())
        print(f"{name} M={M} rows={rows}: products 1 worst error / bound = {worst:.3f}")
        assert worst <= 1.0
        return
    e1 = _rel(o[:rows], r1)
    print(f"{name} M={M} rows={rows}: rel {e1:.2e} ({e1 / REL:.3f} of REL)")
    assert e1 < REL
    if o2 is not None:
        e2 = _rel(o2[:rows, :N - out_cols], ref[:, out_cols:])
        print(f"{name} out2: rel {e2:.2e} ({e2 / REL:.3f} of REL)")
        assert e2 < REL


@pytest.mark.parametrize("name", list(ROWS_TABLE))
def test_x3_gemm_rows_table(name):
    """Every rows-mode call shape at M = 300 rows of capacity (two row tiles), 263 counted (a ragged tile)."""
    _run_rows(name, 300, 263)


@pytest.mark.parametrize("d_rows", [0, 1, 31, 33, 300, 1300, None])
def test_x3_gemm_rows_count(d_rows):
    """The device row count against M: below, equal, far above, and NULL -- exactly min(count, M) rows written
    (the clamp of k_x3rows), the guard rows after them untouched.  On the masked two-output shape."""
    _run_rows("d2_ext", 300, d_rows)


def test_x3_gemm_rows_tile_stride():
    """More row tiles than the launch has row-tile strides (N = 256: 2 column blocks x 128 strides of 256
    rows): the workgroups walk on to a second tile, the last one ragged."""
    _run_rows("d3", 128 * 256 + 257, 128 * 256 + 257)


def test_x3_gemm_rows_zero_delta():
    """All-zero deltas with an amax source word of 0: zeros out, amax_out 0 (no scale from a zero max)."""
    _run_rows("d3", 300, 263, zero=True)


# name: (M, N, A ld, B: (ld, ncols, csplit, ld2, ones_col, act), products, a ones column of A) -> instantiation.
# With a ones column in both operands the product counts the split's rows: the only output that shows whether a
# ones column stops at the split's last row inside a ragged 32-row stage (A's rows past it read 0 anyway).
SPLITK_TABLE = {
    # --- production (ColourStage.__init__)
    "colour4_dw": dict(M=128, N=129, lda=128, b=(128, 128, None, 0, 128, 0)),                       # k_x3tn<1,5>
    "colour4_dw_p1": dict(M=128, N=129, lda=128, b=(128, 128, None, 0, 128, 0), products=1),        # k_x3tn<1,5,P1>
    "colour0_dw": dict(M=128, N=281, lda=128, b=(256, 281, 256, 32, -1, 0)),                        # k_x3tn<1,3>
    "colour0_dw_p1": dict(M=128, N=281, lda=128, b=(256, 281, 256, 32, -1, 0), products=1),         # k_x3tn<1,3,P1>
    # --- production (F32Step._build)
    "block32_dw": dict(M=256, N=257, lda=256, b=(256, 256, None, 0, 256, 1)),                       # k_x3dw<true>, ones column
    "block30_dw": dict(M=256, N=264, lda=256, b=(256, 264, 256, 8, -1, 1)),                         # k_x3dw<true>, p2
    "block10_dw": dict(M=256, N=285, lda=256, b=(288, 285, None, 0, -1, 0)),                        # k_x3dw<false>
    "bpnet_dw": dict(M=256, N=353, lda=256, b=(256, 352, 256, 96, 352, 1)),                         # k_x3dw<true>, p2 + ones
    # --- the remaining instantiations, and columns past ncols inside the output
    "m200_n40": dict(M=200, N=40, lda=200, b=(40, 37, None, 0, 38, 1), a_ones=199),                 # k_x3tn<2,3>, ones x ones
    "m200_n24": dict(M=200, N=24, lda=200, b=(24, 21, None, 0, 22, 0)),                             # k_x3tn<2,1>
    "m100_n24": dict(M=100, N=24, lda=100, b=(24, 21, None, 0, 22, 0)),                             # k_x3tn<1,1>
    "m256_pad4": dict(M=256, N=264, lda=256, b=(256, 260, 256, 8, 262, 1)),                         # k_x3dw<true>: N > ncols
    # ncols inside B's last column quad and N past it: k_x3dw zeroes whole quads only, so the host sends it to
    "m256_pad": dict(M=256, N=264, lda=256, b=(256, 261, 256, 8, 262, 1)),                          # k_x3tn<2,3>
}


def _run_splitk(name, rows, splits, d_null=False, seed=21):
    t = SPLITK_TABLE[name]
    M, N, lda = t["M"], t["N"], t["lda"]
    ldb, ncols, csplit, ld2, ones_col, b_act = t["b"]
    products = t.get("products", 3)
    g = torch.Generator().manual_seed(seed)
    cap = rows if d_null else rows + 37
    a_ones = t.get("a_ones", -1)
    # deltas of the size the step sees, scaled by their amax word; with a ones column in A no scale (a 1 beside
    # 2^14-scaled deltas would leave fp16's range) and values of order 1
    dy = torch.randn(max(cap, 1), lda, generator=g) * (1e-5 if a_ones < 0 else 1.0)
    x1 = torch.randn(max(cap, 1), ldb, generator=g)
    x2 = torch.randn(max(cap, 1), max(ld2, 1), generator=g) if ld2 else None
    k1 = min(ncols, ldb) if csplit is None else csplit
    x1[:, k1:] = NAN                        # columns the operand does not name
    if x2 is not None:
        x2[:, ncols - csplit:] = NAN
    for tns in (dy, x1, x2):
        if tns is not None:
            tns[rows:] = NAN                # rows past the counted ones
    X = x1[:rows, :k1].double()
    if b_act:
        X = torch.where(X > 0, X, X * 0.01)
    if csplit is not None:
        X = torch.cat([X, x2[:rows, :ncols - csplit].double()], 1)
    full = torch.zeros(rows, N, dtype=torch.float64)
    full[:, :ncols] = X
    if ones_col >= 0:
        full[:, ones_col] = 1.0
    D = dy[:rows, :M].double()
    if a_ones >= 0:
        D[:, a_ones] = 1.0
        dy[:, a_ones] = NAN   # never read: the column reads 1
    dyd, x1d, x2d = dy.to(DEV), x1.to(DEV), (x2.to(DEV) if x2 is not None else None)
    nrows = None if d_null else torch.tensor([rows], dtype=torch.int32, device=DEV)
    am = _amax_word(dy[:rows, :M]) if a_ones < 0 else None
    parts = []
    for _ in range(2):   # twice into re-filled partials: bit-identical
        part = torch.full((splits * M * N + 16,), NAN, device=DEV)
        gs = _splitk_gemm(_operand(dyd.data_ptr(), lda, M, 1, ones_col=a_ones, amax=(am.data_ptr() if am is not None else None)),
                          _operand(x1d.data_ptr(), ldb, ncols, 1, p2=(x2d.data_ptr() if x2d is not None else None), ld2=ld2,
                                   csplit=csplit, ones_col=ones_col, act=b_act),
                          M, N, max(cap, 1) if not d_null else rows, nrows.data_ptr() if nrows is not None else None,
                          part.data_ptr(), splits)
        gs.products = products
        _gemm(gs)
        torch.cuda.synchronize()
        parts.append(part.cpu())
    assert torch.equal(parts[0].view(torch.int32), parts[1].view(torch.int32))
    assert bool(torch.isnan(parts[0][splits * M * N:]).all())
    part = parts[0][:splits * M * N].view(splits, M, N)
    assert bool(torch.isfinite(part).all())
    # columns the operand does not name (ncols .. N but the ones column) are zeros in every partial
    pad = [c for c in range(ncols, N) if c != ones_col]
    if pad:
        assert bool((part[:, :, pad] == 0).all()), f"{name}: columns {pad} past ncols are not zero"
    # split s holds the rows [s per, (s + 1) per) of the counted ones, per = the 32-aligned share
    per = (-(-rows // splits) + 31) // 32 * 32
    worst = 0.0
    tot_ref = D.t() @ full
    tot_abs = D.abs().t() @ full.abs()
    scale = float(tot_ref.abs().max()) if rows else 0.0
    for s in range(splits):
        r0, r1 = s * per, min(rows, (s + 1) * per)
        if r1 <= r0:
            assert bool((part[s] == 0).all()), f"{name}: empty split {s} is not zero"
            continue
        ref = D[r0:r1].t() @ full[r0:r1]
        err = (part[s].double() - ref).abs()
        if products == 1:
            bound = (2.0 ** -10 + (r1 - r0) * U) * (D[r0:r1].abs().t() @ full[r0:r1].abs())
            worst = max(worst, float((err / bound.clamp(min=1e-300)).max()))
        else:   # REL against the output tensor's max: the whole gradient's
            worst = max(worst, float(err.max()) / (REL * scale))
    if rows:
        got = part.double().sum(0)
        if products == 1:
            bound = (2.0 ** -10 + rows * U) * tot_abs
            worst = max(worst, float(((got - tot_ref).abs() / bound.clamp(min=1e-300)).max()))
        else:
            worst = max(worst, _rel(got, tot_ref) / REL)
            if ones_col >= 0:   # the bias gradient: the delta's column sums over exactly the counted rows
                assert _rel(got[:, ones_col], D.sum(0)) < REL
    print(f"{name} rows={rows} splits={splits} products={products}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("name", list(SPLITK_TABLE))
def test_x3_gemm_splitk_table(name):
    """Every split-K call shape at 200 rows in 7 splits (one 32-row stage each, the last ragged)."""
    _run_splitk(name, 200, 7)


@pytest.mark.parametrize("rows", [0, 1, 31, 32, 33, 96, 97, 200, 300, 420])
@pytest.mark.parametrize("name", ["block32_dw", "colour4_dw", "m200_n40"])
def test_x3_gemm_splitk_stages(name, rows):
    """Three splits of 0 .. 5 stages of 32 rows, the last stage ragged (the kernels' pipeline prologue, steady
    state and tails), on k_x3dw and k_x3tn."""
    _run_splitk(name, rows, 3)


@pytest.mark.parametrize("name,rows,splits", [("block10_dw", 5000, 84), ("block30_dw", 20011, 84), ("colour0_dw", 5000, 84),
                                              ("bpnet_dw", 2000, 85), ("block32_dw", 1000, 1), ("colour4_dw", 420, 85),
                                              ("m256_pad", 333, 1), ("colour0_dw_p1", 2000, 84)])
def test_x3_gemm_splitk_splits(name, rows, splits):
    """SPLITS_ROWS = 84 (not a multiple of 8: the block order's remainder path), 85, 1."""
    _run_splitk(name, rows, splits)


def test_x3_gemm_splitk_null_count():
    """d_rows NULL: every row of the operands (K) counts."""
    _run_splitk("block32_dw", 97, 3, d_null=True)
    _run_splitk("colour0_dw", 97, 3, d_null=True)


def test_reduce_partials_segments():
    """sgn_reduce_partials, six segments in one launch into one flat buffer that already holds values (the sums
    add onto them): two wide ones (splits >= 512, few outputs: k_reduce_wide), four narrow with 1 / 2 / 3 / 87
    splits, one with ldw > n_in, one without a bias whose extra columns are dropped.  Per element within
    splits u (sum |partials| + |what was there|) -- the value already there is one more term of the fp32 sum --
    everything between and after the destinations unchanged, a second run on a fresh copy bit-identical."""
    g = torch.Generator().manual_seed(4)
    #        splits, M,  N,   n_in, bias_col, ldw
    shapes = [(1024, 1, 257, 256, 256, 256),
              (512, 3, 129, 128, 128, 128),
              (1, 5, 9, 8, 8, 8),
              (2, 4, 12, 8, -1, 8),
              (3, 6, 10, 9, 9, 13),
              (87, 16, 33, 32, 32, 32)]
    offs, pos = [], 3
    for sp, M, N, n_in, bc, ldw in shapes:
        offs.append((pos, pos + M * ldw + 2))
        pos += M * ldw + 2 + M + 3
    flat0 = torch.randn(pos + 11, generator=g) * 0.01
    parts = [torch.randn(sp, M, N, generator=g) for sp, M, N, *_ in shapes]
    pd = [p.to(DEV) for p in parts]
    segs = []
    results = []
    for _ in range(2):
        flat = flat0.to(DEV)
        segs = (_lib.PartialSegment * len(shapes))()
        for i, ((sp, M, N, n_in, bc, ldw), (ow, ob)) in enumerate(zip(shapes, offs)):
            s = segs[i]
            s.part, s.splits, s.M, s.N, s.n_in, s.bias_col, s.ldw = pd[i].data_ptr(), sp, M, N, n_in, bc, ldw
            s.dst_w = flat.data_ptr() + 4 * ow
            s.dst_b = flat.data_ptr() + 4 * ob if bc >= 0 else None
        _lib.check(_lib.lib().sgn_reduce_partials(len(shapes), segs, _lib.stream_handle()), "sgn_reduce_partials")
        torch.cuda.synchronize()
        results.append(flat.cpu())
    assert torch.equal(results[0].view(torch.int32), results[1].view(torch.int32))
    ref = flat0.double().clone()
    bound = torch.zeros_like(ref)
    for p, (sp, M, N, n_in, bc, ldw), (ow, ob) in zip(parts, shapes, offs):
        tot, ab = p.double().sum(0), p.double().abs().sum(0)
        for m in range(M):
            row = slice(ow + m * ldw, ow + m * ldw + n_in)
            ref[row] += tot[m, :n_in]
            bound[row] = sp * U * (ab[m, :n_in] + flat0[row].double().abs())
            if bc >= 0:
                ref[ob + m] += tot[m, bc]
                bound[ob + m] = sp * U * (ab[m, bc] + abs(float(flat0[ob + m])))
    err = (results[0].double() - ref).abs()
    untouched = bound == 0
    assert torch.equal(results[0][untouched].view(torch.int32), flat0[untouched].view(torch.int32))
    assert int(untouched.sum()) > 40 and int((~untouched).sum()) == sum(M * n_in + (M if bc >= 0 else 0)
                                                                          for _, M, _, n_in, bc, _ in shapes)
    worst = float((err[~untouched] / bound[~untouched]).max())
    print(f"reduce_partials: worst error / bound = {worst:.3f}")
    assert worst <= 1.0
