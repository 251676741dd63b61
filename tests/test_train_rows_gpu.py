"""The fp32 training step's six per-row / per-item kernels (csrc/train_x3.hip), each called directly
through the C ABI on the synthetic scene of tests/train_rows_ref.py and compared element by element
with that module's float64 references (proven against autograd in test_train_rows_ref_cpu.py).

Lists come from compact_lists (torch), not sgn_train_lists, so a failure names one kernel.  Every output
buffer is pre-filled with a sentinel and has guard rows after the counted ones, which must stay as they
were.  Cases (K, items): no item, one, two (one wave of k_row_inputs holds two), 777 (odd), and three more
than the kernel's launch covers in one pass (P + 3, every sample with one neighbour): the grid-stride wrap.

Bounds are per element, never a norm; u = 2^-24 (fp32 unit roundoff).  A sum of n fp32 terms, products
rounded first, is within 2 n u sum|terms| of the exact value in any order; that error passes through what
follows with its Lipschitz constant (sigmoid' <= 1/4, softplus' <= 1, LeakyReLU' <= 1).  Each bound
tensor's max must stay below GRAD_TOL_F32 = 1e-4 of the reference tensor's max abs (asserted), so no bound
can grow until it hides a failure.  Each test prints its worst error / bound ratio."""
import ctypes
import functools

import pytest
import torch

import sgnerf_amd  # noqa: F401
from sgnerf_amd import _lib

import train_rows_ref as rr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
U = 2.0 ** -24
CAP = 1e-4          # the project's GRAD_TOL_F32: no bound above this fraction of the reference's scale
PE_ATOL = 2e-6      # sin / cos of an exact fp32 argument (the bar test_colour_inputs_kernel_matches_torch holds)
GUARD = 3
NAN = float("nan")
# one-pass capacities of the launches: work items per pass = workgroups x 4 waves (x 2 for k_row_inputs), from
# ROW_GRID, ROW_HEAD_BLOCKS and HEAD_BLOCKS of csrc/train_x3.hip (a comment there points here).  The two head
# kernels' are checked against their partial counts (test_head_capacities_match_the_launches): a launch that
# grows would otherwise quietly take the P + 3 cases' grid-stride wrap away.
P_INPUTS, P_ROWGRID, P_HEAD, P_CBWD = 32768, 16384, 4096, 1024


def _cases(P):
    return [(8, 0), (8, 1), (8, 2), (3, 777), (1, P + 3)]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _all_nan(t):
    return bool(torch.isnan(t).all())


def _ratio(got, ref, bound, what):
    """max |got - ref| / bound over the elements (an element may differ only where its bound is > 0), printed
    and asserted <= 1."""
    got, ref = got.detach().cpu().double(), ref.double()
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    if ref.numel() == 0:
        print(f"{what}: empty")
        return 0.0
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(ref)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
    err = (got - ref).abs()
    r = torch.where(err > 0, err / bound.clamp(min=1e-300), torch.zeros_like(err))
    worst = float(r.max())
    i = int(r.argmax())
    print(f"{what}: worst error / bound = {worst:.3f} (element {i}: error {float(err.reshape(-1)[i]):.3e}, "
          f"bound {float(bound.reshape(-1)[i]):.3e})")
    assert worst <= 1.0, f"{what}: element {i} off by {float(err.reshape(-1)[i]):.3e}, bound {float(bound.reshape(-1)[i]):.3e}"
    return worst


def _capped(bound, ref, what):
    """The bound tensor stays below CAP x the reference's scale."""
    if ref.numel() == 0:
        return
    b, s = float(torch.as_tensor(bound).max()), float(ref.abs().max())
    assert b < CAP * s, f"{what}: bound {b:.3e} is not below {CAP} x the reference's scale {s:.3e}"


class Case:
    """One (K, items) scene: CPU tensors, compact lists, row indices, and everything on the device."""

    def __init__(self, K, items):
        self.K = K
        self.points, self.camera, self.raydir, self.query = rr.synthetic_scene(K, items)
        q = self.query
        self.S, self.S_cap = q["S"], q["S_cap"]
        work, row_off, counts = rr.compact_lists(q["samp_nnb"], self.S)
        self.work, self.items, self.rows = work, int(counts[0]), int(counts[1])
        assert self.items == items
        self.rs, self.rk, self.pid, self.item = rr.row_index(q, K)
        pad = lambda t, n: torch.cat([t, torch.full((n - t.numel(),), -1, dtype=torch.int32)])  # noqa: E731
        up = lambda t: t.contiguous().to(DEV)  # noqa: E731
        self.d = dict(xyz=up(self.points["xyz"]), emb=up(self.points["embedding"]), color=up(self.points["color"]),
                      dir=up(self.points["dir"]), conf=up(self.points["conf"]), campos=up(self.camera[0]),
                      rot=up(self.camera[1]), raydir=up(self.raydir), samp_ray=up(q["samp_ray"]),
                      samp_locw=up(q["samp_locw"]), samp_nnb=up(q["samp_nnb"]), pidx=up(q["pidx"]),
                      counters=up(q["counters"]), work=up(pad(work, self.S_cap)), row_off=up(pad(row_off, self.S_cap)),
                      counts=up(counts), none=torch.zeros(4, dtype=torch.int32, device=DEV))
        d = self.d
        pt = self.pt = _lib.PointTables()
        pt.xyz, pt.embedding, pt.color, pt.dir, pt.conf = (d[k].data_ptr() for k in ("xyz", "emb", "color", "dir", "conf"))
        pt.n_points = rr.N_POINTS
        pt.campos, pt.camrotc2w, pt.raydir = d["campos"].data_ptr(), d["rot"].data_ptr(), d["raydir"].data_ptr()
        qo = self.qo = _lib.QueryOut()
        qo.ray_ns = qo.ray_soff = qo.samp_d = d["none"].data_ptr()   # not read by these kernels
        for k in ("samp_ray", "samp_nnb", "pidx", "work", "counters", "samp_locw"):
            setattr(qo, k, d[k].data_ptr())

    def gen(self, salt):
        return torch.Generator().manual_seed(1000 * salt + 10 * self.K + self.items % 7)


@functools.lru_cache(maxsize=None)
def case(K, items):
    return Case(K, items)


def _reduce(part, splits, M, N, n_in, bias_col):
    """sgn_reduce_partials of one segment into a zeroed flat buffer, as train_f32._FlatAddr.segment lays it
    out: [M][n_in] weights then [M] biases."""
    flat = torch.zeros(M * n_in + M + 4, device=DEV)
    seg = _lib.PartialSegment()
    seg.part, seg.splits, seg.M, seg.N, seg.n_in, seg.bias_col, seg.ldw = part.data_ptr(), splits, M, N, n_in, bias_col, n_in
    seg.dst_w, seg.dst_b = flat.data_ptr(), flat.data_ptr() + 4 * M * n_in
    _lib.check(_lib.lib().sgn_reduce_partials(1, ctypes.byref(seg), _lib.stream_handle()), "sgn_reduce_partials")
    torch.cuda.synchronize()
    assert bool((flat[M * n_in + M:] == 0).all())
    return flat[:M * n_in].view(M, n_in).cpu(), flat[M * n_in:M * n_in + M].cpu()


def test_head_capacities_match_the_launches():
    """One partial per workgroup, 4 waves each: the P of the two head kernels is what their launches cover."""
    L = _lib.lib()
    assert int(L.sgn_train_head_partial_floats(0)) // (3 * 129) * 4 == P_CBWD
    assert int(L.sgn_train_head_partial_floats(1)) // 257 * 4 == P_HEAD


# ---- sgn_train_row_inputs ------------------------------------------------------------------------

@pytest.mark.parametrize("K,items", _cases(P_INPUTS))
def test_row_inputs(K, items):
    c = case(K, items)
    d, rows = c.d, c.rows
    x0 = torch.full((rows + GUARD, 288), NAN, device=DEV)
    ext = torch.full((rows + GUARD, 8), NAN, device=DEV)
    rw = torch.full((rows + GUARD, 2), NAN, device=DEV)
    vpe = torch.full((items + GUARD, 32), NAN, device=DEV)
    p = _lib.ptr
    _lib.check(_lib.lib().sgn_train_row_inputs(ctypes.byref(c.pt), ctypes.byref(c.qo), K, p(d["row_off"]), p(d["counts"]),
                                               p(x0), p(ext), p(rw), p(vpe), _lib.stream_handle()), "sgn_train_row_inputs")
    torch.cuda.synchronize()
    x0, ext, rw, vpe = x0.cpu(), ext.cpu(), rw.cpu(), vpe.cpu()
    assert _all_nan(x0[rows:]) and _all_nan(ext[rows:]) and _all_nan(rw[rows:]) and _all_nan(vpe[items:])
    x0, ext, rw, vpe = x0[:rows], ext[:rows], rw[:rows], vpe[:items]
    P = c.points
    rx0, rext, rrw, rvpe = rr.row_inputs_ref(P, c.camera, c.raydir, c.query, K)
    # ---- bit-exact parts
    emb32 = P["embedding"][c.pid]
    assert _same_bits(x0[:, :32], emb32)
    assert bool((x0[:, 284] == 1).all()) and bool((x0[:, 285:] == 0).all())
    v32 = c.raydir[c.query["samp_ray"][:c.S].long()]
    vr, pd = v32[c.rs], P["dir"][c.pid]
    assert _same_bits(ext[:, :3], P["color"][c.pid])
    assert _same_bits(ext[:, 3:6], pd - vr)                       # one fp32 subtraction
    dot = (pd[:, 0] * vr[:, 0] + pd[:, 1] * vr[:, 1]) + pd[:, 2] * vr[:, 2]   # single IEEE fp32 operations in this order
    assert _same_bits(ext[:, 6], dot)
    assert bool((ext[:, 7] == 1).all())
    assert bool((vpe[:, 24] == 1).all()) and bool((vpe[:, 25:] == 0).all())

    # ---- PE of an exact fp32 argument (a product with a power of two, or one rounded subtraction times
    # one): against float64 sin / cos of that same fp32 argument
    def pe_of(arg32):   # [n, ch, f] fp32 -> [n, ch * f * 2] float64 (sin, cos) pairs
        a = arg32.double()
        return torch.stack([torch.sin(a), torch.cos(a)], dim=-1).reshape(a.shape[0], a.shape[1] * a.shape[2] * 2)
    worst = {}
    worst["PE(emb)"] = _ratio(x0[:, 32:224], pe_of(emb32[:, :, None] * torch.tensor([1.0, 2.0, 4.0])), PE_ATOL, "x0 PE(emb)")
    if items >= 100:
        assert float((emb32.abs() * 4).max()) >= 2 ** 20   # the rows reach sincos' |x| >= 2^20 branch
    b5 = torch.tensor([1.0, 2.0, 4.0, 8.0, 16.0])
    dw32 = P["xyz"][c.pid] - c.query["samp_locw"][c.rs]           # one fp32 subtraction per component
    worst["PE(world dists)"] = _ratio(x0[:, 224:254], pe_of(dw32[:, :, None] * b5), PE_ATOL, "x0 PE(world dists)")
    # camera-space dists: two fp32 evaluations of one formula in different operation order differ by E-ish
    # (measured here: 4 x the fp32-vs-float64 difference of train.aggregate's formula on these inputs);
    # the PE at frequency 2^f moves by at most 2^f E.  A wrong frequency / channel / formula is off by O(0.1).
    d64 = rr.row_dists(P, c.camera, c.query, K)
    d32 = rr.row_dists(P, c.camera, c.query, K, dtype=torch.float32)
    E = 4 * float((d32[:, 3:].double() - d64[:, 3:]).abs().max()) if rows else 0.0
    print(f"E (camera-space dists, K={K}, items={items}) = {E:.3e}")
    bcam = (PE_ATOL + b5.double() * E)[None, None, :, None].expand(rows, 3, 5, 2).reshape(rows, 30)
    _capped(bcam, rx0[:, 254:284], "PE(camera dists)")   # E is measured here: its bound is capped like the others
    worst["PE(camera dists)"] = _ratio(x0[:, 254:284], rx0[:, 254:284], bcam, "x0 PE(camera dists)")
    arg_v = (v32[c.work.long()][:, :, None] * torch.tensor([1.0, 2.0, 4.0, 8.0])).reshape(items, 12).double()
    worst["PE(viewdir)"] = _ratio(vpe[:, :24], torch.cat([torch.sin(arg_v), torch.cos(arg_v)], 1), PE_ATOL, "vpe")
    worst["rw"] = _ratio(rw, rrw, 32 * U * rrw.abs(), "rw")
    if rows:   # the float64 reference agrees with the fp32-argument forms above (they are the same quantities)
        assert float((rx0[:, 32:224] - pe_of(emb32[:, :, None] * torch.tensor([1.0, 2.0, 4.0]))).abs().max()) < 1e-12
        assert float((rext[:, :7] - torch.cat([P["color"][c.pid], pd - vr, dot[:, None]], 1).double()).abs().max()) < 1e-6
        assert float((rvpe[:, :24] - torch.cat([torch.sin(arg_v), torch.cos(arg_v)], 1)).abs().max()) < 1e-12
    print("row_inputs worst ratios:", {k: round(v, 3) for k, v in worst.items()})


# ---- sgn_train_row_gather ------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [96, 4])
@pytest.mark.parametrize("K,items", _cases(P_ROWGRID))
def test_row_gather(K, items, dim):
    c = case(K, items)
    src = torch.randn(rr.N_POINTS, dim, generator=c.gen(1))
    dst = torch.full((c.rows + GUARD, dim), NAN, device=DEV)
    sd = src.to(DEV)
    p = _lib.ptr
    _lib.check(_lib.lib().sgn_train_row_gather(ctypes.byref(c.qo), K, p(c.d["row_off"]), p(c.d["counts"]), p(sd), dim, p(dst),
                                               _lib.stream_handle()), "sgn_train_row_gather")
    torch.cuda.synchronize()
    dst = dst.cpu()
    assert _same_bits(dst[:c.rows], src[c.pid]) and _all_nan(dst[c.rows:])


# ---- sgn_train_colour_head / _bwd ----------------------------------------------------------------

def _colour_inputs(c):
    """h3 (a LeakyReLU output: its negatives are small), a small W6 and a bias that drives one channel
    towards each end of the sigmoid; d feat with positive colour gradients (the sums below then have
    sum|terms| ~ |sum|, so a relative bound on them means something)."""
    g = c.gen(2)
    h3 = rr.lrelu(torch.randn(c.items + GUARD, 128, generator=g))
    if c.items:
        h3[0, :4] = 0.0   # LeakyReLU'(0) = 0.01
    w6 = torch.randn(3, 128, generator=g) * 0.02
    b6 = torch.tensor([6.0, -6.0, 0.1])
    dfeat = torch.rand(c.S_cap, 4, generator=g) * 1e-3 + 1e-5
    dfeat[:, 0] = torch.randn(c.S_cap, generator=g)
    return h3, w6, b6, dfeat


def _y_bound(h3, w6, b6):
    """|error| of y = h3 W6^T + b6 in fp32: the 128-term dot product in any order, then the bias added to it
    (one rounding of a value no larger than sum|terms| + |b|; counted twice)."""
    dot_abs = h3.double().abs() @ w6.double().abs().t()
    return 2 * 128 * U * dot_abs + 2 * U * (dot_abs + b6.double().abs())


@pytest.mark.parametrize("K,items", _cases(P_ROWGRID))
def test_colour_head(K, items):
    c = case(K, items)
    h3, w6, b6, _ = _colour_inputs(c)
    feat0 = torch.randn(c.S_cap, 4, generator=c.gen(3))
    feat = feat0.to(DEV)
    hd, wd, bd = h3.to(DEV), w6.to(DEV), b6.to(DEV)
    p = _lib.ptr
    _lib.check(_lib.lib().sgn_train_colour_head(ctypes.byref(c.qo), p(c.d["counts"]), p(hd), p(wd), p(bd), p(feat),
                                                _lib.stream_handle()), "sgn_train_colour_head")
    torch.cuda.synchronize()
    feat = feat.cpu()
    is_item = torch.zeros(c.S_cap, dtype=torch.bool)
    is_item[c.work.long()] = True
    assert _same_bits(feat[:, 0], feat0[:, 0])                     # alpha is not this kernel's
    assert _same_bits(feat[~is_item], feat0[~is_item])             # samples without neighbours, and the slack
    ref = rr.colour_head_ref(h3[:items], w6, b6)
    # rgb = sigmoid(y) 1.002 - 0.001: y's error through sigmoid' <= 1/4, then expf (<= 2 ulp), the add, the
    # division, the multiply and the subtraction, each <= 2 u of a value <= 1.002: 8 u in all
    bound = 1.002 * 0.25 * _y_bound(h3[:items], w6, b6) + 8 * U
    _capped(bound, ref, "rgb")
    _ratio(feat[c.work.long(), 1:], ref, bound, f"colour_head rgb (K={K}, items={items})")


def _run_colour_bwd(c, h3, w6, b6, dfeat):
    L = _lib.lib()
    n0 = int(L.sgn_train_head_partial_floats(0))
    dy3 = torch.full((c.items + GUARD, 128), NAN, device=DEV)
    part = torch.full((n0 + 8,), NAN, device=DEV)
    amax = torch.zeros(2, dtype=torch.int32, device=DEV)
    p = _lib.ptr
    _lib.check(L.sgn_train_colour_head_bwd(ctypes.byref(c.qo), p(c.d["counts"]), p(h3), p(w6), p(b6), p(dfeat), p(dy3),
                                           p(amax), p(part), _lib.stream_handle()), "sgn_train_colour_head_bwd")
    torch.cuda.synchronize()
    return dy3, part, amax, n0


@pytest.mark.parametrize("K,items", _cases(P_CBWD))
def test_colour_head_bwd(K, items):
    c = case(K, items)
    h3, w6, b6, dfeat = _colour_inputs(c)
    dev = [t.to(DEV) for t in (h3, w6, b6, dfeat)]
    dy3, part, amax, n0 = _run_colour_bwd(c, *dev)
    dy3b, partb, amaxb, _ = _run_colour_bwd(c, *dev)               # determinism: re-filled buffers, same bits
    assert _same_bits(dy3[:items], dy3b[:items]) and _same_bits(part[:n0], partb[:n0]) and torch.equal(amax, amaxb)
    assert _all_nan(dy3[items:]) and _all_nan(part[n0:]) and int(amax[1]) == 0
    splits = n0 // (3 * 129)
    dW6, db6 = _reduce(part, splits, 3, 129, 128, 128)
    dy3 = dy3[:items].cpu()
    got_amax = float(amax[:1].view(torch.float32).item())
    assert got_amax == (float(dy3.abs().max()) if items else 0.0)  # the word is max |.| of what the kernel wrote
    h, w = h3[:items].double(), w6.double()
    drgb = dfeat[c.work.long(), 1:]
    rdy3, rdW, rdb, ramax = rr.colour_head_bwd_ref(h3[:items], w6, b6, drgb)
    # sigmoid's error: y's through sigmoid' <= 1/4, plus 4 u for expf / add / divide; s (1 - s) has
    # derivative |1 - 2 s| <= 1, so it moves by no more than that, plus 2 u of its value for its two
    # operations; dy4 = d rgb 1.002 s (1 - s) adds two more roundings
    sg = torch.sigmoid(h @ w.t() + b6.double())
    e_sg = 0.25 * _y_bound(h3[:items], w6, b6) + 4 * U
    dy4 = drgb.double() * 1.002 * sg * (1 - sg)
    e_dy4 = drgb.double().abs() * 1.002 * (e_sg + 2 * U * sg * (1 - sg)) + 4 * U * dy4.abs()
    # dy3 = (sum over 3 channels of dy4 w) LReLU': dy4's error times |w|, the 3-term sum, one rounding for x 0.01
    b_dy3 = e_dy4 @ w.abs() + (2 * 3 + 1) * U * (dy4.abs() @ w.abs())
    _capped(b_dy3, rdy3, "dy3")
    r1 = _ratio(dy3, rdy3, b_dy3, f"colour_head_bwd dy3 (K={K}, items={items})")
    assert abs(got_amax - float(ramax)) <= (float(b_dy3.max()) if items else 0.0)
    # dW6 / db6: sums over the items.  A term passes through at most n additions: its wave's chain (the items
    # the wave walks), the workgroup's 4 waves, then the partial reduction (chains of ceil(splits / 4), + 2)
    n = -(-items // P_CBWD) + 4 + -(-splits // 4) + 2
    b_dW = e_dy4.t() @ h.abs() + 2 * n * U * (dy4.abs().t() @ h.abs())
    b_db = e_dy4.sum(0) + 2 * n * U * dy4.abs().sum(0)
    if items:
        _capped(b_dW, rdW, "dW6")
        _capped(b_db, rdb, "db6")
    r2 = _ratio(dW6, rdW, b_dW, "colour_head_bwd dW6")
    r3 = _ratio(db6, rdb, b_db, "colour_head_bwd db6")
    print(f"colour_head_bwd worst ratios: dy3 {r1:.3f} dW6 {r2:.3f} db6 {r3:.3f}")


# ---- sgn_train_row_head --------------------------------------------------------------------------

# z4 rows planted as +- c sign(wa): the alpha logit is then ~ +- c sum over wa > 0 of |wa|
PLANT_C = (14.0, -20.0, 1.5, 2.5, 4.0, 6.0, 8.0, 9.5, 12.2, 12.8)


def _head_inputs(c):
    g = c.gen(4)
    rows, items = c.rows, c.items
    wa = torch.randn(256, generator=g) * 0.02
    ba = torch.tensor([0.3])
    z4 = torch.randn(rows + GUARD, 256, generator=g)
    # (the one- and two-item cases are about the wave's item pairing, not these branches: nothing planted there)
    planted = list(range(len(PLANT_C))) if rows > 100 else []
    for r in planted:
        z4[r] = PLANT_C[r] * torch.sign(wa)
    if rows > len(PLANT_C) + 2:
        z4[len(PLANT_C):len(PLANT_C) + 2, ::7] = 0.0     # LeakyReLU'(0) = 0.01, as torch defines it
        z4[rows - 1, 5:9] = 0.0
    dfs = torch.rand(items + GUARD, 256, generator=g) * 1e-3 + 1e-5   # positive: <h4, d f_s> ~ sum |terms|
    dfeat = torch.randn(c.S_cap, 4, generator=g)
    das = torch.rand(c.S_cap, generator=g) * 1e-2 + 1e-4
    if items > 8:
        das[c.work[5::9].long()] = 0.0                   # items whose d alpha_s is 0
    for r in planted:                                    # the saturated rows must not carry the tensors' max
        das[int(c.work[int(c.item[r])])] *= 0.1
    dfeat[:, 0] = das
    gconf0 = torch.randn(rr.N_POINTS, generator=g) * 1e-4   # the kernel accumulates into it
    return z4, dfs, dfeat, wa, ba, gconf0


def _run_row_head(c, z4, dfs, dfeat, rw, wa, ba, gconf0):
    L = _lib.lib()
    n1 = int(L.sgn_train_head_partial_floats(1))
    zd = z4.to(DEV)
    gc = gconf0.to(DEV)
    part = torch.full((n1 + 8,), NAN, device=DEV)
    amax = torch.zeros(2, dtype=torch.int32, device=DEV)
    p = _lib.ptr
    _lib.check(L.sgn_train_row_head(ctypes.byref(c.pt), ctypes.byref(c.qo), c.K, p(c.d["row_off"]), p(c.d["counts"]), p(zd),
                                    p(dfs), p(dfeat), p(rw), p(wa), p(ba), p(gc), p(amax), p(part), _lib.stream_handle()),
               "sgn_train_row_head")
    torch.cuda.synchronize()
    return zd, gc, part, amax, n1


@pytest.mark.parametrize("K,items", _cases(P_HEAD))
def test_row_head(K, items):
    c = case(K, items)
    rows = c.rows
    z4, dfs, dfeat, wa, ba, gconf0 = _head_inputs(c)
    _, _, rrw, _ = rr.row_inputs_ref(c.points, c.camera, c.raydir, c.query, K)
    rw32 = torch.cat([rrw.float(), torch.full((GUARD, 2), NAN)])     # the kernel's input: the reference's, in fp32
    dev = [t.to(DEV) for t in (dfs, dfeat, rw32, wa, ba)]
    d4, gc, part, amax, n1 = _run_row_head(c, z4, *dev, gconf0)
    d4b, _, partb, amaxb, _ = _run_row_head(c, z4, *dev, gconf0)      # determinism (g_conf is atomic: excluded)
    assert _same_bits(d4[:rows], d4b[:rows]) and _same_bits(part[:n1], partb[:n1]) and torch.equal(amax, amaxb)
    d4 = d4.cpu()
    assert _same_bits(d4[rows:], z4[rows:]) and _all_nan(part[n1:]) and int(amax[1]) == 0
    d4 = d4[:rows]
    splits = n1 // 257
    dWa, dba = _reduce(part, splits, 1, 257, 256, 256)
    got_amax = float(amax[:1].view(torch.float32).item())
    assert got_amax == (float(d4.abs().max()) if rows else 0.0)
    das = dfeat[c.work.long(), 0]
    r_d4, r_dconf, r_dWa, r_dba, r_amax = rr.row_head_ref(c.points, c.camera, c.raydir, c.query, K, z4[:rows], dfs[:items], das,
                                                          rw32[:rows], wa, ba)
    # ---- bounds, in float64 next to the reference
    z, w = z4[:rows].double(), wa.double()
    h4 = rr.lrelu(z)
    wc, wn = rw32[:rows, 0].double(), rw32[:rows, 1].double()
    dfs_r, das_r = dfs[:items].double()[c.item], das.double()[c.item]
    x = h4 @ w + float(ba) - 1.0
    if rows > 100:   # the planted logits reach both ends: softplus' x > 20 branch and a vanishing sigmoid
        assert float(x[0]) > 20 and float(x[1]) < -30 and 2 < float(x[2]) < 20 and 2 < float(x[6]) < 20
        assert float(x[8]) > 20 and bool((z == 0).any()) and bool((z < 0).any())
    sg, al = torch.sigmoid(x), torch.nn.functional.softplus(x)
    # x = za - 1: the 256-term dot product in any order, then the bias and the 1, one rounding each of values no
    # larger than sum|terms| + |ba| + 1
    dot_wa = h4.abs() @ w.abs()
    e_x = 2 * 256 * U * dot_wa + 2 * U * (dot_wa + abs(float(ba)) + 1)
    e_sg = 0.25 * e_x + 4 * U                    # sigmoid' <= 1/4; expf, add, divide
    e_al = e_x + 4 * U * al + 4 * U              # softplus' <= 1; expf, log1pf
    dza = wc * das_r * sg
    e_dza = (wc * das_r).abs() * e_sg + 3 * U * dza.abs()
    # delta4 = (wc d f_s + dza wa) LReLU'(z4): dza's error times |wa|, two products and an add, x 0.01
    t_abs = wc[:, None] * dfs_r.abs() + dza.abs()[:, None] * w.abs()[None, :]
    b_d4 = e_dza[:, None] * w.abs()[None, :] + 5 * U * t_abs
    _capped(b_d4, r_d4, "delta4")
    r1 = _ratio(d4, r_d4, b_d4, f"row_head delta4 (K={K}, items={items})")
    assert abs(got_amax - float(r_amax)) <= (float(b_d4.max()) if rows else 0.0)
    # d conf[p] = g0[p] + sum over p's rows of (<h4, d f_s> + alpha d alpha_s) wn: per row the 256-term dot
    # (257 with the alpha term), alpha's error times |d alpha_s|, the products; then the atomic adds of the
    # point's n rows onto g0 in any order: 2 (n + 1) u (|g0| + sum |terms|)
    dot_abs = (h4.abs() * dfs_r.abs()).sum(-1) + (al * das_r).abs()
    e_row = (2 * 258 * U * dot_abs + e_al * das_r.abs()) * wn + 2 * U * dot_abs * wn
    n_p = torch.zeros(rr.N_POINTS, dtype=torch.float64).index_add(0, c.pid, torch.ones(rows, dtype=torch.float64))
    zp = lambda: torch.zeros(rr.N_POINTS, dtype=torch.float64)  # noqa: E731
    b_gc = zp().index_add(0, c.pid, e_row) + 2 * (n_p + 1) * U * (gconf0.double().abs() + zp().index_add(0, c.pid, dot_abs * wn))
    ref_gc = gconf0.double() + r_dconf
    _capped(b_gc, ref_gc, "g_conf")
    r2 = _ratio(gc.cpu(), ref_gc, b_gc.clamp(min=1e-300), "row_head g_conf")
    assert _same_bits(gc.cpu()[n_p == 0], gconf0[n_p == 0])    # points no row names: untouched
    # dWa / dba: sums over the rows.  A term passes through at most n additions: its wave's chain (the rows of
    # the items the wave walks), the workgroup's 4 waves, then the partial reduction (ceil(splits / 4) + 2
    # covers both of its kernels)
    n = -(-items // P_HEAD) * K + 4 + -(-splits // 4) + 2
    b_dWa = e_dza @ h4.abs() + 2 * n * U * (dza.abs() @ h4.abs())
    b_dba = (e_dza.sum() + 2 * n * U * dza.abs().sum()).reshape(1)
    if rows:
        _capped(b_dWa, r_dWa, "dWa")
        _capped(b_dba, r_dba, "dba")
    r3 = _ratio(dWa.reshape(-1), r_dWa, b_dWa.clamp(min=1e-300), "row_head dWa")
    r4 = _ratio(dba, r_dba, b_dba.clamp(min=1e-300), "row_head dba")
    print(f"row_head worst ratios: delta4 {r1:.3f} g_conf {r2:.3f} dWa {r3:.3f} dba {r4:.3f}")


# ---- sgn_train_row_tail --------------------------------------------------------------------------

@pytest.mark.parametrize("K,items", _cases(P_ROWGRID))
def test_row_tail(K, items):
    c = case(K, items)
    rows, N = c.rows, rr.N_POINTS
    g = c.gen(5)
    dx0 = torch.rand(rows + GUARD, 224, generator=g) * 1e-3 + 1e-5    # positive: a point's rows add up, not cancel
    dext = torch.rand(rows + GUARD, 8, generator=g) * 1e-3 + 1e-5
    g0 = [torch.randn(N, n, generator=g) * 1e-4 for n in (32, 3, 3)]   # the kernel accumulates into them
    ge, gcol, gdir = (t.to(DEV) for t in g0)
    gconf = torch.full((N,), NAN, device=DEV)                          # not this kernel's
    grads = _lib.PointGrads(ge.data_ptr(), gcol.data_ptr(), gdir.data_ptr(), gconf.data_ptr())
    p = _lib.ptr
    xd, ed = dx0.to(DEV), dext.to(DEV)
    _lib.check(_lib.lib().sgn_train_row_tail(ctypes.byref(c.pt), ctypes.byref(c.qo), K, p(c.d["row_off"]), p(c.d["counts"]),
                                             p(xd), p(ed), ctypes.byref(grads), _lib.stream_handle()), "sgn_train_row_tail")
    torch.cuda.synchronize()
    assert _all_nan(gconf)
    r_e, r_c, r_d = rr.row_tail_ref(c.points, c.camera, c.raydir, c.query, K, dx0[:rows], dext[:rows])
    n_p = torch.zeros(N, dtype=torch.float64).index_add(0, c.pid, torch.ones(rows, dtype=torch.float64))[:, None]
    acc = lambda t: torch.zeros(N, t.shape[1], dtype=torch.float64).index_add(0, c.pid, t)  # noqa: E731
    # d emb per row: dx0[c] + sum over f < 3 of (d sin cos(e 2^f) - d cos sin(e 2^f)) 2^f: 7 terms, each sin /
    # cos within PE_ATOL; then the point's n rows added onto g0 by atomics in any order
    dd = dx0[:rows].double()
    dpe = dd[:, 32:].reshape(rows, 32, 3, 2).abs()
    bands = torch.tensor([1.0, 2.0, 4.0], dtype=torch.float64)
    t_abs = dd[:, :32].abs() + (dpe.sum(-1) * bands).sum(-1)           # sum |terms| with |sin|, |cos| <= 1
    e_row = PE_ATOL * (dpe.sum(-1) * bands).sum(-1) + 2 * 7 * U * t_abs
    b_e = acc(e_row) + 2 * (n_p + 1) * U * (g0[0].double().abs() + acc(t_abs))
    de = dext[:rows].double()
    b_c = 2 * (n_p + 1) * U * (g0[1].double().abs() + acc(de[:, :3].abs()))
    # d dir per row: dext[3 + j] + dext[6] v_j: a product and an add
    td = de[:, 3:6].abs() + de[:, 6:7].abs()
    b_d = acc(3 * U * td) + 2 * (n_p + 1) * U * (g0[2].double().abs() + acc(td))
    out = {}
    for name, got, ref, b, base in (("g_emb", ge, r_e, b_e, g0[0]), ("g_color", gcol, r_c, b_c, g0[1]),
                                    ("g_dir", gdir, r_d, b_d, g0[2])):
        full = base.double() + ref
        _capped(b, full, name)
        out[name] = round(_ratio(got.cpu(), full, b.clamp(min=1e-300), f"row_tail {name} (K={K}, items={items})"), 3)
        assert _same_bits(got.cpu()[n_p[:, 0] == 0], base[n_p[:, 0] == 0])   # points no row names: untouched
    print("row_tail worst ratios:", out)
