"""GPU tests of the Adam kernels (csrc/optim.hip) through the C ABI and through PointAdam:

* sgn_adam_step / sgn_adam_step_multi per element against the float64 step of tests/adam_ref.py on the
  kernel's own fp32 inputs, under the operation-count bound of adam_ref.adam_step_bound (u = 2^-24),
  on planted gradient classes that straddle eps;
* sgn_adam_rows across kSchedWin (the constants' LDS window), at the corners of its list contract and
  past one pass of either of its launches, bit for bit against the dense kernel;
* PointAdam(rows=True) over 1,100 steps with rows that sleep for more than kSchedWin steps, bit for
  bit against the dense PointAdam.

Every buffer a kernel writes ends in guard words that must keep their sentinel."""
import ctypes

import pytest
import torch

import adam_ref as ar
from sgnerf_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BETAS, EPS = (0.9, 0.999), 1e-8

# The grid caps of csrc/optim.hip's host code (a comment there points here).
N_PASS = 4096 * 256 * 2 * 4     # ADAM_GRID workgroups x 256 threads x 2 float4 per trip x 4 elements (k_adam)
CLAIM_PASS = 1024 * 512         # CLAIM_GRID x CLAIM_PER entries (k_rows_claim)
UPDATE_PASS = 16384 * 256       # UPDATE_GRID x 256 (row, element) pairs (k_rows_update)
SCHED_WIN = 1024                # kSchedWin: the steps whose constants k_rows_update stages in LDS
INT32_MAX = 2 ** 31 - 1

GUARD = 32
FSENT, ISENT = -7.0e33, 0x5A5A5A5A


def _guarded(n, dtype=torch.float32):
    """(base, view): n elements followed by GUARD sentinel words."""
    base = torch.full((n + GUARD,), FSENT if dtype.is_floating_point else ISENT, dtype=dtype, device=DEV)
    return base, base[:n]


def _guards_ok(bases_and_n):
    for base, n in bases_and_n:
        s = FSENT if base.dtype.is_floating_point else ISENT
        assert bool((base[n:] == s).all()), "a guard word was overwritten"


def _arr(ts):
    return (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def _dense_launch(ps, gs, ms, vs, lr, step, zero_grad, single=False):
    L = _lib.lib()
    if single:
        assert len(ps) == 1
        _lib.check(L.sgn_adam_step(_lib.ptr(ps[0]), _lib.ptr(gs[0]), _lib.ptr(ms[0]), _lib.ptr(vs[0]), ps[0].numel(),
                                   lr, BETAS[0], BETAS[1], EPS, step, zero_grad, _lib.stream_handle()), "sgn_adam_step")
        return
    n = len(ps)
    _lib.check(L.sgn_adam_step_multi(n, _arr(ps), _arr(gs), _arr(ms), _arr(vs),
                                     (ctypes.c_int64 * n)(*[p.numel() for p in ps]), lr, BETAS[0], BETAS[1], EPS,
                                     step, zero_grad, _lib.stream_handle()), "sgn_adam_step_multi")


# ---- 1. the dense kernel per element ---------------------------------------------------------------
# planted classes by element index % 10: 0 g = 0 with m = v = 0; 1-4 |g| = 1e-12 .. 1e-6 (sqrt(v) / bc2_sqrt
# from 1e-4 eps to 100 eps: eps's place and bc2_sqrt decide p); 5-7 |g| = 1e-3, 1, 1e4; 8 g = 0 with the
# moments of an earlier large gradient; 9 a normal draw.  Signs are random.  Classes 1-7 and 9 carry
# moments of their own magnitude in every second group of ten and start from m = v = 0 in the others.
MAGS = (0.0, 1e-12, 1e-10, 1e-8, 1e-6, 1e-3, 1.0, 1e4, 0.0, 1.0)
RAGGED8 = (38_401, 3_601, 7, 1_201, 5, 2, 1_023, 333)


def _planted(n, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    rnd = lambda: torch.rand(n, generator=g, device=DEV, dtype=torch.float64)  # noqa: E731
    i = torch.arange(n, device=DEV)
    cls = i % 10
    mags = torch.tensor(MAGS, dtype=torch.float64, device=DEV)[cls]
    sign = torch.where(rnd() < 0.5, -1.0, 1.0)
    normal = torch.randn(n, generator=g, device=DEV, dtype=torch.float64)
    gr = torch.where(cls == 9, normal, sign * mags)
    scale = torch.where(cls == 8, torch.full_like(mags, 3e3), mags)
    carried = ((cls == 8) | (((i // 10) % 2 == 1) & (cls != 0))).double()
    m = (2 * rnd() - 1) * scale * carried
    v = (0.05 + rnd()) * scale * scale * carried
    p = torch.randn(n, generator=g, device=DEV, dtype=torch.float64)
    return p.float(), gr.float(), m.float(), v.float(), cls


def _check_step(name, out, inp, lr, step, worst):
    """Kernel outputs (p, m, v) against the float64 step on `inp` = (p, g, m, v) under the bound, and the
    bound against DESIGN §4's bar for this kernel."""
    ref = ar.adam_step(*inp, lr, BETAS, EPS, step)
    bnd = ar.adam_step_bound(*inp, lr, BETAS, EPS, step)
    for k, o, r, b in zip("pmv", out, ref, bnd):
        err = (o.double() - r).abs()
        ratio = float((err / b).max())
        worst[k] = max(worst.get(k, 0.0), ratio)
        assert ratio <= 1.0, f"{name} {k}: error / bound {ratio:.3f} at element {int((err / b).argmax())}"
    assert float(bnd[0].max()) < 1e-6 * max(float(ref[0].abs().max()), lr)
    assert float(bnd[1].max()) < 1e-6 * float(ref[1].abs().max())
    assert float(bnd[2].max()) < 1e-6 * float(ref[2].abs().max())


@pytest.mark.parametrize("step", [1, 2, 10, 1000, 100000])
@pytest.mark.parametrize("sizes", [(3,), (1_003,), (N_PASS + 7,), RAGGED8], ids=["n3", "n1003", "npass7", "ragged8"])
def test_dense_step_per_element_against_float64(sizes, step):
    assert all(n % 4 for n in RAGGED8) and N_PASS + 7 > N_PASS   # ragged tails; a second trip of k_adam's loop
    lr = 1.7e-3 * 0.97 ** (step % 7)
    worst = {}
    for zero_grad in (0, 1):
        bufs, views, inps, classes = [], [], [], []
        for t, n in enumerate(sizes):
            p, gr, m, v, cls = _planted(n, 1000 * step + 10 * t + zero_grad)
            bv = [_guarded(n) for _ in range(4)]
            for (_, view), x in zip(bv, (p, gr, m, v)):
                view.copy_(x)
            bufs += [(b, n) for b, _ in bv]
            views.append([view for _, view in bv])
            inps.append((p, gr, m, v))
            classes.append(cls)
        cols = list(zip(*views))
        _dense_launch(cols[0], cols[1], cols[2], cols[3], lr, step, zero_grad)
        torch.cuda.synchronize()
        _guards_ok(bufs)
        for t, (vw, inp, cls) in enumerate(zip(views, inps, classes)):
            _check_step(f"tensor {t} (n = {sizes[t]})", (vw[0], vw[2], vw[3]), inp, lr, step, worst)
            z = cls == 0   # g = m = v = 0: p - 0 / eps keeps p's bits
            assert torch.equal(vw[0][z].view(torch.int32), inp[0][z].view(torch.int32))
            assert not bool(vw[2][z].any()) and not bool(vw[3][z].any())
            if zero_grad:
                assert not bool(vw[1].any())
            else:
                assert torch.equal(vw[1].view(torch.int32), inp[1].view(torch.int32))
        if len(sizes) == 1:   # the single-tensor entry: the same bits
            n = sizes[0]
            bv = [_guarded(n) for _ in range(4)]
            for (_, view), x in zip(bv, inps[0]):
                view.copy_(x)
            _dense_launch([bv[0][1]], [bv[1][1]], [bv[2][1]], [bv[3][1]], lr, step, zero_grad, single=True)
            torch.cuda.synchronize()
            _guards_ok([(b, n) for b, _ in bv])
            for j in range(4):
                assert torch.equal(bv[j][1].view(torch.int32), views[0][j].view(torch.int32))
    print(f"adam dense sizes={sizes if len(sizes) < 3 else 'ragged8'} step={step}: worst error / bound "
          + " ".join(f"{k} {w:.3f}" for k, w in worst.items()))


# ---- the row-sparse entry, called directly ---------------------------------------------------------
WIDTHS = (32, 3, 3, 1)


class Rows:
    """The point group twice -- dense (sgn_adam_step_multi every step) and row-sparse (sgn_adam_rows,
    called directly) -- with a host model of the list contract: which rows a launch brings forward
    (d_last), what its pend list holds and how many list-1 ids lie past the table."""

    def __init__(self, n_rows, packed, seed, sched_steps=64):
        self.n, self.packed = n_rows, packed
        g = torch.Generator().manual_seed(seed)
        self.gen = g
        self.bases = []
        mk = lambda numel, dtype=torch.float32: self._mk(numel, dtype)  # noqa: E731
        p0 = [torch.randn(n_rows, w, generator=g) for w in WIDTHS]
        self.dp, self.dm, self.dv, self.sp, self.sm, self.sv = [], [], [], [], [], []
        if packed:   # the narrow tensors' moments in one [n, 16] buffer: m in columns 0-7, v in 8-15
            self.mv = mk(n_rows * 16).view(n_rows, 16)
            self.mv[:, :7] = 0.0
            self.mv[:, 8:15] = 0.0
        off = 0
        for i, w in enumerate(WIDTHS):
            for lst in (self.dp, self.sp):
                t = mk(n_rows * w).view(n_rows, w)
                t.copy_(p0[i])
                lst.append(t)
            for lst in (self.dm, self.dv):
                lst.append(mk(n_rows * w).view(n_rows, w).zero_())
            if packed and w <= 8:
                self.sm.append(self.mv[:, off:off + w])
                self.sv.append(self.mv[:, 8 + off:8 + off + w])
                off += w
            else:
                self.sm.append(mk(n_rows * w).view(n_rows, w).zero_())
                self.sv.append(mk(n_rows * w).view(n_rows, w).zero_())
        self.stride = (ctypes.c_int32 * 4)(*[16 if packed and w <= 8 else w for w in WIDTHS]) if packed else None
        self.width = (ctypes.c_int32 * 4)(*WIDTHS)
        self.last = mk(n_rows, torch.int32).zero_()
        self.claim = mk(n_rows, torch.int32).zero_()
        self.claim2 = mk(n_rows, torch.int32).zero_()
        self.sched = mk(2 * sched_steps).zero_()
        self.tag = 0
        self.t = 0                                            # the dense side's step
        self.exp_last = torch.zeros(n_rows, dtype=torch.long)   # the model's d_last
        self.dg = [torch.zeros(n_rows, w, device=DEV) for w in WIDTHS]
        self.sg = [torch.zeros(n_rows, w, device=DEV) for w in WIDTHS]

    def _mk(self, numel, dtype):
        base, view = _guarded(numel, dtype)
        self.bases.append((base, numel))
        return view

    def brought(self, rows=None, count=None, is64=0, mul=1, n_max=None, row0=1, rows2=None, count2=0, n_max2=0):
        """The model: (rows brought forward, pend rows, list-1 ids >= n_rows) of a launch."""
        n_max = (self.n if rows is None else rows.numel()) if n_max is None else n_max
        assert n_max <= (self.n if rows is None else rows.numel())   # the launch reads d_rows[0 .. n_max)
        n1 = n_max if count is None else min(n_max, count * mul)
        l1 = torch.arange(n1) if rows is None else rows[:n1].long()
        l2 = rows2[:min(n_max2, count2)].long() if rows2 is not None else torch.zeros(0, dtype=torch.long)
        ok = lambda l: l[(l >= 0) & (l < self.n)]  # noqa: E731
        zero = torch.zeros(1 if row0 else 0, dtype=torch.long)
        return (torch.unique(torch.cat([ok(l1), ok(l2), zero])), torch.unique(torch.cat([ok(l1), zero])),
                int((l1 >= self.n).sum()))

    def grads_on(self, rows, scale=1.0):
        """A gradient on `rows` (a third of them stay zero, as rows a step lists but does not move)."""
        rows = rows[torch.rand(rows.numel(), generator=self.gen) < 0.67]
        for d, s, w in zip(self.dg, self.sg, WIDTHS):
            gr = torch.zeros(self.n, w)
            gr[rows] = torch.randn(rows.numel(), w, generator=self.gen) * scale
            d.copy_(gr)
            s.copy_(gr)

    def dense_step(self, lr):
        self.t += 1
        _dense_launch(self.dp, self.dg, self.dm, self.dv, lr, self.t, 1)

    def sparse(self, step, apply, lr=0.0, rows=None, count=None, is64=0, mul=1, n_max=None, row0=1, rows2=None,
               count2=0, n_max2=0, pend=True):
        """One sgn_adam_rows launch, then the model's checks: d_last, the compact list's length, the pend
        list exactly (nothing written past its count), the out-of-table count, every guard word."""
        L = _lib.lib()
        n_max = (self.n if rows is None else rows.numel()) if n_max is None else n_max
        assert rows2 is None or n_max2 <= rows2.numel()
        got, pend_rows, oob = self.brought(rows, count, is64, mul, n_max, row0, rows2, count2, n_max2)
        self.exp_last[got] = step
        entries = n_max + (n_max2 if rows2 is not None else 0) + (1 if row0 else 0)
        ws_bytes = int(L.sgn_adam_rows_workspace_bytes(min(entries, self.n)))
        wb, ws = _guarded(ws_bytes // 4, torch.int32)
        d_rows = rows.to(DEV) if rows is not None else None
        d_rows2 = rows2.to(DEV) if rows2 is not None else None
        d_count = None
        if count is not None:   # the count in word 0, a poisoned word after it (an int32 count read as int64)
            d_count = torch.tensor([count, 0] if is64 else [count, 123456], dtype=torch.int64 if is64 else torch.int32,
                                   device=DEV)
        d_count2 = torch.tensor([count2], dtype=torch.int64, device=DEV) if rows2 is not None else None
        pb = pv = None
        pend_bytes = 0
        if pend:
            pend_bytes = int(L.sgn_adam_rows_pend_bytes(min(n_max + 1, self.n)))
            pb, pv = _guarded(pend_bytes // 4, torch.int32)
            pv.fill_(ISENT)
        self.tag += 1
        _lib.check(L.sgn_adam_rows(
            4, _arr(self.sp), _arr(self.sg) if apply else None, _arr(self.sm), _arr(self.sv), self.width, self.stride,
            self.n, _lib.ptr(d_rows), _lib.ptr(d_count), is64, mul, n_max, row0, _lib.ptr(d_rows2), _lib.ptr(d_count2),
            n_max2, _lib.ptr(self.last), _lib.ptr(self.claim), _lib.ptr(self.claim2), self.tag, _lib.ptr(ws), ws_bytes,
            _lib.ptr(pv), pend_bytes, _lib.ptr(self.sched), lr, BETAS[0], BETAS[1], EPS, step, apply, 1,
            _lib.stream_handle()), "sgn_adam_rows")
        torch.cuda.synchronize()
        _guards_ok(self.bases + [(wb, ws_bytes // 4)] + ([(pb, pend_bytes // 4)] if pend else []))
        if self.packed:   # the packed buffer's unused columns
            assert bool((self.mv[:, 7] == FSENT).all()) and bool((self.mv[:, 15] == FSENT).all())
        assert torch.equal(self.last.cpu().long(), self.exp_last)
        assert int(ws[0]) == got.numel()
        if pend:
            n_p = int(pv[:2].view(torch.int64).item())
            assert n_p == pend_rows.numel()
            assert int(pv[2:4].view(torch.int64).item()) == oob
            assert torch.equal(torch.sort(pv[4:4 + n_p].cpu().long()).values, pend_rows)
            assert bool((pv[4 + n_p:] == ISENT).all()), "the pend list was written past its count"
        return got, pv

    def both_step(self, lr, scale=1.0, **lists):
        """One training step on both sides: the gradient lives on rows the sparse launch brings forward."""
        got, _, _ = self.brought(**lists)
        self.grads_on(got, scale)
        self.dense_step(lr)
        out = self.sparse(self.t, 1, lr=lr, **lists)
        self.check_current()
        return out

    def check_current(self):
        """Rows the model holds at the dense step equal the dense state bit for bit."""
        idx = torch.nonzero(self.exp_last == self.t).reshape(-1).to(DEV)
        assert idx.numel() > 0
        for d, s in zip(self.dp + self.dm + self.dv, self.sp + self.sm + self.sv):
            assert torch.equal(d[idx].view(torch.int32), s[idx].contiguous().view(torch.int32))
        for s in self.sg:   # an applied row's gradient is cleared; no other row had one
            assert not bool(s.any())

    def flush_and_check(self):
        self.sparse(self.t, 0, pend=False)
        assert bool((self.exp_last == self.t).all())
        self.check_current()

    def table(self, n_s, K=8, hi=None):
        """A neighbour table's list as a query leaves it: -1 slots, duplicates."""
        hi = self.n if hi is None else hi
        tb = torch.randint(0, hi, (n_s, K), generator=self.gen, dtype=torch.int32)
        tb[torch.rand(n_s, K, generator=self.gen) < 0.3] = -1
        tb[: n_s // 4, 1] = tb[: n_s // 4, 0]
        return tb.reshape(-1)


def _warm(r, steps=3):
    """A dense-equivalent first step on every row, then sparse steps that leave most rows behind."""
    r.both_step(2e-3)                                        # d_rows = NULL: rows 0 .. n_max - 1
    for it in range(steps):
        r.both_step(2e-3 * 0.97 ** it, scale=10.0 ** (it % 3 - 1), rows=r.table(max(2, r.n // 40)))


CORNERS = ["count64", "n_max_cuts", "no_row0", "list2_overlap", "ids_past_table", "only_minus_one"]


@pytest.mark.parametrize("packed", [True, False], ids=["packed_mv", "mv_stride_null"])
@pytest.mark.parametrize("corner", CORNERS)
def test_rows_contract_corners_match_dense_bit_for_bit(corner, packed):
    """The corners of sgn_adam_rows' list contract at n_rows = 5003 (ten workgroups of the claim launch),
    each inside a run of sparse steps and ended by a flush, against the dense kernel bit for bit;
    mv_stride_null runs the same with unpacked moments and mv_stride = NULL."""
    n = 5_003
    r = Rows(n, packed, seed=len(corner) + 2 * packed)
    _warm(r)
    g = r.gen
    if corner == "count64":      # an int64 device count, count_mul = 1; entries past it name rows it must not touch
        lst = r.table(300)
        cnt = 1_501
        lst[cnt:] = torch.randint(0, n, (lst.numel() - cnt,), generator=g, dtype=torch.int32)
        got, _ = r.both_step(1.5e-3, rows=lst, count=cnt, is64=1, mul=1, n_max=lst.numel())
        assert got.numel() < torch.unique(lst[lst >= 0]).numel()
    elif corner == "n_max_cuts":   # n_max below count x count_mul: the entries past it stay behind
        lst = r.table(300)
        got, _ = r.both_step(1.5e-3, rows=lst, count=300, mul=8, n_max=1_000)
        past = torch.unique(lst[1_000:][lst[1_000:] >= 0].long())
        behind = past[r.exp_last[past] < r.t]
        assert behind.numel() > 100 and 1_000 < 300 * 8
    elif corner == "no_row0":      # row 0 is brought forward only if listed
        lst = r.table(300)
        lst[lst == 0] = 1
        r.both_step(1.5e-3, rows=lst, n_max=lst.numel(), row0=0)
        assert int(r.exp_last[0]) == r.t - 1
        lst = r.table(300)
        lst[17] = 0
        r.both_step(1.4e-3, rows=lst, n_max=lst.numel(), row0=0)
        assert int(r.exp_last[0]) == r.t
    elif corner == "list2_overlap":   # list 2 (a pend list) shares half its rows with list 1: each row once
        lst = r.table(300)
        l1 = torch.unique(lst[lst >= 0])
        half = l1[torch.randperm(l1.numel(), generator=g)[: l1.numel() // 2]]
        other = torch.randint(0, n, (half.numel(),), generator=g, dtype=torch.int32)
        l2 = torch.cat([half, other])[torch.randperm(2 * half.numel(), generator=g)].to(torch.int32)
        tail = torch.randint(0, n, (64,), generator=g, dtype=torch.int32)   # past list 2's count
        got, _ = r.both_step(1.5e-3, rows=lst, n_max=lst.numel(), rows2=torch.cat([l2, tail]), count2=l2.numel(),
                             n_max2=l2.numel() + 64)
        assert half.numel() > 500 and got.numel() < l1.numel() + l2.numel()
    elif corner == "ids_past_table":   # ids n_rows, n_rows + 5, INT32_MAX among valid ones
        lst = r.table(300)
        bad = torch.tensor([n, n + 5, INT32_MAX, n, INT32_MAX], dtype=torch.int32)
        pos = torch.randperm(lst.numel(), generator=g)[: bad.numel()]
        lst[pos] = bad
        _, pv = r.both_step(1.5e-3, rows=lst, n_max=lst.numel())
        assert int(pv[2:4].view(torch.int64).item()) == bad.numel()
    else:   # a list of only -1: row 0 alone, then nothing at all
        lst = torch.full((777,), -1, dtype=torch.int32)
        got, _ = r.both_step(1.5e-3, rows=lst, n_max=lst.numel())
        assert got.tolist() == [0]
        before = [x.clone() for x in r.sp + r.sm + r.sv]
        got, _ = r.sparse(r.t, 0, rows=lst, n_max=lst.numel(), row0=0)
        assert got.numel() == 0
        for x, y in zip(before, r.sp + r.sm + r.sv):
            assert torch.equal(x.view(torch.int32), y.contiguous().view(torch.int32))
    r.both_step(1.3e-3, rows=r.table(100))   # one more ordinary step, then every row
    r.flush_and_check()


def test_rows_claim_loop_wraps_on_a_long_list():
    """A list of CLAIM_PASS + 3 entries over 5003 rows (each row ~100 times): k_rows_claim's grid-stride
    loop takes a second trip, whose entries must still be claimed once."""
    n = 5_003
    r = Rows(n, True, seed=11)
    _warm(r)
    n_list = CLAIM_PASS + 3
    assert n_list + 1 > CLAIM_PASS   # entries (list 1 + row 0) exceed one pass of the claim launch
    lst = torch.randint(0, n - 1, (n_list,), generator=r.gen, dtype=torch.int32)
    lst[torch.rand(n_list, generator=r.gen) < 0.3] = -1
    lst[:CLAIM_PASS][lst[:CLAIM_PASS] >= n - 3] = 5     # rows n - 3, n - 2 only ever appear in the second trip
    lst[CLAIM_PASS] = n - 3
    lst[CLAIM_PASS + 1] = n - 2
    lst[CLAIM_PASS + 2] = n - 3
    got, _ = r.both_step(1.5e-3, rows=lst, n_max=n_list)
    assert int(r.exp_last[n - 3]) == r.t and int(r.exp_last[n - 2]) == r.t and int(r.exp_last[n - 1]) < r.t
    r.flush_and_check()


def test_rows_update_loop_wraps_on_a_flush():
    """A d_rows = NULL flush at n_rows = 107,600: 107,600 x 39 (row, element) pairs exceed one pass of
    k_rows_update's launch, and the claim launch runs 211 workgroups over n_max = n_rows."""
    n = 107_600
    assert n * sum(WIDTHS) > UPDATE_PASS and n > 512
    r = Rows(n, True, seed=12)
    _warm(r)
    assert int((r.exp_last < r.t).sum()) > n // 2   # most rows have steps to replay
    r.flush_and_check()
    # and an applied step over every row: the same wrap with the gradient read
    r.both_step(1.2e-3)
    assert bool((r.exp_last == r.t).all())


# ---- 2. one replay launch across the LDS window ----------------------------------------------------
def _lr_at(k):
    return 2e-3 * 0.9995 ** k


def _sched_table(T):
    """d_sched for steps 1 .. T as the apply launches write it: float(lr_k / bc1_k), float(sqrt(bc2_k)),
    formed in double as the host code forms them."""
    rows = [ar.adam_constants(_lr_at(k), BETAS, k) for k in range(1, T + 1)]
    return torch.tensor(rows, dtype=torch.float64).float().reshape(-1)


@pytest.mark.parametrize("apply", [0, 1], ids=["replay", "replay_then_step"])
def test_rows_replay_across_the_sched_window(apply):
    """One launch over d_rows = NULL at T = 3000 with d_last planted on both sides of lo = upto -
    kSchedWin: rows below it read the table for steps last + 1 .. lo and the LDS window after, rows
    at or above it the window alone.  Against the lazy float64 model under the summed per-step bounds
    and, bit for bit, against T - last dense launches at g = 0; apply: the launch then takes step
    T + 1 with a planted gradient."""
    T, n = 3000, 64
    upto = T
    lo = upto - SCHED_WIN
    planted = [0, 1, T - 1026, T - 1025, T - 1024, T - 1023, T - 1, T]
    assert lo > 0 and min(planted) < lo - 1 and lo in planted and lo + 1 in planted and lo - 1 in planted
    r = Rows(n, True, seed=21 + apply, sched_steps=T + 1)
    g = r.gen
    last = torch.tensor(planted * (n // len(planted)), dtype=torch.int32)
    r.last.copy_(last)
    r.exp_last = last.long().clone()
    r.sched[:2 * T].copy_(_sched_table(T))
    for w, m, v in zip(WIDTHS, r.sm, r.sv):   # moments of an earlier gradient (a row that sleeps holds some)
        m.copy_(torch.randn(n, w, generator=g) * 0.1)
        v.copy_(0.002 + 0.01 * torch.rand(n, w, generator=g))
    p0 = [x.clone() for x in r.sp]
    m0 = [x.clone() for x in r.sm]
    v0 = [x.clone() for x in r.sv]
    lr_t = _lr_at(T + 1)
    if apply:
        for s, w in zip(r.sg, WIDTHS):
            s.copy_(torch.randn(n, w, generator=g) * 0.3)
        g0 = [x.clone() for x in r.sg]
    # the dense chain on a copy: a row joins at the step after the one it holds
    wp, wm, wv = ([x.clone() for x in q] for q in (p0, m0, v0))
    zero = [torch.zeros_like(x) for x in p0]
    join = {}
    for row, l in enumerate(last.tolist()):
        join.setdefault(l, []).append(row)
    for k in range(1, T + 1):
        if k - 1 in join:
            idx = torch.tensor(join[k - 1], device=DEV)
            for work, orig in ((wp, p0), (wm, m0), (wv, v0)):
                for a, b in zip(work, orig):
                    a[idx] = b[idx]
        _dense_launch(wp, zero, wm, wv, _lr_at(k), k, 0)
    idx = torch.tensor(join[T], device=DEV)
    for work, orig in ((wp, p0), (wm, m0), (wv, v0)):
        for a, b in zip(work, orig):
            a[idx] = b[idx]
    if apply:
        _dense_launch(wp, [x.clone() for x in g0], wm, wv, lr_t, T + 1, 0)
    # the launch under test
    r.sparse(T + apply, apply, lr=lr_t, pend=False)
    assert bool((r.last == T + apply).all())
    for d, s in zip(wp + wm + wv, r.sp + r.sm + r.sv):
        assert torch.equal(d.view(torch.int32), s.contiguous().view(torch.int32))
    if apply:   # the step's constants are in the table for later catch-ups
        assert torch.equal(r.sched[2 * T:2 * T + 2].cpu(), ar.sched_entry(lr_t, BETAS, T + 1))
        assert all(not bool(s.any()) for s in r.sg)
    else:       # the row that holds T keeps its bits
        keep = torch.nonzero(last == T).reshape(-1).to(DEV)
        for a, b in zip(r.sp + r.sm + r.sv, p0 + m0 + v0):
            assert torch.equal(a[keep].contiguous().view(torch.int32), b[keep].contiguous().view(torch.int32))
    # float64: the lazy model, per element under the per-step bounds summed over the replayed steps
    cat = lambda ts: torch.cat([t.detach().cpu().double() for t in ts], dim=1)  # noqa: E731
    lrs = [_lr_at(k) for k in range(1, T + 1)]
    (rp, rm, rv), (bp, bm, bv) = ar.replay_zero_grad(cat(p0), cat(m0), cat(v0), last.long(), lrs, BETAS, EPS, T)
    if apply:
        gg = cat(g0)
        b = ar.adam_step_bound(rp, gg, rm, rv, lr_t, BETAS, EPS, T + 1)
        rp, rm, rv = ar.adam_step(rp, gg, rm, rv, lr_t, BETAS, EPS, T + 1)
        bp, bm, bv = bp + b[0], bm + b[1], bv + b[2]
    worst = {}
    for k, got, ref, bnd in zip("pmv", (cat(r.sp), cat(r.sm), cat(r.sv)), (rp, rm, rv), (bp, bm, bv)):
        moved = bnd > 0
        assert torch.equal(got[~moved], ref[~moved])
        worst[k] = float(((got - ref).abs()[moved] / bnd[moved]).max())
        assert worst[k] <= 1.0, (k, worst[k])
    print(f"adam rows replay T={T} apply={apply}: worst error / summed bound "
          + " ".join(f"{k} {w:.4f}" for k, w in worst.items()))


# ---- 5. the horizon through PointAdam ---------------------------------------------------------------
def test_point_adam_rows_over_a_long_horizon():
    """PointAdam(rows=True, flush_every=4096) against the dense PointAdam over 1,100 steps at 300 rows:
    twelve rows are touched at step 3 and listed next at step 1,060, a replay of more than kSchedWin
    steps through PointAdam's own constant table and across its growth at step 1024."""
    from sgnerf_amd.train_hip import PointAdam
    n, steps, K = 300, 1_100, 8
    sleep_at, wake_at = 3, 1_060
    sleepers = torch.arange(n - 12, n)
    assert wake_at - 2 - sleep_at > SCHED_WIN and wake_at - 2 - SCHED_WIN > sleep_at   # lo > last: the table loop
    g = torch.Generator().manual_seed(5)
    p0 = [torch.randn(n, w, generator=g) for w in WIDTHS]
    a = [torch.nn.Parameter(x.clone().to(DEV)) for x in p0]
    b = [torch.nn.Parameter(x.clone().to(DEV)) for x in p0]
    od = PointAdam(a, lr=2e-3)
    orow = PointAdam(b, lr=2e-3, rows=True, flush_every=4096)
    pool = [[(torch.randn(n, w, generator=g) * 10.0 ** (j % 3 - 1)).to(DEV) for w in WIDTHS] for j in range(8)]
    for x, y, w in zip(a, b, WIDTHS):
        x.grad = torch.zeros(n, w, device=DEV)
        y.grad = torch.zeros(n, w, device=DEV)
    table0 = orow._sched.numel()
    assert table0 == 2 * SCHED_WIN
    for it in range(steps):
        step = it + 1
        n_s = 6
        table = torch.randint(0, n - 12, (n_s, K), generator=g, dtype=torch.int32)
        table[torch.rand(n_s, K, generator=g) < 0.3] = -1
        table[:2, 1] = table[:2, 0]
        if step in (sleep_at, wake_at):
            table[3, :] = sleepers[:8].to(torch.int32)
            table[4, :4] = sleepers[8:].to(torch.int32)
        used = torch.unique(torch.cat([table[table >= 0].long(), torch.zeros(1, dtype=torch.long)]))
        if step not in (sleep_at, wake_at):
            assert not bool((used >= n - 12).any())
        rows = table.reshape(-1).to(DEV)
        count = torch.tensor([n_s, 0], dtype=torch.int32, device=DEV)
        orow.set_rows(rows, count, False, K)
        if step % 50 == 0 or step == wake_at:   # the rows a step reads: the dense state at its start
            read = used.to(DEV)
            for x, y in zip(a, b):
                assert torch.equal(x.detach()[read], y.detach()[read]), step
            if step == wake_at:
                assert orow._sched.numel() > table0   # the table grew before this replay read it
        mask = torch.zeros(n, 1)
        mask[used] = 1.0
        mask = mask.to(DEV)
        for x, y, gr in zip(a, b, pool[it % 8]):
            torch.mul(gr, mask, out=x.grad)
            y.grad.copy_(x.grad)
        for o in (od, orow):
            o.param_groups[0]["lr"] = 2e-3 * 0.999 ** it
        od.step()
        orow.step()
        if step == SCHED_WIN - 1:
            assert orow._sched.numel() == table0
    assert orow._sched.numel() > table0 and orow._flushed == 0   # no flush shortened the sleepers' replay
    orow.flush()
    assert bool((orow._last == steps).all())
    for x, y in zip(a, b):
        assert torch.equal(x.detach(), y.detach())
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(od.state[x][k], orow.state[y][k])
