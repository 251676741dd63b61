"""k_rows16's two exposed vector phases (csrc/mlp_x3.hip): PE(dists) inside block1.0's k-loop and the block3.2
epilogue, whose accumulators start at the bias (2^s3 b3) so that LeakyReLU reads the raw accumulator.
Per-element float64 checks with the bound functions of tests/agg_rows_ref.py, on the smallest shapes that reach every path: K = 8 and a hand-built
neighbour-count list whose slot table (restated by agg_rows_ref.pair_slots, asserted below) has 21 halves -- one
render tile of 16 plus a partly filled one (two save tiles of 8 plus one) -- with nA = 1..8, the pairs 7+1, 6+2,
5+3, 4+4, B-less halves, and idle halves in a wave that also holds work and in waves that hold none.

  PE        save mode with block1.0's PE(dists) columns one-hot (unit j = PE input j) and P zeroed: z1 shows each
            sin / cos.  Planted world distances put d 2^f next to multiples of pi/2 at every frequency.
  epilogue  f_s and alpha_s from the kernel's own z3 against blend_ref, with block3.2 biases far larger than the
            products, biases of both signs at the products' size, and block3.2 weights scaled so the layer's shift
            s3 sits at a small, a large and the zero-layer value.
  bits      render (NS = 2) = save (NS = 1); paired = SGN_PAIR=0 (every sample alone, as segment A: the samples the
            pairing puts into segment B keep their bits)."""
import ctypes
import math

import pytest
import torch

import sgnerf_amd  # noqa: F401
from sgnerf_amd import _lib
from sgnerf_amd.weights import init_mlp, pack_mlp

import agg_rows_ref as ar
import test_agg_rows_gpu as tg
import train_rows_ref as rr
from test_train_rows_gpu import _all_nan, _ratio, _same_bits

pytestmark = pytest.mark.gpu
DEV = tg.DEV
NAN = float("nan")

# 8 | 7+1 6+2 5+3 4+4 | leftovers 1 1 2 2 3 3 4, twice, three more 8s and a seventh 4 (the odd leftover, alone)
BASE = [8, 7, 1, 6, 2, 5, 3, 4, 4, 1, 1, 2, 2, 3, 3, 4]
COUNTS = ar.with_empties(BASE + [8, 8] + BASE + [8, 4])
_STATE = {}


def scene(planted=False):
    key = ("scene", planted)
    if key not in _STATE:
        sc = ar.Scene(8, COUNTS, seed=29, bpnet=True)
        if planted:
            _plant(sc)
        _STATE[key] = (sc, tg.Dev(sc))
    return _STATE[key]


def test_slot_table_covers_the_paths():
    sc, _ = scene()
    slots = ar.pair_slots(sc.work_counts)
    assert len(slots) == 21                                             # 16 + 5: slot 20's wave has three idle halves
    assert {nA for _, nA, _, _ in slots} == set(range(1, 9))
    pairs = {(nA, nB) for _, nA, b, nB in slots if b >= 0}
    assert {(7, 1), (6, 2), (5, 3), (4, 4), (1, 1), (2, 2), (3, 3)} <= pairs
    assert {nA for _, nA, b, _ in slots if b < 0} == {8, 4}             # B-less halves
    assert any(c == 0 for c in COUNTS)                                  # samples without a neighbour in between


def _plant(sc):
    """World distances of the first neighbour of the first work items next to multiples of pi/2 at some frequency:
    loc = xyz[pid] - t, so the kernel's d = fp32(xyz - loc) is within an ulp or two of t.  t = k pi/32 (d 2^4 = k pi/2,
    and d 2^3, d 2^2 for the even k), k = 1..8 on each axis in turn with either sign, and pi/2 itself on one axis
    (every frequency a multiple of pi/2 at once; the sample moves away from the camera, so it stays in front of it)."""
    q, xyz = sc.query, sc.points["xyz"]
    loc = q["samp_locw"]
    work = sc.work.long().tolist()
    ts = [(k * math.pi / 32 * (-1) ** k, ax) for k in range(1, 9) for ax in range(3)] + [(-math.pi / 2, 2), (-math.pi / 4, 0)]
    assert len(ts) <= len(work)
    for (t, ax), s in zip(ts, work):
        p = xyz[int(q["pidx"][s, 0])]
        v = p.clone()
        v[ax] = p[ax] - torch.tensor(t, dtype=torch.float32)
        loc[s] = v
    sc.planted = len(ts)


def onehot_state():
    st = init_mlp(5, bias_std=0.1)
    w = torch.zeros_like(st["block1.0.weight"])
    for j in range(60):
        w[j, 224 + j] = 1.0
    st["block1.0.weight"] = w
    st["block1.0.bias"] = torch.zeros_like(st["block1.0.bias"])
    return st


def epi_state(kind):
    st = init_mlp(5, bias_std=0.1)
    g = torch.Generator().manual_seed(41)
    b = torch.randn(256, generator=g)
    w = st["block3.2.weight"]
    if kind == "bias_far":       # |b| ~ 100 against products of order 1
        st["block3.2.bias"] = b * 100.0
    elif kind == "bias_signs":   # both LeakyReLU branches, bias and products of one size
        st["block3.2.bias"] = b
    elif kind == "s3_large":     # tiny weights: the layer's shift far up (the accumulator is all bias)
        st["block3.2.weight"], st["block3.2.bias"] = w * 2.0 ** -30, b
    elif kind == "s3_small":     # large weights: the shift near zero
        st["block3.2.weight"], st["block3.2.bias"] = w * 2.0 ** 10, b
    elif kind == "s3_zero":      # a zero layer: shift 0, z4 = b exactly
        st["block3.2.weight"], st["block3.2.bias"] = torch.zeros_like(w), b
    else:
        raise KeyError(kind)
    return st


def packed(kind):
    if kind not in _STATE:
        st = onehot_state() if kind == "onehot" else epi_state(kind)
        _STATE[kind] = (st, pack_mlp(st, DEV, "f32"))
    return _STATE[kind]


def proj_of(dv, blob, zero_p=False):
    buf = tg.project(dv.pt, dv.sc.N, blob)
    if zero_p:
        buf[:dv.sc.N * 256] = 0.0          # P; the 64-B records behind it stay
    return buf


def run_save(dv, blob, proj):
    sc = dv.sc
    z = [torch.full((sc.S_cap * sc.K + tg.GUARD, 256), NAN, device=DEV) for _ in range(3)]
    feat0 = tg.feat0_of(sc)
    feat = feat0.to(DEV)
    ws = tg.new_ws(sc.S_cap)
    _lib.check(tg.L().sgn_aggregate_train_fwd_f32(0, 0, None, _lib.ptr(proj), ctypes.byref(dv.pt), ctypes.byref(dv.qo), sc.S_cap, sc.K,
                                                  _lib.ptr(blob), _lib.ptr(feat), _lib.ptr(z[0]), _lib.ptr(z[1]), None, _lib.ptr(z[2]),
                                                  None, _lib.ptr(ws), ws.numel(), _lib.stream_handle()), "sgn_aggregate_train_fwd_f32")
    torch.cuda.synchronize()
    return dict(feat=feat.cpu(), feat0=feat0, z1=z[0].cpu(), z2=z[1].cpu(), z3=z[2].cpu(), fs=tg.fs_of(ws, sc.S_cap).cpu())


def run_render(dv, blob, proj):
    sc = dv.sc
    feat0 = tg.feat0_of(sc)
    feat = feat0.to(DEV)
    ws = tg.new_ws(sc.S_cap)
    _lib.check(tg.L().sgn_aggregate_f32(0, 0, None, _lib.ptr(proj), ctypes.byref(dv.pt), ctypes.byref(dv.qo), sc.S_cap, sc.K,
                                        _lib.ptr(blob), _lib.ptr(feat), None, None, _lib.ptr(ws), ws.numel(), 1,
                                        _lib.stream_handle()), "sgn_aggregate_f32")
    torch.cuda.synchronize()
    return dict(feat=feat.cpu(), feat0=feat0, fs=tg.fs_of(ws, sc.S_cap).cpu())


def saved(kind):
    key = ("saved", kind)
    if key not in _STATE:
        _, dv = scene()
        _, blob = packed(kind)
        _STATE[key] = run_save(dv, blob, proj_of(dv, blob))
    return _STATE[key]


def test_pe_through_the_kernel():
    sc, dv = scene(planted=True)
    st, blob = packed("onehot")
    assert ar.layer_shift(st["block1.0.weight"]) == 13
    r = run_save(dv, blob, proj_of(dv, blob, zero_p=True))
    idx = sc.rs * sc.K + sc.rk
    keep = torch.zeros(r["z1"].shape[0], dtype=torch.bool)
    keep[idx] = True
    assert _all_nan(r["z1"][~keep])
    z1 = r["z1"][idx]
    P = sc.points
    d64 = rr.row_dists(P, sc.camera, sc.query, sc.K)
    dk = torch.cat([(P["xyz"][sc.pid] - sc.query["samp_locw"][sc.rs]).double(), d64[:, 3:]], dim=1)   # the kernel's own world argument
    # the planting took: some world argument of every frequency within 1e-5 of a multiple of pi/2
    for f in range(5):
        a = dk[:, :3] * 2.0 ** f / (math.pi / 2)
        near = ((a - a.round()).abs() < 1e-5) & (a.round() != 0)
        assert int(near.sum()) >= (3 if f else 1), f
    ref = ar.z1_ref(torch.zeros(sc.rows, 256, dtype=torch.float64), dk, st)
    assert bool((ref[:, 60:] == 0).all()) and ar.amax(ref) <= 1.0
    b = ar.bound_z1(ref, st, ar.cam_E(sc))
    _ratio(z1, ref, b, "PE(dists) through z1 (one-hot W0b)")
    err = (z1[:, :30].double() - ref[:, :30]).abs().max()       # the world components: exact fp32 arguments
    print(f"PE(dists) world columns: max |sin / cos - float64| = {float(err):.3e} = {float(err) * 2 ** 24:.2f} x 2^-24 "
          f"(the fragments carry 22 bits)")
    assert bool((z1[:, 60:] == 0).all())


EPI_KINDS = ["bias_far", "bias_signs", "s3_large", "s3_small", "s3_zero"]


@pytest.mark.parametrize("kind", EPI_KINDS)
def test_epilogue(kind):
    sc, _ = scene()
    st, _ = packed(kind)
    r = saved(kind)
    s3 = ar.layer_shift(st["block3.2.weight"])
    assert {"s3_large": s3 >= 40, "s3_small": s3 <= 8, "s3_zero": s3 == 0}.get(kind, 10 <= s3 <= 20), s3
    idx = sc.rs * sc.K + sc.rk
    z3 = r["z3"][idx]
    _, _, rw, _ = rr.row_inputs_ref(sc.points, sc.camera, sc.raydir, sc.query, sc.K)
    fs_r, a_r, z4_r, _ = ar.blend_ref(z3.double(), rw[:, 0], sc.item, sc.items, st)
    if kind == "bias_far":
        prod = z4_r - st["block3.2.bias"].double()[None, :]
        assert float(st["block3.2.bias"].abs().median()) > 20 * float(prod.abs().median())
    if kind in ("bias_far", "bias_signs"):
        assert 0.2 < float((z4_r < 0).double().mean()) < 0.8          # both LeakyReLU branches
    b = ar.bound_fs(z4_r, rw[:, 0], sc.item, sc.items)
    what = f"epilogue {kind} (s3 = {s3})"
    _ratio(r["fs"][:sc.items], fs_r, b.clamp(min=1e-300), f"{what} f_s")
    b = ar.alpha_bar(z3, rw[:, 0], sc.item, sc.items, st, a_r)
    _ratio(r["feat"][sc.work.long(), 0], a_r, b, f"{what} alpha_s")
    tg.check_feat_untouched(sc, r["feat"], r["feat0"], rgb_written=False)


@pytest.mark.parametrize("kind", ["bias_signs", "bias_far"])
def test_bit_identity(kind, monkeypatch):
    sc, dv = scene()
    _, blob = packed(kind)
    proj = proj_of(dv, blob)
    s = saved(kind)
    rn = run_render(dv, blob, proj)
    n = sc.items
    assert _same_bits(rn["feat"], s["feat"]) and _same_bits(rn["fs"][:n], s["fs"][:n])          # NS = 2 against NS = 1
    # the samples the pairing puts into segment B (sizes 1..4, behind nA = 7, 6, 5, 4 and behind a leftover)
    assert {nB for _, _, b, nB in ar.pair_slots(sc.work_counts) if b >= 0} == {1, 2, 3, 4}
    monkeypatch.setenv("SGN_PAIR", "0")                                                          # every sample alone: segment A
    s0 = run_save(dv, blob, proj)
    rn0 = run_render(dv, blob, proj)
    for k in ("feat", "z1", "z2", "z3", "fs"):
        assert _same_bits(s[k], s0[k]), k
    assert _same_bits(rn["feat"], rn0["feat"]) and _same_bits(rn["fs"][:n], rn0["fs"][:n])
