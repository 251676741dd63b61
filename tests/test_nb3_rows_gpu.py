"""The viewmlp without block3 on the split-fp16 row GEMMs (opts.rows_gemm = 1) on the GPU: the window, row-input,
gather and blend entries called directly on hand-built scenes, the whole launch sequence (rows_gemm.RowsGemmNb3)
on those scenes, then HipRenderer and the model plugin against the reference's own outputs
(tests/golden/reference_nb3.npz) and against the plain-fp32 renderer.

The kernel bar is tests/nb3_ref.py's: max(1e-5, 4 x floor) x max(1, |ref|) per element, the floor measured as the
same restatement in torch fp32 on the GPU against the CPU, and printed with the measured worst case per output
(profiles/nb3_rows_tests.txt keeps them)."""
import argparse
import ctypes
import functools
import types
from dataclasses import replace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sgnerf_amd  # noqa: F401
from sgnerf_amd import _lib
from sgnerf_amd.model import HipPointsVolumetricModel
from sgnerf_amd.render import HipRenderer
from sgnerf_amd.rows_gemm import FP16_RANGE_BITS, RowsGemmNb3, plan_windows
from sgnerf_amd.weights import init_mlp

import nb3_ref as nb
from test_agg_rows_gpu import Dev
from test_api_gpu import _inputs
from test_nb3_gpu import _check_frame, _opts, _render, _tables, golden, scene
from test_train_rows_gpu import _all_nan, _same_bits

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32_TOL = 1e-5
GUARD = 3
NAN = float("nan")
VARIANTS = [(0, 0), (1, 0), (1, 96)]
SCENES = [(8, 1), (8, 7), (8, 9), (8, 17), (5, 9), (5, 17), (1, 7)]
INF_BITS = 0x7f800000


def L():
    return _lib.lib()


def p(t):
    return _lib.ptr(t)


@functools.lru_cache(maxsize=None)
def weights(variant):
    return init_mlp(7, bias_std=0.1, bpnet_layers=variant[0], bpnet_dim=variant[1], block3_layers=0)


@functools.lru_cache(maxsize=None)
def reference(K, items, variant=(0, 0)):
    """The float64 restatement of a scene and the fp32 floors, computed once and shared."""
    sc = scene(K, items)
    st = weights(variant)
    with torch.no_grad():
        o = nb.chain(sc, st)
    fl = nb.floor(sc, st, DEV)
    return o, fl, {k: max(F32_TOL, 4.0 * v) for k, v in fl.items()}


@functools.lru_cache(maxsize=None)
def device_scene(K, items):
    """The scene on the device, colour and dir NULL, with the counts sgn_train_lists would write."""
    sc = scene(K, items)
    dv = Dev(sc)
    dv.pt.color = dv.pt.dir = None
    dv.d["counts"] = torch.tensor([sc.items, sc.rows, 0, 0], dtype=torch.int32, device=DEV)
    return sc, dv


def window_words(sc, dv, ci):
    """sgn_rows_windows on a scene: the words (checked against the lists) as a device tensor."""
    wins = plan_windows(sc.items, ci)
    win = torch.full((2 * len(wins) + GUARD,), -7, dtype=torch.int32, device=DEV)
    _lib.check(L().sgn_rows_windows(ctypes.byref(dv.qo), sc.K, p(dv.d["row_off"]), p(dv.d["counts"]), ci, len(wins), p(win),
                                    _lib.stream_handle()), "sgn_rows_windows")
    torch.cuda.synchronize()
    got = win.cpu()
    want = [x for i0, n in wins for x in (n, sum(sc.work_counts[i0:i0 + n]))]
    assert got[:2 * len(wins)].tolist() == want and bool((got[2 * len(wins):] == -7).all())
    return wins, win


def window_rows(sc, i0, n):
    """Global row indices of a window's items (sample-major: contiguous) and the window's first row."""
    sel = torch.nonzero((sc.item >= i0) & (sc.item < i0 + n)).reshape(-1)
    assert bool((sel == torch.arange(int(sel[0]), int(sel[0]) + sel.numel())).all())
    return sel, int(sel[0])


def x0_of(sc, dtype=torch.float64):
    """block1.0's input rows [rows, 288]: [emb | PE(emb, 3) | PE(dists, 5) | 1 | 0 0 0] (the weight's column order)."""
    d, _ = nb.row_inputs(sc, dtype)
    emb = sc.points["embedding"].to(dtype)[sc.pid]
    one = torch.ones(emb.shape[0], 1, dtype=dtype, device=emb.device)
    return torch.cat([emb, nb.pe(emb, 3), nb.pe(d, 5), one, torch.zeros_like(one).expand(-1, 3)], dim=-1)


def ci_list(items):
    return sorted({1, 4, items})


# ---- 1. the entries on hand-built scenes -----------------------------------------------------------------
@pytest.mark.parametrize("K,items", SCENES)
def test_windows_and_row_inputs(K, items):
    """Windows of 1 item, of 4 (ending mid-list, item0 > 0) and of the whole list: every window's words, x0, rw and
    vpe against the float64 restatement, rows from 0 in every window, nothing written past the window's rows and
    items; the colour and dir tables are NULL."""
    sc, dv = device_scene(K, items)
    o, fl, bar = reference(K, items)
    x0ref = x0_of(sc)
    x0_floor = nb.rel(x0_of(nb._On(sc, DEV), torch.float32).cpu(), x0_of(sc, torch.float32))
    x0_bar = max(F32_TOL, 4.0 * x0_floor)
    v = sc.raydir.double()[sc.query["samp_ray"][:sc.S].long()][sc.work.long()]
    arg = (v[:, :, None] * 2.0 ** torch.arange(4, dtype=torch.float64)).reshape(-1, 12)
    vref = torch.cat([torch.sin(arg), torch.cos(arg), torch.ones(items, 1, dtype=torch.float64),
                      torch.zeros(items, 7, dtype=torch.float64)], dim=-1)
    worst = dict(x0=0.0, rw=0.0, vpe=0.0)
    for ci in ci_list(items):
        wins, win = window_words(sc, dv, ci)
        for w, (i0, n) in enumerate(wins):
            x0 = torch.full((ci * K + GUARD, 288), NAN, device=DEV)
            rw = torch.full((ci * K + GUARD, 2), NAN, device=DEV)
            vpe = torch.full((ci + GUARD, 32), NAN, device=DEV)
            _lib.check(L().sgn_rows_inputs_nb3(ctypes.byref(dv.pt), ctypes.byref(dv.qo), K, p(dv.d["row_off"]),
                                               ctypes.c_void_p(win.data_ptr() + 8 * w), i0, ci, p(x0), p(rw), p(vpe),
                                               _lib.stream_handle()), "sgn_rows_inputs_nb3")
            torch.cuda.synchronize()
            x0, rw, vpe = x0.cpu(), rw.cpu(), vpe.cpu()
            sel, _ = window_rows(sc, i0, n)
            nr = sel.numel()
            assert _all_nan(x0[nr:]) and _all_nan(rw[nr:]) and _all_nan(vpe[n:])
            assert _same_bits(x0[:nr, :32], sc.points["embedding"][sc.pid][sel])
            assert bool((x0[:nr, 284] == 1).all()) and bool((x0[:nr, 285:] == 0).all())
            assert bool((vpe[:n, 24] == 1).all()) and bool((vpe[:n, 25:] == 0).all())
            worst["x0"] = max(worst["x0"], nb.rel(x0[:nr], x0ref[sel]))
            worst["rw"] = max(worst["rw"], nb.rel(rw[:nr], o["rw"][sel]))
            worst["vpe"] = max(worst["vpe"], nb.rel(vpe[:n], vref[i0:i0 + n]))
    print(f"rows inputs K={K} items={items}: fp32 floor x0 {x0_floor:.2e}, rw {fl['rw']:.2e}; max error / max(1, |ref|) "
          + ", ".join(f"{k} {e:.2e}" for k, e in worst.items()))
    assert worst["x0"] <= x0_bar and worst["rw"] <= bar["rw"] and worst["vpe"] <= F32_TOL


@pytest.mark.parametrize("K,items", [(8, 17), (5, 9), (1, 7)])
def test_window_gather(K, items):
    """The BPNet rows of a window, from row 0: bit copies of the table's rows."""
    sc, dv = device_scene(K, items)
    src = sc.points["bpnet"]
    for ci in ci_list(items):
        wins, win = window_words(sc, dv, ci)
        for w, (i0, n) in enumerate(wins):
            dst = torch.full((ci * K + GUARD, 96), NAN, device=DEV)
            _lib.check(L().sgn_rows_gather_nb3(ctypes.byref(dv.qo), K, p(dv.d["row_off"]), ctypes.c_void_p(win.data_ptr() + 8 * w),
                                               i0, ci, p(dv.d["bpnet"]), 96, p(dst), _lib.stream_handle()), "sgn_rows_gather_nb3")
            torch.cuda.synchronize()
            sel, _ = window_rows(sc, i0, n)
            dst = dst.cpu()
            assert _same_bits(dst[:sel.numel()], src[sc.pid][sel]) and _all_nan(dst[sel.numel():])


def _blend(sc, dv, ci, z32, rw32, wa, ba, want_slots=True):
    """sgn_rows_blend_nb3 window by window on given rows: feat, f_s (by item), blend, wnorm, the flag word."""
    K, n_slots = sc.K, sc.S_cap * sc.K
    feat0 = torch.randn(sc.S_cap + GUARD, 4, generator=torch.Generator().manual_seed(5 + sc.S_cap))
    feat = feat0.to(DEV)
    blend, wnorm = (torch.full((n_slots + GUARD,), NAN, device=DEV) for _ in range(2))
    flag = torch.zeros(1 + GUARD, dtype=torch.int32, device=DEV)
    fs_all = torch.full((sc.items, 256), NAN)
    wad, bad = wa.to(DEV), ba.to(DEV)
    wins, win = window_words(sc, dv, ci)
    for w, (i0, n) in enumerate(wins):
        sel, _ = window_rows(sc, i0, n)
        zw = torch.full((ci * K + GUARD, 256), NAN, device=DEV)
        rww = torch.full((ci * K + GUARD, 2), NAN, device=DEV)
        zw[:sel.numel()] = z32[sel].to(DEV)
        rww[:sel.numel()] = rw32[sel].to(DEV)
        fs = torch.full((ci + GUARD, 256), NAN, device=DEV)
        _lib.check(L().sgn_rows_blend_nb3(ctypes.byref(dv.qo), K, p(dv.d["row_off"]), ctypes.c_void_p(win.data_ptr() + 8 * w), i0,
                                          ci, p(zw), p(rww), p(wad), p(bad), p(feat), p(fs), p(blend) if want_slots else None,
                                          p(wnorm) if want_slots else None, p(flag), _lib.stream_handle()), "sgn_rows_blend_nb3")
        torch.cuda.synchronize()
        fs = fs.cpu()
        assert _all_nan(fs[n:])
        fs_all[i0:i0 + n] = fs[:n]
    return dict(feat=feat.cpu(), feat0=feat0, blend=blend.cpu(), wnorm=wnorm.cpu(), fs=fs_all, flag=flag.cpu())


@pytest.mark.parametrize("K,items", SCENES)
def test_blend(K, items):
    """The forward head on the reference's last-layer rows (rounded to fp32): alpha_s, f_s against float64 of those
    same rows; blend / wnorm bit copies of rw on the items' valid slots, 0 on their empty slots, every other word
    (samples without a neighbour, slack samples, guard rows, feat's colour) untouched; every window size gives
    the same bits."""
    sc, dv = device_scene(K, items)
    o, fl, bar = reference(K, items)
    st = weights((0, 0))
    z32 = torch.where(o["h"] > 0, o["h"], o["h"] * 100.0).float()     # LReLU^-1 of the reference's activations
    rw32 = o["rw"].float()
    wa, ba = st["alpha_branch.0.weight"].reshape(256).contiguous(), st["alpha_branch.0.bias"].reshape(1)
    h = F.leaky_relu(z32.double(), 0.01)
    al = F.softplus(h @ wa.double() + ba.double() - 1)
    wk = rw32.double()[:, 0]
    fs_ref = torch.zeros(sc.items, 256, dtype=torch.float64).index_add(0, sc.item, wk[:, None] * h)
    a_ref = torch.zeros(sc.items, dtype=torch.float64).index_add(0, sc.item, wk * al)
    work, idx, n_slots = sc.work.long(), sc.rs * K + sc.rk, sc.S_cap * K
    first = None
    for ci in ci_list(items):
        r = _blend(sc, dv, ci, z32, rw32, wa, ba)
        err = dict(alpha=nb.rel(r["feat"][work, 0], a_ref), fs=nb.rel(r["fs"], fs_ref))
        print(f"rows blend K={K} items={items} ci={ci}: fp32 floor alpha {fl['alpha']:.2e}, fs {fl['fs']:.2e}; "
              f"max error / max(1, |ref|) alpha {err['alpha']:.2e}, fs {err['fs']:.2e}")
        assert err["alpha"] <= bar["alpha"] and err["fs"] <= bar["fs"]
        assert _same_bits(r["blend"][idx], rw32[:, 0]) and _same_bits(r["wnorm"][idx], rw32[:, 1])
        slot_of_item = torch.zeros(n_slots + GUARD, dtype=torch.bool)
        slot_of_item[(work[:, None] * K + torch.arange(K)[None, :]).reshape(-1)] = True
        valid = torch.zeros(n_slots + GUARD, dtype=torch.bool)
        valid[idx] = True
        for t in (r["blend"], r["wnorm"]):
            assert bool((t[slot_of_item & ~valid] == 0).all()) and _all_nan(t[~slot_of_item])
        is_item = torch.zeros(sc.S_cap + GUARD, dtype=torch.bool)
        is_item[work] = True
        assert _same_bits(r["feat"][~is_item], r["feat0"][~is_item]) and _same_bits(r["feat"][:, 1:], r["feat0"][:, 1:])
        assert r["flag"].tolist() == [0] * (1 + GUARD)
        keep = {k: r[k] for k in ("feat", "fs", "blend", "wnorm")}
        assert first is None or all(_same_bits(first[k], keep[k]) for k in keep)
        first = first or keep
    # the slot outputs are optional
    r = _blend(sc, dv, items, z32, rw32, wa, ba, want_slots=False)
    assert _same_bits(r["feat"], first["feat"]) and _all_nan(r["blend"]) and _all_nan(r["wnorm"])


def test_blend_flags_fp16_range():
    """A blended feature at or above 65504 (finite arithmetic, no bad address) leaves +inf's bits in the flag word;
    just below it the word stays 0."""
    sc, dv = device_scene(8, 9)
    st = weights((0, 0))
    wa, ba = torch.zeros(256), st["alpha_branch.0.bias"].reshape(1)
    rw32 = torch.zeros(sc.rows, 2)
    rw32[:, 0] = 1.0
    for value, want in ((65504.0, INF_BITS), (60000.0 / 8, 0)):
        z32 = torch.zeros(sc.rows, 256)
        z32[int(torch.nonzero(sc.item == 4)[0]), 77] = value      # one row of one item
        if not want:
            z32[:, 77] = value                                    # every row: up to 8 x 7500 < 65504
        r = _blend(sc, dv, 4, z32, rw32, wa, ba)
        assert r["flag"].tolist() == [want] + [0] * GUARD
    assert FP16_RANGE_BITS == int(torch.tensor(65504.0).view(torch.int32)) and INF_BITS >= FP16_RANGE_BITS


def _run_rows(sc, dv, variant, ci):
    """The whole launch sequence (lists, windows, row inputs, GEMMs, blend, colour MLP) on a hand-built scene."""
    K, n = sc.K, sc.S_cap * sc.K
    rg = RowsGemmNb3(weights(variant), variant, K, ci, DEV)
    feat0 = torch.randn(sc.S_cap + GUARD, 4, generator=torch.Generator().manual_seed(3 + sc.S_cap))
    feat = feat0.to(DEV)
    blend, wnorm = (torch.full((n + GUARD,), NAN, device=DEV) for _ in range(2))
    q = types.SimpleNamespace(counters=dv.d["counters"], samp_nnb=dv.d["samp_nnb"], work=dv.d["work"])
    got = rg.run(dv.pt, dv.qo, q, sc.S_cap, dv.bp(variant), feat, blend[:n], wnorm[:n])
    torch.cuda.synchronize()
    assert got == sc.items and int(rg.flag().item()) == 0
    return dict(feat=feat.cpu(), feat0=feat0, blend=blend.cpu(), wnorm=wnorm.cpu(), amax=rg.amax.cpu())


@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: f"{v[0]}_{v[1]}")
@pytest.mark.parametrize("K,items", [(8, 17), (5, 9), (1, 7)])
def test_launch_sequence(K, items, variant):
    """RowsGemmNb3.run on hand-built scenes (K = 5 and 1 cannot be queried, so the renderer never sees them):
    alpha, rgb, blend and wnorm against the float64 restatement at its own bar; samples without a neighbour get 0
    (sgn_train_lists), slack samples and guard rows keep their bits; windows of 1, 4 and all items give the same bits."""
    sc, dv = device_scene(K, items)
    o, fl, bar = reference(K, items, variant)
    work, idx, n = sc.work.long(), sc.rs * K + sc.rk, sc.S_cap * K
    first = None
    for ci in ci_list(items):
        r = _run_rows(sc, dv, variant, ci)
        err = dict(alpha=nb.rel(r["feat"][work, 0], o["alpha"]), rgb=nb.rel(r["feat"][work, 1:], o["rgb"]),
                   blend=nb.rel(r["blend"][idx], o["rw"][:, 0]), wnorm=nb.rel(r["wnorm"][idx], o["rw"][:, 1]))
        print(f"rows sequence {variant} K={K} items={items} ci={ci}: fp32 floor " + ", ".join(f"{k} {v:.2e}" for k, v in fl.items())
              + "; max error / max(1, |ref|) " + ", ".join(f"{k} {v:.2e}" for k, v in err.items()))
        assert err["alpha"] <= bar["alpha"] and err["rgb"] <= bar["rgb"]
        assert err["blend"] <= bar["rw"] and err["wnorm"] <= bar["rw"]
        is_item = torch.zeros(sc.S_cap + GUARD, dtype=torch.bool)
        is_item[work] = True
        listed = torch.arange(sc.S_cap + GUARD) < sc.S
        assert bool((r["feat"][listed & ~is_item] == 0).all()) and _same_bits(r["feat"][~listed], r["feat0"][~listed])
        valid = torch.zeros(n, dtype=torch.bool)
        valid[idx] = True
        assert bool((r["blend"][:n][~valid] == 0).all()) and bool((r["wnorm"][:n][~valid] == 0).all())
        assert _all_nan(r["blend"][n:]) and _all_nan(r["wnorm"][n:])
        keep = {k: r[k] for k in ("feat", "blend", "wnorm")}
        assert first is None or all(_same_bits(first[k], keep[k]) for k in keep)
        first = first or keep


# ---- 2. the renderer and the plugin against the reference's outputs --------------------------------------
def _rows_renderer(name, ci=None, **kw):
    return HipRenderer(_tables(name, kw.pop("colour", False)), golden(name)[1], _opts(name, **kw), DEV, rows_gemm=1, rows_ci=ci)


def _frame(out, blend=True):
    """A frame's outputs (feat over the frame's samples with a neighbour, blend over its samples: the plain-fp32
    path leaves the other words of a renderer's buffers unset)."""
    S = int(out.query.counters[0])
    per_sample = [out.feat[:S][out.query.samp_nnb[:S] > 0]] + ([out.blend[:S]] if blend else [])
    return [t.clone() for t in [out.rgb, out.opacity, out.bg_transmission, out.ray_mask] + per_sample]


@pytest.mark.parametrize("name", ["base", "bp256", "bp352"])
def test_renderer_matches_reference(name):
    """HipRenderer(rows_gemm=1): ray_mask and the neighbour indices bit-exact, RGB, decoded features, opacity and
    bg_transmission within 1e-5 of the reference's; the renderer stays off the plain-fp32 path; the frame rendered
    twice, and with windows of 1 item, of 7 and of the whole frame, is bitwise equal."""
    r = _rows_renderer(name)
    assert r.rows is not None and not r.exact and r.packed is None
    _, out = _render(name, r, want_blend=True)
    assert not r.exact and r._rows_frame and r._proj is None and r._fp is None
    keep = _check_frame(name, out, "HipRenderer (rows_gemm)")
    c = golden(name)[2]
    oerr = float(np.abs(out.opacity.cpu().numpy()[keep] - c["opacity"]).max())
    berr = float(np.abs(out.bg_transmission.cpu().numpy()[keep] - c["bg_transmission"]).max())
    print(f"HipRenderer (rows_gemm) {name}: max |opacity - reference| = {oerr:.3e}, bg_transmission {berr:.3e}; "
          f"amax words {[float(x) for x in r.rows.amax.view(torch.float32).cpu()]}")
    assert oerr <= F32_TOL and berr <= F32_TOL
    first = _frame(out)
    _, out2 = _render(name, r, want_blend=True)
    assert all(_same_bits(a, b) for a, b in zip(first, _frame(out2)))
    for ci in (1, 7):
        rc = _rows_renderer(name, ci)
        _, oc = _render(name, rc, want_blend=True)
        assert rc.rows.ci == ci and not rc.exact
        assert all(_same_bits(a, b) for a, b in zip(first, _frame(oc))), f"windows of {ci} items"


def test_renderer_weights_blend_and_depth_match_plain_fp32():
    """want_weights, want_blend and the depth map against the plain-fp32 renderer on the same frame."""
    name = "base"
    _, plain = _render(name, want_weights=True, want_blend=True, want_depth=True)
    ref = {k: getattr(plain, k).clone() for k in ("wnorm", "blendw", "blend", "depth", "opacity", "rgb")}
    r = _rows_renderer(name)
    _, out = _render(name, r, want_weights=True, want_blend=True, want_depth=True)
    assert not r.exact and r._rows_frame
    S = int(out.query.counters[0])
    K = int(golden(name)[2]["K"])
    err = {}
    for k, v in ref.items():
        a, b = getattr(out, k), v
        if k in ("wnorm", "blend"):
            a, b = a.reshape(-1)[:S * K], b.reshape(-1)[:S * K]
        err[k] = nb.rel(a.cpu(), b.cpu())
    print("HipRenderer (rows_gemm) against the plain-fp32 renderer: " + ", ".join(f"{k} {v:.2e}" for k, v in err.items()))
    assert all(v <= F32_TOL for v in err.values())
    assert float(ref["wnorm"].abs().max()) > 0 and float(ref["depth"].max()) > 0


def test_range_guard_falls_back_to_plain_fp32():
    """block1.2 scaled until its pre-activation leaves fp16 range: with check_range="sync" the frame is the
    plain-fp32 renderer's, bit for bit, and the renderer stays on that path."""
    name = "base"
    pts, st, c = golden(name)
    big = dict(st)
    big["block1.2.weight"] = st["block1.2.weight"] * 4.0e5
    big["block1.2.bias"] = st["block1.2.bias"] * 4.0e5
    plain = HipRenderer(_tables(name), big, _opts(name), DEV)
    _, po = _render(name, plain, want_blend=True)
    want = _frame(po)
    r = HipRenderer(_tables(name), big, _opts(name), DEV, rows_gemm=1)
    assert not r.exact
    _, out = _render(name, r, want_blend=True, check_range="sync")
    z2 = float(r.rows.amax.view(torch.float32)[RowsGemmNb3.A_Z2])
    print(f"range guard: max |z2| = {z2:.3e}")
    assert z2 >= 65504.0 and r.exact
    assert all(_same_bits(a, b) for a, b in zip(want, _frame(out)))
    _, out2 = _render(name, r, want_blend=True)       # later frames go there directly
    assert r.exact and not r._rows_frame and all(_same_bits(a, b) for a, b in zip(want, _frame(out2)))
    # without the check the renderer keeps its path (and the frame is not the plain-fp32 one)
    r2 = HipRenderer(_tables(name), big, _opts(name), DEV, rows_gemm=1)
    _render(name, r2, check_range=False)
    assert not r2.exact


def test_deferred_range_check_raises_on_the_next_frame():
    name = "base"
    pts, st, c = golden(name)
    big = dict(st)
    big["block1.2.weight"] = st["block1.2.weight"] * 4.0e5
    r = HipRenderer(_tables(name), big, _opts(name), DEV, rows_gemm=1)
    _render(name, r, check_range="deferred")
    with pytest.raises(_lib.SgnError, match="fp16 range"):
        r.finish()
    assert r.exact


def test_fallbacks_render_on_plain_fp32():
    """Rotated points and early-stop tiers: the option is accepted, the frame is the default renderer's bit for bit."""
    _, plain = _render("rot", want_blend=True)
    want = _frame(plain)
    r = _rows_renderer("rot")
    _, out = _render("rot", r, want_blend=True)
    assert r.rows is not None and not r._rows_frame and not r.exact and not r._pending
    assert all(_same_bits(a, b) for a, b in zip(want, _frame(out)))
    _, plain = _render("base")
    want = _frame(plain, blend=False)
    es = _rows_renderer("base", early_stop=1e-2)
    _, oe = _render("base", es)
    assert not es._rows_frame and oe.stop_slot is None and oe.skipped is None
    assert all(_same_bits(a, b) for a, b in zip(want, _frame(oe, blend=False)))
    # per-slot outputs render in full on the stock path too: such frames take the row GEMMs
    _, ow = _render("base", es, want_blend=True)
    assert es._rows_frame and not es.exact


def test_refusals_on_construction():
    pts, st, c = golden("base")
    with pytest.raises(NotImplementedError, match="rows_gemm"):
        HipRenderer(_tables("base"), init_mlp(0), replace(_opts("base"), shading_feature_mlp_layer3=2), DEV, rows_gemm=1)
    with pytest.raises(NotImplementedError, match="rows_gemm"):
        HipRenderer(_tables("base"), st, replace(_opts("base"), K=16), DEV, rows_gemm=1)
    with pytest.raises(ValueError, match="rows_gemm"):
        HipRenderer(_tables("base"), st, _opts("base"), DEV, rows_gemm=1, rows_ci=1 << 20)


@pytest.mark.parametrize("name", ["base", "bp352"])
def test_model_test_matches_reference(name, tmp_path):
    """The plugin with rows_gemm = 1 in the driver's namespace."""
    pts, st, c = golden(name)
    nl, dim = nb.VARIANT[name]
    n = pts["xyz"].shape[0]
    sd = {"neural_points.xyz": torch.from_numpy(pts["xyz"]), "neural_points.points_embeding": torch.from_numpy(pts["embedding"])[None],
          "neural_points.points_conf": torch.from_numpy(pts["conf"]).reshape(1, n, 1)}
    if dim:
        sd["neural_points.bpnet_points_embedding"] = torch.from_numpy(pts["bpnet"])[None]
        sd["neural_points.points_label"] = torch.zeros(n, 1, dtype=torch.int32)
    sd.update({"aggregator." + k: v for k, v in st.items()})
    (tmp_path / "scene").mkdir()
    torch.save(sd, tmp_path / "scene" / "5_net_ray_marching.pth")
    opt = argparse.Namespace(SR=int(c["SR"]), K=int(c["K"]), gpu_ids=[0], is_train=False, checkpoints_dir=str(tmp_path),
                             name="scene", bg_color="white", shading_feature_mlp_layer3=0,
                             shading_feature_mlp_layer2_bpnet=nl, predict_semantic=1 if dim else 0,
                             semantic_guidance=1 if dim else 0, rows_gemm=1)
    m = HipPointsVolumetricModel()
    m.initialize(opt)
    assert m.opts.rows_gemm == 1
    m.load_networks(5)
    inp = _inputs(c)
    if dim:
        inp["pixel_label"] = torch.zeros(1, c["raydir"].shape[0], 1, dtype=torch.int32, device=DEV)
    m.set_input(inp)
    out = m.test()
    r = m.net_ray_marching.renderer
    assert r.rows is not None and r._rows_frame and not r.exact
    np.testing.assert_array_equal(out["ray_mask"][0].cpu().numpy(), c["ray_mask"])
    err = float(np.abs(out["coarse_raycolor"][0].cpu().numpy() - c["full_color"]).max())
    keep = c["ray_mask"].astype(bool)
    werr = float(np.abs(out["weight"][0].cpu().numpy()[keep] - c["weight"]).max())
    cerr = float(np.abs(out["conf_coefficient"][0].cpu().numpy()[keep] - c["conf_coefficient"]).max())
    print(f"model.test() rows_gemm {name}: max |rgb - reference| = {err:.3e}, weight {werr:.3e}, conf_coefficient {cerr:.3e}")
    assert err <= F32_TOL and werr <= F32_TOL and cerr <= F32_TOL
