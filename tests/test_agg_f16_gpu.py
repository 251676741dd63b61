"""The f16 training aggregator's two kernels -- k_agg_rows<V, true> (sgn_aggregate_train_fwd, csrc/mlp.hip) and
k_agg_bwd<SG> (sgn_aggregate_backward, csrc/agg_train.hip) -- called directly through the C ABI on hand-built scenes
and compared per element with the one-layer float64 references of tests/agg_f16_ref.py (proven on the CPU in
test_agg_f16_ref_cpu.py), each fed the tensor the kernel itself wrote on the previous cut: x0, h1, h2 (h2b), h3, f_s,
alpha_s; h4, dza, d4, d3, d2 (db), d1 and the four point gradients.  The references run in float64 on the device, in
chunks of CHUNK items.

Bounds and the interval check: agg_f16_ref.py's docstring.  Every output is pre-filled (fp16 / fp32 NaN, seeded
values where the kernel accumulates or must leave finite values alone) in exact-size buffers with GUARD rows after
them, which must keep their bits.  Item counts are the smallest at which the kernels' paths differ: the forward's
workgroup is 8 waves x 4 items under a grid cap of 256 (8195 items: the persistent loop's second trip), the
backward's 4 waves x 4 items under a cap of 2048 (32771 items: a second tile, whose product 0 the `more` branch
prefetches); at 1, 3, 4, 5, 13, 16, 17 items waves have no rows at all or tiles of 8, 16, 24 rows.  Smaller counts run
on the first n items of a 300-item scene, so the rows of items >= n are there to be left alone.
Each test prints its worst error / bound ratio per cut."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import sgnerf_amd  # noqa: F401
from sgnerf_amd import _lib
from sgnerf_amd.weights import init_mlp, layers_for, pack_mlp

import agg_f16_ref as fr
from test_agg_rows_gpu import Dev
from test_train_rows_gpu import _all_nan, _same_bits

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
VARIANTS = [(0, 0), (1, 96), (1, 0)]
GUARD = 3
NAN = float("nan")
CHUNK = 8192     # items per float64 reference chunk (65536 rows)
# the render instantiation k_agg_rows<V, false> (sgn_aggregate, stages = 1, no point projection) against the save
# instantiation on the same scene: f_s and alpha_s found bit-identical on the MI355X for the three variants (K = 8 in
# order, K = 4 shuffled), asserted from then on
RENDER_EQUALS_SAVE = True


def L():
    return _lib.lib()


@functools.lru_cache(maxsize=None)
def weights(variant):
    """(state, forward blob, transposed blob, Net on the device, the fp16 BPNet table or None)."""
    st = init_mlp(5, bias_std=0.1, bpnet_layers=variant[0], bpnet_dim=variant[1])
    blob = pack_mlp(st, DEV)
    names = [n for n, *_ in layers_for(*variant)]
    ws = [np.ascontiguousarray(st[n + ".weight"].numpy()) for n in names[:4] + names[9:]]
    wp = (ctypes.c_void_p * len(ws))(*[w.ctypes.data for w in ws])
    tblob = torch.zeros(int(L().sgn_train_tblob_bytes()), dtype=torch.uint8, device=DEV)
    _lib.check(L().sgn_train_pack_t(variant[0], variant[1], wp, _lib.ptr(tblob), _lib.stream_handle()), "sgn_train_pack_t")
    return st, blob, tblob, fr.Net(st, DEV)


@functools.lru_cache(maxsize=None)
def dev(name):
    return Dev(fr.scene(name))


@functools.lru_cache(maxsize=None)
def bp16(name):
    """sgn_bpnet_pack's fp16 table of the scene's BPNet rows."""
    dv = dev(name)
    out = torch.full((dv.sc.N, 96), NAN, dtype=torch.float16, device=DEV)
    _lib.check(L().sgn_bpnet_pack(_lib.ptr(dv.d["bpnet"]), dv.sc.N, 96, _lib.ptr(out), _lib.stream_handle()), "sgn_bpnet_pack")
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), dv.sc.points["bpnet"].half())
    return out


def rows_of(name, variant, n):
    return fr.Rows(fr.scene(name), n, bp16=bp16(name) if variant == (1, 96) else None)


def nan16(*shape):
    return torch.full(shape, NAN, dtype=torch.float16, device=DEV)


def run_forward(name, variant, n=None):
    """sgn_aggregate_train_fwd over the first n work items into exact-size NaN-filled buffers with guard rows."""
    dv = dev(name)
    sc = dv.sc
    n = sc.items if n is None else n
    _, blob, _, _ = weights(variant)
    R = 8 * n
    t = dict(x0=nan16(R + GUARD, 288), h1=nan16(R + GUARD, 256), h2=nan16(R + GUARD, 272), h3=nan16(R + GUARD, 256),
             h2b=nan16(R + GUARD, 256), fs=nan16(n + GUARD, 256))
    feat0 = torch.randn(sc.S_cap + GUARD, 4, generator=torch.Generator().manual_seed(3 + sc.S_cap))
    feat = feat0.to(DEV)
    saved = _lib.AggSaved(*(t[k].data_ptr() for k in ("x0", "h1", "h2", "h3")))
    rc = L().sgn_aggregate_train_fwd(variant[0], variant[1], _lib.ptr(bp16(name)) if variant[1] else None, ctypes.byref(dv.pt),
                                     ctypes.byref(dv.qo), n, sc.K, _lib.ptr(blob), _lib.ptr(feat), _lib.ptr(t["fs"]),
                                     ctypes.byref(saved), _lib.ptr(t["h2b"]) if variant[0] else None, _lib.stream_handle())
    _lib.check(rc, "sgn_aggregate_train_fwd")
    torch.cuda.synchronize()
    t.update(feat=feat, feat0=feat0, n=n)
    return t


@functools.lru_cache(maxsize=None)
def forward(name, variant):
    """The whole-scene forward of a small scene, shared by the forward and backward tests."""
    return run_forward(name, variant)


def check_forward_run(name, variant, t, what):
    sc = fr.scene(name)
    n, R = t["n"], 8 * t["n"]
    net = weights(variant)[3]
    for k in ("x0", "h1", "h2", "h3"):
        assert _all_nan(t[k][R:]), f"{what}: {k} wrote a guard row"
    assert _all_nan(t["h2b"][R:] if variant[0] else t["h2b"]) and _all_nan(t["fs"][n:])
    # out_feat: alpha of the first n work items is the kernel's; every other word keeps its bits
    feat, feat0 = t["feat"].cpu(), t["feat0"]
    mine = torch.zeros(feat.shape[0], dtype=torch.bool)
    mine[sc.work[:n].long()] = True
    assert _same_bits(feat[:, 1:], feat0[:, 1:]) and _same_bits(feat[~mine], feat0[~mine])
    rows = rows_of(name, variant, n)
    rep = fr.Report()
    work = sc.work.long().to(DEV)
    for i0 in range(0, n, CHUNK):
        i1 = min(n, i0 + CHUNK)
        c = {k: t[k][8 * i0:8 * i1] for k in ("x0", "h1", "h2", "h3", "h2b")}
        c["fs"], c["alpha"] = t["fs"][i0:i1], t["feat"][work[i0:i1], 0]
        fr.check_forward(rep, rows.chunk(i0, i1, DEV), net, c)
    rep.show(what)
    rep.assert_ok(what)
    return rep


def run_backward(name, variant, fw, n, scale):
    """sgn_aggregate_backward over the first n items of a forward run's saved tensors."""
    dv = dev(name)
    sc = dv.sc
    _, blob, tblob, _ = weights(variant)
    R = 8 * n
    dfs, dalpha, g0 = fr.upstream(n)
    pad = lambda x: torch.cat([x, torch.full((GUARD,) + x.shape[1:], NAN)]).to(DEV)  # noqa: E731
    t = {k: nan16(R + GUARD, 256) for k in ("d4", "d3", "d2", "d1", "h4", "db")}
    t["dza"] = torch.full((R + GUARD,), NAN, device=DEV)
    t["dfs"], t["dalpha"] = pad(dfs), pad(dalpha)
    g = {k: v.clone().to(DEV) for k, v in g0.items()}
    sc_t = torch.tensor([scale], device=DEV)
    saved = _lib.AggSaved(*(fw[k].data_ptr() for k in ("x0", "h1", "h2", "h3")))
    deltas = _lib.AggDeltas(*(t[k].data_ptr() for k in ("d4", "d3", "d2", "d1", "h4", "dza")))
    grads = _lib.PointGrads(*(g[k].data_ptr() for k in ("embedding", "color", "dir", "conf")))
    sgv = variant[0] == 1
    rc = L().sgn_aggregate_backward(variant[0], variant[1], ctypes.byref(dv.pt), ctypes.byref(dv.qo), n, sc.K, _lib.ptr(blob),
                                    _lib.ptr(tblob), ctypes.byref(saved), _lib.ptr(fw["h2b"]) if sgv else None, _lib.ptr(t["dfs"]),
                                    _lib.ptr(t["dalpha"]), _lib.ptr(sc_t), ctypes.byref(deltas), _lib.ptr(t["db"]) if sgv else None,
                                    ctypes.byref(grads), _lib.stream_handle())
    _lib.check(rc, "sgn_aggregate_backward")
    torch.cuda.synchronize()
    t.update(g=g, g0=g0, n=n, scale=scale)
    return t


def check_backward_run(name, variant, fw, t, what):
    sc = fr.scene(name)
    n, R, scale = t["n"], 8 * t["n"], t["scale"]
    net = weights(variant)[3]
    names = ["d4", "d3", "d2", "d1", "h4"] + (["db"] if variant[0] else [])
    for k in names + ["dza"]:
        assert _all_nan(t[k][R:]), f"{what}: {k} wrote a row of an item >= n_items"
    if not variant[0]:
        assert _all_nan(t["db"])
    rows = rows_of(name, variant, n)
    rep = fr.Report()
    acc = fr.GradAcc(sc.N, DEV)
    for i0 in range(0, n, CHUNK):
        i1 = min(n, i0 + CHUNK)
        c = {k: t[k][8 * i0:8 * i1] for k in names + ["dza"]}
        c.update({k: fw[k][8 * i0:8 * i1] for k in ("h1", "h2", "h3", "h2b")})
        c.update(dfs=t["dfs"][i0:i1], dalpha=t["dalpha"][i0:i1], scale=scale)
        rc = rows.chunk(i0, i1, DEV)
        fr.check_backward(rep, rc, net, c, acc)
        assert fr.masked_rows_zero(rc, c, variant[0] == 1), f"{what}: a masked slot's delta is not +-0"
    fr.check_point_grads(rep, acc, t["g0"], t["g"], scale)
    none = (acc.cnt == 0).cpu()
    for k, v in t["g"].items():     # points no valid row names keep their bits
        assert _same_bits(v.cpu()[none], t["g0"][k][none]), f"{what}: g_{k} of a point without a row changed"
    rep.show(what)
    rep.assert_ok(what)       # every cut inside its bound, and the ambiguity cap on the GPU's own h3
    return rep


# ---- forward -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS, ids=str)
@pytest.mark.parametrize("name", fr.SMALL_SCENES)
def test_forward(name, variant):
    check_forward_run(name, variant, forward(name, variant), f"forward {name} {variant}")


FWD_COUNTS = [(n, (0, 0)) for n in (1, 5, 31, 32, 33)] + [(n, v) for n in (5, 33) for v in VARIANTS[1:]]


@pytest.mark.parametrize("n,variant", FWD_COUNTS, ids=str)
def test_forward_item_counts(n, variant):
    """S_capacity = n below the work count: the rows, f_s and alpha of items >= n keep their pre-fill."""
    check_forward_run("rand8_300", variant, run_forward("rand8_300", variant, n), f"forward rand8_300[:{n}] {variant}")


@pytest.mark.parametrize("variant", VARIANTS, ids=str)
def test_forward_second_trip(variant):
    """8195 items: 256 workgroups x 32 items + 3, the persistent loop's second trip."""
    assert fr.scene("rand3_8195").items == 8195
    check_forward_run("rand3_8195", variant, run_forward("rand3_8195", variant), f"forward rand3_8195 {variant}")


def test_no_items_touch_nothing():
    t = run_forward("rand8_300", (0, 0), 0)
    assert all(_all_nan(t[k]) for k in ("x0", "h1", "h2", "h3", "h2b", "fs")) and _same_bits(t["feat"].cpu(), t["feat0"])
    fw = forward("rand8_300", (0, 0))
    b = run_backward("rand8_300", (0, 0), fw, 0, 4096.0)
    assert all(_all_nan(b[k]) for k in ("d4", "d3", "d2", "d1", "h4", "db", "dza"))
    assert all(_same_bits(b["g"][k].cpu(), b["g0"][k]) for k in b["g"])


# ---- backward ------------------------------------------------------------------------------------------------
# loss scales: powers of two only, as sgn_pow2_scale produces
BWD_CASES = [(n, v, 4096.0) for n in fr.SMALL_SCENES for v in VARIANTS] + [(n, v, 1.0) for n in ("rand8_300", "pairs") for v in VARIANTS]


@pytest.mark.parametrize("name,variant,scale", BWD_CASES, ids=str)
def test_backward(name, variant, scale):
    fw = forward(name, variant)
    t = run_backward(name, variant, fw, fw["n"], scale)
    check_backward_run(name, variant, fw, t, f"backward {name} {variant} scale {scale}")


@pytest.mark.parametrize("variant", [(0, 0), (1, 96)], ids=str)
@pytest.mark.parametrize("n", [1, 3, 4, 5, 13, 16, 17])
def test_backward_item_counts(n, variant):
    """n_items below the forward's: waves without rows, tiles of 8 / 16 / 24 rows; rows of items >= n untouched."""
    fw = forward("rand8_300", variant)
    t = run_backward("rand8_300", variant, fw, n, 4096.0)
    check_backward_run("rand8_300", variant, fw, t, f"backward rand8_300[:{n}] {variant}")


@pytest.mark.parametrize("variant", [(0, 0), (1, 96)], ids=str)
def test_backward_second_tile(variant):
    """32771 items: 2048 workgroups x 16 items + 3, so three workgroups run a second tile and take the `more`
    branch (product 0 of the next tile prefetched behind the last product); 12 products (base) and 14 (SG)."""
    name = "rand2_32771"
    assert fr.scene(name).items == 32771
    fw = run_forward(name, variant)
    t = run_backward(name, variant, fw, fw["n"], 4096.0)
    check_backward_run(name, variant, fw, t, f"backward {name} {variant}")
    del fw, t
    torch.cuda.empty_cache()


# ---- the render instantiation against the save instantiation ---------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS, ids=str)
@pytest.mark.parametrize("name", ["rand8_300", "rand4_300"])
def test_render_instantiation_against_save(name, variant):
    """sgn_aggregate(d_point_proj = NULL, stages = 1) runs k_agg_rows<V, false>: its f_s (the workspace) and alpha_s
    hold the save instantiation's bounds (the reference evaluated from the save run's h3), and are compared with the
    save run's bit for bit."""
    dv = dev(name)
    sc = dv.sc
    fw = forward(name, variant)
    _, blob, _, net = weights(variant)
    nb = int(L().sgn_aggregate_workspace_bytes(sc.S_cap))
    ws = torch.full((nb + 512 * GUARD,), 255, dtype=torch.uint8, device=DEV)
    feat = fw["feat0"].to(DEV)
    rc = L().sgn_aggregate(variant[0], variant[1], _lib.ptr(bp16(name)) if variant[1] else None, None, ctypes.byref(dv.pt),
                           ctypes.byref(dv.qo), sc.S_cap, sc.K, _lib.ptr(blob), _lib.ptr(feat), None, None, _lib.ptr(ws), nb, 1,
                           _lib.stream_handle())
    _lib.check(rc, "sgn_aggregate")
    torch.cuda.synchronize()
    n = sc.items
    fs = ws[:nb].view(torch.float16).view(-1, 256)
    assert _all_nan(fs[n:]) and bool((ws[nb:] == 255).all())
    mine = torch.zeros(feat.shape[0], dtype=torch.bool)
    mine[sc.work.long()] = True
    assert _same_bits(feat.cpu()[:, 1:], fw["feat0"][:, 1:]) and _same_bits(feat.cpu()[~mine], fw["feat0"][~mine])
    rows = rows_of(name, variant, n).chunk(0, n, DEV)
    o = fr.blend_ref(fr.to_nat(fw["h3"][:8 * n], net.cm[0], 256), rows, net)
    work = sc.work.long().to(DEV)
    rep = fr.Report()
    fr._absbound(rep, "f_s (render)", fs[:n], o["fs"], 0.5 * fr.ulp16(o["fs"].abs() + o["Efs"]) + o["Efs"], o["Efs"])
    fr._absbound(rep, "alpha_s (render)", feat[work, 0], o["alpha"], o["Ealpha"])
    rep.show(f"render {name} {variant}")
    rep.assert_ok(f"render {name} {variant}")
    same = _same_bits(fs[:n].cpu(), fw["fs"][:n].cpu()) and _same_bits(feat[work, 0].cpu(), fw["feat"][work, 0].cpu())
    print(f"render {name} {variant}: f_s and alpha_s bit-identical to the save instantiation's: {same}")
    assert same == RENDER_EQUALS_SAVE
