"""The viewmlp without block3 (shading_feature_mlp_layer3 = 0) on the GPU: sgn_aggregate_exact_nb3 called
directly on hand-built scenes against the float64 restatement (tests/nb3_ref.py), then HipRenderer, the
reference-API mirrors and the model plugin against the reference's own outputs (tests/golden/reference_nb3.npz).

The kernel bar is max(1e-5, 4 x floor) x max(1, |ref|) per element, the floor measured as
tests/test_render_gpu.py does (the same restatement in torch fp32 on the GPU against the CPU) and printed."""
import argparse
import ctypes
import functools

import numpy as np
import pytest
import torch

import sgnerf_amd  # noqa: F401
from sgnerf_amd import _lib
from sgnerf_amd.model import HipPointsVolumetricModel
from sgnerf_amd.opts import HotPathOpts
from sgnerf_amd.ray_marching import NeuralPoints, NeuralPointsRayMarching, PointAggregator, fill_invalid
from sgnerf_amd.render import HipRenderer, PointTables
from sgnerf_amd.weights import init_mlp, pack_mlp

import agg_rows_ref as ar
import nb3_ref as nb
import rw2c_ref as rw
from test_agg_rows_gpu import Dev
from test_api_gpu import _gathered, _inputs
from test_render_gpu import _dense_feat
from test_train_rows_gpu import _all_nan, _same_bits

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32_TOL = 1e-5
GUARD = 3
NAN = float("nan")
VARIANTS = [(0, 0), (1, 0), (1, 96)]
# sgn_query finds K = 1, 4, 8 or 16 neighbours, so a frame of the K = 5 case cannot be queried (by any network):
# HipRenderer and model.test() are held to refusing it, and the case's reference outputs are checked where the
# project takes K = 5 -- the aggregate entry and PointAggregator.forward on the golden's own neighbours
QUERY_K = (1, 4, 8, 16)


def L():
    return _lib.lib()


# ---- 1. the aggregate entry on hand-built scenes ---------------------------------------------------------
def counts(K, items):
    """`items` work items with 1 .. K neighbours (the first two K and 1), a sample without any neighbour in front
    and after every third item."""
    c = [K, 1] + [(3 * i) % K + 1 for i in range(2, items)]
    return ar.with_empties(c[:items] if items > 1 else [1])


@functools.lru_cache(maxsize=None)
def scene(K, items):
    sc = ar.Scene(K, counts(K, items), seed=29, bpnet=True)
    assert sc.items == items and sc.S > items and 1 in sc.work_counts
    return sc


@functools.lru_cache(maxsize=None)
def weights(variant):
    st = init_mlp(7, bias_std=0.1, bpnet_layers=variant[0], bpnet_dim=variant[1], block3_layers=0)
    return st, pack_mlp(st, DEV, "exact", block3_layers=0)


def run(sc, variant=(0, 0), pers=False, rot=None, ws_items=None, null_tables=True):
    """sgn_aggregate_exact_nb3 on a scene: feat, blend, wnorm (CPU, with guard rows), f_s of a one-chunk run."""
    dv = Dev(sc, pers)
    if null_tables:
        dv.pt.color = dv.pt.dir = None
    if rot is not None:
        dv.d["rot9"] = rot.reshape(sc.N, 9).contiguous().to(DEV)
        dv.pt.rot = dv.d["rot9"].data_ptr()
        dv.d["viewdir"] = torch.full((sc.S_cap + GUARD, 3), NAN, device=DEV)
        _lib.check(L().sgn_sample_viewdirs(ctypes.byref(dv.pt), ctypes.byref(dv.qo), sc.S_cap, sc.K,
                                           _lib.ptr(dv.d["viewdir"]), _lib.stream_handle()), "sgn_sample_viewdirs")
        dv.pt.samp_viewdir = dv.d["viewdir"].data_ptr()
    _, packed = weights(variant)
    n = sc.S_cap * sc.K
    blend, wnorm = (torch.full((n + GUARD,), NAN, device=DEV) for _ in range(2))
    feat0 = torch.randn(sc.S_cap + GUARD, 4, generator=torch.Generator().manual_seed(3 + sc.S_cap))
    feat = feat0.to(DEV)
    cap = sc.S_cap if ws_items is None else ws_items
    ws = torch.full(((cap + GUARD) * 1024,), 255, dtype=torch.uint8, device=DEV)
    _lib.check(L().sgn_aggregate_exact_nb3(variant[0], variant[1], dv.bp(variant), ctypes.byref(dv.pt), ctypes.byref(dv.qo),
                                           sc.S_cap, sc.K, _lib.ptr(packed), _lib.ptr(feat), _lib.ptr(blend), _lib.ptr(wnorm),
                                           _lib.ptr(ws), cap * 1024, _lib.stream_handle()), "sgn_aggregate_exact_nb3")
    torch.cuda.synchronize()
    assert bool((ws[cap * 1024:] == 255).all()), "the workspace was written past its size"
    fs = ws[:sc.items * 1024].view(torch.float32).view(sc.items, 256).cpu() if ws_items is None else None
    return dict(feat=feat.cpu(), feat0=feat0, blend=blend.cpu(), wnorm=wnorm.cpu(), fs=fs, pers=getattr(dv, "pers", None))


def check(sc, variant, r, what, rot=None):
    st, _ = weights(variant)
    o = nb.chain(sc, st, pers=r["pers"], rot=rot)
    fl = nb.floor(sc, st, DEV, pers=r["pers"], rot=rot)
    bar = {k: max(F32_TOL, 4.0 * v) for k, v in fl.items()}
    work = sc.work.long()
    idx = sc.rs * sc.K + sc.rk
    n = sc.S_cap * sc.K
    err = dict(alpha=nb.rel(r["feat"][work, 0], o["alpha"]), rgb=nb.rel(r["feat"][work, 1:], o["rgb"]),
               blend=nb.rel(r["blend"][idx], o["rw"][:, 0]), wnorm=nb.rel(r["wnorm"][idx], o["rw"][:, 1]))
    if r["fs"] is not None:
        err["fs"] = nb.rel(r["fs"], o["fs"])
    print(f"{what}: fp32 floor (torch GPU vs CPU) " + ", ".join(f"{k} {v:.2e}" for k, v in fl.items()) +
          "; max error / max(1, |ref|) " + ", ".join(f"{k} {v:.2e}" for k, v in err.items()) +
          f" (max |alpha| {float(o['alpha'].abs().max()):.2e}, max |f_s| {float(o['fs'].abs().max()):.2e})")
    assert err["alpha"] <= bar["alpha"] and err["rgb"] <= bar["rgb"]
    assert err["blend"] <= bar["rw"] and err["wnorm"] <= bar["rw"]
    assert err.get("fs", 0.0) <= bar["fs"]
    # every other word keeps its bits: samples without a neighbour, slack samples, guard rows, empty slots are 0
    is_item = torch.zeros(sc.S_cap + GUARD, dtype=torch.bool)
    is_item[work] = True
    assert _same_bits(r["feat"][~is_item], r["feat0"][~is_item])
    assert _all_nan(r["blend"][n:]) and _all_nan(r["wnorm"][n:])
    valid = torch.zeros(n, dtype=torch.bool)
    valid[idx] = True
    assert bool((r["blend"][:n][~valid] == 0).all()) and bool((r["wnorm"][:n][~valid] == 0).all())
    return o


@pytest.mark.parametrize("K,items", [(8, 1), (8, 7), (8, 9), (8, 17), (5, 9), (5, 17), (1, 7)])
def test_entry_base(K, items):
    """1, 7, 9 and 17 work items (a workgroup's tile is 8), K 1 / 5 / 8, samples without a neighbour and with a
    single one, the colour and dir tables NULL; a second run gives the same bits."""
    sc = scene(K, items)
    r = run(sc)
    check(sc, (0, 0), r, f"nb3 K={K} items={items}")
    r2 = run(sc)
    assert all(_same_bits(r[k], r2[k]) for k in ("feat", "blend", "wnorm", "fs"))


@pytest.mark.parametrize("variant", VARIANTS[1:], ids=lambda v: f"{v[0]}_{v[1]}")
@pytest.mark.parametrize("K,items", [(8, 17), (5, 9)])
def test_entry_bpnet(K, items, variant):
    """block2_bpnet.0 on 256 and on 352 inputs as the last row layer."""
    sc = scene(K, items)
    check(sc, variant, run(sc, variant), f"nb3 bpnet {variant} K={K} items={items}")


@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: f"{v[0]}_{v[1]}")
def test_entry_given_pers(variant):
    """The caller's camera-space coordinates (the compatibility path's instantiations)."""
    sc = scene(8, 17)
    check(sc, variant, run(sc, variant, pers=True), f"nb3 pers {variant}")


@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: f"{v[0]}_{v[1]}")
@pytest.mark.parametrize("ws_items", [8, 3])
def test_entry_chunked_workspace(variant, ws_items):
    """A workspace for fewer items than S: three chunks (8 + 8 + 1 work items) and six; the same bits as one chunk."""
    sc = scene(8, 17)
    full = run(sc, variant)
    part = run(sc, variant, ws_items=ws_items)
    check(sc, variant, part, f"nb3 {variant} workspace of {ws_items} items")
    assert all(_same_bits(full[k], part[k]) for k in ("feat", "blend", "wnorm"))


def test_entry_rotated():
    """Per-point Rw2c: rule 1 (the world half of dists) and rule 2 (the colour MLP's view direction); the
    unrotated restatement misses."""
    sc = scene(8, 17)
    rot = rw.palette_rot(sc.N)
    r = run(sc, rot=rot)
    o = check(sc, (0, 0), r, "nb3 rotated", rot=rot)
    plain = nb.chain(sc, weights((0, 0))[0])
    assert nb.rel(plain["rgb"], o["rgb"]) > 1e-3 and torch.equal(plain["rw"], o["rw"])


def test_entry_does_not_read_colour_and_dir():
    """With the tables present, whatever they hold: the same bits as with NULL."""
    sc = scene(8, 9)
    a = run(sc)
    keep = dict(sc.points)
    try:
        sc.points = dict(keep, color=torch.full_like(keep["color"], NAN), dir=torch.full_like(keep["dir"], 1e30))
        b = run(sc, null_tables=False)
    finally:
        sc.points = keep
    assert all(_same_bits(a[k], b[k]) for k in ("feat", "blend", "wnorm", "fs"))


# ---- 2. the renderer, the API mirrors and the plugin against the reference's outputs ---------------------
@functools.lru_cache(maxsize=None)
def golden(name):
    return nb.load_case(name)


def _opts(name, **kw):
    nl, dim = nb.VARIANT[name]
    c = golden(name)[2]
    return HotPathOpts(SR=int(c["SR"]), K=int(c["K"]), shading_feature_mlp_layer3=0, shading_feature_mlp_layer2_bpnet=nl,
                       predict_semantic=1 if dim else 0, semantic_guidance=1 if dim else 0, **kw)


def _tables(name, colour=False):
    pts, _, c = golden(name)
    return PointTables(pts["xyz"], pts["embedding"], pts["color"] if colour else None, pts["dir"] if colour else None,
                       pts["conf"], DEV, bpnet=pts["bpnet"] if nb.VARIANT[name][1] else None, rot=c.get("rot"))


def _render(name, r=None, colour=False, **kw):
    pts, st, c = golden(name)
    r = r or HipRenderer(_tables(name, colour), st, _opts(name), DEV)
    R = c["raydir"].shape[0]
    if nb.VARIANT[name][1]:   # labels all 0 pass the semantic filter: the query is the golden's plain one
        kw.update(point_labels=torch.zeros(pts["xyz"].shape[0], dtype=torch.int32, device=DEV),
                  ray_labels=torch.zeros(R, dtype=torch.int32, device=DEV), seconds=5)
    near, far = (float(x) for x in c["near_far"])
    out = r.render(torch.from_numpy(c["campos"]), torch.from_numpy(c["camrotc2w"]), torch.from_numpy(c["raydir"]), near, far, **kw)
    torch.cuda.synchronize()
    return r, out


def _check_frame(name, out, what):
    """ray_mask and the neighbour indices bit-exact, RGB and the decoded features within 1e-5."""
    c = golden(name)[2]
    R, SR, K = c["raydir"].shape[0], int(c["SR"]), int(c["K"])
    np.testing.assert_array_equal(out.ray_mask.cpu().numpy(), c["ray_mask"])
    keep = c["ray_mask"].astype(bool)
    dense, sr, slot, valid = _dense_feat(out, R, SR)
    S = len(valid)
    pid = np.full((R, SR, K), -1, np.int32)
    pid[sr, slot] = out.query.pidx[:S * K].view(S, K).cpu().numpy()
    np.testing.assert_array_equal(pid[keep], c["sample_pidx"])
    err = float(np.abs(out.rgb.cpu().numpy() - c["full_color"]).max())
    ferr = float((np.abs(dense[keep] - c["decoded"]) / np.maximum(1.0, np.abs(c["decoded"]))).max())
    print(f"{what} {name}: max |rgb - reference| = {err:.3e}, max |decoded - reference| / max(1, |ref|) = {ferr:.3e}")
    assert err <= F32_TOL and ferr <= F32_TOL
    return keep


@pytest.mark.parametrize("name", nb.CASES)
def test_renderer_matches_reference(name):
    """HipRenderer on point tables without colour and dir; the frame rendered twice is bitwise equal; the renderer
    packed only the plain-fp32 blob and ran no projection, frame-point list or range check."""
    if int(golden(name)[2]["K"]) not in QUERY_K:
        with pytest.raises(_lib.SgnError, match="K must be 1, 4, 8 or 16"):
            _render(name, want_blend=True)
        return
    r, out = _render(name, want_blend=True)
    assert r.exact and r.packed is None and r._proj is None and r._fp is None and not r._pending
    keep = _check_frame(name, out, "HipRenderer")
    c = golden(name)[2]
    op = out.opacity.cpu().numpy()
    assert float(np.abs(op[keep] - c["opacity"]).max()) <= F32_TOL
    assert float(np.abs(out.bg_transmission.cpu().numpy()[keep] - c["bg_transmission"]).max()) <= F32_TOL
    first = [t.clone() for t in (out.rgb, out.opacity, out.bg_transmission, out.feat, out.blend)]
    _, out2 = _render(name, r, want_blend=True)
    assert all(torch.equal(a, b) for a, b in zip(first, (out2.rgb, out2.opacity, out2.bg_transmission, out2.feat, out2.blend)))


def test_renderer_weights_depth_and_probe():
    """want_weights (the reference's `weight`), the depth map and the hole-probe maps of one case (tables with
    colour and dir: the probe averages them); early_stop is accepted and the frame rendered in full."""
    name = "base"
    pts, st, c = golden(name)
    r, out = _render(name, colour=True, want_weights=True, want_depth=True, want_probe=True)
    keep = _check_frame(name, out, "HipRenderer (weights, depth, probe)")
    R, SR, K = c["raydir"].shape[0], int(c["SR"]), int(c["K"])
    _, sr, slot, valid = _dense_feat(out, R, SR)
    S = len(valid)
    w = np.zeros((R, SR, K), np.float32)
    w[sr, slot] = out.wnorm[:S].cpu().numpy()
    assert float(np.abs(w[keep] - c["weight"]).max()) <= F32_TOL
    # depth = sum w z / (sum w + 1e-6) over the blend weights and the samples' camera-space z
    locw = out.query.samp_locw[:S * 3].view(S, 3).cpu().double()
    z = ((locw - torch.from_numpy(c["campos"]).double()) @ torch.from_numpy(c["camrotc2w"]).double().reshape(3, 3))[:, 2]
    zd = np.zeros((R, SR))
    zd[sr, slot] = z.numpy()
    bw = out.blendw.cpu().double().numpy()
    depth = (bw * zd).sum(1) / (bw.sum(1) + 1e-6)
    got = out.depth.cpu().numpy()
    assert float(np.abs(got[keep] - depth[keep]).max()) <= F32_TOL * max(1.0, float(depth.max()))
    assert bool((got[~keep] == 0).all()) and float(got[keep].min()) > 0
    assert out.probe.shape == (R, _lib.PROBE_RECORD) and bool(torch.isfinite(out.probe).all())
    pr = out.probe.cpu().numpy()
    assert bool((pr[~keep] == 0).all()) and float(np.abs(pr[keep][:, 0] - c["opacity"].max(1)).max()) <= F32_TOL
    # the probe refuses tables without colour and dir instead of reading NULL
    with pytest.raises(ValueError, match="colour and dir"):
        _render(name, want_probe=True)
    # early ray termination: accepted, rendered in full (as on the plain-fp32 path of the stock network)
    es = HipRenderer(_tables(name), st, _opts(name, early_stop=1e-2), DEV)
    _, plain = _render(name)
    rgb = plain.rgb.clone()
    _, oe = _render(name, es)
    assert oe.stop_slot is None and oe.skipped is None and torch.equal(oe.rgb, rgb)


def test_renderer_refuses_stock_tables_misuse():
    """The stock network on tables without colour / dir raises instead of reading NULL."""
    pts, _, c = golden("base")
    r = HipRenderer(_tables("base"), init_mlp(0), HotPathOpts(SR=int(c["SR"])), DEV)
    with pytest.raises(ValueError, match="colour / dir"):
        _render("base", r)


@pytest.mark.parametrize("name", nb.CASES)
def test_model_test_matches_reference(name, tmp_path):
    """The plugin: initialize from a namespace with shading_feature_mlp_layer3 = 0, load_networks of a
    reference-layout .pth without block3 keys (and, for two cases, without points_color / points_dir), test()."""
    pts, st, c = golden(name)
    nl, dim = nb.VARIANT[name]
    n = pts["xyz"].shape[0]
    sd = {"neural_points.xyz": torch.from_numpy(pts["xyz"]), "neural_points.points_embeding": torch.from_numpy(pts["embedding"])[None],
          "neural_points.points_conf": torch.from_numpy(pts["conf"]).reshape(1, n, 1)}
    if name not in ("base", "rot"):
        sd["neural_points.points_color"] = torch.from_numpy(pts["color"])[None]
        sd["neural_points.points_dir"] = torch.from_numpy(pts["dir"])[None]
    if dim:
        sd["neural_points.bpnet_points_embedding"] = torch.from_numpy(pts["bpnet"])[None]
        sd["neural_points.points_label"] = torch.zeros(n, 1, dtype=torch.int32)
    if "rot" in c:
        sd["neural_points.Rw2c"] = torch.from_numpy(c["rot"])
    sd.update({"aggregator." + k: v for k, v in st.items()})
    (tmp_path / "scene").mkdir()
    torch.save(sd, tmp_path / "scene" / "5_net_ray_marching.pth")
    opt = argparse.Namespace(SR=int(c["SR"]), K=int(c["K"]), gpu_ids=[0], is_train=False, checkpoints_dir=str(tmp_path),
                             name="scene", bg_color="white", shading_feature_mlp_layer3=0,
                             shading_feature_mlp_layer2_bpnet=nl, predict_semantic=1 if dim else 0,
                             semantic_guidance=1 if dim else 0)
    m = HipPointsVolumetricModel()
    m.initialize(opt)
    m.load_networks(5)
    inp = _inputs(c)
    if dim:
        inp["pixel_label"] = torch.zeros(1, c["raydir"].shape[0], 1, dtype=torch.int32, device=DEV)
    m.set_input(inp)
    if int(c["K"]) not in QUERY_K:
        with pytest.raises(_lib.SgnError, match="K must be 1, 4, 8 or 16"):
            m.test()
        return
    out = m.test()
    np.testing.assert_array_equal(out["ray_mask"][0].cpu().numpy(), c["ray_mask"])
    err = float(np.abs(out["coarse_raycolor"][0].cpu().numpy() - c["full_color"]).max())
    keep = c["ray_mask"].astype(bool)
    werr = float(np.abs(out["weight"][0].cpu().numpy()[keep] - c["weight"]).max())
    cerr = float(np.abs(out["conf_coefficient"][0].cpu().numpy()[keep] - c["conf_coefficient"]).max())
    print(f"model.test() {name}: max |rgb - reference| = {err:.3e}, weight {werr:.3e}, conf_coefficient {cerr:.3e}")
    assert err <= F32_TOL and werr <= F32_TOL and cerr <= F32_TOL
    with pytest.raises(NotImplementedError, match="shading_feature_mlp_layer3"):
        m.setup_optimizer(opt)
    with pytest.raises(NotImplementedError, match="shading_feature_mlp_layer3"):
        m.optimize_parameters()


@pytest.mark.parametrize("name", ["base", "base_k5", "bp352"])
def test_api_mirrors_match_reference(name):
    """NeuralPointsRayMarching.forward (bg_ray included; the cases sgn_query can find) and PointAggregator.forward
    with an identity rotation (every case, K = 5 included), neither given the points' colour or dir."""
    pts, st, c = golden(name)
    dim = nb.VARIANT[name][1]
    n = pts["xyz"].shape[0]
    err = berr = 0.0
    if int(c["K"]) in QUERY_K:
        npnts = NeuralPoints(pts["xyz"], pts["embedding"], None, None, pts["conf"], DEV)
        if dim:
            npnts.set_bpnet_feats(None, torch.zeros(n, dtype=torch.int32), torch.from_numpy(pts["bpnet"]))
        rm = NeuralPointsRayMarching(npnts, {"aggregator." + k: v for k, v in st.items()}, _opts(name), DEV)
        inp = _inputs(c)
        R = c["raydir"].shape[0]
        if dim:
            inp["pixel_label"] = torch.zeros(1, R, 1, dtype=torch.int32, device=DEV)
        out = fill_invalid(rm.forward(inp), inp)
        np.testing.assert_array_equal(out["ray_mask"][0].cpu().numpy(), c["ray_mask"])
        err = float(np.abs(out["coarse_raycolor"][0].cpu().numpy() - c["full_color"]).max())
        # a per-ray background: T_bg * bg_ray + the colour composited without background
        bg_ray = torch.rand(1, R, 3, generator=torch.Generator().manual_seed(4)).to(DEV)
        full = rm.render(dict(inp, bg_ray=bg_ray))
        black = rm.render(dict(inp, bg_color=torch.zeros(1, 3, device=DEV)))
        want = black["coarse_raycolor"] + black["coarse_is_background"] * bg_ray
        berr = float((full["coarse_raycolor"] - want).abs().max())
    # the sub-boundary: pre-gathered neighbours, the colour and dir arguments None
    args = _gathered(pts, c)
    args["sampled_color"] = args["sampled_dir"] = None
    if dim:
        pidx = c["sample_pidx"]
        lab = pts["bpnet"][np.clip(pidx, 0, None).reshape(-1)].reshape(pidx.shape + (96,))
        args["sampled_label_embedding"] = torch.from_numpy(np.ascontiguousarray(lab))[None].to(DEV)
    dec, valid, weight, conf = PointAggregator(st, _opts(name), DEV)(**args)
    np.testing.assert_array_equal(valid[0].cpu().numpy(), c["ray_valid"])
    derr = float((np.abs(dec[0].cpu().numpy() - c["decoded"]) / np.maximum(1.0, np.abs(c["decoded"]))).max())
    werr = float(np.abs(weight[0].cpu().numpy() - c["weight"]).max())
    print(f"API mirrors {name}: forward max |rgb - reference| = {err:.3e}, bg_ray {berr:.3e}; PointAggregator decoded "
          f"{derr:.3e}, weight {werr:.3e}")
    assert err <= F32_TOL and berr <= F32_TOL and derr <= F32_TOL and werr <= F32_TOL
    assert float(np.abs(conf[0].cpu().numpy() - c["conf_coefficient"]).max()) == 0.0
    # a non-identity rotation stays refused on the compatibility path
    with pytest.raises(NotImplementedError, match="sampled_Rw2c"):
        PointAggregator(st, _opts(name), DEV)(**dict(args, sampled_Rw2c=rw.palette()[1]))
