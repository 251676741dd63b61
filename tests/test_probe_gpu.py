"""GPU tests of the hole-probing outputs (opt.prob = 1): k_probe through the C ABI on the planted scene of
tests/probe_ref.py, then the feature end to end -- NeuralPointsRayMarching.render / forward, the renderer's
query_size override and range fallback, and the model plugin -- against the reference's lines
(models/neural_points_volumetric_model.py:636-657) restated in float64 on each call's own dense outputs.

Bounds (probe_ref.check_records; derived, not measured): the copies bit for bit; avg_* within
2^-20 sum_k |w_k x_k|; far_dist within 2^-20 of itself; zero records outside the mask."""
import argparse
import ctypes

import numpy as np
import pytest
import torch

import probe_ref as P
from helpers import load_golden
from sgnerf_amd import _lib
from sgnerf_amd.opts import HotPathOpts
from sgnerf_amd.querier import LightningFastQuerier
from sgnerf_amd.ray_marching import PROBE_FIELDS, PROBE_KEYS, NeuralPoints, NeuralPointsRayMarching, fill_invalid
from sgnerf_amd.render import HipRenderer, PointTables

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHANNELS = dict(zip(PROBE_KEYS, (1, 3, 1, 1, 3, 3, 1, 32)))


# ---- the kernel through ctypes ---------------------------------------------------------------------------
def _run_probe(sc):
    d = {k: sc[k].to(DEV) for k in ("ray_ns", "ray_soff", "samp_locw", "samp_nnb", "pidx", "xyz", "embedding", "color",
                                    "dir", "conf", "opacity", "blend", "mask")}
    pt, q = _lib.PointTables(), _lib.QueryOut()
    pt.xyz, pt.embedding, pt.color, pt.dir, pt.conf = (d[k].data_ptr() for k in ("xyz", "embedding", "color", "dir", "conf"))
    pt.n_points = sc["xyz"].shape[0]
    q.ray_ns, q.ray_soff, q.samp_locw, q.samp_nnb, q.pidx = (d[k].data_ptr() for k in ("ray_ns", "ray_soff", "samp_locw",
                                                                                         "samp_nnb", "pidx"))
    R = sc["R"]
    out = torch.full((R + 1, P.REC), float("nan"), dtype=torch.float32, device=DEV)   # one record of slack
    _lib.check(_lib.lib().sgn_probe(ctypes.byref(pt), ctypes.byref(q), _lib.ptr(d["opacity"]), _lib.ptr(d["blend"]),
                                    _lib.ptr(d["mask"]), R, sc["SR"], sc["K"], _lib.ptr(out), _lib.stream_handle()),
               "sgn_probe")
    torch.cuda.synchronize()
    out = out.cpu()
    assert bool(torch.isnan(out[R]).all()), "wrote past the last ray's record"
    return out[:R]


@pytest.mark.parametrize("K", [1, 3, 8])
@pytest.mark.parametrize("SR", [1, 7, 24, 64])
@pytest.mark.parametrize("R", [1, 63, 64, 65, 200])
def test_probe_kernel_on_planted_scene(R, SR, K):
    sc = P.probe_scene(R, SR, K)
    if (R, SR, K) == (200, 24, 8):
        assert sc["skipped"] == []
    ref = P.probe_ref(sc)
    got = _run_probe(sc)
    P.check_records(got, ref, sc["mask"], what=f"R {R} SR {SR} K {K} (skipped: {','.join(sc['skipped']) or 'none'}): ")


# ---- end to end on the golden patch --------------------------------------------------------------------------
def _inputs(case):
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    R = case["raydir"].shape[0]
    near, far = (float(x) for x in case["near_far"])
    return {"campos": d(case["campos"])[None], "raydir": d(case["raydir"])[None],
            "camrotc2w": d(case["camrotc2w"])[None], "near": torch.tensor([[[near]]]), "far": torch.tensor([[[far]]]),
            "bg_color": torch.tensor([[1.0, 1.0, 1.0]], dtype=torch.float32, device=DEV),
            "pixel_idx": torch.zeros(1, R, 2, device=DEV), "h": 1, "w": R}


@pytest.fixture(scope="module")
def patch():
    return load_golden("reference_aggregator.npz", "patch")


def _net(patch, **kw):
    pts, mlp, case = patch
    o = HotPathOpts(SR=int(case["SR"]), **{"K": int(case["K"]), **kw})
    npnts = NeuralPoints(pts["xyz"], pts["embedding"], pts["color"], pts["dir"], pts["conf"], DEV)
    return NeuralPointsRayMarching(npnts, {"aggregator." + k: v for k, v in mlp.items()}, o, DEV), o


def _check_against_dense(out, patch, o, inp, what):
    """The eight keys of a prob = 1 render against lines 636-657 (float64, CPU) on the same call's dense
    outputs and the dense query of the same rays."""
    pts, _, case = patch
    near, far = (float(x) for x in case["near_far"])
    xyz = torch.from_numpy(pts["xyz"]).to(DEV)
    qr = LightningFastQuerier(DEV, o).query_points(None, None, xyz[None], None, 1, 1, None, near, far, inp["raydir"],
                                                   inp["campos"], inp["camrotc2w"])
    pidx, loc_w, qmask = qr[0].cpu(), qr[2].cpu(), qr[4].cpu()
    mask = out["ray_mask"][0].cpu()
    assert torch.equal(qmask[0], mask)
    keep = torch.nonzero(mask).reshape(-1)
    assert keep.numel() > 50
    R = mask.numel()
    for k in PROBE_KEYS:
        assert out[k].shape == (1, R, CHANNELS[k]) and out[k].dtype == torch.float32, k
    assert float(out["ray_max_sample_label"].abs().max()) == 0.0
    opacity = out["coarse_point_opacity"].cpu()[:, keep]                       # fp32: decides the slot
    wc = (out["weight"] * out["conf_coefficient"]).cpu()[:, keep].double()     # the reference's fp32 product
    p = pidx.clamp(min=0).long()
    tab = {k: torch.from_numpy(pts[k]).double() for k in ("xyz", "color", "dir", "conf", "embedding")}
    g = lambda k, c: tab[k].reshape(-1, c)[p]  # noqa: E731
    ref, ind = P.reference_lines_636_657(opacity, loc_w.double(), wc, g("xyz", 3), g("color", 3), g("dir", 3), g("conf", 1),
                                         g("embedding", 32))
    assert torch.equal(ind[0], P.select_slot(opacity[0]))    # CPU torch.max: the first of tied slots
    # the same bounds as the kernel test, on records put together from the keys
    got = torch.zeros(R, P.REC)
    rec = torch.zeros(R, P.REC, dtype=torch.float64)
    sumabs = torch.zeros(R, P.REC, dtype=torch.float64)
    w_sel = torch.gather(wc, 2, ind[..., None, None].expand(-1, -1, 1, wc.shape[-1]))[0, :, 0]    # [R', K]
    p_sel = torch.gather(p, 2, ind[..., None, None].expand(-1, -1, 1, p.shape[-1]))[0, :, 0]
    for key, field in P.KEY_FIELD.items():
        o_, c = P.FIELDS[field]
        assert PROBE_FIELDS[key] == (o_, c)
        got[:, o_:o_ + c] = out[key][0].cpu()
        rec[keep, o_:o_ + c] = ref[key][0].double()
        if field.startswith("avg_"):
            x = tab[field[4:]].reshape(-1, c)[p_sel]
            sumabs[keep, o_:o_ + c] = (w_sel[:, :, None] * x).abs().sum(1)
    P.check_records(got, dict(rec=rec, sumabs=sumabs), mask, what=what)


@pytest.mark.parametrize("kw", [dict(), dict(precision="f16"), dict(K=4)], ids=["f32", "f16", "K4"])
def test_render_prob_matches_reference_lines(patch, kw):
    net, o = _net(patch, **kw)
    inp = _inputs(patch[2])
    before = net.render(inp)                      # before the probe was ever requested on this renderer
    assert net.renderer.probe is None
    out = net.render(inp, prob=1)
    assert set(out) == set(before) | set(PROBE_KEYS)
    _check_against_dense(out, patch, o, inp, what=f"{kw}: ")
    # forward + fill_invalid == render
    full = fill_invalid(net.forward(inp, prob=1), inp)
    n_keep = int(out["ray_mask"].sum())
    for k in PROBE_KEYS:
        assert torch.equal(full[k], out[k]), k
    assert net.forward(inp, prob=1)["shading_avg_embedding"].shape == (1, n_keep, 32)
    # the switch off again: today's outputs, bit for bit
    for off in (net.render(inp), net.render(inp, prob=0)):
        assert set(off) == set(before)
        for k in before:
            assert torch.equal(off[k], before[k]), k
    assert set(net.forward(inp)) == set(net.forward(inp, prob=0)) and "shading_avg_conf" not in net.forward(inp)


def test_prob_read_from_namespace_at_call_time(patch):
    pts, mlp, case = patch
    opt = argparse.Namespace(SR=int(case["SR"]), K=int(case["K"]), prob=0)
    npnts = NeuralPoints(pts["xyz"], pts["embedding"], pts["color"], pts["dir"], pts["conf"], DEV)
    net = NeuralPointsRayMarching(npnts, mlp, opt, DEV)
    inp = _inputs(case)
    assert "ray_max_far_dist" not in net.render(inp)
    opt.prob = 1
    assert "ray_max_far_dist" in net.render(inp) and "ray_max_far_dist" not in net.render(inp, prob=0)


# ---- query_size override -----------------------------------------------------------------------------------
def test_query_size_override_reuses_the_grid(patch):
    pts, mlp, case = patch
    SR, K = int(case["SR"]), int(case["K"])
    tab = PointTables(pts["xyz"], pts["embedding"], pts["color"], pts["dir"], pts["conf"], DEV)
    near, far = (float(x) for x in case["near_far"])
    args = (torch.from_numpy(case["campos"]), torch.from_numpy(case["camrotc2w"]), torch.from_numpy(case["raydir"]), near, far)
    R = case["raydir"].shape[0]

    def neighbours(out):
        S = out.query.n_samples()
        return out.query.ray_ns[:R].cpu(), out.query.pidx[:S * K].cpu(), out.query.samp_locw[:S * 3].cpu()
    r3 = HipRenderer(tab, mlp, HotPathOpts(SR=SR, K=K, query_size=(3, 3, 3)), DEV)
    r1 = HipRenderer(tab, mlp, HotPathOpts(SR=SR, K=K, query_size=(1, 1, 1)), DEV)
    n3 = neighbours(r3.render(*args))
    grid, handle, info = r3.querier._grid, r3.querier._grid.handle.value, r3.grid_info()
    over = r3.render(*args, query_size=(1, 1, 1))
    n31 = neighbours(over)
    rgb31 = over.rgb.clone()
    want = r1.render(*args)
    n1 = neighbours(want)
    assert not torch.equal(n3[0], n1[0])     # the two sizes select different samples on this scene
    for a, b in zip(n31, n1):
        assert torch.equal(a, b)
    assert torch.equal(rgb31, want.rgb)
    # the redrawn flags are those of a grid built with that query_size (coor_occ), nothing else moved
    built1, built3 = r1.querier._grid.export(), HipRenderer(tab, mlp, r3.opts, DEV).querier.grid_for(tab.xyz).export()
    for a, b in zip(grid.export(), built1):
        assert torch.equal(a, b)
    assert not torch.equal(built1[0], built3[0])
    assert r3.querier._grid is grid and grid.handle.value == handle and r3.grid_info() == info   # not rebuilt
    assert r3.opts.query_size == (3, 3, 3)
    for a, b in zip(neighbours(r3.render(*args)), n3):   # for that call only
        assert torch.equal(a, b)
    assert r3.querier._grid is grid and r3.grid_info() == info
    for a, b in zip(grid.export(), built3):
        assert torch.equal(a, b)


# ---- plugin -------------------------------------------------------------------------------------------------
def test_plugin_reads_prob_and_query_size_every_call(patch, tmp_path):
    from sgnerf_amd.model import HipPointsVolumetricModel
    pts, mlp, case = patch
    opt = argparse.Namespace(SR=int(case["SR"]), K=8, gpu_ids=[0], is_train=False, checkpoints_dir=str(tmp_path),
                             name="scene", bg_color="white", prob=0)
    m = HipPointsVolumetricModel()
    m.initialize(opt)
    m.set_points(points_xyz=pts["xyz"], points_embedding=pts["embedding"], points_conf=pts["conf"],
                 points_dir=pts["dir"], points_color=pts["color"], aggregator_state=mlp)
    m.set_input(_inputs(case))
    plain = {k: v.clone() for k, v in m.test().items()}
    assert not set(PROBE_KEYS) & set(plain)
    visual = list(m.visual_names)
    R = case["raydir"].shape[0]
    m.opt.prob = 1
    m.opt.query_size = np.asarray([1, 1, 1])
    out = m.test()
    for k in PROBE_KEYS:
        assert out[k].shape == (1, R, CHANNELS[k]), k
    assert m.opts.query_size == (3, 3, 3) and m.visual_names == visual
    assert not torch.equal(out["ray_mask"], plain["ray_mask"]) or not torch.equal(out["coarse_point_opacity"],
                                                                                  plain["coarse_point_opacity"])
    # the override reached the query: the same frame from a model built with query_size 1 1 1
    m1 = HipPointsVolumetricModel()
    m1.initialize(argparse.Namespace(**{**vars(opt), "query_size": [1, 1, 1], "prob": 1}))
    m1.set_points(points_xyz=pts["xyz"], points_embedding=pts["embedding"], points_conf=pts["conf"],
                  points_dir=pts["dir"], points_color=pts["color"], aggregator_state=mlp)
    m1.set_input(_inputs(case))
    out1 = m1.test()
    for k in PROBE_KEYS + ("coarse_raycolor", "ray_mask"):
        assert torch.equal(out[k], out1[k]), k
    m.opt.prob = 0
    m.opt.query_size = [3, 3, 3]
    back = m.test()
    assert set(back) == set(plain)
    for k in plain:
        assert torch.equal(back[k], plain[k]), k


# ---- range fallback -----------------------------------------------------------------------------------------
def test_probe_follows_the_range_fallback(patch):
    """block1.2 x 30000 (test_render_gpu.test_f32_fp16_range_falls_back_to_plain_fp32's weights) leaves fp16
    range: the synchronous check re-renders the frame on the plain-fp32 path, and the probe records handed
    out are those of that pass, not of the discarded one."""
    pts, mlp, case = patch
    big = dict(mlp)
    big["block1.2.weight"] = mlp["block1.2.weight"] * 30000.0
    tab = PointTables(pts["xyz"], pts["embedding"], pts["color"], pts["dir"], pts["conf"], DEV)
    near, far = (float(x) for x in case["near_far"])
    args = (torch.from_numpy(case["campos"]), torch.from_numpy(case["camrotc2w"]), torch.from_numpy(case["raydir"]), near, far)
    r = HipRenderer(tab, big, HotPathOpts(SR=int(case["SR"]), K=int(case["K"])), DEV)
    assert not r.exact
    out = r.render(*args, want_probe=True, check_range="sync")
    assert r.exact
    first = out.probe.clone()
    assert first.shape == (case["raydir"].shape[0], P.REC) and bool(torch.isfinite(first).all())
    assert float(first[:, 0].max()) > 0
    second = r.render(*args, want_probe=True, check_range="sync").probe    # the plain-fp32 path directly
    assert torch.equal(first, second)
    direct = HipRenderer(tab, big, HotPathOpts(SR=int(case["SR"]), K=int(case["K"])), DEV)
    direct.exact = True
    assert torch.equal(first, direct.render(*args, want_probe=True).probe)
