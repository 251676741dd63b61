"""The viewmlp without block3 (shading_feature_mlp_layer3 = 0) without a GPU: the float64 restatement
(tests/nb3_ref.py) against the reference's own outputs (tests/golden/reference_nb3.npz), the options, the weight
handling, the C entries' argument checks and the model plugin."""
import argparse
import ctypes

import numpy as np
import pytest
import torch

import sgnerf_amd  # noqa: F401
from sgnerf_amd import _lib, weights
from sgnerf_amd.opts import HotPathOpts
from sgnerf_amd.ray_marching import NeuralPoints
from sgnerf_amd.render import PointTables

import agg_rows_ref as ar
import nb3_ref as nb
from test_plugin_cpu import N, _model


# ---- the restatement against the reference ----------------------------------------------------------
@pytest.mark.parametrize("name", nb.CASES)
def test_chain_reproduces_reference(name):
    """decoded (alpha_s, rgb), weight and conf_coefficient of the reference's PointAggregator, per element, at the
    bar the float64 restatements of the stock network hold an fp32 golden to (test_rw2c_ref_cpu.py: 1e-5 x
    max(1, |ref|)); the figures are recorded in profiles/nb3_tests.txt."""
    pts, st, case = nb.load_case(name)
    sc = nb.GoldenScene(pts, case)
    o = nb.chain(sc, st, rot=sc.rot)
    ref = torch.from_numpy(case["decoded"]).double()
    err = nb.rel(sc.decoded(o), ref)
    werr = nb.rel(sc.slots(o), torch.from_numpy(case["weight"]))
    conf = torch.clamp(sc.points["conf"].reshape(-1)[sc.query["pidx"].clamp(min=0).long()], 1e-4, 1.0).view(sc.Rv, sc.SR, sc.K)
    cerr = nb.rel(conf, torch.from_numpy(case["conf_coefficient"]))
    print(f"{name}: max |chain - reference| / max(1, |ref|): decoded {err:.3e} (max |decoded| {float(ref.abs().max()):.3e}), "
          f"weight {werr:.3e}, conf_coefficient {cerr:.3e}")
    assert err <= ar.F32_TOL and werr <= ar.F32_TOL and cerr <= ar.F32_TOL
    assert np.array_equal(case["ray_valid"], (case["sample_pidx"] >= 0).any(-1))
    # what the file promises: partial and full neighbour sets, the parameter count, no block3
    nnb = sc.query["samp_nnb"]
    assert int(((nnb > 0) & (nnb < sc.K)).sum()) > 0 and int((nnb == sc.K).sum()) > 0
    assert sum(v.numel() for v in st.values()) == nb.N_PARAMS[nb.VARIANT[name]]
    if name == "rot":   # really rotated: the unrotated chain misses
        assert nb.rel(sc.decoded(nb.chain(sc, st)), ref) >= 1e-3


def test_restatement_shares_its_pieces_with_the_stock_one():
    """Row inputs (dists, weights) and the colour MLP are the stock restatement's, bit for bit, on a hand-built
    scene; the colour and dir tables do not enter."""
    sc = ar.scene("pairs")
    st = weights.init_mlp(5, bias_std=0.1, block3_layers=0)
    d, _, rw = ar.row_inputs(sc, torch.float64)
    o = nb.chain(sc, st)
    assert torch.equal(o["dists"], d) and torch.equal(o["rw"], rw)
    assert torch.equal(o["rgb"], ar.colour_ref(o["fs"], o["v"], st))
    pers = sc.pers32()
    d, _, rw = ar.row_inputs(sc, torch.float64, pers)
    op = nb.chain(sc, st, pers=pers)
    assert torch.equal(op["dists"], d) and torch.equal(op["rw"], rw)
    keep = dict(sc.points)
    try:
        sc.points = {k: v for k, v in keep.items() if k not in ("color", "dir")}
        o2 = nb.chain(sc, st)
    finally:
        sc.points = keep
    assert all(torch.equal(o[k], o2[k]) for k in ("alpha", "rgb", "fs"))


# ---- options ------------------------------------------------------------------------------------------
def test_options():
    assert HotPathOpts().shading_feature_mlp_layer3 == 2 and HotPathOpts().block3_layers == 2
    HotPathOpts().check_supported()
    o = HotPathOpts(shading_feature_mlp_layer3=0).check_supported()
    assert o.block3_layers == 0
    for bad in (1, 3):
        with pytest.raises(NotImplementedError, match="layer counts"):
            HotPathOpts(shading_feature_mlp_layer3=bad).check_supported()
    with pytest.raises(NotImplementedError, match="shading_feature_mlp_layer3.*f16"):
        HotPathOpts(shading_feature_mlp_layer3=0, precision="f16").check_supported()
    with pytest.raises(NotImplementedError, match="shading_feature_mlp_layer3.*train"):
        HotPathOpts(shading_feature_mlp_layer3=0, is_train=1).check_supported()
    HotPathOpts(precision="f16", is_train=1).check_supported()            # the stock network: as before
    HotPathOpts(shading_feature_mlp_layer3=0, early_stop=1e-2).check_supported()   # accepted, rendered in full
    for nl, ps in ((1, 0), (1, 1)):
        HotPathOpts(shading_feature_mlp_layer3=0, shading_feature_mlp_layer2_bpnet=nl, predict_semantic=ps,
                    semantic_guidance=ps).check_supported()
    # a namespace without the setting is the stock network
    ns = argparse.Namespace(SR=24, K=8)
    assert HotPathOpts.from_opt(ns) == HotPathOpts(SR=24, K=8)
    assert HotPathOpts.from_opt(argparse.Namespace(shading_feature_mlp_layer3=0)).block3_layers == 0


def test_trainer_refuses():
    from sgnerf_amd.train_hip import HipTrainer
    for is_train in (0, 1):
        with pytest.raises(NotImplementedError, match="shading_feature_mlp_layer3"):
            HipTrainer(None, {}, HotPathOpts(shading_feature_mlp_layer3=0, is_train=is_train), "cpu")


# ---- weights ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [(0, 0), (1, 0), (1, 96)])
def test_weights(variant):
    nl, dim = variant
    st = weights.init_mlp(3, bias_std=0.01, bpnet_layers=nl, bpnet_dim=dim, block3_layers=0)
    assert sum(v.numel() for v in st.values()) == nb.N_PARAMS[variant]
    layers = weights.layers_for(nl, dim, block3_layers=0)
    assert [n for n, *_ in layers] == ["block1.0", "block1.2", "alpha_branch.0", "color_branch.0", "color_branch.2",
                                       "color_branch.4", "color_branch.6"] + (["block2_bpnet.0"] if nl else [])
    assert weights.block3_layers(st) == 0 and weights.mlp_variant(st) == variant
    full = {"aggregator." + k: v for k, v in st.items()}
    full["neural_points.xyz"] = torch.zeros(3, 3)
    assert weights.block3_layers(full) == 0
    assert sorted(weights.strip_prefix(full, block3_layers=0)) == sorted(st)
    weights.check_shapes(st, block3_layers=0)
    with pytest.raises(KeyError, match="block3"):      # the present arguments behave as before
        weights.strip_prefix(full)
    stock = weights.init_mlp(3, bpnet_layers=nl, bpnet_dim=dim)
    assert weights.block3_layers(stock) == 2
    with pytest.raises(ValueError, match="shading_feature_mlp_layer3"):
        weights.strip_prefix(stock, block3_layers=0)
    bad = dict(st)
    bad["block1.2.weight"] = torch.zeros(256, 255)
    with pytest.raises(ValueError, match="block1.2"):
        weights.check_shapes(bad, block3_layers=0)
    with pytest.raises(NotImplementedError):
        weights.layers_for(nl, dim, block3_layers=1)
    with pytest.raises(NotImplementedError):
        weights.block3_layers({"block3.0.weight": 0, "block3.0.bias": 0})
    # defaults unchanged
    assert weights.layers_for(nl, dim)[:9] == weights.LAYERS and len(weights.LAYERS) == 9 and weights.N_PARAMS == 341_764
    a, b = weights.init_mlp(3, bpnet_layers=nl, bpnet_dim=dim), weights.init_mlp(3, bpnet_layers=nl, bpnet_dim=dim, block3_layers=2)
    assert all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("key", ["base", "bp256", "bp352"])
def test_keys_equal_the_reference_state_dict(key):
    """The golden file records the key order of the reference module's state dict (no block3.* among them):
    init_mlp draws exactly those (golden_state also pins the weights to the checksums the reference was run on)."""
    g = np.load(nb.GOLDEN, allow_pickle=False)
    keys = [str(k) for k in g[f"mlp_{key}/keys"]]
    st = nb.golden_state(key)
    assert sorted(keys) == sorted(st) and not any(k.startswith("block3.") for k in keys)
    nl, dim = (int(x) for x in g[f"mlp_{key}/variant"])
    want = [n + s for n, *_ in weights.layers_for(nl, dim, block3_layers=0) for s in (".weight", ".bias")]
    assert sorted(want) == sorted(keys)


def test_renderer_and_pack_refuse_mismatched_weights():
    """Weights and options that disagree raise ValueError before anything is packed (no GPU needed)."""
    from sgnerf_amd.render import HipRenderer
    r = HipRenderer.__new__(HipRenderer)
    r.device = torch.device("cpu")
    r.opts = HotPathOpts(shading_feature_mlp_layer3=0)
    with pytest.raises(ValueError, match="shading_feature_mlp_layer3"):
        r.set_mlp(weights.init_mlp(0))
    r.opts = HotPathOpts()
    with pytest.raises(ValueError, match="shading_feature_mlp_layer3"):
        r.set_mlp(weights.init_mlp(0, block3_layers=0))
    r.opts = HotPathOpts(shading_feature_mlp_layer3=0, shading_feature_mlp_layer2_bpnet=1)
    with pytest.raises(ValueError, match="block2_bpnet"):
        r.set_mlp(weights.init_mlp(0, block3_layers=0))
    with pytest.raises(ValueError, match="exact"):
        weights.pack_mlp(weights.init_mlp(0, block3_layers=0), "cpu", "f32", block3_layers=0)


def test_point_tables_without_colour_and_dir():
    z = torch.zeros(5, 3)
    t = PointTables(z, torch.zeros(5, 32), None, None, torch.ones(5, 1), "cpu")
    assert t.color is None and t.dir is None and t.n == 5
    p = NeuralPoints(z, torch.zeros(1, 5, 32), None, None, torch.ones(1, 5, 1), "cpu")
    assert p.points_color is None and p.points_dir is None
    sd = p.state_dict()
    assert "neural_points.points_color" not in sd and "neural_points.points_dir" not in sd
    q = NeuralPoints.from_state_dict(sd, "cpu")
    assert q.points_color is None and torch.equal(q.points_embeding, p.points_embeding)
    assert p.tables().color is None and p._version_key() == p._version_key()


# ---- C entries ----------------------------------------------------------------------------------------
def test_entries_exported_and_sized():
    L = _lib.lib()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in ("sgn_mlp_packed_bytes_exact_nb3", "sgn_mlp_pack_exact_nb3", "sgn_aggregate_exact_nb3"):
        assert n in _lib.SIGNATURES and hasattr(raw, n)
    assert _lib.ABI_VERSION == 23 and L.sgn_abi_version() == 23
    assert _lib.SIGNATURES["sgn_aggregate_exact_nb3"] == _lib.SIGNATURES["sgn_aggregate_exact"]
    assert _lib.SIGNATURES["sgn_mlp_pack_exact_nb3"] == _lib.SIGNATURES["sgn_mlp_pack_exact"]
    base, b256, b352 = (L.sgn_mlp_packed_bytes_exact_nb3(nl, dim) for nl, dim in ((0, 0), (1, 0), (1, 96)))
    assert 0 < base < b256 < b352
    for (nl, dim), nb3 in (((0, 0), base), ((1, 0), b256), ((1, 96), b352)):
        assert nb3 < L.sgn_mlp_packed_bytes_exact(nl, dim)
        assert nb3 >= 4 * nb.N_PARAMS[(nl, dim)]              # every parameter as fp32 (+ padding)
        # block3.0 (272 padded inputs) and block3.2 with their biases are what is gone
        assert L.sgn_mlp_packed_bytes_exact(nl, dim) - nb3 == 4 * (272 * 256 + 256 + 256 * 256 + 256)
    assert L.sgn_mlp_packed_bytes_exact_nb3(2, 0) == 0 and L.sgn_mlp_packed_bytes_exact(2, 0) == 0
    assert L.sgn_mlp_packed_bytes_exact_nb3(1, 64) == 0


def test_argument_errors_are_reported_before_any_hip_call():
    """Pointers are never dereferenced: the checks come first (addresses that nothing could read)."""
    L = _lib.lib()
    A = 4096
    p = ctypes.c_void_p(A)
    pt = _lib.PointTables()
    for k in ("xyz", "embedding", "conf", "campos", "camrotc2w", "raydir"):   # colour and dir stay NULL
        setattr(pt, k, A)
    pt.n_points = 8
    qo = _lib.QueryOut()
    for k, _ in qo._fields_:
        setattr(qo, k, A)
    P, Q = ctypes.byref(pt), ctypes.byref(qo)
    big = 1 << 20

    def refused(rc, what, *words):
        assert rc != 0, what
        msg = L.sgn_last_error().decode()
        assert "invalid argument" in msg and all(w in msg for w in words), f"{what}: {msg}"

    agg = L.sgn_aggregate_exact_nb3
    refused(agg(0, 0, None, P, Q, 8, 9, p, p, None, None, p, big, None), "K = 9", "K = 1 .. 8")
    refused(agg(0, 0, None, P, Q, 8, 0, p, p, None, None, p, big, None), "K = 0", "K = 1 .. 8")
    refused(agg(0, 0, None, P, Q, 8, 8, p, p, None, None, p, 1023, None), "workspace", "workspace too small")
    refused(agg(2, 0, None, P, Q, 8, 8, p, p, None, None, p, big, None), "two bpnet layers", "block2_bpnet")
    refused(agg(1, 96, None, P, Q, 8, 8, p, p, None, None, p, big, None), "no bpnet table", "bpnet_dim")
    refused(agg(0, 0, None, P, Q, 8, 8, ctypes.c_void_p(A + 4), p, None, None, p, big, None), "alignment", "alignment")
    refused(agg(0, 0, None, P, Q, 8, 8, None, p, None, None, p, big, None), "no blob", "null")
    pt.conf = None
    refused(agg(0, 0, None, P, Q, 8, 8, p, p, None, None, p, big, None), "no conf", "point tables")
    pt.conf = A
    pt.rot = A
    refused(agg(0, 0, None, P, Q, 8, 8, p, p, None, None, p, big, None), "rot without viewdirs", "samp_viewdir")
    pt.samp_viewdir = A
    for nl, dim in ((1, 0), (1, 96)):
        refused(agg(nl, dim, p, P, Q, 8, 8, p, p, None, None, p, big, None), "rot with bpnet", "rot", "base network")
    pt.pers = pt.samp_pers = A
    refused(agg(0, 0, None, P, Q, 8, 8, p, p, None, None, p, big, None), "rot with pers", "rot", "pers")
    pt.rot = pt.samp_viewdir = None
    pt.samp_pers = None
    refused(agg(0, 0, None, P, Q, 8, 8, p, p, None, None, p, big, None), "pers alone", "pers and samp_pers")
    # the stock entry still needs colour and dir
    pt.pers = None
    refused(L.sgn_aggregate_exact(0, 0, None, P, Q, 8, 8, p, p, None, None, p, big, None), "stock, no colour", "point tables")
    refused(L.sgn_mlp_pack_exact_nb3(0, 0, None, None, p, None), "pack", "null")
    # nothing to do is not an error, and launches nothing
    assert agg(0, 0, None, P, Q, 0, 8, p, p, None, None, p, big, None) == 0


# ---- the model plugin -----------------------------------------------------------------------------------
def test_plugin_loads_a_block3_less_state_and_refuses_training(tmp_path, monkeypatch):
    from sgnerf_amd import model as model_mod
    m = _model(tmp_path, shading_feature_mlp_layer3=0)
    assert m.opts.block3_layers == 0 and m.opts.precision == "f32"
    st = weights.init_mlp(2, bias_std=0.01, block3_layers=0)
    m.net_ray_marching.renderer.mlp_state = st
    m.save_networks(3)
    sd = torch.load(tmp_path / "scene" / "3_net_ray_marching.pth", map_location="cpu", weights_only=True)
    assert not any("block3." in k for k in sd) and "aggregator.block1.2.weight" in sd
    seen = {}

    def fake(points, state, opts, device, return_weights=True):   # no renderer on the CPU: what load_networks hands it
        seen.update(state=state, opts=opts, points=points)
        return object()
    monkeypatch.setattr(model_mod, "NeuralPointsRayMarching", fake)
    m.load_networks(3, directory=str(tmp_path / "scene"))
    assert sorted(seen["state"]) == sorted(st) and all(torch.equal(seen["state"][k], st[k]) for k in st)
    assert seen["opts"].block3_layers == 0 and seen["points"].xyz.shape == (N, 3)
    for call in (lambda: m.setup_optimizer(m.opt), lambda: m.optimize_parameters()):
        with pytest.raises(NotImplementedError, match="shading_feature_mlp_layer3"):
            call()
    # points without colour and dir are taken by this network only
    g = torch.Generator().manual_seed(1)
    r = lambda *s: torch.rand(*s, generator=g)  # noqa: E731
    m.set_points(r(9, 3), points_embedding=r(1, 9, 32), points_conf=r(1, 9, 1), aggregator_state=st)
    assert m.neural_points.points_color is None and m.neural_points.points_dir is None
    stock = _model(tmp_path)
    with pytest.raises(NotImplementedError, match="points_color"):
        stock.set_points(r(9, 3), points_embedding=r(1, 9, 32), points_conf=r(1, 9, 1), aggregator_state=st)
    # a stock checkpoint under these options is refused, naming the option
    m2 = _model(tmp_path, shading_feature_mlp_layer3=0)
    m2.net_ray_marching.renderer.mlp_state = weights.init_mlp(2)
    m2.save_networks(4)
    monkeypatch.undo()
    with pytest.raises(ValueError, match="shading_feature_mlp_layer3"):
        m2.load_networks(4, directory=str(tmp_path / "scene"))
