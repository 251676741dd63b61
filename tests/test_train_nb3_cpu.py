"""Training the viewmlp without block3 (shading_feature_mlp_layer3 = 0, opts.train_rows = 1), the parts that need
no GPU: the option and its refusals, the torch reference (train.ViewMLP / aggregate / Trainer on a state without
block3.*) against the float64 restatement tests/nb3_ref.chain, and three reference steps on the CPU."""
import argparse

import pytest
import torch

import sgnerf_amd  # noqa: F401
from sgnerf_amd.opts import HotPathOpts
from sgnerf_amd.train import PointParams, Trainer, ViewMLP, aggregate
from sgnerf_amd.weights import init_mlp, layers_for

import train_nb3_ref as tn

NB3 = dict(shading_feature_mlp_layer3=0)
SG = dict(shading_feature_mlp_layer2_bpnet=1, predict_semantic=1, semantic_guidance=1)


# ---- the option --------------------------------------------------------------------------------------------
def test_option_defaults_to_off_and_is_accepted():
    assert HotPathOpts().train_rows == 0 and HotPathOpts(**NB3).train_rows == 0
    o = HotPathOpts(**NB3, is_train=1, train_rows=1).check_supported()
    assert o.train_rows == 1 and o.block3_layers == 0
    HotPathOpts(**NB3, train_rows=1).check_supported()                 # rendering options may carry it
    HotPathOpts(**NB3, **SG, is_train=1, train_rows=1).check_supported()
    # colour and dir are outside this network's graph, whatever their switches say
    assert o.trained_points == ("points_embeding", "points_conf")
    assert HotPathOpts(**NB3, train_rows=1, feat_grad=0).trained_points == ("points_conf",)
    assert HotPathOpts().trained_points == ("points_embeding", "points_color", "points_dir", "points_conf")


@pytest.mark.parametrize("kw", [dict(train_rows=1), dict(train_rows=1, is_train=1),
                                dict(train_rows=1, shading_feature_mlp_layer3=2, is_train=1),
                                dict(train_rows=1, precision="f16", **NB3), dict(train_rows=2, **NB3),
                                dict(train_rows=-1, **NB3), dict(train_rows=True, **NB3), dict(train_rows=1.0, **NB3),
                                dict(train_rows="1", **NB3), dict(train_rows=True, is_train=1, **NB3)],
                         ids=lambda kw: ",".join(f"{k}={v!r}" for k, v in kw.items()))
def test_refusals_name_the_option(kw):
    """1 only for the viewmlp without block3 in f32; anything but the integers 0 / 1 is refused."""
    with pytest.raises(NotImplementedError, match="train_rows"):
        HotPathOpts(**kw).check_supported()


def test_rows_gemm_with_is_train_stays_refused():
    for tr in (0, 1):
        with pytest.raises(NotImplementedError, match="rows_gemm"):
            HotPathOpts(**NB3, rows_gemm=1, is_train=1, train_rows=tr).check_supported()


def test_off_changes_no_refusal():
    """With 0 every pinned refusal reads as before and does not mention the option."""
    from sgnerf_amd.train_hip import HipTrainer
    cases = [(dict(**NB3, is_train=1), "shading_feature_mlp_layer3.*train"),
             (dict(**NB3, precision="f16"), "shading_feature_mlp_layer3.*f16"),
             (dict(**NB3, rows_gemm=1, is_train=1), "rows_gemm"), (dict(**NB3, rows_gemm=2), "rows_gemm"),
             (dict(**NB3, rows_gemm=True), "rows_gemm")]
    for kw, pat in cases:
        with pytest.raises(NotImplementedError, match=pat) as e:
            HotPathOpts(**kw, train_rows=0).check_supported()
        assert "train_rows" not in str(e.value), kw
    assert str(pytest.raises(NotImplementedError, HotPathOpts(**NB3, is_train=1, train_rows=0).check_supported).value) == \
        "shading_feature_mlp_layer3 = 0 renders only: training (is_train) is not implemented"
    for is_train in (0, 1):
        with pytest.raises(NotImplementedError, match="shading_feature_mlp_layer3") as e:
            HipTrainer(None, {}, HotPathOpts(**NB3, is_train=is_train, train_rows=0), "cpu")
        assert "train_rows" not in str(e.value)


def test_from_opt_and_command_line_switch():
    base = dict(shading_feature_mlp_layer3=0, SR=24)
    assert HotPathOpts.from_opt(argparse.Namespace(**base)).train_rows == 0
    assert HotPathOpts.from_opt(argparse.Namespace(**base, train_rows=None)).train_rows == 0
    assert HotPathOpts.from_opt(argparse.Namespace(**base, train_rows=0)).train_rows == 0
    o = HotPathOpts.from_opt(argparse.Namespace(**base, train_rows=1), is_train=1)
    assert o.train_rows == 1 and o.check_supported() is o
    assert HotPathOpts.from_opt(argparse.Namespace(**base), train_rows=1).train_rows == 1
    from sgnerf_amd.model import HipPointsVolumetricModel
    p = HipPointsVolumetricModel.modify_commandline_options(argparse.ArgumentParser(), is_train=True)
    assert p.parse_args([]).sgn_train_rows == 0 and p.parse_args(["--sgn_train_rows", "1"]).sgn_train_rows == 1


def test_hip_trainer_needs_f32():
    """The constructor's default precision is "f16": refused naming the option, before anything is built."""
    from sgnerf_amd.train_hip import HipTrainer
    with pytest.raises(NotImplementedError, match="train_rows"):
        HipTrainer(None, {}, HotPathOpts(**NB3, is_train=1, train_rows=1), "cpu")


# ---- the torch reference -----------------------------------------------------------------------------------
SCENES = [(1, 7), (5, 1), (5, 17), (8, 7), (8, 17)]


def _state():
    return init_mlp(5, bias_std=0.1, block3_layers=0)


def test_viewmlp_reads_its_layers_from_the_state():
    m = ViewMLP(_state())
    assert [n for n, *_ in m.layers] == [n for n, *_ in layers_for(block3_layers=0)]
    assert sorted(m.state()) == sorted(_state()) and not any("block3" in k for k in m.state())
    assert len(ViewMLP(init_mlp(5)).layers) == 9


@pytest.mark.parametrize("K,items", SCENES, ids=lambda v: str(v))
def test_aggregate_equals_the_restatement(K, items):
    """train.aggregate in float64 against nb3_ref.chain: alpha, f_s (through the colour MLP's input gradient) and
    rgb to 1e-12, every gradient to 1e-10 relative L2; colour and dir get no gradient and are not read."""
    sc = tn.synthetic(K, items)
    assert int((sc.nnb == 0).sum()) > 0 and int((sc.nnb == 1).sum()) > 0
    state = _state()
    campos, rot = (t.double() for t in sc.camera)
    G = torch.randn(sc.S, 4, generator=torch.Generator().manual_seed(9), dtype=torch.float64)

    def run(color, pdir):
        P = PointParams(sc.points["xyz"], sc.points["embedding"], color, pdir, sc.points["conf"], "cpu").double()
        mlp = ViewMLP(state).double()
        feat, _, mask = aggregate(P, mlp, campos, rot, sc.raydir.double(), sc.query["samp_ray"],
                                  sc.query["samp_locw"].double(), sc.query["pidx"])
        (feat * G).sum().backward()
        return P, mlp, feat.detach()
    P, mlp, feat = run(sc.points["color"], sc.points["dir"])
    pts, st = tn.leaves(sc, state)
    o, feat_c = tn.chain_feat(sc, pts, st)
    (feat_c * G).sum().backward()
    work = sc.work
    assert float((feat[work, 0] - o["alpha"].detach()).abs().max()) <= 1e-12
    assert float((feat[work, 1:] - o["rgb"].detach()).abs().max()) <= 1e-12
    assert bool((feat[sc.nnb == 0] == 0).all())
    err = {}
    for name, *_ in mlp.layers:
        err[name + ".weight"] = tn.rel_l2(mlp.w(name).grad, st[name + ".weight"].grad)
        err[name + ".bias"] = tn.rel_l2(mlp.b(name).grad, st[name + ".bias"].grad)
    err["points_embeding"] = tn.rel_l2(P.points_embeding.grad, pts["embedding"].grad)
    err["points_conf"] = tn.rel_l2(P.points_conf.grad, pts["conf"].grad.reshape(-1, 1))
    assert max(err.values()) <= 1e-10, err
    assert float(P.points_embeding.grad.abs().max()) > 0 and float(P.points_conf.grad.abs().max()) > 0
    assert P.points_color.grad is None and P.points_dir.grad is None
    # garbage in colour and dir, or neither at all: the same bits
    for color, pdir in ((torch.full_like(sc.points["color"], float("nan")), sc.points["dir"] * 1e30), (None, None)):
        P2, mlp2, feat2 = run(color, pdir)
        assert torch.equal(feat2, feat) and torch.equal(P2.points_embeding.grad, P.points_embeding.grad)
        assert torch.equal(mlp2.w("block1.0").grad, mlp.w("block1.0").grad)


def test_fs_equals_the_restatement():
    """f_s itself (aggregate does not return it): the colour MLP of the restatement on aggregate's inputs gives
    aggregate's rgb only if the blended features agree -- checked directly on a hook of color_branch.0's input."""
    sc = tn.synthetic(8, 17)
    state = _state()
    P = PointParams(sc.points["xyz"], sc.points["embedding"], None, None, sc.points["conf"], "cpu").double()
    mlp = ViewMLP(state).double()
    seen = {}
    mlp.lin["color_branch_0"].register_forward_pre_hook(lambda m, x: seen.update(x=x[0].detach()))
    import sgnerf_amd.train as train_mod
    keep = train_mod._linear
    train_mod._linear = lambda m, name, x, split=False: m.f(name, x)   # the hook sees nn.Linear calls only
    try:
        aggregate(P, mlp, sc.camera[0].double(), sc.camera[1].double(), sc.raydir.double(), sc.query["samp_ray"],
                  sc.query["samp_locw"].double(), sc.query["pidx"])
    finally:
        train_mod._linear = keep
    pts, st = tn.leaves(sc, state)
    o, _ = tn.chain_feat(sc, pts, st)
    assert float((seen["x"][sc.work, :256] - o["fs"].detach()).abs().max()) <= 1e-12


# ---- train.Trainer on the CPU ------------------------------------------------------------------------------
def _tiny():
    """A synthetic scene whose samples are grouped by ray (what the composite needs): sorted ray ids."""
    sc = tn.synthetic(8, 17)
    sr = torch.sort(sc.query["samp_ray"]).values
    R = sc.raydir.shape[0]
    ns = torch.bincount(sr, minlength=R)
    assert int(ns.max()) <= 24
    q = {"ray_ns": ns, "ray_soff": torch.cumsum(ns, 0) - ns, "samp_ray": sr, "samp_locw": sc.query["samp_locw"],
         "pidx": sc.query["pidx"]}
    gt = torch.rand(R, 3, generator=torch.Generator().manual_seed(2))
    return sc, q, gt


def test_trainer_refuses_without_the_option():
    sc, q, gt = _tiny()
    P = PointParams(sc.points["xyz"], sc.points["embedding"], None, None, sc.points["conf"], "cpu")
    with pytest.raises(NotImplementedError, match="shading_feature_mlp_layer3"):
        Trainer(P, _state(), HotPathOpts(**NB3), "cpu")


@pytest.mark.parametrize("with_colour", [True, False])
def test_trainer_steps_on_the_cpu(with_colour):
    """Three steps: colour and dir keep their bits (or are absent), embedding and conf move, no block3 in the state."""
    sc, q, gt = _tiny()
    opts = HotPathOpts(**NB3, is_train=1, train_rows=1).check_supported()
    col, pdir = (sc.points["color"], sc.points["dir"]) if with_colour else (None, None)
    P = PointParams(sc.points["xyz"], sc.points["embedding"], col, pdir, sc.points["conf"], "cpu")
    p0 = {k: None if getattr(P, k) is None else getattr(P, k).detach().clone()
          for k in ("points_embeding", "points_color", "points_dir", "points_conf")}
    st = _state()
    st["alpha_branch.0.bias"] = st["alpha_branch.0.bias"] + 50.0   # opaque samples: the colour loss has a gradient
    tr = Trainer(P, st, opts, "cpu")
    for _ in range(3):
        parts, full, mask = tr.step(sc.camera[0], sc.camera[1], sc.raydir, 0.1, 8.0, gt, q=q)
    assert bool(torch.isfinite(parts["total"])) and bool(mask.any())
    for k in ("points_color", "points_dir"):
        p = getattr(P, k)
        assert (p is None) if not with_colour else (torch.equal(p.detach(), p0[k]) and p.grad is None)
    assert not torch.equal(P.points_embeding.detach(), p0["points_embeding"])
    assert not torch.equal(P.points_conf.detach(), p0["points_conf"])
    assert not any("block3" in k for k in tr.mlp_state())
    assert not torch.equal(tr.mlp_state()["block1.0.weight"], st["block1.0.weight"])
