"""CPU tests of the driver's loss options: tests/loss_opts_ref.py (the explicit-loop float64 restatement of
compute_losses, base_rendering_model.py:534-664) against train.composite_losses under torch float64 autograd, the
options' parsing and refusals (opts.HotPathOpts), and the plugin reading the flags from an argparse namespace
shaped like the reference's.

Bar of the comparison: 1e-5 of each tensor's largest magnitude, as tests/test_depth_ref_cpu.py and
test_ray_stage_ref_cpu.py hold their references to composite_losses.  The restatement takes the slot distances, the
depths z and the clamps in fp32 as the kernels do (relative 2^-24 each), the float64 torch side does not, so the two
agree to about 1e-6, not to float64 rounding."""
import argparse
import dataclasses
import functools
import types

import pytest
import torch

from sgnerf_amd.opts import COLOR_LOSS_ITEMS, SCANNET, HotPathOpts
from sgnerf_amd.train import DepthTarget, composite_losses

import depth_ref as dr
import loss_opts_ref as lr

BAR = 1e-5
MASKED, MISS, ALL = COLOR_LOSS_ITEMS

# (colour items, colour weights, zero-one items, zero-one weights, zero_epsilon, sparse weight)
SETTINGS = {
    "scannet": (COLOR_LOSS_ITEMS, (1.0, 0.0, 0.0), ("conf_coefficient",), (1e-4,), 1e-3, 0.0),
    "permuted": ((ALL, MASKED, MISS), (0.25, 0.5, 2.0), ("conf_coefficient",), (1e-2,), 1e-3, 0.0),
    "two_items": ((MISS, ALL), (2.0, 1.0), ("conf_coefficient",), (1e-4,), 0.05, 0.0),
    "one_weight": ((MASKED, ALL), (0.5,), ("conf_coefficient",), (1e-4,), 1e-3, 1e-3),
    "zero_one_off": (COLOR_LOSS_ITEMS, (0.0, 0.0, 1.0), (), (1.0,), 1e-3, 0.0),
    "zero_one_weight_0": ((MASKED,), (1.0,), ("conf_coefficient",), (0.0,), 1e-3, 1.0),
    "sparse_on": (COLOR_LOSS_ITEMS, (0.5, 2.0, 0.25), ("conf_coefficient",), (1e-4,), 0.05, 1.0),
}


@functools.lru_cache(maxsize=None)
def scene(K):
    sc = lr.small_scene(70, 6, K, seed=5, camera=K % 2)
    # conf values one fp32 step from a threshold would fall on the other side of it in float64: spread, for this
    # comparison alone, values that are clear of every clamp edge over the planted points
    conf = sc["conf"].clone()
    vals = torch.tensor([0.0, 5e-5, 2e-4, 5e-4, 2e-3, 0.03, 0.06, 0.3, 0.5, 0.7, 0.94, 0.97, 0.9985, 0.9995, 1.0, 1.2, -0.1,
                         0.2, 0.8, 0.04, 0.96])
    conf[1:1 + vals.numel()] = vals
    sc["conf"] = conf
    return sc


def _rel_max(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp(min=1e-300))


def _composite_f64(sc, opts, unit, bgr, depth):
    """train.composite_losses in float64 (torch's default dtype switched for the call): (total, parts, d feat,
    d conf)."""
    S, R = sc["S"], sc["R"]
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        points = types.SimpleNamespace(xyz=sc["xyz"].double(), points_conf=sc["conf"].double()[:, None].requires_grad_(True))
        q = {"ray_ns": sc["ray_ns"], "ray_soff": sc["ray_soff"], "samp_ray": sc["samp_ray"][:S],
             "samp_locw": sc["samp_locw"][:S].double(), "pidx": sc["pidx"][:S]}
        feat = sc["feat"][:S].double().requires_grad_(True)
        bg = sc["bg_ray"].double() if bgr else (1.0, 1.0, 1.0)
        out = composite_losses(points, q, feat, sc["samp_nnb"][:S] > 0, sc["campos"].double(), sc["rot"].double(),
                               torch.zeros(R, 3), sc["gt"].double(), opts, bg=bg, depth=depth)
        out[0].backward()
        dconf = points.points_conf.grad
        return out[0].detach(), out[1], feat.grad, (torch.zeros(sc["conf"].shape[0]) if dconf is None else dconf[:, 0])
    finally:
        torch.set_default_dtype(old)


@pytest.mark.parametrize("K", [3, 8])
@pytest.mark.parametrize("with_depth", [False, True])
@pytest.mark.parametrize("name", list(SETTINGS))
def test_reference_agrees_with_composite_losses(name, with_depth, K):
    items, weights, zo_items, zo_weights, eps, sparse = SETTINGS[name]
    sc = scene(K)
    unit, bgr = K % 2, K == 8
    S, R = sc["S"], sc["R"]
    depth = dref = None
    if with_depth:
        gt_d, gt_m = dr.targets(sc, dr.depth_map(sc, unit)["D"], seed=K)
        depth, dref = DepthTarget(gt_d, gt_m, 0.5), (gt_d, gt_m, 0.5)
    opts = HotPathOpts(SR=sc["SR"], K=K, raydist_mode_unit=unit, color_loss_items=items, color_loss_weights=weights,
                       zero_one_loss_items=zo_items, zero_one_loss_weights=zo_weights, zero_epsilon=eps,
                       sparse_loss_weight=sparse).check_supported()
    ref = lr.reference(sc, unit, bgr, items, weights, zo_items, zo_weights, eps, sparse, depth=dref)
    tot, parts, dfeat, dconf = _composite_f64(sc, opts, unit, bgr, depth)
    assert 10 < ref["n"] < R
    assert set(parts) == set(ref["parts"]) and ("sparse" in parts) == (sparse > 0)
    for k, b in ref["parts"].items():
        assert abs(float(parts[k]) - b) <= BAR * max(abs(b), 1e-12), (k, float(parts[k]), b)
    assert abs(float(tot) - ref["total"]) <= BAR * abs(ref["total"])
    # the total is the weighted sum of the parts plus 1e-6 per listed colour item
    want = sum(lr.item_weight(items, weights, n) * ref["parts"][n] + 1e-6 for n in items)
    want += lr.item_weight(zo_items, zo_weights, "conf_coefficient") * ref["parts"]["conf_coefficient"]
    want += sparse * ref["parts"].get("sparse", 0.0) + (0.5 * ref["parts"]["coarse_depth"] if with_depth else 0.0)
    assert abs(ref["total"] - want) <= 1e-12 * max(abs(want), 1e-6)
    w_masked, _, w_all = opts.color_weights
    if w_masked or w_all or with_depth:
        assert _rel_max(dfeat, ref["dfeat"][:S]) <= BAR
    else:
        assert float(dfeat.abs().max()) == 0 and float(ref["dfeat"].abs().max()) == 0
    if opts.zero_one_weight or sparse:
        assert _rel_max(dconf, ref["dconf"]) <= BAR
    else:
        assert float(dconf.abs().max()) == 0 and float(ref["dconf"].abs().max()) == 0
    print(f"{name}, depth {with_depth}, K {K}: d feat {_rel_max(dfeat, ref['dfeat'][:S]) if float(ref['dfeat'].abs().max()) else 0:.2e}, "
          f"d conf {_rel_max(dconf, ref['dconf']) if float(ref['dconf'].abs().max()) else 0:.2e} of the tensor's max")


def test_miss_weight_moves_the_total_alone():
    sc = scene(3)
    a = lr.reference(sc, 0, False, color_weights=(1.0, 0.0, 0.0))
    b = lr.reference(sc, 0, False, color_weights=(1.0, 3.0, 0.0))
    assert torch.equal(a["dfeat"], b["dfeat"]) and torch.equal(a["dconf"], b["dconf"])
    assert abs(b["total"] - a["total"] - 3.0 * a["parts"][MISS]) <= 1e-12 and a["parts"][MISS] > 0


def test_sparse_gradient_by_finite_differences():
    """d total / d conf with the sparse loss on, central differences in float64 on points clear of the clamps."""
    sc = dict(scene(8))
    kw = dict(color_weights=(1.0, 0.0, 0.0), zero_one_weights=(1e-2,), zero_eps=0.05, sparse_weight=1.0)
    ref = lr.reference(sc, 0, False, **kw)
    conf = sc["conf"]
    named = torch.unique(sc["pidx"][:sc["S"]][sc["pidx"][:sc["S"]] >= 0]).tolist()
    pts = [p for p in named if 0.1 < float(conf[p]) < 0.9][:6]
    assert len(pts) >= 4
    h = 2.0 ** -10    # exact in fp32 on these values' binade or above: the scene's conf is an fp32 tensor
    for p in pts:
        tot = []
        for sgn in (1, -1):
            c = conf.clone()
            c[p] = c[p] + sgn * h
            assert float(c[p]) == float(conf[p]) + sgn * h
            tot.append(lr.reference(dict(sc, conf=c), 0, False, **kw)["total"])
        fd = (tot[0] - tot[1]) / (2 * h)
        assert abs(fd - float(ref["dconf"][p])) <= 1e-4 * abs(fd) + 1e-9, (p, fd, float(ref["dconf"][p]))


# ---- options -------------------------------------------------------------------------------------------

def test_defaults_are_scannet():
    """The new fields' defaults, and every earlier field untouched by them."""
    o = HotPathOpts()
    assert o == SCANNET
    assert o.color_loss_items == COLOR_LOSS_ITEMS and o.color_loss_weights == (1.0, 0.0, 0.0)
    assert o.zero_one_loss_items == ("conf_coefficient",) and o.zero_one_loss_weights == (1e-4,)
    assert o.zero_epsilon == 1e-3 and o.sparse_loss_weight == 0.0
    assert o.color_weights == (1.0, 0.0, 0.0) and o.zero_one_weight == 1e-4 and o.stock_loss
    new = {"color_loss_items", "color_loss_weights", "zero_one_loss_items", "zero_one_loss_weights", "zero_epsilon",
           "sparse_loss_weight", "bg_loss_items", "l2_size_loss_items"}
    names = [f.name for f in dataclasses.fields(HotPathOpts)]
    assert new <= set(names)
    # a namespace without the flags gives SCANNET in every earlier field (and in the new ones)
    ns = argparse.Namespace(**{n: getattr(SCANNET, n) for n in names if n not in new})
    assert HotPathOpts.from_opt(ns) == SCANNET
    o.check_supported()
    # the default total keeps its order of additions: ray_masked + 3e-6 + 1e-4 * conf_coefficient
    p = {MASKED: torch.tensor(0.123456789), "conf_coefficient": torch.tensor(-3.3)}
    assert float(o.total_loss(p)) == float(p[MASKED] + 3e-6 + 1e-4 * p["conf_coefficient"])


def test_from_opt_parses_lists_none_and_bare_values():
    ns = argparse.Namespace(color_loss_items=[ALL, MASKED], color_loss_weights=[0.5, 2.0], zero_one_loss_items=None,
                            zero_one_loss_weights=0.01, zero_epsilon=0.02, sparse_loss_weight=1e-3, bg_loss_items=[],
                            l2_size_loss_items=None)
    o = HotPathOpts.from_opt(ns).check_supported()
    assert o.color_loss_items == (ALL, MASKED) and o.color_loss_weights == (0.5, 2.0)
    assert o.color_weights == (2.0, 0.0, 0.5)                       # weights follow the item order
    assert o.zero_one_loss_items == ("conf_coefficient",)           # None: unset
    assert o.zero_one_loss_weights == (1e-4,)                       # a lone weight beside unset items: argparse's default
    assert o.zero_epsilon == 0.02 and o.sparse_loss_weight == 1e-3 and not o.stock_loss
    assert o.bg_loss_items == () and o.l2_size_loss_items == ()
    o = HotPathOpts.from_opt(argparse.Namespace(color_loss_items=MASKED, color_loss_weights=2.0,
                                                zero_one_loss_items="conf_coefficient", zero_one_loss_weights=0.0,
                                                zero_epsilon=None, sparse_loss_weight=None)).check_supported()
    assert o.color_loss_items == (MASKED,) and o.color_loss_weights == (2.0,) and o.color_weights == (2.0, 0.0, 0.0)
    assert o.zero_one_loss_items == ("conf_coefficient",) and o.zero_one_weight == 0.0
    assert o.zero_epsilon == 1e-3 and o.sparse_loss_weight == 0.0
    # one weight serves every item; an empty zero-one list drops the term
    o = HotPathOpts(color_loss_items=(MISS, ALL), color_loss_weights=(0.5,), zero_one_loss_items=()).check_supported()
    assert o.color_weights == (0.0, 0.5, 0.5) and o.zero_one_weight == 0.0
    # the reference's argparse defaults beside unset items leave the ScanNet objective
    o = HotPathOpts.from_opt(argparse.Namespace(color_loss_items=None, color_loss_weights=[1.0], zero_one_loss_items=None,
                                                zero_one_loss_weights=[1.0], sparse_loss_weight=0))
    assert o == SCANNET


@pytest.mark.parametrize("kw,field", [
    (dict(color_loss_items=(MASKED, "ray_depth_masked_coarse_raycolor")), "color_loss_items"),
    (dict(color_loss_items=(MASKED, MASKED), color_loss_weights=(1.0,)), "color_loss_items"),
    (dict(color_loss_items=(MASKED, ALL), color_loss_weights=(1.0, 0.0, 0.0)), "color_loss_weights"),
    (dict(color_loss_weights=(1.0, 0.0)), "color_loss_weights"),
    (dict(color_loss_weights=(1.0, -0.5, 0.0)), "color_loss_weights"),
    (dict(color_loss_weights=(1.0, float("nan"), 0.0)), "color_loss_weights"),
    (dict(color_loss_weights=(float("inf"),)), "color_loss_weights"),
    (dict(zero_one_loss_items=("coarse_raycolor",)), "zero_one_loss_items"),
    (dict(zero_one_loss_weights=(1e-4, 1e-4)), "zero_one_loss_weights"),
    (dict(zero_one_loss_weights=(-1e-4,)), "zero_one_loss_weights"),
    (dict(zero_one_loss_weights=(float("inf"),)), "zero_one_loss_weights"),
    (dict(zero_epsilon=0.0), "zero_epsilon"),
    (dict(zero_epsilon=0.5), "zero_epsilon"),
    (dict(zero_epsilon=-1e-3), "zero_epsilon"),
    (dict(zero_epsilon=float("nan")), "zero_epsilon"),
    (dict(sparse_loss_weight=-1.0), "sparse_loss_weight"),
    (dict(sparse_loss_weight=float("nan")), "sparse_loss_weight"),
    (dict(sparse_loss_weight=float("inf")), "sparse_loss_weight"),
    (dict(bg_loss_items=("coarse_mask",)), "bg_loss_items"),
    (dict(l2_size_loss_items=("conf_coefficient",)), "l2_size_loss_items"),
])
def test_refusals_name_the_field(kw, field):
    with pytest.raises(NotImplementedError) as e:
        HotPathOpts(**kw).check_supported()
    assert field in str(e.value)


def test_bg_and_l2_items_come_from_the_namespace():
    with pytest.raises(NotImplementedError, match="bg_loss_items"):
        HotPathOpts.from_opt(argparse.Namespace(bg_loss_items=["coarse_mask"])).check_supported()
    with pytest.raises(NotImplementedError, match="l2_size_loss_items"):
        HotPathOpts.from_opt(argparse.Namespace(l2_size_loss_items="conf_coefficient")).check_supported()


# ---- the plugin ----------------------------------------------------------------------------------------

def _reference_style_parser():
    """The loss flags as base_rendering_model.py:30-129 declares them."""
    p = argparse.ArgumentParser()
    p.add_argument("--sparse_loss_weight", type=float, default=0)
    p.add_argument("--color_loss_items", type=str, nargs="+", default=None)
    p.add_argument("--color_loss_weights", type=float, nargs="+", default=[1.0])
    p.add_argument("--bg_loss_items", type=str, nargs="+", default=[])
    p.add_argument("--depth_loss_items", type=str, nargs="+", default=[])
    p.add_argument("--depth_loss_weights", type=float, nargs="+", default=[1.0])
    p.add_argument("--zero_one_loss_items", type=str, nargs="+", default=[])
    p.add_argument("--zero_one_loss_weights", type=float, nargs="+", default=[1.0])
    p.add_argument("--l2_size_loss_items", type=str, nargs="+", default=[])
    p.add_argument("--zero_epsilon", type=float, default=1e-3)
    return p


def _plugin(tmp_path, argv):
    from sgnerf_amd.model import HipPointsVolumetricModel
    opt = _reference_style_parser().parse_args(argv)
    for k, v in dict(SR=24, K=8, gpu_ids=[0], is_train=True, checkpoints_dir=str(tmp_path), name="scene",
                     bg_color="white").items():
        setattr(opt, k, v)
    m = HipPointsVolumetricModel()
    m.initialize(opt)
    return m


def test_plugin_reads_the_flags(tmp_path):
    m = _plugin(tmp_path, ["--color_loss_items", MASKED, MISS, ALL, "--color_loss_weights", "0.0", "0.0", "1.0",
                           "--zero_one_loss_items", "conf_coefficient", "--zero_one_loss_weights", "0",
                           "--zero_epsilon", "0.002", "--sparse_loss_weight", "1e-3"])
    o = m.opts
    assert o.color_weights == (0.0, 0.0, 1.0) and o.zero_one_weight == 0.0 and o.zero_epsilon == 0.002
    assert o.sparse_loss_weight == 1e-3 and not o.stock_loss
    # the scripts' line (scene241.sh): the ScanNet objective plus the sparse loss
    m = _plugin(tmp_path, ["--color_loss_items", MASKED, MISS, ALL, "--color_loss_weights", "1.0", "0.0", "0.0",
                           "--zero_one_loss_items", "conf_coefficient", "--zero_one_loss_weights", "0.0001",
                           "--sparse_loss_weight", "0"])
    for f in dataclasses.fields(HotPathOpts):
        if f.name not in ("SR", "K", "is_train", "bg_color"):
            assert getattr(m.opts, f.name) == getattr(SCANNET, f.name), f.name
    with pytest.raises(NotImplementedError, match="bg_loss_items"):
        _plugin(tmp_path, ["--bg_loss_items", "coarse_mask"])
