"""Depth maps and the depth loss without a GPU: tests/depth_ref.py (the float64 reference the GPU tests use)
agrees with train.composite_losses(depth=...) and with central finite differences; the options, the C ABI's
new entries (exported, bound, ABI still 23, argument errors before any HIP call) and the plugin's refusal of a
depth-supervised batch without gt_depth."""
import argparse
import ctypes
import functools
import os
import re
import types

import pytest
import torch

import depth_ref as dr
import ray_stage_ref as rs
from sgnerf_amd import _lib
from sgnerf_amd.model import HipPointsVolumetricModel
from sgnerf_amd.opts import HotPathOpts
from sgnerf_amd.ray_marching import NeuralPoints
from sgnerf_amd.train import DepthTarget, PointParams, composite_losses, depth_target

SCENES = [(37, 24, 8), (20, 33, 3), (9, 64, 16)]
BAR = 1e-5
W_D = 0.5
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sgn_hip.h")


@functools.lru_cache(maxsize=None)
def scene(R, SR, K, camera):
    return rs.ray_scene(R, SR, K, seed=3, camera=camera)


def _rel_max(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp(min=1e-300))


@pytest.mark.parametrize("R,SR,K", SCENES)
@pytest.mark.parametrize("unit,bgr,camera,explicit", [(0, False, 0, False), (1, True, 1, True), (1, False, 0, True),
                                                      (0, True, 1, False)])
def test_reference_agrees_with_composite_losses(R, SR, K, unit, bgr, camera, explicit):
    sc = scene(R, SR, K, camera)
    S = sc["S"]
    fwd = dr.depth_map(sc, unit)
    gt_d, gt_m = dr.targets(sc, fwd["D"], seed=R)
    gt_m = gt_m if explicit else None
    ref = dr.reference(sc, unit, bgr, gt_d, gt_m, W_D, zero_one_weight=1.0)
    assert torch.equal(ref["D"], fwd["D"])
    N = rs.N_POINTS
    points = PointParams(sc["xyz"], torch.zeros(N, 32), torch.zeros(N, 3), torch.zeros(N, 3), sc["conf"], "cpu")
    q = {"ray_ns": sc["ray_ns"], "ray_soff": sc["ray_soff"], "samp_ray": sc["samp_ray"][:S], "samp_locw": sc["samp_locw"][:S],
         "pidx": sc["pidx"][:S]}
    opts = HotPathOpts(SR=SR, K=K, raydist_mode_unit=unit)
    args = (points, q, None, sc["samp_nnb"][:S] > 0, sc["campos"], sc["rot"], torch.zeros(R, 3), sc["gt"], opts)
    kw = dict(bg=sc["bg_ray"] if bgr else (1.0, 1.0, 1.0), zero_one_weight=1.0, zero_eps=rs.ZO_EPS)

    def run(depth):
        feat = sc["feat"][:S].clone().requires_grad_(True)
        points.points_conf.grad = None
        out = composite_losses(*args[:2], feat, *args[3:], **kw, depth=depth)
        out[0].backward()
        return out, feat.grad

    (tot, parts, full, mask, dmap), g = run(depth_target(gt_d, gt_m, W_D, R, "cpu"))
    (tot0, parts0, full0, mask0), g0 = run(None)
    assert "coarse_depth" not in parts0 and torch.equal(full, full0) and torch.equal(mask, mask0)
    assert torch.equal(mask, ref["mask"]) and dmap.shape == (R,)
    assert bool((dmap[~mask] == 0).all()) and bool((ref["D"][~mask] == 0).all())
    # the depth map, the loss and the total
    assert float((dmap.double() - ref["D"]).abs().max()) <= BAR * max(1.0, float(ref["D"].abs().max()))
    a, b = float(parts["coarse_depth"]), float(ref["l_depth"])
    assert b > 0 and abs(a - b) <= BAR * b, (a, b)
    assert abs(float((tot - tot0).detach()) - W_D * b) <= BAR * max(abs(float(tot.detach())), W_D * b)
    # the gradient: colour channels as without depth, sigma with the depth term
    assert torch.equal(g[:, 1:], g0[:, 1:])
    e = _rel_max(g, ref["dfeat_depth"][:S])
    print(f"d feat {e:.2e} of the tensor's max; depth term {_rel_max(g - g0, ref['dfeat_depth'][:S] - ref['dfeat'][:S]):.2e}")
    assert e <= BAR
    assert float((ref["dfeat_depth"][:S] - ref["dfeat"][:S]).abs().max()) > 0      # the term is there
    sr = sc["samp_ray"][:S].long()
    assert bool((ref["dfeat_depth"][:S][~mask[sr]] == 0).all())                     # rays off the mask: no gradient


def test_masked_out_rays_still_count_in_the_loss():
    """A ray without a valid sample has D = 0 and contributes (m g)^2 / R."""
    sc = scene(37, 24, 8, 0)
    fwd = dr.depth_map(sc, 0)
    gt_d, gt_m = dr.targets(sc, fwd["D"], seed=1)
    off = ~fwd["mask"]
    assert int(off.sum()) >= 2
    gt_d = gt_d.clone()
    gt_d[off] = 0.7
    only = torch.where(off, gt_m.clamp(min=0.5), torch.zeros_like(gt_m))   # every other ray masked out
    want = float(((only.double() * gt_d.double()) ** 2).sum() / sc["R"])
    got = float(dr.depth_loss(fwd["D"], gt_d, only))
    assert want > 0 and abs(got - want) <= 1e-15


@pytest.mark.parametrize("R,SR,K", SCENES)
@pytest.mark.parametrize("unit,camera", [(0, 0), (1, 1)])
def test_reference_gradient_by_finite_differences(R, SR, K, unit, camera):
    """d (losses[0] + w_d L_depth) / d feat.x on a handful of samples: central differences in float64."""
    sc = scene(R, SR, K, camera)
    S = sc["S"]
    fwd = dr.depth_map(sc, unit)
    gt_d, gt_m = dr.targets(sc, fwd["D"], seed=R + 1)
    ref = dr.reference(sc, unit, True, gt_d, gt_m, W_D)
    z = ref["z"]

    def total(feat64):
        m = rs.march_ref(ref["dist"], ref["valid"], rs.densify(sc, feat64), ref["bg"])
        full, mask, _ = rs.fill_invalid(m["rgb"], m["bgT"], ref["valid"], ref["bg"])
        losses, _ = rs.loss_ref(full, mask, sc["gt"], sc["conf"].double(), sc["conf"], ref["pd"])
        D, _, _ = dr.depth_of(m["w"], z, mask)
        return float(losses[0] + W_D * dr.depth_loss(D, gt_d, gt_m))

    g = ref["dfeat_depth"][:S, 0]
    big = torch.argsort(g.abs(), descending=True)[:4].tolist()
    some = torch.linspace(0, S - 1, 4).round().long().tolist()
    checked = 0
    for s in sorted(set(big + some)):
        x = float(sc["feat"][s, 0])
        h = 1e-6 * max(abs(x), 1.0)
        fp, fm = sc["feat"].double().clone(), sc["feat"].double().clone()
        fp[s, 0] += h
        fm[s, 0] -= h
        fd = (total(fp) - total(fm)) / (2 * h)
        tol = 1e-6 * float(g.abs().max()) + 1e-5 * abs(float(g[s]))
        assert abs(fd - float(g[s])) <= tol, (s, fd, float(g[s]))
        checked += 1
    assert checked >= 4 and float(g.abs().max()) > 0


# ---- options ---------------------------------------------------------------------------------------

def test_options():
    o = HotPathOpts()
    assert (o.compute_depth, o.depth_loss_items, o.depth_loss_weights) == (0, (), (1.0,))
    assert not o.want_depth and o.depth_loss_weight is None
    ns = argparse.Namespace(compute_depth=1, depth_loss_items=["coarse_depth"], depth_loss_weights=[0.25], SR=24)
    o = HotPathOpts.from_opt(ns).check_supported()
    assert o.compute_depth == 1 and o.depth_loss_items == ("coarse_depth",) and o.depth_loss_weights == (0.25,)
    assert o.want_depth and o.depth_loss_weight == 0.25
    assert HotPathOpts(compute_depth=1).check_supported().want_depth
    assert HotPathOpts(depth_loss_items=("coarse_depth",)).check_supported().depth_loss_weight == 1.0
    with pytest.raises(NotImplementedError, match="fine_depth"):
        HotPathOpts(depth_loss_items=("coarse_depth", "fine_depth")).check_supported()
    with pytest.raises(NotImplementedError, match="depth_loss_weights"):
        HotPathOpts(depth_loss_items=("coarse_depth",), depth_loss_weights=(1.0, 2.0)).check_supported()
    with pytest.raises(NotImplementedError, match="depth_loss_weights"):
        HotPathOpts(depth_loss_items=("coarse_depth",), depth_loss_weights=()).check_supported()


def test_depth_target_shapes():
    t = depth_target(torch.ones(1, 6, 1), torch.ones(2, 3), 0.5, 6, "cpu")
    assert isinstance(t, DepthTarget) and t.gt.shape == (6,) and t.mask.shape == (6,) and t.weight == 0.5
    assert depth_target(torch.ones(6), None, 1.0, 6, "cpu").mask is None
    with pytest.raises(ValueError, match="gt_depth"):
        depth_target(torch.ones(5), None, 1.0, 6, "cpu")
    with pytest.raises(ValueError, match="gt_mask"):
        depth_target(torch.ones(6), torch.ones(7), 1.0, 6, "cpu")


# ---- the C ABI -------------------------------------------------------------------------------------

NEW = ("sgn_composite_depth", "sgn_loss_train_depth", "sgn_loss_depth_workspace_bytes")


def test_new_entries_exported_and_bound():
    hdr = open(HEADER).read()
    assert int(re.search(r"#define SGN_ABI_VERSION (\d+)", hdr).group(1)) == 23 == _lib.ABI_VERSION
    L = _lib.lib()
    assert L.sgn_abi_version() == 23
    for name in NEW:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in _lib.SIGNATURES and getattr(L, name).argtypes == _lib.SIGNATURES[name][1]
    assert "sgn_loss_depth" in hdr and ctypes.sizeof(_lib.LossDepth) == 32
    # the depth stage's workspace holds the stock one's slots, W per ray and one more partial sum per block
    for R, SR in ((64, 24), (8229, 4), (1, 1)):
        assert L.sgn_loss_depth_workspace_bytes(R, SR) >= L.sgn_loss_workspace_bytes(R, SR) + 4 * R
    assert L.sgn_loss_depth_workspace_bytes(4, 0) == 0 and L.sgn_loss_workspace_bytes(64, 24) == 64 * 24 * 12 + 3 * 20 + 64


def test_argument_errors_before_any_hip_call():
    L = _lib.lib()
    fake = ctypes.c_void_p(256)
    qo = _lib.QueryOut()
    cp = _lib.CompositeParams()
    cp.SR = 24
    comp = lambda cp, depth: L.sgn_composite_depth(ctypes.byref(cp), fake, fake, fake, 4, fake, 0, 400, ctypes.byref(qo),  # noqa: E731
                                                   fake, fake, fake, fake, None, None, depth, None)
    assert comp(cp, None) != 0 and b"null" in L.sgn_last_error()
    cp.SR = 0
    assert comp(cp, fake) != 0 and b"SR" in L.sgn_last_error()
    lp = _lib.LossParams()
    lp.SR, lp.K = 24, 8
    dp = _lib.LossDepth(256, None, 0.5, 256)
    args = (fake, fake, 64, ctypes.byref(qo), fake, fake, fake, fake, fake, fake, fake, fake)
    big = 1 << 20
    assert L.sgn_loss_train_depth(ctypes.byref(lp), None, *args, fake, big, None) != 0 and b"null" in L.sgn_last_error()
    for bad in (_lib.LossDepth(None, None, 0.5, 256), _lib.LossDepth(256, None, 0.5, None)):
        assert L.sgn_loss_train_depth(ctypes.byref(lp), ctypes.byref(bad), *args, fake, big, None) != 0
        assert b"null" in L.sgn_last_error()
    assert L.sgn_loss_train_depth(ctypes.byref(lp), ctypes.byref(dp), *args, None, big, None) != 0 and b"null" in L.sgn_last_error()
    # the stock stage's size is too small for the depth stage
    small = L.sgn_loss_workspace_bytes(64, 24)
    assert L.sgn_loss_train_depth(ctypes.byref(lp), ctypes.byref(dp), *args, fake, small, None) != 0
    assert b"workspace" in L.sgn_last_error()
    lp.SR = 0
    assert L.sgn_loss_train_depth(ctypes.byref(lp), ctypes.byref(dp), *args, fake, big, None) != 0
    assert b"positive" in L.sgn_last_error()


# ---- the plugin ------------------------------------------------------------------------------------

def _model(tmp_path, **extra):
    opt = argparse.Namespace(SR=24, K=8, gpu_ids=[0], is_train=True, checkpoints_dir=str(tmp_path), name="scene",
                             bg_color="white", **extra)
    m = HipPointsVolumetricModel()
    m.initialize(opt)
    m.device = torch.device("cpu")     # host-only: no renderer, no kernels
    m.is_train = False
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.rand(*s, generator=g)  # noqa: E731
    m.neural_points = NeuralPoints(r(50, 3), r(1, 50, 32), r(1, 50, 3), r(1, 50, 3), r(1, 50, 1), "cpu")
    m.net_ray_marching = types.SimpleNamespace(renderer=types.SimpleNamespace(mlp_state={}))
    return m


def test_depth_supervision_without_gt_depth_raises(tmp_path):
    m = _model(tmp_path, depth_loss_items=["coarse_depth"], depth_loss_weights=[0.5])
    assert m.opts.depth_loss_weight == 0.5
    m.input = {"gt_image": torch.zeros(1, 4, 3)}
    with pytest.raises(ValueError, match="gt_depth"):
        m.optimize_parameters(total_steps=1)
    with pytest.raises(NotImplementedError, match="depth_loss_items"):
        _model(tmp_path, depth_loss_items=["fine_depth"])
