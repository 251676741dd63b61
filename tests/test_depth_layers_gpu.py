"""Depth through the layers above the kernels (tests/test_depth_gpu.py checks the kernels): HipRenderer.render
(want_depth), NeuralPointsRayMarching.forward / render / fill_invalid and the plugin's test() (coarse_depth), and
depth supervision (depth_loss_items = coarse_depth) on the three HIP step paths -- the f32 runner, the f16 step's
captured loss-stage graph and its eager path -- against train.Trainer's fp32 autograd on the CPU.  The scene is
tests/test_point_grad_switches_gpu.py's: the small room, one 12 x 16 view (192 rays), SR 24."""
import argparse
import dataclasses
import functools

import pytest
import torch

from sgnerf_amd import _lib  # noqa: F401
from sgnerf_amd.ray_marching import NeuralPoints, NeuralPointsRayMarching, fill_invalid
from sgnerf_amd.render import HipRenderer, PointTables
from sgnerf_amd.train import PointParams, Trainer, depth_target
from sgnerf_amd.train_hip import HipTrainer, grads_named
from sgnerf_amd.weights import LAYERS

import depth_ref as dr
import test_depth_gpu as tdg
import test_point_grad_switches_gpu as sw
from test_point_grad_switches_gpu import DEV, NAMES, O, _d, _rel, _setup

pytestmark = pytest.mark.gpu
# the room's opaque MLP leaves sigma little room to move depth: a weight at which the depth term moves the
# alpha branch's and the conf gradients by more than ten times the f16 bars (asserted below)
W_D = 50.0
F32 = torch.float32


@functools.lru_cache(maxsize=None)
def _targets(seed=0):
    """gt_depth [R] around the room's depths with every fifth ray at 0, and a mask over {0, 0.5, 1}."""
    R = _setup(seed=3)[1].raydir.shape[0]
    g = torch.Generator().manual_seed(50 + seed)
    gt = 0.6 + 1.2 * torch.rand(R, generator=g)
    gt[torch.arange(R) % 5 == 4] = 0.0
    return gt, torch.randint(0, 3, (R,), generator=g).float() * 0.5


def _loss64(D, gt_d, gt_m):
    return float(dr.depth_loss(D.detach().cpu().double().reshape(-1), gt_d, gt_m))


def _view(view):
    return _d(view.campos), _d(view.camrotc2w), _d(view.raydir)


# ---- rendering -------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_render_depth_is_the_weighted_mean_of_the_samples_z(precision):
    """RenderOut.depth against sum blendw z / (sum blendw + 1e-6) in float64 from the same call's blendw and the
    query's samp_locw (z in fp32 as pers_z computes it), within test_depth_gpu's bound with E_w = 0; the other
    outputs are those of a call without depth, bit for bit."""
    pc, view, qd, mlp, gt = _setup(seed=3)
    o = dataclasses.replace(O, precision=precision)
    rnd = HipRenderer(PointTables.from_cloud(pc, DEV), mlp, o, DEV)
    plain = rnd.render(*_view(view), 0.1, 8.0, want_weights=True)
    assert plain.depth is None
    rgb0, mask0, bw0 = plain.rgb.clone(), plain.ray_mask.clone(), plain.blendw.clone()
    out = rnd.render(*_view(view), 0.1, 8.0, want_weights=True, want_depth=True)
    torch.cuda.synchronize()
    R, SR = view.raydir.shape[0], o.SR
    assert out.depth.shape == (R,) and out.depth.dtype == F32
    assert torch.equal(out.rgb, rgb0) and torch.equal(out.ray_mask, mask0) and torch.equal(out.blendw, bw0)
    q = out.query
    ns, soff = q.ray_ns[:R].long().cpu(), q.ray_soff[:R].long().cpu()
    S = int(ns.sum())
    locw = q.samp_locw[:S * 3].view(S, 3).cpu()
    sr = torch.repeat_interleave(torch.arange(R), ns)
    dense = torch.zeros(R, SR, 3).index_put((sr, torch.arange(S) - soff[sr]), locw)
    c, r = torch.from_numpy(view.campos).reshape(3), torch.from_numpy(view.camrotc2w).reshape(-1)
    z = ((dense[..., 0] - c[0]) * r[2] + (dense[..., 1] - c[1]) * r[5]) + (dense[..., 2] - c[2]) * r[8]
    assert z.dtype == F32
    w = out.blendw.cpu().double()
    mask = out.ray_mask.cpu().bool()
    assert 0 < int(mask.sum()) and bool((w[~mask] == 0).all())
    D, W, _ = dr.depth_of(w, z, mask)
    ED, _, _ = tdg.depth_bounds(z, w, torch.zeros_like(w), D, W, mask)
    assert tdg._same_bits(out.depth.cpu()[~mask], torch.zeros(int((~mask).sum())))
    tdg._ratio(out.depth, D, ED, f"render depth [{precision}]")
    assert float(D.max()) > 0.1


def test_ray_marching_and_plugin_return_coarse_depth(tmp_path):
    """forward: [1, R'] compacted; fill_invalid / render / the plugin's test(): [1, R], zero off ray_mask; no such
    key without the options."""
    from sgnerf_amd.model import HipPointsVolumetricModel
    pc, view, qd, mlp, gt = _setup(seed=3)
    R = view.raydir.shape[0]
    inputs = {"campos": _d(view.campos)[None], "raydir": _d(view.raydir)[None], "camrotc2w": _d(view.camrotc2w)[None],
              "near": torch.tensor([[[0.1]]]), "far": torch.tensor([[[8.0]]])}
    pts = NeuralPoints.from_cloud(pc, DEV)
    for o in (O, dataclasses.replace(O, compute_depth=1), dataclasses.replace(O, depth_loss_items=("coarse_depth",))):
        net = NeuralPointsRayMarching(pts, mlp, o, DEV)
        full, comp = net.render(inputs), net.forward(inputs)
        if not o.want_depth:
            assert "coarse_depth" not in full and "coarse_depth" not in comp
            continue
        mask = full["ray_mask"][0].bool()
        assert full["coarse_depth"].shape == (1, R) and comp["coarse_depth"].shape == (1, int(mask.sum()))
        assert 0 < int(mask.sum()) < R
        assert bool((full["coarse_depth"][0][~mask] == 0).all()) and bool((full["coarse_depth"][0][mask] > 0).all())
        assert torch.equal(comp["coarse_depth"][0], full["coarse_depth"][0][mask])
        filled = fill_invalid(comp, inputs)
        assert torch.equal(filled["coarse_depth"], full["coarse_depth"])
    for extra in ({}, {"compute_depth": 1}):
        opt = argparse.Namespace(SR=24, K=8, gpu_ids=[0], is_train=False, checkpoints_dir=str(tmp_path), name="scene",
                                 bg_color="white", **extra)
        m = HipPointsVolumetricModel()
        m.initialize(opt)
        m.set_points(points_xyz=pc.xyz, points_feats=pc.color * 255.0, points_embedding=pc.embedding,
                     points_color=pc.color, points_dir=pc.dir, points_conf=pc.conf, aggregator_state=mlp)
        m.set_input(inputs)
        out = m.test()
        if not extra:
            assert "coarse_depth" not in out
        else:
            assert out["coarse_depth"].shape == (1, R)
            assert float((out["coarse_depth"] - full["coarse_depth"]).abs().max()) <= 1e-6   # another renderer, same frame
            assert bool((out["coarse_depth"][0][~out["ray_mask"][0].bool()] == 0).all())


# ---- training --------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _reference(explicit):
    """train.Trainer (fp32 autograd, CPU) with depth supervision on the oracle's query: computed once."""
    pc, view, qd, mlp, gt = _setup(seed=3)
    gt_d, gt_m = _targets()
    pts = PointParams(pc.xyz, pc.embedding, pc.color, pc.dir, pc.conf, "cpu")
    ref = Trainer(pts, mlp, O, "cpu")
    R = view.raydir.shape[0]
    parts, full, mask, dmap = ref.backward(torch.from_numpy(view.campos), torch.from_numpy(view.camrotc2w),
                                           torch.from_numpy(view.raydir), 0.1, 8.0, gt, q=qd,
                                           depth=depth_target(gt_d, gt_m if explicit else None, W_D, R, "cpu"))
    g = {}
    for name, *_ in LAYERS:
        m = ref.mlp.lin[name.replace(".", "_")]
        g[name + ".weight"], g[name + ".bias"] = m.weight.grad.clone(), m.bias.grad.clone()
    for k in NAMES:
        g[k] = getattr(pts, k).grad.clone()
    return {k: float(v) for k, v in parts.items()}, full.clone(), mask.clone(), dmap.clone(), g


def _trainer(precision, graph=True):
    pc, view, qd, mlp, gt = _setup(seed=3)
    tr = HipTrainer(sw._points(pc), mlp, O, DEV, precision=precision)
    tr.use_graph = graph
    return tr


PATHS = [("f32", True), ("f16", True), ("f16", False)]


@pytest.mark.parametrize("explicit", [False, True])
@pytest.mark.parametrize("precision,graph", PATHS)
def test_backward_with_depth_matches_fp32_autograd(precision, graph, explicit):
    """One HIP backward with depth supervision against train.Trainer on the CPU: the depth map, the loss parts
    and every gradient within the bars tests/test_point_grad_switches_gpu.py uses for the precision -- on a
    scene where the depth term moves the reference gradients by far more than those bars."""
    pc, view, qd, mlp, gt = _setup(seed=3)
    gt_d, gt_m = _targets()
    parts_c, full_c, mask_c, dmap_c, ref_g = _reference(explicit)
    plain_g = sw._reference(())[3]
    moved = {k: _rel(ref_g[k], plain_g[k]) for k in ref_g}
    assert moved["alpha_branch.0.weight"] > 10 * sw.GRAD_TOL_MLP and moved["points_conf"] > 10 * sw.GRAD_TOL_POINTS, moved
    tr = _trainer(precision, graph)
    R = view.raydir.shape[0]
    dt = depth_target(gt_d, gt_m if explicit else None, W_D, R, DEV)
    parts, full, ray_mask, dmap = tr.backward(*_view(view), 0.1, 8.0, gt.to(DEV), depth=dt)
    torch.cuda.synchronize()
    assert torch.equal(ray_mask.cpu(), mask_c) and dmap.shape == (R,)
    assert bool((dmap.cpu()[~mask_c] == 0).all())
    assert float((dmap.cpu() - dmap_c).abs().max()) <= 1e-3
    assert float((full.cpu() - full_c).abs().max()) <= 1e-3
    # the reported loss is the definition applied to the step's own depth map
    want = _loss64(dmap, gt_d, gt_m if explicit else None)
    assert abs(float(parts["coarse_depth"]) - want) <= 1e-5 * want, (float(parts["coarse_depth"]), want)
    for k in ("total", "coarse_depth"):
        print(f"[{precision}, graph {graph}] {k}: hip {float(parts[k]):.8e} ref {parts_c[k]:.8e}")
        assert abs(float(parts[k]) - parts_c[k]) <= 1e-3 * abs(parts_c[k])
    stock = float(parts["ray_masked_coarse_raycolor"]) + 3e-6 + 1e-4 * float(parts["conf_coefficient"])
    assert abs(float(parts["total"]) - (stock + W_D * float(parts["coarse_depth"]))) <= 1e-6 * abs(float(parts["total"]))
    g = grads_named(tr)
    worst = {k: _rel(g[k].cpu().reshape(b.shape), b) for k, b in ref_g.items()}
    print(f"[{precision}, graph {graph}] relative L2 gradient errors:", {k: f"{v:.2e}" for k, v in worst.items()})
    if precision == "f32":
        bad = {k: v for k, v in worst.items() if v > (sw.GRAD_TOL_F32_ORACLE_Q if k.startswith("points_") else sw.GRAD_TOL_F32)}
    else:
        bad = {k: v for k, v in worst.items() if v > (sw.GRAD_TOL_POINTS if k.startswith("points_") else sw.GRAD_TOL_MLP)}
    assert not bad, bad


def test_f16_graph_and_eager_agree_with_depth():
    """As tests/test_train_gpu.py::test_graph_captured_step_matches_eager_step holds them together without depth:
    the mask equal, colour within 1e-5, the loss within 1e-5 relative, gradients within 2e-3 relative L2 -- and
    the depth map within 1e-5."""
    pc, view, qd, mlp, gt = _setup(seed=3)
    gt_d, gt_m = _targets()
    R = view.raydir.shape[0]
    runs = []
    for graph in (False, True):
        tr = _trainer("f16", graph)
        parts, full, mask, dmap = tr.backward(*_view(view), 0.1, 8.0, gt.to(DEV), depth=depth_target(gt_d, gt_m, W_D, R, DEV))
        torch.cuda.synchronize()
        runs.append(({k: float(v) for k, v in parts.items()}, full.cpu(), mask.cpu(), dmap.cpu(),
                     {k: v.cpu() for k, v in grads_named(tr).items()}))
        assert bool(tr.stepper._graphs) == graph
    (pe, fe, me, de, ge), (pg, fg, mg, dg, gg) = runs
    assert torch.equal(me, mg) and float((fe - fg).abs().max()) <= 1e-5 and float((de - dg).abs().max()) <= 1e-5
    for k in ("total", "coarse_depth"):
        assert abs(pe[k] - pg[k]) <= 1e-5 * abs(pe[k]), k
    err = {k: _rel(gg[k], ge[k]) for k in ge}
    print("grad rel L2", {k: f"{v:.1e}" for k, v in err.items()})
    assert max(err.values()) <= 2e-3, err


@pytest.mark.parametrize("precision,graph", PATHS)
def test_depth_steps_replay_one_graph_and_leave_the_stock_step_alone(precision, graph):
    """Two backwards with different gt_depth (the second with other values in the same static buffers): one
    capture on the graph path, and each reports its own loss.  A backward without depth afterwards gives the loss
    parts, the colour and the mask of a trainer that never saw depth, bit for bit."""
    pc, view, qd, mlp, gt = _setup(seed=3)
    R = view.raydir.shape[0]
    args = (*_view(view), 0.1, 8.0, gt.to(DEV))
    tr, fresh = _trainer(precision, graph), _trainer(precision, graph)
    seen = []
    for seed in (0, 1):
        gt_d, gt_m = _targets(seed)
        parts, full, mask, dmap = tr.backward(*args, depth=depth_target(gt_d, gt_m, W_D, R, DEV))
        want = _loss64(dmap, gt_d, gt_m)
        assert abs(float(parts["coarse_depth"]) - want) <= 1e-5 * want
        seen.append((float(parts["coarse_depth"]), tr.graph_captures))
    assert seen[0][0] != seen[1][0]
    assert seen[0][1] == seen[1][1] == (1 if precision == "f16" and graph else 0)
    after = tr.backward(*args)
    never = fresh.backward(*args)
    torch.cuda.synchronize()
    assert len(after) == 3 and "coarse_depth" not in after[0]
    assert set(after[0]) == set(never[0])
    for k in after[0]:
        assert tdg._same_bits(after[0][k].reshape(1), never[0][k].reshape(1)), k
    assert tdg._same_bits(after[1], never[1]) and torch.equal(after[2], never[2])


@pytest.mark.parametrize("precision,graph", PATHS)
def test_plugin_step_with_depth_supervision(tmp_path, precision, graph):
    """optimize_parameters under depth_loss_items = coarse_depth: loss_coarse_depth is the definition applied to
    the step's own coarse_depth output ([1, R], zero off ray_mask), the loss is listed, a batch whose gt_depth has
    another length is refused."""
    from sgnerf_amd.model import HipPointsVolumetricModel
    pc, view, qd, mlp, gt = _setup(seed=3)
    gt_d, gt_m = _targets()
    R = view.raydir.shape[0]
    opt = argparse.Namespace(SR=24, K=8, gpu_ids=[0], is_train=True, checkpoints_dir=str(tmp_path), name="scene",
                             lr=5e-4, plr=2e-3, lr_decay_exp=0.1, lr_decay_iters=1_000_000, bg_color="white",
                             precision=precision, depth_loss_items=["coarse_depth"], depth_loss_weights=[0.5])
    m = HipPointsVolumetricModel()
    m.initialize(opt)
    m.set_points(points_xyz=pc.xyz, points_feats=pc.color * 255.0, points_embedding=pc.embedding,
                 points_color=pc.color, points_dir=pc.dir, points_conf=pc.conf, aggregator_state=mlp)
    m.setup(opt)
    m.trainer.use_graph = graph
    assert "coarse_depth" in m.loss_names
    inputs = {"campos": _d(view.campos)[None], "raydir": _d(view.raydir)[None], "camrotc2w": _d(view.camrotc2w)[None],
              "near": torch.tensor([[[0.1]]]), "far": torch.tensor([[[8.0]]]), "gt_image": gt[None].to(DEV),
              "gt_depth": gt_d.reshape(1, R, 1), "gt_mask": gt_m.reshape(1, R, 1)}
    m.set_input(inputs)
    for step in range(2):
        m.optimize_parameters(total_steps=step)
        D = m.output["coarse_depth"]
        mask = m.output["ray_mask"][0].bool()
        assert D.shape == (1, R) and bool((D[0][~mask] == 0).all()) and bool((D[0][mask] > 0).all())
        want = _loss64(D, gt_d, gt_m)
        losses = m.get_current_losses()
        assert abs(float(losses["coarse_depth"]) - want) <= 1e-5 * want
        stock = float(losses["ray_masked_coarse_raycolor"]) + 3e-6 + 1e-4 * float(losses["conf_coefficient"])
        assert abs(float(losses["total"]) - (stock + 0.5 * want)) <= 1e-5 * abs(float(losses["total"]))
    m.set_input(dict(inputs, gt_depth=gt_d[:-1]))
    with pytest.raises(ValueError, match="gt_depth"):
        m.optimize_parameters(total_steps=2)
    m.set_input({k: v for k, v in inputs.items() if k != "gt_depth"})
    with pytest.raises(ValueError, match="gt_depth"):
        m.optimize_parameters(total_steps=2)
