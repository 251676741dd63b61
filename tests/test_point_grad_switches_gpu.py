"""GPU tests of the per-tensor training switches opt.feat_grad / color_grad / dir_grad / conf_grad
(neural_points.py:410-416; opts.HotPathOpts, train_hip.HipTrainer, point_adam.PointAdam, the plugin).

A frozen tensor receives no gradient, has no Adam moments and stays bit-identical to its initial value;
the loss and the trained tensors' and the MLP's gradients are the functions they are with everything
trained.  The scene is the one tests/test_train_gpu.py uses (test_train_cpu._setup restated below: a few
thousand samples of the small room, the oracle's query of the same rays), the bars are that module's."""
import argparse
import ctypes
import dataclasses
import functools
import math

import numpy as np
import pytest
import torch

import oracle_query as oq
import train_rows_ref as rr
from helpers import hyper_for, make_view, small_room, t_table
from sgnerf_amd import _lib
from sgnerf_amd.opts import HotPathOpts
from sgnerf_amd.point_adam import NoPointAdam, PointAdam
from sgnerf_amd.train import PointParams, Trainer
from sgnerf_amd.train_hip import HipTrainer, grads_named
from sgnerf_amd.weights import LAYERS, init_mlp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# the bars of tests/test_train_gpu.py (see its docstring and comments for where they come from)
GRAD_TOL_MLP = 2e-2
GRAD_TOL_POINTS = 6e-2
GRAD_TOL_F32 = 1e-4
GRAD_TOL_F32_ORACLE_Q = 5e-3
UPDATE_TOL = 0.1

O = HotPathOpts(SR=24)
NAMES = ("points_embeding", "points_color", "points_dir", "points_conf")
SWITCH = {"points_embeding": "feat_grad", "points_color": "color_grad", "points_dir": "dir_grad",
          "points_conf": "conf_grad"}
# the frozen tensors of each switch set
SETS = {"dir": ("points_dir",), "conf": ("points_conf",), "feat": ("points_embeding",),
        "color_dir": ("points_color", "points_dir"), "none_trained": NAMES}


def _opts(frozen, base=O, **kw):
    return dataclasses.replace(base, **{SWITCH[k]: 0 for k in frozen}, **kw)


@functools.lru_cache(maxsize=None)
def _setup(seed=0, h=12, w=16, yaw=30.0):
    """test_train_cpu._setup: the small room, one view, the oracle's sample-major query, an opaque MLP."""
    pc = small_room(60_000, seed=seed)
    view = make_view(h, w, yaw=yaw, pitch=-8.0)
    q = oq.OracleGrid(pc.xyz, hyper_for(pc, O), O).query(view.campos, view.raydir, t_table(O).numpy())
    R = view.raydir.shape[0]
    rs, ss = np.nonzero(np.arange(O.SR)[None, :] < q["ray_ns"][:, None])
    ray_ns = torch.from_numpy(q["ray_ns"]).long()
    qd = {"ray_ns": ray_ns, "ray_soff": torch.cumsum(ray_ns, 0) - ray_ns, "samp_ray": torch.from_numpy(rs).long(),
          "samp_locw": torch.from_numpy(q["loc_w"][rs, ss]), "pidx": torch.from_numpy(q["pidx"][rs, ss]).long()}
    mlp = init_mlp(seed, bias_std=0.01)
    mlp["alpha_branch.0.bias"] = mlp["alpha_branch.0.bias"] + 100.0
    gt = torch.rand(R, 3, generator=torch.Generator().manual_seed(seed))
    return pc, view, qd, mlp, gt


def _points(pc, dev=DEV):
    return PointParams(pc.xyz, pc.embedding, pc.color, pc.dir, pc.conf, dev)


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _rel(a, b):
    return float(torch.linalg.vector_norm(a.double() - b.double()) / max(torch.linalg.vector_norm(b.double()), 1e-30))


@functools.lru_cache(maxsize=None)
def _reference(frozen, seed=3):
    """train.Trainer (fp32 autograd, CPU) on the oracle's query under the switch set: computed once per
    set, shared by the precisions, never changed.  Returns (parts, full, mask, gradients by name)."""
    pc, view, qd, mlp, gt = _setup(seed=seed)
    pts = _points(pc, "cpu")
    ref = Trainer(pts, mlp, _opts(frozen), "cpu")
    parts, full, mask = ref.backward(torch.from_numpy(view.campos), torch.from_numpy(view.camrotc2w),
                                     torch.from_numpy(view.raydir), 0.1, 8.0, gt, q=qd)
    g = {}
    for name, *_ in LAYERS:
        m = ref.mlp.lin[name.replace(".", "_")]
        g[name + ".weight"], g[name + ".bias"] = m.weight.grad.clone(), m.bias.grad.clone()
    for k in NAMES:
        t = getattr(pts, k).grad
        g[k] = None if t is None else t.clone()
    return {k: float(v) for k, v in parts.items()}, full.clone(), mask.clone(), g


# ---- 1. one backward per switch set and precision ------------------------------------------------

@pytest.mark.parametrize("precision", ["f16", "f32"])
@pytest.mark.parametrize("which", list(SETS))
def test_backward_matches_fp32_autograd_under_the_switches(which, precision):
    """One HIP backward against train.Trainer on the CPU with the same switches on the oracle's query:
    every trained tensor and every MLP layer within the bars of test_train_gpu._grads_vs_fp32 for the
    precision, the loss within 1e-3 relative and the colour within 1e-3 (that test's bounds), the ray mask
    equal; each frozen tensor's .grad is None or all zero -- while its all-trained reference gradient is
    non-zero on this scene, so the freeze is what removed it."""
    frozen = SETS[which]
    full_ref = _reference(())[3]
    for k in frozen:
        assert float(torch.linalg.vector_norm(full_ref[k])) > 0, f"{k}: the scene gives it no gradient"
    parts_c, full_c, mask_c, ref_g = _reference(frozen)
    for k in frozen:   # the reference freezes the reference's way: no gradient
        assert ref_g[k] is None
    # the loss values do not depend on the switches (conf frozen: the zero-one term is still reported)
    parts_all = _reference(())[0]
    for k, v in parts_all.items():
        assert parts_c[k] == v, k
    pc, view, qd, mlp, gt = _setup(seed=3)
    points = _points(pc)
    tr = HipTrainer(points, mlp, _opts(frozen), DEV, precision=precision)
    parts, full, ray_mask = tr.backward(_d(view.campos), _d(view.camrotc2w), _d(view.raydir), 0.1, 8.0, gt.to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(ray_mask.cpu(), mask_c)
    for k in ("total", "ray_masked_coarse_raycolor", "conf_coefficient"):
        print(f"{which} [{precision}] {k}: hip {float(parts[k]):.8e} ref {parts_c[k]:.8e}")
    assert abs(float(parts["total"]) - parts_c["total"]) <= 1e-3 * abs(parts_c["total"])
    assert abs(float(parts["conf_coefficient"]) - parts_c["conf_coefficient"]) <= 1e-3 * abs(parts_c["conf_coefficient"])
    assert float((full.cpu() - full_c).abs().max()) <= 1e-3
    g = grads_named(tr)
    for k in frozen:
        assert getattr(points, k).grad is None and not getattr(points, k).requires_grad
        assert g[k] is None or not bool(g[k].any())
    worst = {k: _rel(g[k].cpu().reshape(b.shape), b) for k, b in ref_g.items() if b is not None}
    assert set(worst) == {k for k in ref_g if k not in frozen}
    print(f"{which} [{precision}]: relative L2 gradient errors:", {k: f"{v:.2e}" for k, v in worst.items()})
    if precision == "f32":
        bad = {k: v for k, v in worst.items() if v > (GRAD_TOL_F32_ORACLE_Q if k.startswith("points_") else GRAD_TOL_F32)}
    else:
        bad = {k: v for k, v in worst.items() if v > (GRAD_TOL_POINTS if k.startswith("points_") else GRAD_TOL_MLP)}
    assert not bad, bad
    # the point group holds the trained tensors only; nothing trained: no point Adam at all
    if len(frozen) == 4:
        assert isinstance(tr.opt_pts, NoPointAdam) and tr.point_params == []
    else:
        assert tr.opt_pts.param_groups[0]["point_tensors"] == [k for k in NAMES if k not in frozen]
        assert len(tr.opt_pts.param_groups[0]["params"]) == 4 - len(frozen)
    if precision == "f32":   # a frozen embedding: neither block1.0's input-gradient GEMM nor its buffer
        step = tr.stepper.step
        assert (step.dx0 is None) == ("points_embeding" in frozen)
        assert ("dx0" in [n for n, _ in step.g_row_bwd]) == ("points_embeding" not in frozen)
        assert "d1" in [n for n, _ in step.g_row_bwd]   # the rest of the chain is there


# ---- 2. steps: frozen tensors never move, the row-sparse Adam equals the dense one ---------------

@pytest.mark.parametrize("precision", ["f16", "f32"])
@pytest.mark.parametrize("which", list(SETS))
def test_steps_leave_frozen_tensors_and_match_the_dense_adam(which, precision):
    """Three step() calls at flush_every = 2 (a flush inside the run), then sync_points(): frozen tensors
    torch.equal their initial values and have no optimizer state, trained ones moved, and the trained
    tensors torch.equal what the dense PointAdam(rows=False) over the same subset makes of the same
    batches' gradients.  The dense optimizer is fed each step's gradient tensors as the HIP backward
    wrote them: a second trainer's own backward would differ from the first's in the last bits (the
    point gradients are accumulated by atomics in no fixed order), which says nothing about the Adam."""
    frozen = SETS[which]
    pc, view, qd, mlp, gt = _setup(seed=7)
    points = _points(pc)
    tr = HipTrainer(points, mlp, _opts(frozen), DEV, precision=precision)
    trained = [k for k in NAMES if k not in frozen]
    p0 = {k: getattr(points, k).detach().clone() for k in NAMES}
    dense_p = [torch.nn.Parameter(p0[k].clone()) for k in trained]
    dense = PointAdam(dense_p, lr=2e-3, betas=(0.9, 0.999), rows=False, names=trained) if trained else None
    if trained:
        assert tr.opt_pts.rows_mode and tr.opt_pts.row0 == ("points_conf" in trained)
        tr.opt_pts.flush_every = 2
    oob_watches = 0
    watch = tr._watch_oob

    def counted(count):
        nonlocal oob_watches
        oob_watches += 1
        return watch(count)
    tr._watch_oob = counted
    for it in range(3):
        torch.manual_seed(100 + it)
        gti = torch.rand(gt.shape, generator=torch.Generator().manual_seed(it)).to(DEV)
        tr.backward(_d(view.campos), _d(view.camrotc2w), _d(view.raydir), 0.1, 8.0, gti)
        for k, p in zip(trained, dense_p):
            p.grad = getattr(points, k).grad.detach().clone()
        tr.apply()
        if dense is not None:
            dense.param_groups[0]["lr"] = tr.opt_pts.param_groups[0]["lr"]
            dense.step()
    tr.sync_points()
    tr.check_touched()
    torch.cuda.synchronize()
    assert oob_watches == 3   # the out-of-range-id watch saw every step, point Adam launch or not
    for k in frozen:
        p = getattr(points, k)
        assert torch.equal(p.detach(), p0[k]), k
        assert p not in tr.opt_pts.state
    for k, dp in zip(trained, dense_p):
        p = getattr(points, k).detach()
        assert not torch.equal(p, p0[k]), k
        assert torch.equal(p, dense_p[trained.index(k)].detach()), k
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(tr.opt_pts.state[getattr(points, k)][key].reshape(dp.shape), dense.state[dp][key]), (k, key)
    if trained:   # the state round-trips under the same switches and refuses another set's
        sd = tr.opt_pts.state_dict()
        tr2 = HipTrainer(_points(pc), mlp, _opts(frozen), DEV, precision=precision)
        tr2.opt_pts.load_state_dict(sd)
        sd2 = tr2.opt_pts.state_dict()
        assert sd2["param_groups"][0]["point_tensors"] == trained
        for i in sd["state"]:
            for key in ("step", "exp_avg", "exp_avg_sq"):
                assert torch.equal(torch.as_tensor(sd["state"][i][key]).cpu(), torch.as_tensor(sd2["state"][i][key]).cpu())
        other = ("points_color",) if frozen != ("points_color",) else ("points_dir",)
        tr3 = HipTrainer(_points(pc), mlp, _opts(other), DEV, precision=precision)
        with pytest.raises(ValueError, match="dir_grad"):
            tr3.opt_pts.load_state_dict(sd)


# ---- 3. the SG variant at f32 with dir_grad = 0: the scripts' combination -------------------------

def test_sg_f32_backward_with_frozen_dir_matches_fp32_autograd():
    """block2_bpnet (bpnet_dim 96, the semantic-guided query) at precision "f32" with dir_grad = 0: one
    backward against fp32 autograd through oracle/agg_ref.py's SG aggregator on the very samples the HIP
    query produced, as test_hip_sg_f32_training_gradients_match_fp32_autograd does it and at its bar
    (GRAD_TOL_F32 for the colour, the loss and every gradient); points_dir takes no gradient."""
    import agg_ref
    dim, seed, K = 96, 3, 8
    pc, view, _, mlp, gt = _setup(seed=seed)
    n = pc.xyz.shape[0]
    g = torch.Generator().manual_seed(11)
    bound = math.sqrt(6.0 / (256 + dim + 256)) * 0.5
    mlp = dict(mlp)
    mlp["block2_bpnet.0.weight"] = (torch.rand(256, 256 + dim, generator=g) * 2 - 1) * bound
    mlp["block2_bpnet.0.bias"] = torch.randn(256, generator=g) * 0.01
    bp = torch.rand(n, dim, generator=g) - 0.5
    o = _opts(("points_dir",), shading_feature_mlp_layer2_bpnet=1, predict_semantic=1, semantic_guidance=1, K=K)
    points = _points(pc)
    tr = HipTrainer(points, mlp, o, DEV, bpnet=bp, precision="f32")
    R = view.raydir.shape[0]
    labels = (torch.zeros(n, dtype=torch.int32), torch.ones(R, dtype=torch.int32), 10)
    parts, full, mask = tr.backward(_d(view.campos), _d(view.camrotc2w), _d(view.raydir), 0.1, 8.0, gt.to(DEV), labels)
    torch.cuda.synchronize()
    hg = grads_named(tr)
    assert hg["points_dir"] is None and points.points_dir.grad is None
    qd = {k: v.long() if v.dtype == torch.int32 else v for k, v in tr.last_query.items()}
    pts = {k: torch.from_numpy(getattr(pc, k)).to(DEV).requires_grad_(k not in ("xyz", "dir"))
           for k in ("xyz", "embedding", "color", "dir", "conf")}
    pts["bpnet"] = bp.to(DEV)
    m = {k: v.to(DEV).requires_grad_(True) for k, v in mlp.items()}
    campos, rot, raydir = _d(view.campos), _d(view.camrotc2w), _d(view.raydir)
    feat, _ = agg_ref.aggregate(pts, m, campos, rot, raydir, qd["samp_ray"], qd["samp_locw"], qd["pidx"])
    nnb = (qd["pidx"] >= 0).sum(-1)
    fd, vd, ld = agg_ref.densify(R, O.SR, qd["ray_ns"], qd["samp_ray"], qd["samp_locw"], feat, nnb)
    color, _, _ = agg_ref.composite(fd, vd, ld, rot, campos)
    ray_mask = vd.any(-1)
    gtd = gt.to(DEV)
    l_col = torch.mean((color[ray_mask] - gtd[ray_mask]) ** 2)
    S = qd["samp_ray"].shape[0]
    slot = torch.arange(S, device=DEV) - qd["ray_soff"][qd["samp_ray"]]
    pd = torch.full((R, O.SR, K), -1, dtype=torch.long, device=DEV)
    pd[qd["samp_ray"], slot] = qd["pidx"]
    cd = pts["conf"][torch.clamp(pd[ray_mask], min=0).reshape(-1), 0]
    val = torch.clamp(torch.clamp(cd, 1e-4, 1.0), 1e-3, 1 - 1e-3)
    l_zo = torch.mean(torch.log(val) + torch.log(1 - val))
    total = l_col + 3e-6 + 1e-4 * l_zo
    total.backward()
    torch.cuda.synchronize()
    assert torch.equal(mask, ray_mask)
    assert _rel(full[ray_mask], color[ray_mask].detach()) <= GRAD_TOL_F32
    assert abs(float(parts["total"]) - float(total)) <= GRAD_TOL_F32 * abs(float(total))
    names = {"points_embeding": "embedding", "points_color": "color", "points_conf": "conf"}
    worst = {}
    for k, v in hg.items():
        if k == "points_dir":
            continue
        ref = pts[names[k]].grad if k in names else m[k].grad
        worst[k] = _rel(v.reshape(ref.shape), ref)
    print("SG f32 dim 96, dir frozen: relative L2 gradient errors (same query):", {k: f"{v:.2e}" for k, v in worst.items()})
    assert "block2_bpnet.0.weight" in worst and "block3.0.weight" in worst
    bad = {k: v for k, v in worst.items() if v > GRAD_TOL_F32}
    assert not bad, bad


# ---- 4. the plugin -------------------------------------------------------------------------------

def test_plugin_keeps_a_frozen_points_dir(tmp_path):
    """The plugin under an opt with dir_grad = 0 (SG-NeRF's semantic-guidance scripts): points_dir is
    bit-identical to what went in after three optimize_parameters, and after prune_points (masked only),
    grow_points (the passed rows appended, nothing else changed), a checkpoint save / load and two more
    steps; the other tensors train.  Before the switches existed points_dir moved at the first step."""
    from sgnerf_amd.model import HipPointsVolumetricModel
    pc, view, qd, mlp, gt = _setup(seed=3)
    opt = argparse.Namespace(SR=24, K=8, gpu_ids=[0], is_train=True, checkpoints_dir=str(tmp_path), name="scene",
                             lr=5e-4, plr=2e-3, lr_decay_exp=0.1, lr_decay_iters=1_000_000, bg_color="white",
                             feat_grad=1, color_grad=1, conf_grad=1, dir_grad=0, xyz_grad=0)
    m = HipPointsVolumetricModel()
    m.initialize(opt)
    m.set_points(points_xyz=pc.xyz, points_feats=pc.color * 255.0, points_embedding=pc.embedding,
                 points_color=pc.color, points_dir=pc.dir, points_conf=pc.conf, aggregator_state=mlp)
    m.setup(opt)
    assert m.opts.dir_grad == 0 and m.trainer.opts.dir_grad == 0
    inputs = {"campos": _d(view.campos)[None], "raydir": _d(view.raydir)[None], "camrotc2w": _d(view.camrotc2w)[None],
              "near": torch.tensor([[[0.1]]]), "far": torch.tensor([[[8.0]]]), "gt_image": gt[None].to(DEV)}
    m.set_input(inputs)
    dir0 = torch.from_numpy(pc.dir).to(DEV).reshape(1, -1, 3)
    col0 = torch.from_numpy(pc.color).to(DEV).reshape(1, -1, 3)
    for step in range(3):
        m.optimize_parameters(total_steps=step)
    assert torch.equal(m.neural_points.points_dir, dir0)
    # still a view of the trainer's tensor, which is in no optimizer group
    assert m.neural_points.points_dir.data_ptr() == m.trainer.points.points_dir.data_ptr()
    assert m.optimizers[1].param_groups[0]["point_tensors"] == ["points_embeding", "points_color", "points_conf"]
    m.test()   # brings every row to the optimizer's step
    assert not torch.equal(m.neural_points.points_color, col0)
    # prune: masked only
    thresh = float(torch.quantile(m.neural_points.points_conf.reshape(-1), 0.25))
    mask = m.neural_points.points_conf[0, :, 0] >= thresh
    m.clean_optimizer()
    m.clean_scheduler()
    assert m.prune_points(thresh) > 0
    m.setup_optimizer(opt)
    m.init_scheduler(3, opt)
    assert torch.equal(m.neural_points.points_dir, dir0[:, mask])
    m.optimize_parameters(total_steps=3)
    assert torch.equal(m.neural_points.points_dir, dir0[:, mask])
    # grow: the passed rows appended
    k = 64
    g = torch.Generator().manual_seed(0)
    add = [torch.rand(k, c, generator=g) for c in (3, 32, 3, 3, 1)]
    add[0] = add[0] * 0.1 + torch.from_numpy(pc.xyz[:1])
    m.clean_optimizer_scheduler()
    m.grow_points(*add, add_label=None)
    want = torch.cat([dir0[:, mask], add[3].to(DEV)[None]], 1)
    assert torch.equal(m.neural_points.points_dir, want)
    m.optimize_parameters(total_steps=4)
    assert torch.equal(m.neural_points.points_dir, want)
    # checkpoint round trip, the optimizer rebuilt over the loaded points
    m.save_networks("latest")
    m.load_networks("latest")
    m.reset_optimizer(opt)
    assert m.trainer.opts.dir_grad == 0 and not m.trainer.points.points_dir.requires_grad
    m.set_input(inputs)
    for step in (5, 6):
        m.optimize_parameters(total_steps=step)
        assert np.isfinite(float(m.get_current_losses()["total"]))
    m.test()
    assert torch.equal(m.neural_points.points_dir, want)
    assert m.neural_points.points_dir.shape[1] == int(mask.sum()) + k


def test_plugin_refuses_xyz_grad():
    from sgnerf_amd.model import HipPointsVolumetricModel
    opt = argparse.Namespace(SR=24, K=8, gpu_ids=[0], is_train=True, xyz_grad=1)
    with pytest.raises(NotImplementedError, match="xyz_grad"):
        HipPointsVolumetricModel().initialize(opt)


# ---- 5. two emulated ranks -----------------------------------------------------------------------

def _fake_two_ranks(monkeypatch, gathered):
    """test_train_gpu._fake_two_ranks: torch.distributed as two ranks holding the same batch; the
    shapes of what is all-gathered are recorded."""
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_available", lambda: True)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    monkeypatch.setattr(dist, "all_reduce", lambda t, *a, **k: t.mul_(2))

    def gather(out, inp, *a, **k):
        assert out.numel() == 2 * inp.numel()
        gathered.append((tuple(inp.shape), inp.dtype))
        out.view(2, -1).copy_(inp.reshape(1, -1).expand(2, -1))
    monkeypatch.setattr(dist, "all_gather_into_tensor", gather)


@pytest.mark.parametrize("precision", ["f16", "f32"])
def test_data_parallel_step_with_frozen_dir(precision, monkeypatch):
    """test_data_parallel_step_matches_single_rank with dir_grad = 0: two emulated ranks holding the same
    batch equal the one-rank step at that test's bar, points_dir stays where it was, and the sparse row
    exchange carries the trained tensors' 32 + 3 + 1 columns -- no dir columns."""
    pc, view, qd, mlp, gt = _setup(seed=7)
    trained = ("points_embeding", "points_color", "points_conf")
    runs, gathered = {}, []
    for mode in ("one", "one_again", "dp"):
        if mode == "dp":
            _fake_two_ranks(monkeypatch, gathered)
        points = _points(pc)
        tr = HipTrainer(points, mlp, _opts(("points_dir",)), DEV, precision=precision)
        p0 = {k: getattr(points, k).detach().clone() for k in NAMES}
        p0["mlp"] = tr.mlp.flat.detach().clone()
        losses = []
        for it in range(3):
            torch.manual_seed(100 + it)
            gti = torch.rand(gt.shape, generator=torch.Generator().manual_seed(it)).to(DEV)
            parts, _, _ = tr.step(_d(view.campos), _d(view.camrotc2w), _d(view.raydir), 0.1, 8.0, gti)
            losses.append(float(parts["total"]))
        tr.sync_points()
        assert torch.equal(points.points_dir.detach(), p0["points_dir"])
        upd = {k: getattr(points, k).detach() - p0[k] for k in trained}
        upd["mlp"] = tr.mlp.flat.detach() - p0["mlp"]
        runs[mode] = (losses, upd)
        monkeypatch.undo()
    rows = [s for s, dt in gathered if dt == torch.float32 and len(s) == 2]
    assert len(rows) == 3 and all(s[1] == 32 + 3 + 1 for s in rows), rows
    rel = lambda x, y: {k: float(torch.linalg.vector_norm((x[k] - y[k]).double())  # noqa: E731
                                 / torch.linalg.vector_norm(y[k].double())) for k in y}
    spread = rel(runs["one_again"][1], runs["one"][1])
    err = rel(runs["dp"][1], runs["one"][1])
    print("one-rank spread", {k: f"{v:.1e}" for k, v in spread.items()})
    print("dp vs one-rank", {k: f"{v:.1e}" for k, v in err.items()})
    assert abs(runs["dp"][0][0] - runs["one"][0][0]) <= 1e-5 * abs(runs["one"][0][0])
    for a, b in zip(runs["dp"][0], runs["one"][0]):
        assert abs(a - b) <= 1e-3 * abs(b)
    for k in err:
        assert float(torch.linalg.vector_norm(runs["dp"][1][k])) > 0
        assert err[k] <= max(UPDATE_TOL if precision == "f16" else 1e-2, 3 * spread[k]), (k, err, spread)


# ---- 6. the C ABI: NULL gradient outputs ---------------------------------------------------------
# the hand-built rows of tests/test_train_rows_gpu.py (257 points, rays of 0 .. SR samples), its helpers
# and the per-element bounds of its test_row_tail / test_row_head, against tests/train_rows_ref.py

ROW_CASES = [(8, 777), (3, 777)]


@pytest.mark.parametrize("null", [("embedding",), ("dir",), ("color",), ("color", "dir"), ("embedding", "color"),
                                  ("embedding", "color", "dir")])
@pytest.mark.parametrize("K,items", ROW_CASES)
def test_row_tail_with_null_members(K, items, null):
    """sgn_train_row_tail with NULL members of sgn_point_grads (and the NULL input gradient that goes with
    them: d_dx0 without the embedding, d_dext without colour and dir): the other outputs within
    test_row_tail's per-element bounds of the float64 reference; all three NULL: success, nothing written."""
    import test_train_rows_gpu as T
    c = T.case(K, items)
    rows, N, U = c.rows, rr.N_POINTS, T.U
    g = c.gen(5)
    dx0 = torch.rand(rows + T.GUARD, 224, generator=g) * 1e-3 + 1e-5
    dext = torch.rand(rows + T.GUARD, 8, generator=g) * 1e-3 + 1e-5
    g0 = dict(zip(("embedding", "color", "dir"), [torch.randn(N, n, generator=g) * 1e-4 for n in (32, 3, 3)]))
    dev = {k: t.to(DEV) for k, t in g0.items()}
    gconf = torch.full((N,), T.NAN, device=DEV)
    grads = _lib.PointGrads(*[None if k in null else dev[k].data_ptr() for k in ("embedding", "color", "dir")],
                            None if len(null) == 3 else gconf.data_ptr())   # all three frozen: an all-NULL struct
    p = _lib.ptr
    xd = None if "embedding" in null else dx0.to(DEV)
    ed = None if "color" in null and "dir" in null else dext.to(DEV)
    _lib.check(_lib.lib().sgn_train_row_tail(ctypes.byref(c.pt), ctypes.byref(c.qo), K, p(c.d["row_off"]), p(c.d["counts"]),
                                             p(xd), p(ed), ctypes.byref(grads), _lib.stream_handle()), "sgn_train_row_tail")
    torch.cuda.synchronize()
    assert T._all_nan(gconf)
    for k in null:   # never passed to the kernel
        assert T._same_bits(dev[k].cpu(), g0[k])
    r = dict(zip(("embedding", "color", "dir"), rr.row_tail_ref(c.points, c.camera, c.raydir, c.query, K, dx0[:rows], dext[:rows])))
    n_p = torch.zeros(N, dtype=torch.float64).index_add(0, c.pid, torch.ones(rows, dtype=torch.float64))[:, None]
    acc = lambda t: torch.zeros(N, t.shape[1], dtype=torch.float64).index_add(0, c.pid, t)  # noqa: E731
    dd = dx0[:rows].double()
    dpe = dd[:, 32:].reshape(rows, 32, 3, 2).abs()
    bands = torch.tensor([1.0, 2.0, 4.0], dtype=torch.float64)
    t_abs = dd[:, :32].abs() + (dpe.sum(-1) * bands).sum(-1)
    e_row = T.PE_ATOL * (dpe.sum(-1) * bands).sum(-1) + 2 * 7 * U * t_abs
    de = dext[:rows].double()
    td = de[:, 3:6].abs() + de[:, 6:7].abs()
    bounds = {"embedding": acc(e_row) + 2 * (n_p + 1) * U * (g0["embedding"].double().abs() + acc(t_abs)),
              "color": 2 * (n_p + 1) * U * (g0["color"].double().abs() + acc(de[:, :3].abs())),
              "dir": acc(3 * U * td) + 2 * (n_p + 1) * U * (g0["dir"].double().abs() + acc(td))}
    for k in ("embedding", "color", "dir"):
        if k in null:
            continue
        full = g0[k].double() + r[k]
        T._capped(bounds[k], full, k)
        T._ratio(dev[k].cpu(), full, bounds[k].clamp(min=1e-300), f"row_tail g_{k} (K={K}, items={items}, NULL {null})")
        assert T._same_bits(dev[k].cpu()[n_p[:, 0] == 0], g0[k][n_p[:, 0] == 0])


@pytest.mark.parametrize("K,items", ROW_CASES)
def test_row_head_with_null_gconf(K, items):
    """sgn_train_row_head with d_gconf = NULL: delta4, amax and the alpha branch's weight / bias gradient
    within test_row_head's per-element bounds of the float64 reference, and bit-identical to the call
    with d_gconf (which only adds the atomics)."""
    import test_train_rows_gpu as T
    c = T.case(K, items)
    rows, U = c.rows, T.U
    z4, dfs, dfeat, wa, ba, gconf0 = T._head_inputs(c)
    _, _, rrw, _ = rr.row_inputs_ref(c.points, c.camera, c.raydir, c.query, K)
    rw32 = torch.cat([rrw.float(), torch.full((T.GUARD, 2), T.NAN)])
    dev = [t.to(DEV) for t in (dfs, dfeat, rw32, wa, ba)]
    L = _lib.lib()
    n1 = int(L.sgn_train_head_partial_floats(1))
    zd = z4.to(DEV)
    part = torch.full((n1 + 8,), T.NAN, device=DEV)
    amax = torch.zeros(2, dtype=torch.int32, device=DEV)
    p = _lib.ptr
    _lib.check(L.sgn_train_row_head(ctypes.byref(c.pt), ctypes.byref(c.qo), c.K, p(c.d["row_off"]), p(c.d["counts"]), p(zd),
                                    p(dev[0]), p(dev[1]), p(dev[2]), p(dev[3]), p(dev[4]), None, p(amax), p(part),
                                    _lib.stream_handle()), "sgn_train_row_head")
    torch.cuda.synchronize()
    d4b, _, partb, amaxb, _ = T._run_row_head(c, z4, *dev, gconf0)
    assert T._same_bits(zd[:rows], d4b[:rows]) and T._same_bits(part[:n1], partb[:n1]) and torch.equal(amax, amaxb)
    d4 = zd.cpu()
    assert T._same_bits(d4[rows:], z4[rows:]) and T._all_nan(part[n1:]) and int(amax[1]) == 0
    d4 = d4[:rows]
    splits = n1 // 257
    dWa, dba = T._reduce(part, splits, 1, 257, 256, 256)
    das = dfeat[c.work.long(), 0]
    r_d4, _, r_dWa, r_dba, r_amax = rr.row_head_ref(c.points, c.camera, c.raydir, c.query, K, z4[:rows], dfs[:items], das,
                                                    rw32[:rows], wa, ba)
    z, w = z4[:rows].double(), wa.double()
    h4 = rr.lrelu(z)
    wc = rw32[:rows, 0].double()
    dfs_r, das_r = dfs[:items].double()[c.item], das.double()[c.item]
    x = h4 @ w + float(ba) - 1.0
    sg = torch.sigmoid(x)
    dot_wa = h4.abs() @ w.abs()
    e_x = 2 * 256 * U * dot_wa + 2 * U * (dot_wa + abs(float(ba)) + 1)
    e_sg = 0.25 * e_x + 4 * U
    dza = wc * das_r * sg
    e_dza = (wc * das_r).abs() * e_sg + 3 * U * dza.abs()
    t_abs = wc[:, None] * dfs_r.abs() + dza.abs()[:, None] * w.abs()[None, :]
    b_d4 = e_dza[:, None] * w.abs()[None, :] + 5 * U * t_abs
    T._capped(b_d4, r_d4, "delta4")
    T._ratio(d4, r_d4, b_d4, f"row_head delta4, NULL g_conf (K={K}, items={items})")
    got_amax = float(amax[:1].view(torch.float32).item())
    assert got_amax == float(d4.abs().max()) and abs(got_amax - float(r_amax)) <= float(b_d4.max())
    n = -(-items // T.P_HEAD) * K + 4 + -(-splits // 4) + 2
    b_dWa = e_dza @ h4.abs() + 2 * n * U * (dza.abs() @ h4.abs())
    b_dba = (e_dza.sum() + 2 * n * U * dza.abs().sum()).reshape(1)
    T._capped(b_dWa, r_dWa, "dWa")
    T._capped(b_dba, r_dba, "dba")
    T._ratio(dWa.reshape(-1), r_dWa, b_dWa.clamp(min=1e-300), "row_head dWa, NULL g_conf")
    T._ratio(dba, r_dba, b_dba.clamp(min=1e-300), "row_head dba, NULL g_conf")


# ---- 7. k_agg_bwd with frozen tensors over several tiles per workgroup ------------------------------
# sgn_aggregate_backward called directly on a hand-built scene of tests/agg_f16_ref.py with the helpers and the
# per-element float64 bounds of tests/test_agg_f16_gpu.py.  The launch is min(ceil(n / 16), 2048) workgroups
# of 16 items a tile: at 65539 items every workgroup runs a second tile -- with the embedding frozen the
# tile's last product prefetches the next tile's product 0 into the other LDS slot (`more`), the slot parity
# flips, the next tile's d f_s DMA follows the epilogue's LDS reads -- and three workgroups run a third, where
# the parity is back at 0.

TILE_SCENE = "rand2_65539"
TILE_CASES = [((0, 0), ("embedding",)), ((1, 96), ("embedding",)), ((0, 0), ("embedding", "color", "dir", "conf")),
              ((0, 0), ("color", "dir", "conf")), ((1, 96), ("dir",))]


def _tile_scene():
    """65539 items of 2 neighbours, shuffled, as agg_f16_ref's rand2_32771 is built; kept in that module's scene
    cache, which test_agg_f16_gpu's helpers look scenes up in."""
    import agg_f16_ref as fr
    import agg_rows_ref as ar
    if TILE_SCENE not in fr._CACHE:
        fr._CACHE[TILE_SCENE] = ar.Scene(2, ar.rand(2, 65539), shuffle=True, bpnet=True)
    return fr._CACHE[TILE_SCENE]


@pytest.mark.parametrize("variant,null", TILE_CASES, ids=str)
def test_agg_backward_with_null_members_over_three_tiles(variant, null):
    """k_agg_bwd<SG, false, true> (embedding NULL) and <SG, true, true> (embedding trained, others NULL), base
    and SG: h4, dza, d4, d3, d2 (db), d1 of all 65539 items and the trained tensors' gradients within
    test_agg_f16_gpu's per-element bounds; masked slots' deltas +-0; guard rows and the NULL members' tensors
    (never passed) keep their bits."""
    import agg_f16_ref as fr
    import test_agg_f16_gpu as T
    sc = _tile_scene()
    assert sc.items == 65539 and sc.items > 2 * 2048 * 16
    name, scale = TILE_SCENE, 4096.0
    fw = T.run_forward(name, variant)
    n = fw["n"]
    dv = T.dev(name)
    _, blob, tblob, net = T.weights(variant)
    R = 8 * n
    dfs, dalpha, g0 = fr.upstream(n)
    pad = lambda x: torch.cat([x, torch.full((T.GUARD,) + x.shape[1:], T.NAN)]).to(T.DEV)  # noqa: E731
    t = {k: T.nan16(R + T.GUARD, 256) for k in ("d4", "d3", "d2", "d1", "h4", "db")}
    t["dza"] = torch.full((R + T.GUARD,), T.NAN, device=T.DEV)
    t["dfs"], t["dalpha"] = pad(dfs), pad(dalpha)
    g = {k: v.clone().to(T.DEV) for k, v in g0.items()}
    sc_t = torch.tensor([scale], device=T.DEV)
    saved = _lib.AggSaved(*(fw[k].data_ptr() for k in ("x0", "h1", "h2", "h3")))
    deltas = _lib.AggDeltas(*(t[k].data_ptr() for k in ("d4", "d3", "d2", "d1", "h4", "dza")))
    grads = _lib.PointGrads(*(None if k in null else g[k].data_ptr() for k in ("embedding", "color", "dir", "conf")))
    sgv = variant[0] == 1
    rc = T.L().sgn_aggregate_backward(variant[0], variant[1], ctypes.byref(dv.pt), ctypes.byref(dv.qo), n, sc.K, _lib.ptr(blob),
                                      _lib.ptr(tblob), ctypes.byref(saved), _lib.ptr(fw["h2b"]) if sgv else None,
                                      _lib.ptr(t["dfs"]), _lib.ptr(t["dalpha"]), _lib.ptr(sc_t), ctypes.byref(deltas),
                                      _lib.ptr(t["db"]) if sgv else None, ctypes.byref(grads), _lib.stream_handle())
    _lib.check(rc, "sgn_aggregate_backward")
    torch.cuda.synchronize()
    what = f"backward {name} {variant} NULL {null}"
    names = ["d4", "d3", "d2", "d1", "h4"] + (["db"] if sgv else [])
    for k in names + ["dza"]:
        assert T._all_nan(t[k][R:]), f"{what}: {k} wrote a guard row"
    if not sgv:
        assert T._all_nan(t["db"])
    rows = T.rows_of(name, variant, n)
    rep = fr.Report()
    acc = fr.GradAcc(sc.N, T.DEV)
    for i0 in range(0, n, T.CHUNK):
        i1 = min(n, i0 + T.CHUNK)
        c = {k: t[k][8 * i0:8 * i1] for k in names + ["dza"]}
        c.update({k: fw[k][8 * i0:8 * i1] for k in ("h1", "h2", "h3", "h2b")})
        c.update(dfs=t["dfs"][i0:i1], dalpha=t["dalpha"][i0:i1], scale=scale)
        rcs = rows.chunk(i0, i1, T.DEV)
        fr.check_backward(rep, rcs, net, c, acc)
        assert fr.masked_rows_zero(rcs, c, sgv), f"{what}: a masked slot's delta is not +-0"
    # the trained tensors' gradients: check_point_grads' bound and cap, over the non-NULL members
    for k in ("embedding", "color", "dir", "conf"):
        if k in null:
            assert T._same_bits(g[k].cpu(), g0[k]), f"{what}: g_{k} is frozen"
            continue
        s, b, a, carried = acc.t[k]
        f = 1.0 if k == "conf" else 1.0 / scale
        base = g0[k].double().reshape(s.shape).to(s.device)
        ref = base + s * f
        bound = b * f + (acc.cnt[:, None] + 2) * fr.U * (base.abs() + a * f)
        got = g[k].double().reshape(s.shape).to(s.device)
        fr._flag(rep, "g cap", bool(((bound - carried * f) > 0.25 * (base.abs() + a * f) / (acc.cnt[:, None] + 1)).any()))
        fr._absbound(rep, "g_" + k, got, ref, bound, torch.zeros_like(bound))
        none = acc.cnt == 0
        fr._flag(rep, "g untouched", not torch.equal(got[none], base[none]))
    rep.show(what)
    rep.assert_ok(what)
    del fw, t, g
    torch.cuda.empty_cache()
