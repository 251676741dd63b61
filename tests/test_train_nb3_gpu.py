"""Training the viewmlp without block3 (shading_feature_mlp_layer3 = 0, opts.train_rows = 1) on the GPU:
HipTrainer(precision="f32") -> train_f32.F32RunnerNb3 / F32StepNb3 on the golden cloud (nb3_ref.golden_points,
room_corner(20000, 1)) through the goldens' 14 x 14 view at SR 24 -- 196 rays (every one of them hits: measured;
the batch without hits is a test of its own), samples with 0, 1 and K neighbours.

Forward bar: the render path's, max(1e-5, 4 x floor) x max(1, |ref|) with nb3_ref.floor.  Gradient bar per tensor:
GRAD_TOL_F32 = 1e-4 relative L2 (tests/test_train_gpu.py); for the points_* tensors it may lift to twice the fp32
floor of the batch (the same autograd in torch fp32 on the CPU against the reference), never above
GRAD_TOL_F32_ORACLE_Q = 5e-3.  Reference: train.Trainer in fp32 on the GPU for the base network, float64 autograd of
nb3_ref.chain + train.composite_losses for the block2_bpnet variants (train_nb3_ref.chain_loss), both on the very
samples the step's query produced (HipTrainer.last_query).

The weights are init_mlp(seed, bias_std=0.05, block3_layers=0).  Measured on the CPU before any GPU run (fp32
against float64 autograd of the restatement on the golden query), seed 3's MLP-tensor floors are <= 6.6e-7 and seed
5's <= 2.0e-5 for the three variants, both below 5e-5, so 1e-4 is the effective MLP bar with either; seed 3's point
floors are <= 1.8e-6 (seed 5: points_embeding 3.8e-4 .. 6.3e-4).  base and bp352 use seed 3.  bp256 uses seed 5:
seed 3's bp256 network puts color_branch.0's pre-activation of one item of this batch at -1.2e-7 (float64), inside
the fp32 error of the forward (HIP against float64: 1.7e-6 at most on that layer, within the forward bar).  The HIP
step has it at the other side of 0 -- the only sign that differs from float64's among the LeakyReLU inputs the probe
could compare: z1, z2 and the colour MLP's three; zb, the layer bp256 adds, was NOT compared (after a step its buffer
holds the head's delta; its smallest float64 input is 1.7e-7, and d f_s, which comes before zb in the backward, already
carries the error in one item) -- and LeakyReLU's derivative there is 1 instead of 0.01: that one element moved d points_embeding by 1.0e-3 (one point
carries all of it) and the layers behind it by 2e-5 .. 3e-5, while torch's fp32 on the CPU fell on float64's side, so
the floor did not show it.  Every case prints the smallest |LeakyReLU input| of its float64 reference
(train_nb3_ref.min_preactivation).  profiles/train_nb3_tests.txt holds the measured errors."""
import argparse
import functools

import pytest
import torch

import sgnerf_amd  # noqa: F401
from sgnerf_amd.model import HipPointsVolumetricModel
from sgnerf_amd.opts import HotPathOpts
from sgnerf_amd.train import DepthTarget, PointParams, Trainer
from sgnerf_amd.train_hip import HipTrainer, grads_named
from sgnerf_amd.weights import init_mlp

import nb3_ref as nb
import train_nb3_ref as tn

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32_TOL = 1e-5
GRAD_TOL_F32 = 1e-4
GRAD_TOL_F32_ORACLE_Q = 5e-3
LOSS_CURVE_TOL = 0.05
SEED = {"base": 3, "bp256": 5, "bp352": 3}
VARIANT = {"base": (0, 0), "bp256": (1, 0), "bp352": (1, 96)}
POINTS = ("points_embeding", "points_color", "points_dir", "points_conf")
SETTINGS = {"stock": {}, "depth": dict(depth_loss_items=("coarse_depth",), depth_loss_weights=(0.7,)),
            "loss": dict(color_loss_weights=(0.5, 0.2, 0.3), sparse_loss_weight=0.1)}


# ---- the batch -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def batch():
    pts = {k: torch.from_numpy(v) for k, v in nb.golden_points().items()}
    pts["conf"] = pts["conf"].reshape(-1, 1)
    c = nb.load_case("base")[2]
    R = c["raydir"].shape[0]
    assert R == 196 and int(c["SR"]) == 24
    g = torch.Generator().manual_seed(1)
    view = dict(campos=torch.from_numpy(c["campos"]).reshape(3), rot=torch.from_numpy(c["camrotc2w"]).reshape(3, 3),
                raydir=torch.from_numpy(c["raydir"]).reshape(R, 3), near=float(c["near_far"][0]),
                far=float(c["near_far"][1]), gt=torch.rand(R, 3, generator=g),
                gt_depth=1.0 + 2.0 * torch.rand(R, generator=g))
    return pts, view


@functools.lru_cache(maxsize=None)
def device_view():
    """The view's tensors on the GPU (a step given device tensors copies nothing from the host)."""
    pts, v = batch()
    out = {k: t.to(DEV) if torch.is_tensor(t) else t for k, t in v.items()}
    out["labels"] = (torch.zeros(pts["xyz"].shape[0], dtype=torch.int32, device=DEV),
                     torch.zeros(196, dtype=torch.int32, device=DEV), 5)
    return out


def opts_for(name, K=8, **kw):
    nl, dim = VARIANT[name]
    return HotPathOpts(SR=24, K=K, shading_feature_mlp_layer3=0, shading_feature_mlp_layer2_bpnet=nl,
                       predict_semantic=1 if dim else 0, semantic_guidance=1 if dim else 0, is_train=1, train_rows=1,
                       **kw).check_supported()


def state_for(name):
    nl, dim = VARIANT[name]
    return init_mlp(SEED[name], bias_std=0.05, bpnet_layers=nl, bpnet_dim=dim, block3_layers=0)


def points_on(dev, colour=True):
    p = batch()[0]
    return PointParams(p["xyz"], p["embedding"], p["color"] if colour else None, p["dir"] if colour else None,
                       p["conf"], dev)


def trainer(name, K=8, colour=True, state=None, **kw):
    pts = batch()[0]
    train_kw = {k: kw.pop(k) for k in ("lr", "plr") if k in kw}
    P = points_on(DEV, colour)
    tr = HipTrainer(P, state or state_for(name), opts_for(name, K, **kw), DEV, precision="f32",
                    bpnet=pts["bpnet"] if VARIANT[name][1] else None, **train_kw)
    return tr, P


def call(tr, name, fn="backward", depth=None, campos=None, seed=7):
    v = device_view()
    labels = v["labels"] if VARIANT[name][1] else None   # labels all 0 pass the semantic filter: the plain query
    torch.manual_seed(seed)   # the query's depth jitter
    return getattr(tr, fn)(v["campos"] if campos is None else campos, v["rot"], v["raydir"], v["near"], v["far"], v["gt"],
                           labels=labels, depth=depth)


def _depth(setting, dev):
    if setting != "depth":
        return None
    return DepthTarget(batch()[1]["gt_depth"].to(dev), None, 0.7)


# ---- one step and its references, computed once per (network, K, setting) and left unchanged -----------------
@functools.lru_cache(maxsize=None)
def case(name, K=8, setting="stock"):
    pts, v = batch()
    st = state_for(name)
    tr, P = trainer(name, K, **SETTINGS[setting])
    parts, full, mask, *_ = call(tr, name, depth=_depth(setting, DEV))
    torch.cuda.synchronize()
    step = tr.stepper.step
    q = {k: t.cpu() for k, t in tr.last_query.items()}
    sc = tn.Scene(pts, (v["campos"], v["rot"]), v["raydir"], q)
    assert sc.pid.numel() > 0 and sc.K == K
    seed, cond = SEED[name], tn.min_preactivation(sc, st)
    print(f"train_rows {name} K={K} [{setting}] seed {seed}: smallest |LeakyReLU input| of the float64 reference {cond:.2e}")
    nnb = sc.nnb
    out = dict(sc=sc, seed=seed, cond=cond, parts={k: float(x) for k, x in parts.items()}, full=full.cpu(), mask=mask.cpu(),
               alpha=step.feat[:sc.S, 0].cpu()[sc.work], rgb=step.feat[:sc.S, 1:].cpu()[sc.work],
               fs=step.fs[:sc.items].cpu(), g={k: None if t is None else t.cpu() for k, t in grads_named(tr).items()},
               counts=(int((nnb == 0).sum()), int((nnb == 1).sum()), int((nnb == K).sum()), int((~mask).sum())),
               amax=[float(x) for x in step.amax.view(torch.float32).cpu()])
    o = tr.opts
    depth_c = _depth(setting, "cpu")
    # the float64 restatement: the forward reference of every network, the gradient reference of block2_bpnet's
    p64, full64, mask64, g64 = tn.chain_loss(sc, st, o, v["gt"], depth=depth_c)
    with torch.no_grad():
        out["chain"] = {k: t for k, t in nb.chain(sc, st).items() if k in ("alpha", "rgb", "fs")}
    out["fwd_floor"] = nb.floor(sc, st, DEV)
    out["full64"], out["mask64"] = full64, mask64
    if name == "base":   # train.Trainer in fp32 on the GPU; the floor: the same on the CPU
        qd = {k: t.to(DEV).long() if t.dtype in (torch.int32, torch.int64) else t.to(DEV) for k, t in q.items()}
        refs = {}
        for dev in (DEV, torch.device("cpu")):
            Pr = points_on(dev)
            ref = Trainer(Pr, st, o, dev)
            pr, fr, mr, *_ = ref.backward(v["campos"].to(dev), v["rot"].to(dev), v["raydir"].to(dev), v["near"], v["far"],
                                          v["gt"].to(dev), q={k: t.to(dev) for k, t in qd.items()},
                                          depth=_depth(setting, dev))
            g = {}
            for ln, *_ in ref.mlp.layers:
                g[ln + ".weight"], g[ln + ".bias"] = ref.mlp.w(ln).grad.cpu(), ref.mlp.b(ln).grad.cpu()
            for k in POINTS:
                t = getattr(Pr, k).grad
                g[k] = None if t is None else t.cpu()
            refs[dev.type] = (pr, fr.cpu(), mr.cpu(), g)
        torch.cuda.synchronize()
        pr, fr, mr, g_ref = refs["cuda"]
        assert g_ref["points_color"] is None and g_ref["points_dir"] is None
        g_ref = {k: t for k, t in g_ref.items() if t is not None}
        g_floor = refs["cpu"][3]
        out.update(ref_parts={k: float(x) for k, x in pr.items()}, ref_full=fr, ref_mask=mr, what="train.Trainer fp32 (GPU)")
        # the restatement and the torch reference are one function: float64 chain against the fp32 Trainer
        out["trainer_vs_chain"] = max(tn.rel_l2(g_ref[k], g64[k]) for k in g64)
    else:
        g_ref = g64
        _, _, _, g_floor = tn.chain_loss(sc, st, o, v["gt"], dtype=torch.float32, depth=depth_c)
        out.update(ref_parts={k: float(x) for k, x in p64.items()}, ref_full=full64, ref_mask=mask64,
                   what="float64 autograd of nb3_ref.chain + composite_losses")
    out["g_ref"] = g_ref
    out["floor"] = {k: tn.rel_l2(g_floor[k], g_ref[k]) for k in g_ref}
    return out


CASES = [("base", 8), ("base", 4), ("base", 1), ("bp256", 8), ("bp352", 8)]


@pytest.mark.parametrize("name,K", CASES)
def test_forward_matches_the_restatement(name, K):
    c = case(name, K)
    n0, n1, nk, miss = c["counts"]
    assert n0 > 0 and n1 > 0 and nk > 0, c["counts"]
    fl = c["fwd_floor"]
    bar = {k: max(F32_TOL, 4.0 * x) for k, x in fl.items()}
    err = dict(alpha=nb.rel(c["alpha"], c["chain"]["alpha"]), rgb=nb.rel(c["rgb"], c["chain"]["rgb"]),
               fs=nb.rel(c["fs"], c["chain"]["fs"]), full=nb.rel(c["full"], c["full64"]))
    print(f"train_rows forward {name} K={K}: samples with 0 / 1 / K neighbours {n0} / {n1} / {nk}, rays without hits "
          f"{miss}; fp32 floor " + ", ".join(f"{k} {x:.2e}" for k, x in fl.items()) + "; max error / max(1, |ref|) " +
          ", ".join(f"{k} {x:.2e}" for k, x in err.items()) + f"; amax words {c['amax'][3:10]}")
    assert torch.equal(c["mask"], c["mask64"])
    assert err["alpha"] <= bar["alpha"] and err["fs"] <= bar["fs"] and err["rgb"] <= bar["rgb"]
    assert err["full"] <= bar["rgb"]


def _check_gradients(c, what):
    g, ref, fl = c["g"], c["g_ref"], c["floor"]
    assert set(ref) == {k for k, t in g.items() if t is not None}, (sorted(ref), sorted(g))
    assert g["points_color"] is None and g["points_dir"] is None
    err = {k: tn.rel_l2(g[k].reshape(b.shape), b) for k, b in ref.items()}
    bar = {k: max(GRAD_TOL_F32, min(2.0 * fl[k], GRAD_TOL_F32_ORACLE_Q)) if k.startswith("points_") else GRAD_TOL_F32
           for k in ref}
    tot = abs(c["parts"]["total"] - c["ref_parts"]["total"]) / abs(c["ref_parts"]["total"])
    col = tn.rel_l2(c["full"], c["ref_full"])
    print(f"train_rows gradients {what} seed {c['seed']} against {c['what']}: loss total {c['parts']['total']:.8e} (relative error "
          f"{tot:.2e}), colour relative L2 {col:.2e}")
    print("    relative L2 errors " + ", ".join(f"{k} {x:.2e}" for k, x in err.items()))
    print("    fp32 floors        " + ", ".join(f"{k} {x:.2e}" for k, x in fl.items()))
    if "trainer_vs_chain" in c:
        print(f"    train.Trainer fp32 against the float64 restatement, worst tensor: {c['trainer_vs_chain']:.2e}")
    assert all(float(b.abs().max()) > 0 for b in ref.values())
    assert torch.equal(c["mask"], c["ref_mask"])
    assert tot <= 1e-4 and col <= 1e-4
    bad = {k: (x, bar[k]) for k, x in err.items() if x > bar[k]}
    assert not bad, bad


@pytest.mark.parametrize("name,K", CASES)
def test_gradients_match_the_reference(name, K):
    _check_gradients(case(name, K), f"{name} K={K}")


@pytest.mark.parametrize("name,setting", [("base", "depth"), ("bp352", "depth"), ("base", "loss"), ("bp352", "loss")])
def test_depth_and_loss_options_reach_the_step(name, setting):
    """ColourStage comes with the depth target and the loss options: same bars, the term is in the total."""
    c = case(name, 8, setting)
    key = "coarse_depth" if setting == "depth" else "sparse"
    assert c["parts"][key] > 0 and abs(c["parts"][key] - c["ref_parts"][key]) <= 1e-4 * abs(c["ref_parts"][key])
    assert c["parts"]["total"] != case(name, 8)["parts"]["total"]
    _check_gradients(c, f"{name} K=8 [{setting}]")


# ---- switches ------------------------------------------------------------------------------------------------
def _three_steps(tr, name):
    for it in range(3):
        call(tr, name, "step", seed=100 + it)
    tr.sync_points()
    tr.check_touched()
    torch.cuda.synchronize()


@pytest.mark.parametrize("frozen", ["feat", "conf"])
def test_grad_switches(frozen):
    tr, P = trainer("base", **{frozen + "_grad": 0})
    p0 = {k: getattr(P, k).detach().clone() for k in POINTS}
    _three_steps(tr, "base")
    step = tr.stepper.step
    names = [n for n, _ in step.g_row_bwd]
    if frozen == "feat":   # neither block1.0's input-gradient GEMM nor its buffer
        assert step.dx0 is None and "dx0" not in names and names == ["d1"]
        assert tr.trained == ("points_conf",)
    else:
        assert step.dx0 is not None and names == ["d1", "dx0"] and tr.trained == ("points_embeding",)
    same = {k: torch.equal(getattr(P, k).detach(), p0[k]) for k in POINTS}
    assert same == {"points_embeding": frozen == "feat", "points_color": True, "points_dir": True,
                    "points_conf": frozen == "conf"}
    assert len(tr.opt_pts.param_groups[0]["params"]) == 1


@pytest.mark.parametrize("name,colour", [("base", True), ("base", False), ("bp352", False)])
def test_points_with_and_without_colour_and_dir(name, colour):
    """Without colour and dir the step trains (NULL tables); with them they keep their bits, have no gradient, no
    Adam moments and the point group holds embedding and conf only, whatever color_grad / dir_grad say."""
    tr, P = trainer(name, colour=colour, color_grad=1, dir_grad=1)
    e0, c0 = P.points_embeding.detach().clone(), P.points_conf.detach().clone()
    keep = None if not colour else (P.points_color.detach().clone(), P.points_dir.detach().clone())
    _three_steps(tr, name)
    assert tr.trained == ("points_embeding", "points_conf")
    assert tr.opt_pts.param_groups[0]["point_tensors"] == ["points_embeding", "points_conf"]
    assert not torch.equal(P.points_embeding.detach(), e0) and not torch.equal(P.points_conf.detach(), c0)
    assert bool(torch.isfinite(P.points_embeding).all()) and bool(torch.isfinite(tr.mlp.flat).all())
    if colour:
        assert torch.equal(P.points_color.detach(), keep[0]) and torch.equal(P.points_dir.detach(), keep[1])
        assert P.points_color.grad is None and P.points_dir.grad is None and not P.points_color.requires_grad
        assert P.points_color not in tr.opt_pts.state and P.points_dir not in tr.opt_pts.state
    else:
        assert P.points_color is None and P.points_dir is None
    pg = tr.point_grads()
    assert not pg.color and not pg.dir and pg.embedding and pg.conf


# ---- determinism, synchronisation, empty batch, range ------------------------------------------------------------
@pytest.mark.parametrize("name", ["base", "bp352"])
def test_flat_gradient_is_deterministic(name):
    """Fixed-order partials: two trainers on the same batch give bitwise equal flat MLP gradients."""
    grads = []
    for _ in range(2):
        tr, _ = trainer(name)
        call(tr, name)
        torch.cuda.synchronize()
        grads.append(tr.mlp.flat.grad.clone())
    assert torch.equal(grads[0], grads[1]) and float(grads[0].abs().max()) > 0


def test_second_backward_issues_no_synchronisation():
    tr, _ = trainer("base")
    call(tr, "base", "step")
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        call(tr, "base")
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    tr.check_touched()


def test_step_without_hits():
    """All rays point away: background colour, zero masked loss, every gradient exactly zero, finite parameters."""
    tr, P = trainer("base")
    campos = device_view()["campos"] + 100.0
    for _ in range(2):
        parts, full, mask = call(tr, "base", campos=campos)
        torch.cuda.synchronize()
        assert not bool(mask.any()) and torch.equal(full.cpu(), torch.ones(196, 3))
        assert float(parts["ray_masked_coarse_raycolor"]) == 0.0
        for k, g in grads_named(tr).items():
            assert g is None or float(g.abs().max()) == 0.0, k
        tr.apply()
        tr.check_touched()
        assert bool(torch.isfinite(P.points_embeding).all()) and bool(torch.isfinite(P.points_conf).all())


def test_range_watch_raises_at_the_next_step():
    """block1.2 scaled by 4e5 (the render test's scale): its pre-activation leaves fp16 range, the step after
    raises an ordinary RuntimeError naming the range, and so does check_touched()."""
    st = state_for("base")
    st["block1.2.weight"] = st["block1.2.weight"] * 4.0e5
    st["block1.2.bias"] = st["block1.2.bias"] * 4.0e5
    tr, _ = trainer("base", state=st)
    call(tr, "base")
    torch.cuda.synchronize()
    z2 = float(tr.stepper.step.amax.view(torch.float32)[tr.stepper.step.A_Z2])
    print(f"train_rows range watch: max |z2| = {z2:.3e}")
    assert z2 >= 65504.0
    with pytest.raises(RuntimeError, match="fp16 range"):
        call(tr, "base")
    call(tr, "base")   # the watch is re-armed by every step
    with pytest.raises(RuntimeError, match="fp16 range"):
        tr.check_touched()
    good, _ = trainer("base")
    call(good, "base")
    good.check_touched()
    call(good, "base")


# ---- data parallel ---------------------------------------------------------------------------------------------
def test_data_parallel_step_matches_single_rank(monkeypatch):
    """test_train_gpu.test_data_parallel_step_matches_single_rank's pattern: two ranks holding the same batch give
    the one-rank update within the one-rank run-to-run spread measured here."""
    from test_train_gpu import _fake_two_ranks
    names = ("points_embeding", "points_conf")
    runs = {}
    for mode in ("one", "one_again", "dp"):
        if mode == "dp":
            _fake_two_ranks(monkeypatch)
        tr, P = trainer("base")
        p0 = {k: getattr(P, k).detach().clone() for k in names}
        p0["mlp"] = tr.mlp.flat.detach().clone()
        losses = []
        for it in range(3):
            parts, _, _ = call(tr, "base", "step", seed=100 + it)
            losses.append(float(parts["total"]))
        tr.sync_points()
        upd = {k: getattr(P, k).detach() - p0[k] for k in names}
        upd["mlp"] = tr.mlp.flat.detach() - p0["mlp"]
        runs[mode] = (losses, upd)
        monkeypatch.undo()
    rel = lambda x, y: {k: tn.rel_l2(x[k], y[k]) for k in y}  # noqa: E731
    spread, err = rel(runs["one_again"][1], runs["one"][1]), rel(runs["dp"][1], runs["one"][1])
    print("train_rows data parallel: one-rank spread", {k: f"{x:.1e}" for k, x in spread.items()},
          "dp vs one-rank", {k: f"{x:.1e}" for k, x in err.items()})
    assert abs(runs["dp"][0][0] - runs["one"][0][0]) <= 1e-5 * abs(runs["one"][0][0])
    for a, b in zip(runs["dp"][0], runs["one"][0]):
        assert abs(a - b) <= 1e-3 * abs(b)
    for k in err:
        assert float(torch.linalg.vector_norm(runs["dp"][1][k])) > 0
        assert err[k] <= max(1e-2, 3 * spread[k]), (k, err, spread)


# ---- loss curve --------------------------------------------------------------------------------------------------
def test_20_step_loss_curve_tracks_fp32_torch():
    pts, v = batch()
    tr, _ = trainer("base")
    ref = Trainer(points_on(DEV), state_for("base"), opts_for("base"), DEV)
    hip, tor = [], []
    for it in range(20):
        parts, _, _ = call(tr, "base", "step", seed=200 + it)
        hip.append(float(parts["ray_masked_coarse_raycolor"]))
        torch.manual_seed(200 + it)
        pr, _, _ = ref.step(v["campos"].to(DEV), v["rot"].to(DEV), v["raydir"].to(DEV), v["near"], v["far"], v["gt"].to(DEV))
        tor.append(float(pr["ray_masked_coarse_raycolor"]))
    a, b = sum(hip[10:]) / 10, sum(tor[10:]) / 10
    print(f"train_rows loss curve: colour loss first / last HIP {hip[0]:.6e} / {hip[-1]:.6e}, torch {tor[0]:.6e} / "
          f"{tor[-1]:.6e}; means of the last 10: {a:.6e} / {b:.6e} (relative difference {abs(a - b) / b:.2e})")
    assert abs(a - b) <= LOSS_CURVE_TOL * b
    assert hip[-1] < hip[0] and tor[-1] < tor[0]


# ---- the plugin ----------------------------------------------------------------------------------------------------
def test_plugin_trains_saves_and_reloads(tmp_path):
    pts, v = batch()
    st = state_for("base")
    ns = dict(SR=24, K=8, gpu_ids=[0], is_train=True, checkpoints_dir=str(tmp_path), name="scene", lr=5e-4, plr=2e-3,
              lr_decay_exp=0.1, lr_decay_iters=1_000_000, bg_color="white", shading_feature_mlp_layer3=0)
    inputs = {"campos": v["campos"][None].to(DEV), "raydir": v["raydir"][None].to(DEV), "camrotc2w": v["rot"][None].to(DEV),
              "near": torch.tensor([[[v["near"]]]]), "far": torch.tensor([[[v["far"]]]]), "gt_image": v["gt"][None].to(DEV)}
    kw = dict(points_xyz=pts["xyz"], points_embedding=pts["embedding"][None], points_color=pts["color"][None],
              points_dir=pts["dir"][None], points_conf=pts["conf"][None], aggregator_state=st)
    # without the option: refused as before
    m0 = HipPointsVolumetricModel()
    m0.initialize(argparse.Namespace(**ns))
    with pytest.raises(NotImplementedError, match="shading_feature_mlp_layer3") as e:
        m0.set_points(**kw)   # training mode: set_points sets the optimizers up
    assert "train_rows" not in str(e.value)
    for callee in (lambda: m0.setup_optimizer(m0.opt), lambda: m0.optimize_parameters()):
        with pytest.raises(NotImplementedError, match="shading_feature_mlp_layer3"):
            callee()
    # with it (and test frames on the row GEMMs): set up by set_points in training mode, two steps, a checkpoint
    opt = argparse.Namespace(**ns, train_rows=1, rows_gemm=1)
    m = HipPointsVolumetricModel()
    m.initialize(opt)
    assert m.opts.train_rows == 1 and m.opts.rows_gemm == 1 and m.opts.is_train == 0
    m.set_points(**kw)
    m.setup(opt)
    m.init_scheduler(0, opt)
    assert m.trainer.opts.is_train == 1 and m.trainer.opts.rows_gemm == 0 and m.trainer.precision == "f32"
    m.set_input(inputs)
    before = m.test()["coarse_raycolor"].clone()
    for step in range(2):
        parts = m.optimize_parameters(total_steps=step)
    assert bool(torch.isfinite(parts["total"])) and "total" in m.get_current_losses()
    after = m.test()["coarse_raycolor"].clone()
    assert m.net_ray_marching.renderer._rows_frame and not torch.equal(after, before)
    m.save_networks("latest")
    sd = torch.load(tmp_path / "scene" / "latest_net_ray_marching.pth", map_location="cpu", weights_only=True)
    assert not any("block3." in k for k in sd) and "aggregator.block1.2.weight" in sd
    assert torch.equal(sd["neural_points.points_color"].reshape(-1, 3), pts["color"])
    assert torch.equal(sd["neural_points.points_dir"].reshape(-1, 3), pts["dir"])
    assert not torch.equal(sd["neural_points.points_embeding"].reshape(-1, 32), pts["embedding"])
    m2 = HipPointsVolumetricModel()
    m2.initialize(argparse.Namespace(**{**vars(opt), "is_train": False, "resume_dir": str(tmp_path / "scene")}))
    m2.load_networks("latest")
    m2.set_input(inputs)
    assert torch.equal(m2.test()["coarse_raycolor"], after)
    # prune, with the optimizers rebuilt, then one more step
    thresh = float(torch.quantile(m.neural_points.points_conf.reshape(-1), 0.25))
    m.clean_optimizer_scheduler()
    assert m.prune_points(thresh) > 0
    m.setup_optimizer(opt)
    m.optimize_parameters(total_steps=2)
    assert bool(torch.isfinite(m.get_current_losses()["total"]))
    # --sgn_train_rows 1 is the same switch
    m3 = HipPointsVolumetricModel()
    m3.initialize(argparse.Namespace(**ns, sgn_train_rows=1))
    assert m3.opts.train_rows == 1
