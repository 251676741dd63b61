"""The driver's loss options on the GPU: sgn_loss_train_opts (csrc/loss.hip: the colour weights in k_loss_reduce's
scale, k_loss_nbw and the SPARSE instantiations of k_loss_fwd / k_loss_reduce / k_loss_bwd) called through the C ABI
on small scenes of tests/ray_stage_ref.py and compared with tests/loss_opts_ref.py's float64 restatement (pinned to
train.composite_losses in test_loss_opts_ref_cpu.py); its stock path against sgn_loss_train / sgn_loss_train_depth
bit for bit; and the options on their way through the trainers and the plugin.

Shapes: R = 70 rays (three 32-ray blocks at 8 lanes per ray, the last one partial), SR = 6, K = 3 and 8, 50 points
(several entries share a d conf row).  The scene plants a ray without a sample, a ray whose samples have no
neighbour, a ray filling all SR slots, empty neighbour slots, and conf values below 1e-4, above 1, at and one fp32
step beside both clamps and both zero_epsilon = 1e-3 edges, and 0.03 / 0.97 (inside zero_epsilon = 0.05 of the ends).

Bars: those of tests/test_loss_gpu.py for the stock stage -- loss parts 1e-5 relative, gradients w.r.t. the features
and conf 1e-4 relative L2 -- and, per element, 1e-4 of the reference tensor's largest magnitude (test_ray_stage_gpu's
GRAD_TOL_F32 cap).  The step tests hold the gradients to tests/test_train_gpu.py's bars (GRAD_TOL_F32 at precision
"f32", GRAD_TOL_MLP / GRAD_TOL_POINTS at "f16") against train.Trainer's fp32 autograd under the same options, on the
very samples the HIP query produced.

Measured on an MI355X (profiles/loss_opts_tests.txt): over all direct calls the worst relative L2 error is 1.4e-7 in
d feat and 2.2e-7 in d conf (bar 1e-4), the worst loss part 2.4e-7 (bar 1e-5); the step's gradients are within 1.2e-6
of the reference at "f32" (bar 1e-4), 7.9e-3 (MLP, bar 2e-2) and 3.6e-2 (points, bar 6e-2) at "f16", and 0.25 away
from the default-options step's."""
import argparse
import ctypes
import dataclasses
import functools
import itertools

import numpy as np
import pytest
import torch

import sgnerf_amd  # noqa: F401
from sgnerf_amd import _lib
from sgnerf_amd.opts import COLOR_LOSS_ITEMS
from sgnerf_amd.train import PointParams, Trainer, neighbour_weights
from sgnerf_amd.train_hip import HipTrainer, grads_named
from sgnerf_amd.weights import LAYERS

import depth_ref as dr
import loss_opts_ref as lr
import ray_stage_ref as rs
import test_ray_stage_gpu as rsg
from test_ray_stage_gpu import BG, DEV, GUARD, NAN, Dev, _all_nan, _same_bits
from test_train_cpu import O, _setup
from test_train_gpu import GRAD_TOL_F32, GRAD_TOL_MLP, GRAD_TOL_POINTS

pytestmark = pytest.mark.gpu
PART_TOL = 1e-5      # tests/test_loss_gpu.py: loss parts, relative
GRAD_TOL = 1e-4      # tests/test_loss_gpu.py: gradients, relative L2; per element: of the tensor's largest magnitude
R_, SR_ = 70, 6
W_D = 0.5
MASKED, MISS, ALL = COLOR_LOSS_ITEMS
PARTS = {"ray_masked_coarse_raycolor": 0, "conf_coefficient": 1, "ray_miss_coarse_raycolor": 2, "coarse_raycolor": 3,
         "coarse_depth": 7, "sparse": 8}
WORST = {"dfeat": 0.0, "dconf": 0.0, "part": 0.0}


def _rel(a, b):
    return float(torch.linalg.vector_norm(a.double() - b.double()) / max(torch.linalg.vector_norm(b.double()), 1e-30))


@functools.lru_cache(maxsize=None)
def scene(K, which="mixed"):
    """mixed: the planted scene; none / all: its rays without / with a valid sample alone."""
    sc = lr.small_scene(R_, SR_, K, seed=7, camera=K % 2)
    if which == "mixed":
        for name in ("full", "ns0", "no_nb"):
            assert name in sc["plant"]
        assert bool((sc["pidx"][:sc["S"]][sc["samp_nnb"][:sc["S"]] > 0] < 0).any()) or K == 1   # empty neighbour slots
        return sc
    valid = torch.zeros(R_, dtype=torch.bool)
    valid[sc["samp_ray"][:sc["S"]].long()[sc["samp_nnb"][:sc["S"]] > 0]] = True
    return _sub_scene(sc, valid if which == "all" else ~valid)


def _sub_scene(sc, keep):
    """The scene of the rays keep [R] alone, their samples compacted (five slack samples after them, as ray_scene)."""
    S = sc["S"]
    sr = sc["samp_ray"][:S].long()
    ks = keep[sr]
    ns = sc["ray_ns"][keep]
    Rk, Sk = int(keep.sum()), int(ks.sum())
    out = dict(sc, R=Rk, S=Sk, S_cap=Sk + 5, plant={}, ray_ns=ns.contiguous(),
               ray_soff=(torch.cumsum(ns, 0) - ns).to(torch.int32).contiguous(), gt=sc["gt"][keep].contiguous(),
               bg_ray=sc["bg_ray"][keep].contiguous())
    out["samp_ray"] = torch.cat([torch.repeat_interleave(torch.arange(Rk), ns.long()), torch.zeros(5, dtype=torch.long)]).to(torch.int32)
    for k in ("samp_locw", "samp_nnb", "pidx", "feat"):
        out[k] = torch.cat([sc[k][:S][ks], sc[k][S:S + 5]]).contiguous()
    assert Rk > 0 and out["samp_ray"].shape[0] == Sk + 5
    return out


class DevX(Dev):
    def __init__(self, sc):
        super().__init__(sc)
        self.xyz = sc["xyz"].contiguous().to(DEV)


def _run_opts(sc, dv, unit, bgr, weights, zo_w, eps, sparse, depth=None, dconf=True, R=None):
    """sgn_loss_train_opts on sentinel-filled outputs.  depth: (gt_depth, gt_mask or None, weight)."""
    R = sc["R"] if R is None else R
    SR, K, S_cap, N = sc["SR"], sc["K"], sc["S_cap"], sc["n_points"]
    d = dv.d
    out = dict(rgb=torch.full((sc["R"] + GUARD, 3), NAN, device=DEV), mask=torch.full((sc["R"] + GUARD,), 77, dtype=torch.int8, device=DEV),
               losses=torch.full((12 + GUARD,), NAN, device=DEV), dfeat=torch.full((S_cap + GUARD, 4), NAN, device=DEV),
               dconf=torch.cat([torch.zeros(N), torch.full((GUARD,), 7.0)]).to(DEV),
               depth=torch.full((sc["R"] + GUARD,), NAN, device=DEV))
    ws = torch.empty(max(int(_lib.lib().sgn_loss_opts_workspace_bytes(R, SR, K)), 16) + 64, dtype=torch.uint8, device=DEV)
    lp = rsg._loss_params(sc, unit, zo_w, d["bg_ray"] if bgr else None)
    lp.zero_one_eps = eps
    lo = _lib.LossOpts(*weights, sparse, dv.xyz.data_ptr())
    dp = None
    if depth is not None:
        g_dev, m_dev = depth[0].to(DEV), None if depth[1] is None else depth[1].to(DEV)
        dp = ctypes.byref(_lib.LossDepth(g_dev.data_ptr(), None if m_dev is None else m_dev.data_ptr(), depth[2],
                                         out["depth"].data_ptr()))
    p = _lib.ptr
    _lib.check(_lib.lib().sgn_loss_train_opts(ctypes.byref(lp), ctypes.byref(lo), dp, p(d["campos"]), p(d["rot"]), R,
                                              ctypes.byref(dv.qo), p(d["feat"]), p(d["gt"]), p(d["conf"]), p(out["rgb"]),
                                              p(out["mask"]), p(out["losses"]), p(out["dfeat"]),
                                              p(out["dconf"]) if dconf else None, p(ws), ws.numel(), _lib.stream_handle()),
               "sgn_loss_train_opts")
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def _depth_targets(sc, unit, seed):
    gt_d, gt_m = dr.targets(sc, dr.depth_map(sc, unit)["D"], seed=seed)
    return gt_d, gt_m


def _check(out, ref, sc, tag, sparse, with_depth):
    """Guards, then the parts and the two gradients against the reference at the module's bars."""
    R, S, N = sc["R"], sc["S"], sc["n_points"]
    assert _all_nan(out["rgb"][R:]) and bool((out["mask"][R:] == 77).all()) and _all_nan(out["losses"][12:]), tag
    assert _all_nan(out["dfeat"][S:]) and bool((out["dconf"][N:] == 7.0).all()), tag
    assert torch.equal(out["mask"][:R].bool(), ref["mask"]), tag
    L = out["losses"]
    assert float(L[6]) == ref["n"] and float(L[11]) == 0.0
    if not sparse:
        assert _same_bits(L[8:12], torch.zeros(4)), tag
    if not with_depth:
        assert float(L[7]) == 0.0
    for name, want in ref["parts"].items():
        got = float(L[PARTS[name]])
        e = abs(got - want) / max(abs(want), 1e-12)
        WORST["part"] = max(WORST["part"], e)
        assert e <= PART_TOL, (tag, name, got, want)
    for k, got, want in (("dfeat", out["dfeat"][:S], ref["dfeat"][:S]), ("dconf", out["dconf"][:N], ref["dconf"])):
        assert bool(torch.isfinite(got).all()), (tag, k)
        top = float(want.abs().max())
        if top == 0.0:
            assert float(got.abs().max()) == 0.0, (tag, k)
            continue
        e = _rel(got, want)
        WORST[k] = max(WORST[k], e)
        assert e <= GRAD_TOL, (tag, k, e)
        assert float((got.double() - want).abs().max()) <= GRAD_TOL * top, (tag, k)


# ---- 1. per-element parity -----------------------------------------------------------------------------------

COLOUR_W = [(1.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.5, 2.0, 0.25)]
ZO_W = [0.0, 1e-4, 1e-2]
ZO_EPS = [1e-3, 0.05]
SPARSE_W = [0.0, 1e-3, 1.0]


@pytest.mark.parametrize("with_depth", [False, True])
@pytest.mark.parametrize("K", [3, 8])
def test_loss_train_opts_matches_float64(K, with_depth):
    sc = scene(K)
    unit, bgr = K % 2, K == 8
    dv = DevX(sc)
    depth = (*_depth_targets(sc, unit, K), W_D) if with_depth else None
    for weights, zo_w, eps, sparse in itertools.product(COLOUR_W, ZO_W, ZO_EPS, SPARSE_W):
        tag = f"K {K}, depth {with_depth}, colour {weights}, zero-one {zo_w} eps {eps}, sparse {sparse}"
        ref = lr.reference(sc, unit, bgr, COLOR_LOSS_ITEMS, weights, ("conf_coefficient",), (zo_w,), eps, sparse,
                           depth=depth, bg=BG)
        assert 10 < ref["n"] < sc["R"]
        out = _run_opts(sc, dv, unit, bgr, weights, zo_w, eps, sparse, depth)
        _check(out, ref, sc, tag, sparse > 0, with_depth)
        if sparse > 0:      # the term is there: far above the bar
            base = lr.reference(sc, unit, bgr, COLOR_LOSS_ITEMS, weights, ("conf_coefficient",), (zo_w,), eps, 0.0,
                                depth=depth, bg=BG)
            assert _rel(ref["dconf"], base["dconf"]) > 10 * GRAD_TOL or float(base["dconf"].abs().max()) == 0
            assert torch.equal(ref["dfeat"], base["dfeat"])      # and adds nothing to d feat
    print(f"K {K}, depth {with_depth}: worst so far, relative L2 d feat {WORST['dfeat']:.2e}, d conf {WORST['dconf']:.2e}; "
          f"loss part {WORST['part']:.2e}")


@pytest.mark.parametrize("which", ["none", "all"])
@pytest.mark.parametrize("K", [3, 8])
def test_frames_without_and_with_only_valid_rays(K, which):
    sc = scene(K, which)
    dv = DevX(sc)
    depth = (*_depth_targets(sc, 0, K), W_D)
    for weights, sparse, dp in (((0.5, 2.0, 0.25), 1.0, None), ((0.0, 0.0, 1.0), 1e-3, depth), ((1.0, 0.0, 0.0), 0.0, None)):
        ref = lr.reference(sc, 0, True, COLOR_LOSS_ITEMS, weights, ("conf_coefficient",), (1e-2,), 0.05, sparse, depth=dp, bg=BG)
        assert ref["n"] == (0 if which == "none" else sc["R"])
        out = _run_opts(sc, dv, 0, True, weights, 1e-2, 0.05, sparse, dp)
        _check(out, ref, sc, f"{which} rays valid, K {K}, colour {weights}, sparse {sparse}", sparse > 0, dp is not None)
        if which == "none":
            assert float(out["dfeat"][:sc["S"]].abs().max() if sc["S"] else 0.0) == 0.0 and float(out["dconf"][:-GUARD].abs().max()) == 0.0
            assert float(out["losses"][8]) == 0.0


def test_no_ray():
    """R = 0: the call succeeds, d_losses is twelve zeros, every other output keeps its sentinel."""
    sc = scene(3)
    out = _run_opts(sc, DevX(sc), 0, False, (0.5, 2.0, 0.25), 1e-4, 1e-3, 1.0, R=0)
    assert _same_bits(out["losses"][:12], torch.zeros(12)) and _all_nan(out["losses"][12:])
    assert _all_nan(out["rgb"]) and bool((out["mask"] == 77).all()) and _all_nan(out["dfeat"])
    assert float(out["dconf"][:-GUARD].abs().max()) == 0.0


# ---- 2. bit-identity of the stock path ------------------------------------------------------------------------

def _own_points(sc):
    """The scene with every neighbour entry naming a point of its own (same conf and position as before) and
    conf[0] = 0, where the empty entries' term has no gradient: each d conf row then takes at most one atomic add."""
    S = sc["S"]
    p = sc["pidx"].clone()
    ok = p[:S] >= 0
    old = p[:S][ok].long()
    p[:S][ok] = 1 + torch.arange(old.numel(), dtype=p.dtype)
    return dict(sc, pidx=p.contiguous(), n_points=old.numel() + 1,
                conf=torch.cat([torch.zeros(1), sc["conf"][old]]).contiguous(),
                xyz=torch.cat([sc["xyz"][:1], sc["xyz"][old]]).contiguous())


@pytest.mark.parametrize("own", [True, False])
@pytest.mark.parametrize("K", [3, 8])
def test_default_options_equal_the_stock_entries(K, own):
    """(1, 0, 0), sparse 0: d_losses, d_dfeat and d_dconf torch.equal those of sgn_loss_train, and of
    sgn_loss_train_depth with depth, on the same inputs.

    d conf is accumulated with float atomics, whose order is the hardware's: a row that takes three or more adds
    does not repeat its own bits from one call of the stock entry to the next (test_ray_stage_gpu.py exempts d conf
    from its repeat check for that reason; measured here too: sgn_loss_train_opts against sgn_loss_train at K = 8 on
    the 50-point scene differed in the last bit of some rows, as two sgn_loss_train calls do).  own = True gives every
    entry a point of its own, so that all three outputs are a function of the inputs alone and must be equal; own =
    False is the 50-point scene, where d_losses and d_dfeat must be equal and d conf is held to the float64
    reference by test_loss_train_opts_matches_float64 (the default options are among its settings)."""
    import test_depth_gpu as dg
    sc = _own_points(scene(K)) if own else scene(K)
    unit, bgr = K % 2, K == 8
    S, N = sc["S"], sc["n_points"]
    dv = DevX(sc)
    start = torch.cat([torch.zeros(N), torch.full((GUARD,), 7.0)])
    stock = rsg._run_loss(sc, dv, unit, bgr, 1e-4, start)
    out = _run_opts(sc, dv, unit, bgr, (1.0, 0.0, 0.0), 1e-4, rs.ZO_EPS, 0.0)
    assert torch.equal(out["losses"][:8], stock["losses"][:8]) and _same_bits(out["losses"][8:12], torch.zeros(4))
    assert torch.equal(out["dfeat"][:S], stock["dfeat"][:S]) and (not own or torch.equal(out["dconf"], stock["dconf"]))
    assert float(stock["dconf"][:N].abs().max()) > 0
    assert _same_bits(out["rgb"], stock["rgb"]) and torch.equal(out["mask"], stock["mask"])
    # w_miss is read by no kernel: the same bits under another weight
    miss = _run_opts(sc, dv, unit, bgr, (1.0, 3.0, 0.0), 1e-4, rs.ZO_EPS, 0.0)
    assert torch.equal(miss["losses"][:8], stock["losses"][:8]) and torch.equal(miss["dfeat"][:S], stock["dfeat"][:S])
    gt_d, gt_m = _depth_targets(sc, unit, K)
    for m in (None, gt_m):
        stock_d = dg._run_loss_depth(sc, dv, unit, bgr, start, gt_d, m, W_D)
        out_d = _run_opts(sc, dv, unit, bgr, (1.0, 0.0, 0.0), 1e-4, rs.ZO_EPS, 0.0, (gt_d, m, W_D))
        assert torch.equal(out_d["losses"][:8], stock_d["losses"][:8])
        assert torch.equal(out_d["dfeat"][:S], stock_d["dfeat"][:S]) and (not own or torch.equal(out_d["dconf"], stock_d["dconf"]))
        assert _same_bits(out_d["depth"], stock_d["depth"])


# ---- 5 (kernel side). frozen conf ----------------------------------------------------------------------------

def test_null_dconf_still_reports_the_sparse_loss():
    sc = scene(8)
    dv = DevX(sc)
    a = _run_opts(sc, dv, 0, True, (0.5, 2.0, 0.25), 1e-2, 0.05, 1.0)
    b = _run_opts(sc, dv, 0, True, (0.5, 2.0, 0.25), 1e-2, 0.05, 1.0, dconf=False)
    assert _same_bits(a["losses"][:12], b["losses"][:12]) and _same_bits(a["dfeat"], b["dfeat"])
    assert float(b["losses"][8]) > 0 and float(b["dconf"][:-GUARD].abs().max()) == 0.0 and float(a["dconf"][:-GUARD].abs().max()) > 0


# ---- 3. the options reach the step ----------------------------------------------------------------------------

STEP_OPTS = dict(color_loss_weights=(0.0, 0.0, 1.0), zero_one_loss_weights=(0.0,), sparse_loss_weight=1e-3)


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _trainer_grads(ref, pts):
    out = {}
    for name, *_ in LAYERS:
        m = ref.mlp.lin[name.replace(".", "_")]
        out[name + ".weight"], out[name + ".bias"] = m.weight.grad, m.bias.grad
    for k in ("points_embeding", "points_color", "points_dir", "points_conf"):
        out[k] = getattr(pts, k).grad
    return out


def _bar(k, precision):
    if precision == "f32":
        return GRAD_TOL_F32
    return GRAD_TOL_POINTS if k.startswith("points_") else GRAD_TOL_MLP


@pytest.mark.parametrize("precision,graph", [("f32", False), ("f16", True), ("f16", False)])
def test_options_reach_the_step(precision, graph):
    """One step under colour weights (0, 0, 1), zero-one weight 0 and sparse_loss_weight 1e-3: every gradient within
    the precision's bar of train.Trainer's fp32 autograd under the same options (same samples), and away from the
    default-options step of the same batch by more than that bar."""
    pc, view, _, mlp, gt = _setup(seed=3)
    o = dataclasses.replace(O, **STEP_OPTS).check_supported()
    args = (_d(view.campos), _d(view.camrotc2w), _d(view.raydir), 0.1, 8.0, gt.to(DEV))

    def hip(opts):
        tr = HipTrainer(PointParams(pc.xyz, pc.embedding, pc.color, pc.dir, pc.conf, DEV), mlp, opts, DEV, precision=precision)
        tr.use_graph = graph
        parts, full, ray_mask = tr.backward(*args)
        torch.cuda.synchronize()
        return tr, parts, full, ray_mask

    tr, parts, full, ray_mask = hip(o)
    tr0, parts_0, _, _ = hip(O)
    qd = {k: v.long() if v.dtype == torch.int32 else v for k, v in tr.last_query.items()}
    ref_points = PointParams(pc.xyz, pc.embedding, pc.color, pc.dir, pc.conf, DEV)
    ref = Trainer(ref_points, mlp, o, DEV)
    parts_c, full_c, mask_c = ref.backward(*args, q=qd)
    torch.cuda.synchronize()
    assert torch.equal(ray_mask, mask_c) and 0 < int(ray_mask.sum())
    tol_c = GRAD_TOL_F32 if precision == "f32" else 1e-3
    assert "sparse" in parts and "sparse" in parts_c and "sparse" not in parts_0
    assert abs(float(parts["sparse"]) - float(parts_c["sparse"])) <= tol_c * abs(float(parts_c["sparse"]))
    assert abs(float(parts["total"]) - float(parts_c["total"])) <= tol_c * abs(float(parts_c["total"]))
    want = float(parts["coarse_raycolor"]) + 3e-6 + 1e-3 * float(parts["sparse"])
    assert abs(float(parts["total"]) - want) <= 1e-6 * abs(want)
    g, g0, rg = grads_named(tr), grads_named(tr0), _trainer_grads(ref, ref_points)
    worst = {k: _rel(g[k].reshape(b.shape), b) for k, b in rg.items()}
    moved = {k: _rel(g0[k].reshape(b.shape), b) for k, b in rg.items()}
    print(f"[{precision}, graph {graph}] relative L2 gradient errors:", {k: f"{v:.2e}" for k, v in worst.items()})
    print(f"[{precision}, graph {graph}] the default-options step against the same reference:", {k: f"{v:.2e}" for k, v in moved.items()})
    bad = {k: v for k, v in worst.items() if v > _bar(k, precision)}
    assert not bad, bad
    # every gradient but d conf is the default step's times n_valid / R (the masked mean became the mean over every
    # ray; 0.80 of this batch's rays are valid), d conf lost its zero-one term and gained the sparse one
    still = {k: v for k, v in moved.items() if v <= _bar(k, precision)}
    assert not still, still


# ---- 4. the SG variant -----------------------------------------------------------------------------------------

def test_sg_step_with_the_sparse_loss():
    """block2_bpnet (no BPNet embedding) at precision "f32" with the sparse loss on: every gradient within
    GRAD_TOL_F32 of fp32 autograd through oracle/agg_ref.py's SG aggregator plus the loss terms, same samples."""
    import math

    import agg_ref
    pc, view, _, mlp, gt = _setup(seed=5)
    g = torch.Generator().manual_seed(11)
    mlp = dict(mlp)
    mlp["block2_bpnet.0.weight"] = (torch.rand(256, 256, generator=g) * 2 - 1) * math.sqrt(6.0 / 512) * 0.5
    mlp["block2_bpnet.0.bias"] = torch.randn(256, generator=g) * 0.01
    sp = 1e-3
    o = dataclasses.replace(O, shading_feature_mlp_layer2_bpnet=1, sparse_loss_weight=sp).check_supported()
    K, SR = o.K, o.SR
    points = PointParams(pc.xyz, pc.embedding, pc.color, pc.dir, pc.conf, DEV)
    tr = HipTrainer(points, mlp, o, DEV, precision="f32")
    campos, rot, raydir = _d(view.campos), _d(view.camrotc2w), _d(view.raydir)
    R = raydir.shape[0]
    parts, full, mask = tr.backward(campos, rot, raydir, 0.1, 8.0, gt.to(DEV))
    torch.cuda.synchronize()
    hg = grads_named(tr)
    qd = {k: v.long() if v.dtype == torch.int32 else v for k, v in tr.last_query.items()}
    pts = {k: torch.from_numpy(getattr(pc, k)).to(DEV).requires_grad_(k != "xyz") for k in ("xyz", "embedding", "color", "dir", "conf")}
    m = {k: v.to(DEV).requires_grad_(True) for k, v in mlp.items()}
    feat, _ = agg_ref.aggregate(pts, m, campos, rot, raydir, qd["samp_ray"], qd["samp_locw"], qd["pidx"])
    nnb = (qd["pidx"] >= 0).sum(-1)
    fd, vd, ld = agg_ref.densify(R, SR, qd["ray_ns"], qd["samp_ray"], qd["samp_locw"], feat, nnb)
    color, _, _ = agg_ref.composite(fd, vd, ld, rot, campos)
    ray_mask = vd.any(-1)
    gtd = gt.to(DEV)
    l_col = torch.mean((color[ray_mask] - gtd[ray_mask]) ** 2)
    S = qd["samp_ray"].shape[0]
    slot = torch.arange(S, device=DEV) - qd["ray_soff"][qd["samp_ray"]]
    pd = torch.full((R, SR, K), -1, dtype=torch.long, device=DEV)
    pd[qd["samp_ray"], slot] = qd["pidx"]
    wd = torch.zeros(R, SR, K, device=DEV)
    wd[qd["samp_ray"], slot] = neighbour_weights(pts["xyz"].detach(), qd["samp_locw"], qd["pidx"])
    cd = pts["conf"][torch.clamp(pd[ray_mask], min=0).reshape(-1), 0]
    cc = cd - (cd - torch.clamp(cd, 1e-4, 1.0)).detach()
    val = torch.clamp(cc, 1e-3, 1 - 1e-3)
    l_zo = torch.mean(torch.log(val) + torch.log(1 - val))
    wv = wd[ray_mask].reshape(-1)
    l_sp = torch.sum(wv * torch.abs(1 - torch.exp(-2 * cc))) / (torch.sum(wv) + 1e-6)
    total = l_col + 3e-6 + 1e-4 * l_zo + sp * l_sp
    total.backward()
    torch.cuda.synchronize()
    assert torch.equal(mask, ray_mask)
    l_sp, total = l_sp.detach(), total.detach()
    assert abs(float(parts["sparse"]) - float(l_sp)) <= GRAD_TOL_F32 * abs(float(l_sp)) and float(l_sp) > 0
    assert abs(float(parts["total"]) - float(total)) <= GRAD_TOL_F32 * abs(float(total))
    names = {"points_embeding": "embedding", "points_color": "color", "points_dir": "dir", "points_conf": "conf"}
    worst = {}
    for k, v in hg.items():
        ref = pts[names[k]].grad if k in names else m[k].grad
        worst[k] = _rel(v.reshape(ref.shape), ref)
    print("SG f32 with the sparse loss, relative L2 gradient errors:", {k: f"{v:.2e}" for k, v in worst.items()})
    assert "block2_bpnet.0.weight" in worst
    bad = {k: v for k, v in worst.items() if v > GRAD_TOL_F32}
    assert not bad, bad


# ---- 5. frozen conf ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_frozen_conf_with_the_sparse_loss(precision):
    pc, view, _, mlp, gt = _setup(seed=3)
    o = dataclasses.replace(O, conf_grad=0, sparse_loss_weight=1e-3).check_supported()
    points = PointParams(pc.xyz, pc.embedding, pc.color, pc.dir, pc.conf, DEV)
    conf0 = points.points_conf.detach().clone()
    tr = HipTrainer(points, mlp, o, DEV, precision=precision)
    parts, _, ray_mask = tr.step(_d(view.campos), _d(view.camrotc2w), _d(view.raydir), 0.1, 8.0, gt.to(DEV))
    tr.sync_points()
    torch.cuda.synchronize()
    assert points.points_conf.grad is None and grads_named(tr)["points_conf"] is None      # d conf is not written
    assert torch.equal(points.points_conf.detach(), conf0)
    assert int(ray_mask.sum()) > 0 and float(parts["sparse"]) > 0
    live = HipTrainer(PointParams(pc.xyz, pc.embedding, pc.color, pc.dir, pc.conf, DEV), mlp,
                      dataclasses.replace(o, conf_grad=1), DEV, precision=precision)
    parts_l, _, _ = live.backward(_d(view.campos), _d(view.camrotc2w), _d(view.raydir), 0.1, 8.0, gt.to(DEV))
    assert abs(float(parts["sparse"]) - float(parts_l["sparse"])) <= 1e-6 * float(parts_l["sparse"])


# ---- 6. the plugin ------------------------------------------------------------------------------------------------

def test_plugin_reports_loss_sparse(tmp_path):
    from sgnerf_amd.model import LOSS_NAMES, HipPointsVolumetricModel
    pc, view, _, mlp, gt = _setup(seed=3)
    items, weights, zw, sp = [ALL, MASKED], [0.25, 0.5], 1e-2, 1e-3
    opt = argparse.Namespace(SR=24, K=8, gpu_ids=[0], is_train=True, checkpoints_dir=str(tmp_path), name="scene",
                             lr=5e-4, plr=2e-3, lr_decay_exp=0.1, lr_decay_iters=1_000_000, bg_color="white",
                             color_loss_items=items, color_loss_weights=weights, zero_one_loss_items=["conf_coefficient"],
                             zero_one_loss_weights=[zw], zero_epsilon=0.05, sparse_loss_weight=sp, bg_loss_items=[],
                             l2_size_loss_items=[])
    m = HipPointsVolumetricModel()
    m.initialize(opt)
    m.set_points(points_xyz=pc.xyz, points_feats=pc.color * 255.0, points_embedding=pc.embedding,
                 points_color=pc.color, points_dir=pc.dir, points_conf=pc.conf, aggregator_state=mlp)
    m.setup(opt)
    m.set_input({"campos": _d(view.campos)[None], "raydir": _d(view.raydir)[None], "camrotc2w": _d(view.camrotc2w)[None],
                 "near": torch.tensor([[[0.1]]]), "far": torch.tensor([[[8.0]]]), "gt_image": gt[None].to(DEV)})
    m.optimize_parameters(total_steps=0)
    losses = m.get_current_losses()
    assert set(losses) == set(LOSS_NAMES) | {"sparse"} and hasattr(m, "loss_sparse")
    assert float(m.loss_sparse) > 0
    want = (np.float32(0.25) * np.float32(float(losses[ALL])) + np.float32(0.5) * np.float32(float(losses[MASKED]))
            + np.float32(2e-6) + np.float32(zw) * np.float32(float(losses["conf_coefficient"]))
            + np.float32(sp) * np.float32(float(losses["sparse"])))
    assert abs(float(losses["total"]) - float(want)) <= 4 * 2.0 ** -24 * (abs(float(want)) + zw * abs(float(losses["conf_coefficient"])))
    # the probe ranking keeps reading ray_miss_coarse_raycolor, whatever its weight (here: not listed)
    assert hasattr(m, "loss_ray_miss_coarse_raycolor")
