"""GPU tests of early ray termination (opts.early_stop; sgn_early_stop_tier + the tier loop of
HipRenderer.render) against the restatement tests/early_stop_ref.py.

Bounds (early ray termination; eps = early_stop): against the full render of the same build a colour
channel moves by at most 1.001 eps and bg_transmission rises by at most eps, each + 1e-6 of fp32 summation
noise; ray_mask does not move; a frame in which no ray reaches T <= eps at a boundary is bit-identical."""
import ctypes

import numpy as np
import pytest
import torch

import early_stop_ref as er
from helpers import GOLDEN_DIR, golden_points, load_golden
from sgnerf_amd import _lib, scene
from sgnerf_amd.opts import HotPathOpts
from sgnerf_amd.render import HipRenderer, PointTables

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RGB_BAR = {"f32": 1e-5, "f16": 1e-3}    # tests/test_render_gpu.py: F32_TOL, RGB_TOL
NOISE = 1e-6


# ---- 1. the entry alone on hand-built queries ------------------------------------------------------------

def _hand_query(SR, lo, seed):
    """R = 130 rays (two waves + two): ray_ns cycling through 0, 1, lo, lo + 1, SR and random counts, samples
    without neighbours sprinkled in, z that falls, repeats and jumps (cummax, both distance replacements),
    alphas from 0 (T stays 1) to 1e4 (factor 1e-10)."""
    rng = np.random.default_rng(seed)
    R, vz = 130, 0.008
    pool = [0, 1, lo, lo + 1, SR]
    ns = np.array([pool[r % 5] if r % 3 else rng.integers(0, SR + 1) for r in range(R)], np.int32)
    off = np.concatenate([[0], np.cumsum(ns)[:-1]]).astype(np.int32)
    S = int(ns.sum())
    step = rng.choice([vz, vz, vz, 0.0, -0.5 * vz, 3.0 * vz, 0.3 * vz], S).astype(np.float32)
    campos = np.array([0.3, -0.1, 0.2], np.float32)
    c, s_ = np.cos(0.4), np.sin(0.4)
    rot = np.array([[c, 0, s_], [0, 1, 0], [-s_, 0, c]], np.float32)   # camera z axis = rot[:, 2]
    locw = np.zeros((S, 3), np.float32)
    for r in range(R):
        z = 0.6 + np.cumsum(step[off[r]:off[r] + ns[r]])
        locw[off[r]:off[r] + ns[r]] = campos + z[:, None] * rot[:, 2][None, :] + rng.normal(0, 0.01, (ns[r], 1)) * rot[:, 0]
    nnb = np.where(rng.random(S) < 0.85, rng.integers(1, 9, S), 0).astype(np.int32)
    feat = rng.random((S, 4)).astype(np.float32)
    feat[:, 0] = rng.choice([0.0, 0.05, 0.5, 30.0, 300.0, 1e4], S)
    return dict(R=R, SR=SR, vz=vz, campos=campos, rot=rot, ns=ns, off=off, S=S, locw=locw, nnb=nnb, feat=feat)


def _call_tier(h, dev, unit, lo, hi, eps, prev):
    cp = _lib.CompositeParams()
    cp.SR, cp.vsize_z, cp.raydist_mode_unit = h["SR"], h["vz"], unit
    q = _lib.QueryOut()
    for name, key in (("ray_ns", "ns"), ("ray_soff", "off"), ("samp_nnb", "nnb"), ("samp_locw", "locw"),
                      ("counters", "qcounters")):
        setattr(q, name, dev[key].data_ptr())
    counters = torch.full((4,), 77, dtype=torch.int32, device=DEV)     # the call clears them
    _lib.check(_lib.lib().sgn_early_stop_tier(ctypes.byref(cp), _lib.ptr(dev["campos"]), _lib.ptr(dev["rot"]), h["R"],
                                              ctypes.byref(q), _lib.ptr(dev["feat"]), lo, hi, eps, dev["work"].numel(),
                                              _lib.ptr(dev["work"]), _lib.ptr(counters), _lib.ptr(prev),
                                              _lib.ptr(dev["stop"]), _lib.stream_handle()), "sgn_early_stop_tier")
    torch.cuda.synchronize()
    return counters


@pytest.mark.parametrize("eps", [1e-2, 0.999])
@pytest.mark.parametrize("lo", [0, 4, 5])
@pytest.mark.parametrize("unit", [0, 1])
@pytest.mark.parametrize("SR", [24, 33])
def test_tier_entry_matches_restatement(SR, unit, lo, eps):
    """Two calls, [lo, lo + 6) then [lo + 6, SR): the emitted id sets, the zeroed feats (the whole buffer, bit
    for bit), stop_slot and the counters equal the restatement's; rays finished by the first call stay finished
    in the second.  The restatement's exp is numpy's and the kernel's is the device's expf, so the inputs are
    required (on the restatement alone) to keep every T a relative 1e-4 away from eps."""
    h = _hand_query(SR, lo, seed=SR * 7 + lo)
    R, S = h["R"], h["S"]
    dev = {k: torch.from_numpy(h[k]).to(DEV) for k in ("campos", "rot", "ns", "off", "nnb", "locw", "feat")}
    dev["qcounters"] = torch.tensor([S, 5, 0, 0], dtype=torch.int32, device=DEV)
    dev["work"] = torch.full((S + 8,), -1, dtype=torch.int32, device=DEV)
    dev["stop"] = torch.full((R,), SR, dtype=torch.int32, device=DEV)
    feat, stop = h["feat"].copy(), np.full(R, SR, np.int32)
    prev, skipped, finished_before = None, 0, np.zeros(R, bool)
    for lo_, hi_ in ((lo, lo + 6), (lo + 6, SR)):
        emit, zero, stop, T = er.tier(h["campos"], h["rot"], h["ns"], h["off"], h["nnb"], h["locw"], feat, SR, unit,
                                      h["vz"], lo_, hi_, eps, stop)
        assert (np.abs(T.astype(np.float64) - eps) > 1e-4 * eps).all(), "a T too close to eps: change the seed"
        fin = T <= np.float32(eps)
        assert fin[finished_before].all()                     # a finished ray stays finished
        if lo_ > 0:
            assert fin.any() and not fin.all()                # both branches run
        feat[zero] = 0.0
        skipped += len(zero)
        dev["work"].fill_(-1)
        counters = _call_tier(h, dev, unit, lo_, hi_, eps, prev)
        got = counters.cpu().numpy()
        assert got.tolist() == [S, len(emit), skipped, 0]
        work = dev["work"].cpu().numpy()
        np.testing.assert_array_equal(np.sort(work[:len(emit)]), emit)
        assert (work[len(emit):] == -1).all()
        np.testing.assert_array_equal(dev["feat"].cpu().numpy().view(np.int32), feat.view(np.int32))
        np.testing.assert_array_equal(dev["stop"].cpu().numpy(), stop)
        prev, finished_before = counters, fin
    assert skipped > 0


# ---- 2. frames -------------------------------------------------------------------------------------------

def _golden_case(file, name):
    pts, mlp, c = load_golden(file, name)
    near, far = (float(x) for x in c["near_far"])
    view = scene.View(c["campos"], c["camrotc2w"], c["raydir"], None, None, 0, 0, near, far)
    return pts, mlp, c, view


def _render(pts, mlp, view, o, rot=None, **kw):
    r = HipRenderer(PointTables(pts["xyz"], pts["embedding"], pts["color"], pts["dir"], pts["conf"], DEV, rot=rot),
                    mlp, o, DEV)
    out = r.render(torch.from_numpy(view.campos), torch.from_numpy(view.camrotc2w), torch.from_numpy(view.raydir),
                   view.near, view.far, **kw)
    torch.cuda.synchronize()
    return r, out


def _snap(out, R):
    """Host copies of a frame (the renderer's buffers are reused) + the dense valid mask and sample slots."""
    q = out.query
    S = q.n_samples()
    sr = q.samp_ray[:S].cpu().numpy()
    slot = np.arange(S) - q.ray_soff[:R].cpu().numpy()[sr]
    valid = q.samp_nnb[:S].cpu().numpy() > 0
    d = dict(rgb=out.rgb.cpu().numpy(), mask=out.ray_mask.cpu().numpy(), bgT=out.bg_transmission.cpu().numpy(),
             opacity=out.opacity.cpu().numpy(), feat=out.feat[:S].cpu().numpy()[valid], sr=sr[valid], slot=slot[valid])
    d["valid"] = np.zeros(d["opacity"].shape, bool)
    d["valid"][d["sr"], d["slot"]] = True
    if out.depth is not None:
        d["depth"] = out.depth.cpu().numpy()
    if out.stop_slot is not None:
        d.update(stop=out.stop_slot.cpu().numpy(), skipped=int(out.skipped.item()), tiers=out.tiers.cpu().numpy())
    return d


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else a.dtype)


def _assert_identical(a, b, keys=("rgb", "mask", "bgT", "opacity", "feat")):
    for k in keys:
        np.testing.assert_array_equal(_bits(a[k]), _bits(b[k]), err_msg=k)


def _check_terminated(es, full, eps, slots, SR, what):
    """The properties of a frame rendered with termination against the full render of the same build."""
    np.testing.assert_array_equal(es["mask"], full["mask"])
    drgb = np.abs(es["rgb"].astype(np.float64) - full["rgb"]).max()
    dbg = es["bgT"].astype(np.float64) - full["bgT"]
    print(f"{what}: skipped {es['skipped']} of {int(es['valid'].sum())} valid samples, max |rgb - full| = {drgb:.3e}, "
          f"bgT - full in [{dbg.min():.3e}, {dbg.max():.3e}]; work items per tier {es['tiers'][:, 1].tolist()}")
    assert drgb <= 1.001 * eps + NOISE
    assert dbg.min() >= -NOISE and dbg.max() <= eps + NOISE
    # the decision, from the run's own opacities: the first boundary with T <= eps
    stop, skipped = er.decide(es["opacity"], es["valid"], eps, slots)
    np.testing.assert_array_equal(es["stop"], stop)
    assert es["skipped"] == int(skipped.sum())
    after = es["slot"] >= stop[es["sr"]]
    assert (es["feat"][after] == 0).all()                                               # skipped: zero feat
    np.testing.assert_array_equal(_bits(es["feat"][~after]), _bits(full["feat"][~after]))   # none before was
    bounds = er.boundaries(slots, SR)
    per_tier = [int((es["valid"][:, lo:hi] & ~skipped[:, lo:hi]).sum()) for lo, hi in zip(bounds[:-1], bounds[1:])]
    assert es["tiers"][:, 1].tolist() == per_tier and es["tiers"][-1, 2] == es["skipped"]


@pytest.mark.parametrize("slots", [(4, 8, 16), (5,)])
@pytest.mark.parametrize("prec", ["f32", "f16"])
@pytest.mark.parametrize("name", ["patch", "patch64", "dense"])
def test_no_termination_is_bit_identical(name, prec, slots):
    """The transparent goldens (final T >= 0.96) at eps = 1e-3: no ray finishes, and the tiered frame equals the
    untouched path bit for bit -- a sample's result does not depend on the list or tile it ran in."""
    pts, mlp, c, view = _golden_case("reference_aggregator.npz", name)
    R, SR = view.raydir.shape[0], int(c["SR"])
    r0, out = _render(pts, mlp, view, HotPathOpts(precision=prec, SR=SR, K=int(c["K"])))
    assert out.stop_slot is None and out.skipped is None and out.tiers is None and r0.es is None
    full = _snap(out, R)
    o = HotPathOpts(precision=prec, SR=SR, K=int(c["K"]), early_stop=1e-3, early_stop_slots=slots)
    r1, out = _render(pts, mlp, view, o)
    es = _snap(out, R)
    _assert_identical(es, full)
    assert es["skipped"] == 0 and (es["stop"] == SR).all()
    assert es["tiers"].shape == (len(o.early_stop_tiers), 4)
    assert es["tiers"][:, 1].sum() == int(out.query.counters[1]) == int(es["valid"].sum())


SATURATED_BIAS = 500.0


def _saturated_prediction(c, eps, slots):
    """Skipped / valid samples the restatement predicts for the golden with the alpha bias raised: the stored
    alphas are softplus(x - 1) blends with x near 50 (the softplus is linear there, the weights sum to 1), so
    the raised bias adds SATURATED_BIAS * sum(weight) to each."""
    valid = c["ray_valid"].astype(bool)
    a = c["decoded"][..., 0] + np.float32(SATURATED_BIAS) * c["weight"].sum(-1)
    op = np.where(valid, 1 - np.exp(-(a * c["ray_dist"])), 0).astype(np.float32)
    return int(er.decide(op, valid, eps, slots)[1].sum()), int(valid.sum())


@pytest.mark.parametrize("saturated", [False, True])
@pytest.mark.parametrize("prec", ["f32", "f16"])
@pytest.mark.parametrize("name", ["corner64", "sparse32"])
def test_termination(name, prec, saturated):
    """The opaque goldens at eps = 1e-2, as stored and saturated: alpha_branch.0.bias + 500 (alpha ~ 550, opacity
    0.988 per 0.008 step, T ~ 1.5e-4 after two samples), chosen on the CPU from the restatement as the offset
    at which the default slots skip more than half of the valid samples (1103 / 2090 and 1028 / 1972)."""
    eps, slots = 1e-2, (4, 8, 16)
    pts, mlp, c, view = _golden_case("reference_opaque.npz", name)
    R, SR = view.raydir.shape[0], int(c["SR"])
    if saturated:
        n_skip, n_valid = _saturated_prediction(c, eps, slots)
        assert n_skip > n_valid / 2
        mlp = dict(mlp)
        mlp["alpha_branch.0.bias"] = mlp["alpha_branch.0.bias"] + SATURATED_BIAS
    kw = dict(precision=prec, SR=SR, K=int(c["K"]))
    full = _snap(_render(pts, mlp, view, HotPathOpts(**kw))[1], R)
    es = _snap(_render(pts, mlp, view, HotPathOpts(early_stop=eps, early_stop_slots=slots, **kw))[1], R)
    _check_terminated(es, full, eps, slots, SR, f"{name} [{prec}{', saturated' if saturated else ''}]")
    assert es["skipped"] > 0
    if saturated:
        assert es["skipped"] > es["valid"].sum() / 2
    else:
        err = np.abs(es["rgb"] - c["full_color"]).max()
        print(f"{name} [{prec}]: max |rgb - reference| = {err:.3e}")
        assert err <= RGB_BAR[prec] + 1.001 * eps


@pytest.mark.parametrize("prec", ["f32", "f16"])
def test_termination_with_depth(prec):
    """want_depth at eps = 1e-2 (corner64): a skipped sample has weight 0.  A stopped ray loses at most eps of
    weight, so its sums move by |dA| <= eps zmax and |dW| <= eps with W >= 1 - 2 eps:
    |d(A / W)| <= 2 eps zmax / (1 - 2 eps); a ray that never stopped keeps its depth bit for bit."""
    eps, slots = 1e-2, (4, 8, 16)
    pts, mlp, c, view = _golden_case("reference_opaque.npz", "corner64")
    R, SR = view.raydir.shape[0], int(c["SR"])
    kw = dict(precision=prec, SR=SR, K=int(c["K"]))
    full = _snap(_render(pts, mlp, view, HotPathOpts(**kw), want_depth=True)[1], R)
    r, out = _render(pts, mlp, view, HotPathOpts(early_stop=eps, early_stop_slots=slots, **kw), want_depth=True)
    es = _snap(out, R)
    _check_terminated(es, full, eps, slots, SR, f"corner64 depth [{prec}]")
    assert es["skipped"] > 0
    S = out.query.n_samples()
    locw = out.query.samp_locw[:S * 3].view(S, 3).cpu().numpy()
    zmax = float(((locw - view.campos) @ view.camrotc2w[:, 2]).max())
    live = es["stop"] == SR
    np.testing.assert_array_equal(_bits(es["depth"][live]), _bits(full["depth"][live]))
    dd = np.abs(es["depth"].astype(np.float64) - full["depth"]).max()
    print(f"corner64 depth [{prec}]: max |depth - full| = {dd:.3e} (zmax {zmax:.3f})")
    assert dd <= 2 * eps * zmax / (1 - 2 * eps) + NOISE


@pytest.mark.parametrize("prec", ["f32", "f16"])
def test_termination_rotated_points(prec):
    """rot_mixed of reference_rw2c.npz (per-point Rw2c, the opaque weights) at eps = 1e-2."""
    eps, slots = 1e-2, (4, 8, 16)
    g = np.load(f"{GOLDEN_DIR}/reference_rw2c.npz", allow_pickle=False)
    pts = golden_points(g, "corner")
    _, mlp, _ = load_golden(str(g["mlp_from"]), "sparse32")
    near, far = (float(x) for x in g["view/near_far"])
    view = scene.View(g["view/campos"], g["view/camrotc2w"], g["view/raydir"], None, None, 0, 0, near, far)
    rot = torch.from_numpy(g["palette"])[torch.from_numpy(g["rot_mixed/index"]).long()]
    R, SR = view.raydir.shape[0], int(g["rot_mixed/SR"])
    kw = dict(precision=prec, SR=SR, K=int(g["rot_mixed/K"]))
    full = _snap(_render(pts, mlp, view, HotPathOpts(**kw), rot=rot)[1], R)
    es = _snap(_render(pts, mlp, view, HotPathOpts(early_stop=eps, early_stop_slots=slots, **kw), rot=rot)[1], R)
    _check_terminated(es, full, eps, slots, SR, f"rot_mixed [{prec}]")
    assert es["skipped"] > 0
    assert np.abs(es["rgb"] - g["rot_mixed/full_color"]).max() <= RGB_BAR[prec] + 1.001 * eps


@pytest.mark.parametrize("prec", ["f32", "f16"])
def test_sg_without_termination_is_bit_identical(prec):
    """SG (block2_bpnet, sg96) at eps = 1e-2: no ray finishes there, so the tiered frame is the full render."""
    g = np.load(f"{GOLDEN_DIR}/reference_sg.npz", allow_pickle=False)
    mlp = {k[len("mlp_sg96/"):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("mlp_sg96/")}
    raydir = torch.from_numpy(g["sg96/raydir"])
    R, SR = raydir.shape[0], int(g["sg96/SR"])
    near, far = (float(x) for x in g["sg96/near_far"])
    snaps = []
    for es in (0.0, 1e-2):
        pts = PointTables(*(g[f"sgpatch/{k}"] for k in ("xyz", "embedding", "color", "dir", "conf")), DEV,
                          bpnet=g["sgpatch/bpnet"])
        o = HotPathOpts(precision=prec, SR=SR, shading_feature_mlp_layer2_bpnet=1, predict_semantic=1,
                        semantic_guidance=1, early_stop=es)
        out = HipRenderer(pts, mlp, o, DEV).render(
            torch.from_numpy(g["sg96/campos"]), torch.from_numpy(g["sg96/camrotc2w"]), raydir, near, far,
            point_labels=torch.zeros(pts.n, dtype=torch.int32, device=DEV),
            ray_labels=torch.zeros(R, dtype=torch.int32, device=DEV), seconds=5)
        torch.cuda.synchronize()
        snaps.append(_snap(out, R))
    full, es = snaps
    _assert_identical(es, full)
    assert es["skipped"] == 0 and (es["stop"] == SR).all() and "stop" not in full


def test_range_guard_accumulates_over_tiers():
    """f32: the colour stage clears the fp16-range flag on every call, so after a tiered frame the workspace
    word speaks for the last tier only.  One point that only samples of slots 0 .. 3 name gets an embedding
    outside fp16 range (slots (4, 8): the golden patch has work in [0, 4), [4, 8) and [8, 24)): the last
    tier's word stays 0, the flag accumulated over the tiers does not, and the
    synchronous check re-renders the frame on the plain-fp32 path -- the same frame, bit for bit, as the
    renderer without early termination gives."""
    pts, mlp, c, view = _golden_case("reference_aggregator.npz", "patch")
    R, SR, K = view.raydir.shape[0], int(c["SR"]), int(c["K"])
    kw = dict(SR=SR, K=K)
    _, out = _render(pts, mlp, view, HotPathOpts(**kw))
    S = out.query.n_samples()
    slot = np.arange(S) - out.query.ray_soff[:R].cpu().numpy()[out.query.samp_ray[:S].cpu().numpy()]
    pidx = out.query.pidx[:S * K].view(S, K).cpu().numpy()
    late = np.unique(pidx[slot >= 4])
    early = np.setdiff1d(np.unique(pidx[slot < 4]), late)
    early = early[early > 0]        # not point 0, which empty neighbour slots read
    assert early.size > 0
    bad = {k: np.array(v, copy=True) for k, v in pts.items()}
    bad["embedding"][early[0]] = 1e5
    args = (torch.from_numpy(view.campos), torch.from_numpy(view.camrotc2w), torch.from_numpy(view.raydir),
            view.near, view.far)
    tab = PointTables(bad["xyz"], bad["embedding"], bad["color"], bad["dir"], bad["conf"], DEV)
    plain = HipRenderer(tab, mlp, HotPathOpts(**kw), DEV)
    ref = _snap(plain.render(*args), R)
    assert plain.exact
    r = HipRenderer(tab, mlp, HotPathOpts(early_stop=1e-3, early_stop_slots=(4, 8), **kw), DEV)
    out = r.render(*args, check_range=False)
    torch.cuda.synchronize()
    assert out.tiers is not None and int(out.tiers[:, 1].min()) > 0 and not r.exact
    assert int(r._ws_flag().item()) == 0 and int(r._flag().item()) != 0
    out = r.render(*args)
    assert r.exact and out.stop_slot is None
    _assert_identical(_snap(out, R), ref)


@pytest.mark.parametrize("prec", ["f32", "f16"])
def test_probe_ignores_early_stop(prec):
    """want_probe with early_stop > 0: the frame is rendered in full, the outputs bit for bit the untouched
    path's (the saturated corner64, where termination would skip more than half of the samples)."""
    pts, mlp, c, view = _golden_case("reference_opaque.npz", "corner64")
    mlp = dict(mlp)
    mlp["alpha_branch.0.bias"] = mlp["alpha_branch.0.bias"] + SATURATED_BIAS
    R, SR = view.raydir.shape[0], int(c["SR"])
    snaps = []
    for es in (0.0, 1e-2):
        r, out = _render(pts, mlp, view, HotPathOpts(precision=prec, SR=SR, K=int(c["K"]), early_stop=es),
                         want_probe=True)
        assert out.stop_slot is None and out.skipped is None and out.tiers is None and r.es is None
        d = _snap(out, R)
        d["probe"] = out.probe.cpu().numpy()
        S = out.query.n_samples()
        d["blend"] = out.blend[:S].cpu().numpy()[out.query.samp_nnb[:S].cpu().numpy() > 0]
        snaps.append(d)
    _assert_identical(snaps[1], snaps[0], keys=("rgb", "mask", "bgT", "opacity", "feat", "probe", "blend"))


def test_ray_marcher_passes_the_option_through():
    """NeuralPointsRayMarching on the saturated corner64 at eps = 1e-2: built with return_weights=False its
    render() / forward() are the renderer's terminated frame, bit for bit; built with the weight outputs
    (the default) the option is ignored and the frame is the full render."""
    from sgnerf_amd.ray_marching import NeuralPoints, NeuralPointsRayMarching
    eps = 1e-2
    pts, mlp, c, view = _golden_case("reference_opaque.npz", "corner64")
    mlp = dict(mlp)
    mlp["alpha_branch.0.bias"] = mlp["alpha_branch.0.bias"] + SATURATED_BIAS
    R, SR = view.raydir.shape[0], int(c["SR"])
    kw = dict(SR=SR, K=int(c["K"]))
    full = _snap(_render(pts, mlp, view, HotPathOpts(**kw))[1], R)
    es = _snap(_render(pts, mlp, view, HotPathOpts(early_stop=eps, **kw))[1], R)
    assert es["skipped"] > es["valid"].sum() / 2 and not np.array_equal(es["rgb"], full["rgb"])
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)[None]  # noqa: E731
    inp = {"campos": d(view.campos), "raydir": d(view.raydir), "camrotc2w": d(view.camrotc2w), "near": view.near,
           "far": view.far}
    npnts = NeuralPoints(pts["xyz"], pts["embedding"], pts["color"], pts["dir"], pts["conf"], DEV)
    for weights, want in ((False, es), (True, full)):
        net = NeuralPointsRayMarching(npnts, mlp, HotPathOpts(early_stop=eps, **kw), DEV, return_weights=weights)
        out = net.render(inp)
        assert ("weight" in out) == weights
        np.testing.assert_array_equal(_bits(out["coarse_raycolor"][0].cpu().numpy()), _bits(want["rgb"]))
        np.testing.assert_array_equal(_bits(out["coarse_point_opacity"][0].cpu().numpy()), _bits(want["opacity"]))
        keep = want["mask"].astype(bool)
        comp = net.forward(inp)
        np.testing.assert_array_equal(_bits(comp["coarse_raycolor"][0].cpu().numpy()), _bits(want["rgb"][keep]))
