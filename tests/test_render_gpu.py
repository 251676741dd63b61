"""GPU parity of the fused renderer (query -> MFMA aggregator -> composite).

Tolerances (BASELINE.json north_star): RGB within 1e-3 L-inf of the reference
PyTorch path; neighbour indices and ray masks bit-exact.  Precision "f32" (the default, the
reference's arithmetic: every fp32 product as three fp16 MFMA products, fp32 accumulate) is held
to fp32-level bars: decoded features and RGB within 1e-5 (relative to max(1, |value|) for the
large alphas of opaque scenes).  Precision "f16" (fp16 MFMA operands) gets the looser, stated
per-sample bound FEAT_TOL."""
import os

import numpy as np
import pytest
import torch

import agg_ref
import oracle_query as oq
from helpers import check_grid, check_query_sample_major, hyper_for, load_golden, make_view, small_room
from sgnerf_amd import scene
from sgnerf_amd.opts import HotPathOpts
from sgnerf_amd.render import HipRenderer, PointTables
from sgnerf_amd.weights import init_mlp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RGB_TOL = 1e-3          # north-star bound on final ray colour
FEAT_TOL = 4e-3         # per-sample alpha / rgb before compositing (fp16 MFMA), absolute
F32_TOL = 1e-5          # precision "f32": decoded features, RGB, opacity (x max(1, |ref|) for features)
# (rgb, feature) bars per precision; "exact": the f32 mode on its plain-fp32 range fallback
# (sgn_aggregate_exact, forced on), held to the same fp32 bars
TOL = {"f32": (F32_TOL, F32_TOL), "f16": (RGB_TOL, FEAT_TOL), "exact": (F32_TOL, F32_TOL)}


def _opts(prec, **kw):
    return HotPathOpts(precision="f32" if prec == "exact" else prec, **kw)


def _dense_feat(out, R, SR):
    q = out.query
    S = q.n_samples()
    sr = q.samp_ray[:S].cpu().numpy()
    slot = np.arange(S) - q.ray_soff[:R].cpu().numpy()[sr]
    dense = np.zeros((R, SR, 4), np.float32)
    valid = q.samp_nnb[:S].cpu().numpy() > 0
    dense[sr[valid], slot[valid]] = out.feat[:S].cpu().numpy()[valid]
    return dense, sr, slot, valid
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_aggregator.npz")


def _render(pts, mlp, view, o, exact=False):
    r = HipRenderer(PointTables(pts["xyz"], pts["embedding"], pts["color"], pts["dir"], pts["conf"], DEV), mlp, o, DEV)
    r.exact = exact
    out = r.render(torch.from_numpy(view.campos), torch.from_numpy(view.camrotc2w), torch.from_numpy(view.raydir),
                   view.near, view.far, want_blend=True)
    torch.cuda.synchronize()
    return r, out


OPAQUE = ["opq_patch", "corner64", "sparse32"]   # reference_opaque.npz (alpha bias +50)


@pytest.mark.parametrize("prec", ["f32", "f16", "exact"])
@pytest.mark.parametrize("name", ["patch", "patch64", "dense"] + OPAQUE)
def test_render_matches_reference_golden(name, prec):
    pts, mlp, case = load_golden("reference_opaque.npz" if name in OPAQUE else "reference_aggregator.npz", name)
    g = {f"{name}/{k}": v for k, v in case.items()}
    near, far = (float(x) for x in g[f"{name}/near_far"])
    view = scene.View(g[f"{name}/campos"], g[f"{name}/camrotc2w"], g[f"{name}/raydir"], None, None, 0, 0, near, far)
    o = _opts(prec, SR=int(g[f"{name}/SR"]), K=int(g[f"{name}/K"]))
    rgb_tol, feat_tol = TOL[prec]
    r, out = _render(pts, mlp, view, o, exact=prec == "exact")
    R = view.raydir.shape[0]
    np.testing.assert_array_equal(out.ray_mask.cpu().numpy(), g[f"{name}/ray_mask"])
    rgb = out.rgb.cpu().numpy()
    err = np.abs(rgb - g[f"{name}/full_color"]).max()
    print(f"{name} [{prec}]: max |rgb - reference| = {err:.3e}")
    assert err <= rgb_tol
    keep = g[f"{name}/ray_mask"].astype(bool)
    bgt = out.bg_transmission.cpu().numpy()[keep]
    assert np.abs(bgt - g[f"{name}/bg_transmission"]).max() <= rgb_tol
    op = out.opacity.cpu().numpy()[keep]
    assert np.abs(op - g[f"{name}/opacity"]).max() <= feat_tol
    # per-sample decoded features, scattered back to the reference's dense layout
    dense, sr, slot, valid = _dense_feat(out, R, o.SR)
    ref = g[f"{name}/decoded"]
    ferr = (np.abs(dense[keep] - ref) / np.maximum(1.0, np.abs(ref))).max()
    print(f"{name} [{prec}]: max |decoded - reference| / max(1, |ref|) = {ferr:.3e}")
    assert ferr <= feat_tol
    # weight * conf_coefficient, the reference's `weight` output (point_aggregators.py:955)
    wd = np.zeros((R, o.SR, o.K), np.float32)
    wd[sr[valid], slot[valid]] = out.blend[:len(valid)].cpu().numpy()[valid]
    ref_w = g[f"{name}/weight"] * g[f"{name}/conf_coefficient"]
    np.testing.assert_allclose(wd[keep], ref_w, atol=1e-5, rtol=1e-4)


@pytest.mark.parametrize("prec", ["f32", "f16", "exact"])
@pytest.mark.parametrize("SR,seed,yaw,alpha_bias", [(24, 0, 30.0, 0.0), (64, 1, 210.0, 0.0), (32, 2, 120.0, 150.0)])
def test_render_matches_oracle_room(SR, seed, yaw, alpha_bias, prec):
    """alpha_bias 150 makes sigma ~150 (opacity ~0.7 per 0.008 step), so colour errors
    are not hidden by a transparent volume."""
    pc = small_room(300_000, seed=seed)
    o = _opts(prec, SR=SR)
    rgb_tol, feat_tol = TOL[prec]
    mlp = init_mlp(seed, bias_std=0.01)
    mlp["alpha_branch.0.bias"] = mlp["alpha_branch.0.bias"] + alpha_bias
    view = make_view(48, 64, yaw=yaw, pitch=-8.0)
    pts = dict(xyz=pc.xyz, embedding=pc.embedding, color=pc.color, dir=pc.dir, conf=pc.conf)
    r, out = _render(pts, mlp, view, o, exact=prec == "exact")
    hy = hyper_for(pc, o)
    q = oq.OracleGrid(pc.xyz, hy, o).query(view.campos, view.raydir, r.querier.depth_table(0.1, 8.0, 0)[0].cpu().numpy())
    tp = {k: torch.from_numpy(v) for k, v in pts.items()}
    with torch.no_grad():
        full, mask, fd, opacity, bg_t = agg_ref.render(tp, mlp, torch.from_numpy(view.campos),
                                                       torch.from_numpy(view.camrotc2w), torch.from_numpy(view.raydir), q, SR)
    np.testing.assert_array_equal(out.ray_mask.cpu().numpy().astype(bool), mask.numpy())
    err = np.abs(out.rgb.cpu().numpy() - full.numpy()).max()
    dense = _dense_feat(out, view.raydir.shape[0], SR)[0]
    ferr = (np.abs(dense - fd.numpy()) / np.maximum(1.0, np.abs(fd.numpy()))).max()
    print(f"room SR={SR} [{prec}]: max |rgb - oracle| = {err:.3e}, max feature error {ferr:.3e}, "
          f"valid rays {int(mask.sum())}/{mask.numel()}")
    assert err <= rgb_tol
    assert ferr <= feat_tol
    assert int(mask.sum()) > 0.5 * mask.numel()


@pytest.mark.parametrize("prec", ["f32", "f16", "exact"])
@pytest.mark.parametrize("K,alpha_bias", [(4, 0.0), (4, 150.0), (1, 0.0)])
def test_render_matches_oracle_room_small_k(K, alpha_bias, prec):
    """K < 8 neighbours per sample (PointAggregator takes any K, point_aggregators.py:868-959; the
    query supports 1 / 4 / 8 / 16): a sample's rows k < K read pidx index s * K + k, rows k >= K are
    empty.  Same bars per precision as K = 8, and the per-slot blend weights (weight * conf) against
    the oracle's query."""
    pc = small_room(300_000, seed=5)
    o = _opts(prec, SR=32, K=K)
    rgb_tol, feat_tol = TOL[prec]
    mlp = init_mlp(5, bias_std=0.01)
    mlp["alpha_branch.0.bias"] = mlp["alpha_branch.0.bias"] + alpha_bias
    view = make_view(48, 64, yaw=60.0, pitch=-8.0)
    pts = dict(xyz=pc.xyz, embedding=pc.embedding, color=pc.color, dir=pc.dir, conf=pc.conf)
    r, out = _render(pts, mlp, view, o, exact=prec == "exact")
    hy = hyper_for(pc, o)
    q = oq.OracleGrid(pc.xyz, hy, o).query(view.campos, view.raydir, r.querier.depth_table(0.1, 8.0, 0)[0].cpu().numpy())
    assert q["pidx"].shape[-1] == K
    tp = {k: torch.from_numpy(v) for k, v in pts.items()}
    with torch.no_grad():
        full, mask, fd, opacity, bg_t = agg_ref.render(tp, mlp, torch.from_numpy(view.campos),
                                                       torch.from_numpy(view.camrotc2w), torch.from_numpy(view.raydir),
                                                       q, o.SR)
    np.testing.assert_array_equal(out.ray_mask.cpu().numpy().astype(bool), mask.numpy())
    err = np.abs(out.rgb.cpu().numpy() - full.numpy()).max()
    dense = _dense_feat(out, view.raydir.shape[0], o.SR)[0]
    ferr = (np.abs(dense - fd.numpy()) / np.maximum(1.0, np.abs(fd.numpy()))).max()
    print(f"room K={K} alpha_bias={alpha_bias} [{prec}]: max |rgb - oracle| = {err:.3e}, max feature error {ferr:.3e}")
    assert err <= rgb_tol and ferr <= feat_tol
    assert int(mask.sum()) > 0.5 * mask.numel()
    # blend weights per (sample, slot): the oracle's linear-kernel weights x clamped conf
    dense_b = np.zeros((view.raydir.shape[0], o.SR, K), np.float32)
    _, sr, slot, valid = _dense_feat(out, view.raydir.shape[0], o.SR)
    dense_b[sr[valid], slot[valid]] = out.blend[:len(valid)].cpu().numpy()[valid]
    pid = q["pidx"]
    d = pid >= 0
    lw = np.linalg.norm(pc.xyz[np.maximum(pid, 0)] - q["loc_w"][..., None, :], axis=-1)
    w = np.where(d, 1.0 / np.maximum(lw, 1e-6), 0.0)
    w = w / np.maximum(w.sum(-1, keepdims=True), 1e-8)
    ref_b = w * np.clip(pc.conf.reshape(-1)[np.maximum(pid, 0)], 1e-4, 1.0)
    np.testing.assert_allclose(dense_b[mask.numpy()], ref_b[mask.numpy()], atol=1e-5, rtol=1e-4)


@pytest.mark.parametrize("theta,alpha_bias", [(30.0, 0.0), (200.0, 150.0)])
def test_render_matches_oracle_lego(theta, alpha_bias):
    """BASELINE config 4 at test size: the NeRF-synthetic camera model
    (get_blender_raydir data_utils.py:41-53, pose_spherical load_blender.py:51-56, near 2,
    far 6) over the lego stand-in cloud, SR = 128: ray masks bit-exact, RGB and decoded features
    within the f32 mode's 1e-5."""
    pc = scene.lego_standin(120_000, seed=4)
    o = HotPathOpts(SR=128)
    mlp = init_mlp(4, bias_std=0.01)
    mlp["alpha_branch.0.bias"] = mlp["alpha_branch.0.bias"] + alpha_bias
    view = scene.lego_view(theta, h=40, w=40, focal=1111.1111 * 40 / 800)
    pts = dict(xyz=pc.xyz, embedding=pc.embedding, color=pc.color, dir=pc.dir, conf=pc.conf)
    r, out = _render(pts, mlp, view, o)
    hy = hyper_for(pc, o)
    tt = r.querier.depth_table(view.near, view.far, 0)[0].cpu().numpy()
    q = oq.OracleGrid(pc.xyz, hy, o).query(view.campos, view.raydir, tt)
    tp = {k: torch.from_numpy(v) for k, v in pts.items()}
    with torch.no_grad():
        full, mask, fd, opacity, bg_t = agg_ref.render(tp, mlp, torch.from_numpy(view.campos),
                                                       torch.from_numpy(view.camrotc2w), torch.from_numpy(view.raydir), q, 128)
    np.testing.assert_array_equal(out.ray_mask.cpu().numpy().astype(bool), mask.numpy())
    err = np.abs(out.rgb.cpu().numpy() - full.numpy()).max()
    ns = out.query.ray_ns[:view.raydir.shape[0]].cpu().numpy()
    dense = _dense_feat(out, view.raydir.shape[0], 128)[0]
    ferr = (np.abs(dense - fd.numpy()) / np.maximum(1.0, np.abs(fd.numpy()))).max()
    print(f"lego theta={theta}: max |rgb - oracle| = {err:.3e}, max feature error {ferr:.3e}, valid rays "
          f"{int(mask.sum())}/{mask.numel()}, max samples/ray {ns.max()}")
    assert err <= F32_TOL and ferr <= F32_TOL        # the default precision is the reference's fp32
    assert int(mask.sum()) > 0.2 * mask.numel()


# ---- SG-NeRF block2_bpnet variant -------------------------------------------------------
GOLD_SG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_sg.npz")


@pytest.mark.parametrize("prec", ["f32", "f16", "exact"])
@pytest.mark.parametrize("name", ["sg96", "sg0"])
def test_render_sg_matches_reference_golden(name, prec):
    """block2_bpnet (point_aggregators.py:345-354, :629-636) in the fused kernel vs the
    reference's own SG aggregator.  Labels are all 0, which passes the semantic filter
    (worldcoords.py:548-553), so the query equals the golden's plain query."""
    g = np.load(GOLD_SG, allow_pickle=False)
    ps = 1 if name == "sg96" else 0
    mlp = {k[len(f"mlp_{name}/"):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(f"mlp_{name}/")}
    pts = PointTables(*(g[f"sgpatch/{k}"] for k in ("xyz", "embedding", "color", "dir", "conf")), DEV,
                      bpnet=g["sgpatch/bpnet"] if ps else None)
    o = _opts(prec, SR=int(g[f"{name}/SR"]), shading_feature_mlp_layer2_bpnet=1, predict_semantic=ps,
              semantic_guidance=ps)
    rgb_tol, feat_tol = TOL[prec]
    near, far = (float(x) for x in g[f"{name}/near_far"])
    raydir = torch.from_numpy(g[f"{name}/raydir"])
    R = raydir.shape[0]
    r = HipRenderer(pts, mlp, o, DEV)
    r.exact = prec == "exact"
    kw = {}
    if ps:
        kw = dict(point_labels=torch.zeros(pts.n, dtype=torch.int32, device=DEV),
                  ray_labels=torch.zeros(R, dtype=torch.int32, device=DEV), seconds=5)
    out = r.render(torch.from_numpy(g[f"{name}/campos"]), torch.from_numpy(g[f"{name}/camrotc2w"]), raydir,
                   near, far, **kw)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.ray_mask.cpu().numpy(), g[f"{name}/ray_mask"])
    err = np.abs(out.rgb.cpu().numpy() - g[f"{name}/full_color"]).max()
    print(f"{name} [{prec}]: max |rgb - reference| = {err:.3e}")
    assert err <= rgb_tol
    dense = _dense_feat(out, R, o.SR)[0]
    keep = g[f"{name}/ray_mask"].astype(bool)
    ref = g[f"{name}/decoded"]
    ferr = (np.abs(dense[keep] - ref) / np.maximum(1.0, np.abs(ref))).max()
    print(f"{name} [{prec}]: max |decoded - reference| / max(1, |ref|) = {ferr:.3e}")
    assert ferr <= feat_tol


def test_render_sg_semantic_matches_oracle_room():
    """SG end to end on a room: semantic-guided kNN with real labels + block2_bpnet(352)."""
    pc = scene.with_semantics(small_room(300_000, seed=5), seed=6, n_classes=4)
    o = HotPathOpts(SR=32, shading_feature_mlp_layer2_bpnet=1, predict_semantic=1, semantic_guidance=1)
    mlp = init_mlp(5, bias_std=0.01, bpnet_layers=1, bpnet_dim=96)
    mlp["alpha_branch.0.bias"] = mlp["alpha_branch.0.bias"] + 150.0
    view = make_view(48, 64, yaw=75.0, pitch=-6.0)
    R = view.raydir.shape[0]
    ray_labels = np.random.default_rng(7).integers(0, 4, R).astype(np.int32)
    secs = 12  # seconds % 10 = 2 > 1: the label filter is active (worldcoords.py:553)
    r = HipRenderer(PointTables(pc.xyz, pc.embedding, pc.color, pc.dir, pc.conf, DEV, bpnet=pc.bpnet), mlp, o, DEV)
    out = r.render(torch.from_numpy(view.campos), torch.from_numpy(view.camrotc2w), torch.from_numpy(view.raydir),
                   view.near, view.far, point_labels=torch.from_numpy(pc.labels).to(DEV),
                   ray_labels=torch.from_numpy(ray_labels).to(DEV), seconds=secs)
    torch.cuda.synchronize()
    hy = hyper_for(pc, o)
    q = oq.OracleGrid(pc.xyz, hy, o).query(view.campos, view.raydir, r.querier.depth_table(0.1, 8.0, 0)[0].cpu().numpy(),
                                           point_labels=pc.labels, ray_labels=ray_labels, seconds=secs)
    tp = {k: torch.from_numpy(getattr(pc, k)) for k in ("xyz", "embedding", "color", "dir", "conf", "bpnet")}
    with torch.no_grad():
        full, mask, fd, opacity, bg_t = agg_ref.render(tp, mlp, torch.from_numpy(view.campos),
                                                       torch.from_numpy(view.camrotc2w), torch.from_numpy(view.raydir), q, o.SR)
    np.testing.assert_array_equal(out.ray_mask.cpu().numpy().astype(bool), mask.numpy())
    err = np.abs(out.rgb.cpu().numpy() - full.numpy()).max()
    dense = _dense_feat(out, R, o.SR)[0]
    ferr = (np.abs(dense - fd.numpy()) / np.maximum(1.0, np.abs(fd.numpy()))).max()
    print(f"SG room: max |rgb - oracle| = {err:.3e}, max feature error {ferr:.3e}, "
          f"valid rays {int(mask.sum())}/{mask.numel()}")
    assert err <= F32_TOL and ferr <= F32_TOL
    assert int(mask.sum()) > 0.5 * mask.numel()


def test_render_without_hits_is_background():
    """No ray reaches an occupied voxel (camera outside the room, looking away): zero work items
    reach the aggregator kernels; every ray is invalid and gets the white background
    (fill_invalid, neural_points_volumetric_model.py:158-195)."""
    pc = small_room(50_000, seed=2)
    o = HotPathOpts(SR=24)
    mlp = init_mlp(2, bias_std=0.01)
    view = make_view(16, 24, yaw=45.0, pitch=0.0, campos=(9.0, 9.0, 1.5))
    pts = dict(xyz=pc.xyz, embedding=pc.embedding, color=pc.color, dir=pc.dir, conf=pc.conf)
    r, out = _render(pts, mlp, view, o)
    assert int(out.query.counters[1]) == 0
    assert not bool(out.ray_mask.any())
    assert torch.equal(out.rgb.cpu(), torch.ones(view.raydir.shape[0], 3))
    assert torch.equal(out.bg_transmission.cpu(), torch.ones(view.raydir.shape[0]))


def _full_frame_check(pc, o, mlp, view, stride, min_work):
    """A full-size frame checked through size-independent properties: (1) rays are independent --
    the frame's values on a strided subset equal a render of those rays alone, bit for bit; (2) the
    renderer's grid equals the oracle's reference-format grid (coor_occ, coor_2_occ, the occupancy
    lists and counts) bit for bit at the full point count; (3) on the subset the query (ray_ns,
    sample_pidx, samp_d, sample_loc_w, neighbour counts, work list) is bit-exact against the oracle
    and RGB, background transmission and decoded features are within the f32 mode's 1e-5."""
    pts = dict(xyz=pc.xyz, embedding=pc.embedding, color=pc.color, dir=pc.dir, conf=pc.conf)
    r = HipRenderer(PointTables(pts["xyz"], pts["embedding"], pts["color"], pts["dir"], pts["conf"], DEV), mlp, o, DEV)
    cam = (torch.from_numpy(view.campos), torch.from_numpy(view.camrotc2w))
    full = r.render(*cam, torch.from_numpy(view.raydir), view.near, view.far)
    rgb_full, mask_full = full.rgb.clone(), full.ray_mask.clone()
    n_work = int(full.query.counters[1])
    assert n_work > min_work
    h, w = view.h, view.w
    idx = np.arange(h * w).reshape(h, w)[::stride, ::stride].reshape(-1)
    sub = r.render(*cam, torch.from_numpy(view.raydir[idx]), view.near, view.far)
    ti = torch.from_numpy(idx).to(DEV)
    assert torch.equal(sub.ray_mask, mask_full[ti])
    assert torch.equal(sub.rgb, rgb_full[ti])
    hy = hyper_for(pc, o)
    og = oq.OracleGrid(pc.xyz, hy, o)
    check_grid(r.querier.grid_for(r.points.xyz), og)
    rd = np.ascontiguousarray(view.raydir[idx])
    q = og.query(view.campos, rd, r.querier.depth_table(view.near, view.far, 0)[0].cpu().numpy())
    S = check_query_sample_major(sub.query, q, len(idx), o.K)
    tp = {k: torch.from_numpy(v) for k, v in pts.items()}
    with torch.no_grad():
        ref, mask, fd, _, bg_t = agg_ref.render(tp, mlp, torch.from_numpy(view.campos),
                                                torch.from_numpy(view.camrotc2w), torch.from_numpy(rd), q, o.SR)
    np.testing.assert_array_equal(sub.ray_mask.cpu().numpy().astype(bool), mask.numpy())
    err = float((sub.rgb.cpu() - ref).abs().max())
    berr = float((sub.bg_transmission.cpu()[mask] - bg_t[mask]).abs().max())
    dense = _dense_feat(sub, len(idx), o.SR)[0]
    ferr = float((np.abs(dense - fd.numpy()) / np.maximum(1.0, np.abs(fd.numpy()))).max())
    print(f"full frame {h}x{w} SR {o.SR}: {n_work} work items; subset of {len(idx)} rays ({S} samples, query "
          f"bit-exact): max |rgb - oracle| {err:.3e}, |bgT - oracle| {berr:.3e}, feature error {ferr:.3e}")
    assert err <= F32_TOL and berr <= F32_TOL and ferr <= F32_TOL
    return n_work


def test_full_frame_config2_properties():
    """BASELINE config 2 at full size (synth-room, 1.2 M points, 800x800 rays, SR 64, the default
    f32 precision): _full_frame_check on a strided 100x100 subset (the oracle's query + torch
    restatement finish in seconds at 10 k rays)."""
    pc = scene.synth_room(1_200_000, seed=0)
    o = HotPathOpts(SR=64)
    mlp = init_mlp(0, bias_std=0.01)
    mlp["alpha_branch.0.bias"] = mlp["alpha_branch.0.bias"] + 50.0
    view = scene.room_view(800, 800, yaw=15.0, pitch=-5.0)
    _full_frame_check(pc, o, mlp, view, 8, 2_000_000)   # ~5 occupied samples per ray over most of the frame


def test_full_frame_config4_lego_properties():
    """BASELINE config 4 at full size: the lego stand-in (300 k points), the NeRF-synthetic camera
    (focal 1111.1, pose_spherical load_blender.py:51-56, near 2, far 6), 800x800 rays, SR 128 --
    the bench's workload -- checked by _full_frame_check on a strided 50x50 subset (lego has ~100
    neighbours per ray, so the CPU restatement of 2.5 k rays is the affordable sample)."""
    pc = scene.lego_standin(300_000, seed=0)
    o = HotPathOpts(SR=128)
    mlp = init_mlp(0, bias_std=0.01)
    mlp["alpha_branch.0.bias"] = mlp["alpha_branch.0.bias"] + 50.0
    view = scene.lego_view(75.0, 800, 800)
    _full_frame_check(pc, o, mlp, view, 16, 500_000)


def test_render_vid_config3_spiral_matches_oracle(tmp_path):
    """BASELINE config 3 through its driver (render_vid.main, run/render_vid.py:26-69): an
    8-frame spiral at 800x800, SR 24, over the 1.2M-point room with the opaque aggregator,
    rendered and written; every 97th ray of each frame (offset by the frame index) is checked
    against the oracle (C query + torch fp32 aggregator / ray_march): RGB within the f32
    mode's 1e-5 (a missed or extra ray would show as a background-coloured error), and the
    written float16 stack equals the frames to fp16 rounding."""
    from sgnerf_amd import raygen, render_vid
    H = W = 800
    frames, ms = render_vid.main(["--frames", "8", "--h", str(H), "--w", str(W), "--sr", "24", "--out",
                                  str(tmp_path)])
    assert frames.shape == (8, H * W, 3) and ms > 0
    stack = np.load(tmp_path / "frames.npy")
    assert stack.shape == (8, H, W, 3) and (tmp_path / "frame_0007.png").exists()
    fr = frames.cpu().numpy()
    np.testing.assert_allclose(stack.reshape(8, -1, 3).astype(np.float32), fr, atol=2.5e-4, rtol=0)
    pc, mlp = render_vid.default_scene()
    o = HotPathOpts(SR=24)
    og = oq.OracleGrid(pc.xyz, hyper_for(pc, o), o)
    tp = {k: torch.from_numpy(getattr(pc, k)) for k in ("xyz", "embedding", "color", "dir", "conf")}
    tt = raygen.depth_table(0.1, 8.0, o.z_depth_dim).numpy()
    worst, n_valid, n_rays, bgt_med = 0.0, 0, 0, []
    for f, v in enumerate(render_vid.spiral_views(8, H, W)):
        idx = np.arange(f, H * W, 97)
        rd = np.ascontiguousarray(v.raydir[idx])
        q = og.query(v.campos, rd, tt)
        with torch.no_grad():
            full, mask, fd, opacity, bg_t = agg_ref.render(tp, mlp, torch.from_numpy(v.campos),
                                                           torch.from_numpy(v.camrotc2w), torch.from_numpy(rd), q, 24)
        err = float(np.abs(fr[f, idx] - full.numpy()).max())
        worst = max(worst, err)
        n_valid += int(mask.sum())
        n_rays += len(idx)
        bgt_med.append(float(bg_t[mask].median()))
        assert err <= F32_TOL, (f, err)          # render_vid runs the f32 (reference-precision) mode
    print(f"config 3: 8 frames {H}x{W} in {ms:.1f} ms; {n_rays} rays checked, {n_valid} valid, "
          f"max |rgb - oracle| {worst:.3e}, median bg_transmission per frame {np.round(bgt_med, 3).tolist()}")
    assert n_valid > 0.9 * n_rays
    assert max(bgt_med) <= 0.5


def test_dense_stress_scene_matches_oracle():
    """SURVEY §8d dense stress variant at full size: 3.9 M points in a 1 m cube, 800x800 rays
    face-on, SR 64 (every candidate inside the cube occupied with K neighbours), the
    reference-precision mode; every 997th ray against the oracle: ray mask bit-exact, RGB and
    background transmission within the f32 mode's 1e-5."""
    pc = scene.dense_cube(3_900_000, seed=0)
    o = HotPathOpts(SR=64)
    mlp = init_mlp(5, bias_std=0.01)
    mlp["alpha_branch.0.bias"] = mlp["alpha_branch.0.bias"] + 50.0
    view = scene.dense_stress_view(800, 800)
    pts = dict(xyz=pc.xyz, embedding=pc.embedding, color=pc.color, dir=pc.dir, conf=pc.conf)
    r, out = _render(pts, mlp, view, o)
    idx = np.arange(3, 800 * 800, 997)
    rd = np.ascontiguousarray(view.raydir[idx])
    q = oq.OracleGrid(pc.xyz, hyper_for(pc, o), o).query(view.campos, rd,
                                                         r.querier.depth_table(0.1, 8.0, 0)[0].cpu().numpy())
    tp = {k: torch.from_numpy(v) for k, v in pts.items()}
    with torch.no_grad():
        full, mask, fd, opacity, bg_t = agg_ref.render(tp, mlp, torch.from_numpy(view.campos),
                                                       torch.from_numpy(view.camrotc2w), torch.from_numpy(rd), q, 64)
    np.testing.assert_array_equal(out.ray_mask.cpu().numpy()[idx].astype(bool), mask.numpy())
    err = np.abs(out.rgb.cpu().numpy()[idx] - full.numpy()).max()
    berr = np.abs(out.bg_transmission.cpu().numpy()[idx][mask.numpy()] - bg_t[mask].numpy()).max()
    S = out.query.n_samples()
    nb = int(out.query.samp_nnb[:S].sum())
    print(f"dense stress: {S / 640000:.1f} samples/ray, {nb / 640000:.1f} neighbours/ray; subset of {len(idx)} rays: "
          f"max |rgb - oracle| {err:.3e}, max |bgT - oracle| {berr:.3e}")
    assert err <= F32_TOL and berr <= F32_TOL
    assert nb / 640000 > 150


def _render_pair_modes(monkeypatch, make):
    """Two renders of the same input, k_rows16's sample pairing on (default) and off (SGN_PAIR=0)."""
    outs = []
    for mode in ("1", "0"):
        monkeypatch.setenv("SGN_PAIR", mode)
        r, out, n_items = make()
        q = out.query
        S = q.n_samples()
        valid = (q.samp_nnb[:S] > 0).cpu()
        outs.append((out.rgb.clone(), out.opacity.clone(), out.bg_transmission.clone(), out.feat[:S][valid].clone(),
                     out.blend[:S][valid].clone()))
    return outs, n_items


@pytest.mark.parametrize("case", ["patch", "room", "sg96"])
def test_paired_rows_bit_identical_to_unpaired(monkeypatch, case):
    """k_rows16 packs two samples whose neighbour counts sum to <= 8 into one 8-row half (sample B at
    row max(nA, 4)); the weight normalisation, K-blend and alpha are arranged so each sample gets the
    bits it gets alone.  A render with pairing equals one without (SGN_PAIR=0), bit for bit: the
    frame's colour, opacity, transmission, per-sample (alpha, rgb) and blend weights.  The golden
    patch has 1,131 B samples among 2,925 work items."""
    def make():
        if case == "patch":
            pts, mlp, c = load_golden("reference_aggregator.npz", "patch")
            near, far = (float(x) for x in c["near_far"])
            view = scene.View(c["campos"], c["camrotc2w"], c["raydir"], None, None, 0, 0, near, far)
            o = HotPathOpts(SR=int(c["SR"]), K=int(c["K"]))
            r, out = _render(pts, mlp, view, o)
            kw = {}
        elif case == "room":
            pc = small_room(300_000, seed=4)
            mlp = init_mlp(4, bias_std=0.01)
            mlp["alpha_branch.0.bias"] = mlp["alpha_branch.0.bias"] + 50.0
            view = make_view(64, 96, yaw=75.0, pitch=-12.0)
            pts = dict(xyz=pc.xyz, embedding=pc.embedding, color=pc.color, dir=pc.dir, conf=pc.conf)
            r, out = _render(pts, mlp, view, HotPathOpts(SR=64))
        else:
            g = np.load(GOLD_SG, allow_pickle=False)
            mlp = {k[len("mlp_sg96/"):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("mlp_sg96/")}
            pts = PointTables(*(g[f"sgpatch/{k}"] for k in ("xyz", "embedding", "color", "dir", "conf")), DEV,
                              bpnet=g["sgpatch/bpnet"])
            o = HotPathOpts(SR=int(g["sg96/SR"]), shading_feature_mlp_layer2_bpnet=1, predict_semantic=1,
                            semantic_guidance=1)
            near, far = (float(x) for x in g["sg96/near_far"])
            raydir = torch.from_numpy(g["sg96/raydir"])
            R = raydir.shape[0]
            r = HipRenderer(pts, mlp, o, DEV)
            out = r.render(torch.from_numpy(g["sg96/campos"]), torch.from_numpy(g["sg96/camrotc2w"]), raydir, near, far,
                           want_blend=True, point_labels=torch.zeros(pts.n, dtype=torch.int32, device=DEV),
                           ray_labels=torch.zeros(R, dtype=torch.int32, device=DEV), seconds=5)
        torch.cuda.synchronize()
        return r, out, int(out.query.counters[1])
    (on, off), n_items = _render_pair_modes(monkeypatch, make)
    assert n_items > 100
    for name, a, b in zip(("rgb", "opacity", "bg_transmission", "feat", "blend"), on, off):
        assert torch.equal(a, b), name


def test_pair_slots_tables():
    """k_pair_slots' tables after a config-2-like room frame (white box: the f32 aggregate workspace
    is [f_s 1 KiB | rows 32 B | entry 16 B] per item + a 2-KiB tail holding the slot count): every work
    item is sample A or B of exactly one slot, nA + nB <= 8, B's rows start at max(nA, 4), the row
    table holds s * 8 + k for exactly the sample's valid neighbour slots (pidx >= 0) and -1 elsewhere,
    and pairing packs the frame into fewer slots than work items."""
    pc = small_room(300_000, seed=5)
    mlp = init_mlp(5, bias_std=0.01)
    view = make_view(96, 128, yaw=200.0, pitch=-10.0)
    pts = dict(xyz=pc.xyz, embedding=pc.embedding, color=pc.color, dir=pc.dir, conf=pc.conf)
    r, out = _render(pts, mlp, view, HotPathOpts(SR=64))
    q = out.query
    nw = int(q.counters[1])
    ws = r.agg_ws
    wsi = (ws.numel() - 2048) // (1024 + 48)
    ns = int(ws[-2048:-2044].view(torch.int32).item())
    rows = ws[wsi * 1024: wsi * 1056].view(torch.int32).cpu().numpy().reshape(-1, 8)[:ns]
    ent = ws[wsi * 1056: wsi * 1072].view(torch.int32).cpu().numpy().reshape(-1, 4)[:ns]
    work = q.work[:nw].cpu().numpy()
    nnb = q.samp_nnb.cpu().numpy()
    pidx = q.pidx.cpu().numpy()
    assert 0 < ns < nw
    seen = np.zeros(nw, np.int32)
    for j in range(ns):
        ea, eb, sa, sb = (int(x) & 0xFFFFFFFF for x in ent[j])
        ia, na, ib, nb_ = ea & 0x0FFFFFFF, ea >> 28, eb & 0x0FFFFFFF, eb >> 28
        assert work[ia] == sa and na == nnb[sa] and 1 <= na <= 8
        seen[ia] += 1
        want = [sa * 8 + k if k < na else -1 for k in range(8)]
        if nb_:
            assert work[ib] == sb and nb_ == nnb[sb] and na + nb_ <= 8
            seen[ib] += 1
            ob = max(na, 4)
            assert ob + nb_ <= 8
            for k in range(nb_):
                want[ob + k] = sb * 8 + k
        assert list(rows[j]) == want, j
        for v in want:
            if v >= 0:
                assert pidx[v] >= 0
    assert (seen == 1).all()
    # the valid slots of every work item are a prefix of its K slots (what the pairing relies on)
    pw = pidx[(work[:, None] * 8 + np.arange(8)[None, :])]
    assert ((pw >= 0) == (np.arange(8)[None, :] < nnb[work][:, None])).all()


def test_f32_fp16_range_falls_back_to_plain_fp32():
    """The f32 mode carries activations as fp16 hi/lo pairs (mlp_x3.hip header), so |x| >= 65504
    cannot be represented there.  With block1.2's weights scaled x 30000 the hidden activations of
    the golden patch exceed 1e5 (checked on the oracle's restatement).  The reference returns a
    value (fp32 nn.Linear), and so must the renderer: the synchronous check re-renders the frame on
    the plain-fp32 path (sgn_aggregate_exact) -- RGB and decoded features within 1e-5 (relative to
    max(1, |value|)) of the oracle on the golden patch's neighbours -- and later frames take that
    path directly.  A frame loop's deferred check raises for the frame it finds flagged (its output
    was handed out) and switches the renderer too.  PointAggregator recovers the same way.  The
    unscaled weights never leave the split path."""
    from sgnerf_amd import _lib
    from sgnerf_amd.ray_marching import PointAggregator
    pts, mlp, c = load_golden("reference_aggregator.npz", "patch")
    near, far = (float(x) for x in c["near_far"])
    view = scene.View(c["campos"], c["camrotc2w"], c["raydir"], None, None, 0, 0, near, far)
    o = HotPathOpts(SR=int(c["SR"]), K=int(c["K"]))
    big = dict(mlp)
    big["block1.2.weight"] = mlp["block1.2.weight"] * 30000.0
    # the scaled block1.2 output (block3.0's input) on the oracle's restatement: above fp16's range
    seen = {}
    lin = agg_ref._lin

    def spy(m, name, x):
        y = lin(m, name, x)
        seen[name] = max(seen.get(name, 0.0), float(y.abs().max()))
        return y
    K = int(c["K"])
    pidx = torch.from_numpy(c["sample_pidx"]).reshape(-1, K).long()
    keep = c["ray_mask"].astype(bool)
    sr = torch.arange(int(keep.sum())).repeat_interleave(int(c["SR"]))
    tp = {k: torch.from_numpy(v) for k, v in pts.items()}
    locw = torch.from_numpy(c["sample_loc_w"]).reshape(-1, 3)
    agg_ref._lin = spy
    try:
        with torch.no_grad():
            agg_ref.aggregate(tp, big, torch.from_numpy(view.campos), torch.from_numpy(view.camrotc2w),
                              torch.from_numpy(view.raydir[keep]), sr, locw, pidx)
    finally:
        agg_ref._lin = lin
    assert seen["block1.2"] > 1e5, seen
    tab = PointTables(pts["xyz"], pts["embedding"], pts["color"], pts["dir"], pts["conf"], DEV)
    args = (torch.from_numpy(view.campos), torch.from_numpy(view.camrotc2w), torch.from_numpy(view.raydir), near, far)
    ok = HipRenderer(tab, mlp, o, DEV)
    ok.render(*args)
    ok.render(*args, check_range="deferred")
    ok.finish()
    assert not ok.exact
    # the oracle on the renderer's own query (same neighbours, same sample positions)
    bad = HipRenderer(tab, big, o, DEV)
    out = bad.render(*args)
    assert bad.exact
    R = view.raydir.shape[0]
    qd = {"pidx": out.query.pidx, "ray_ns": out.query.ray_ns[:R].cpu().numpy()}
    S = out.query.n_samples()
    samp_ray = out.query.samp_ray[:S].long().cpu()
    spidx = out.query.pidx[:S * K].view(S, K).long().cpu()
    slocw = out.query.samp_locw[:S * 3].view(S, 3).cpu()
    with torch.no_grad():
        fref, _ = agg_ref.aggregate(tp, big, torch.from_numpy(view.campos), torch.from_numpy(view.camrotc2w),
                                    torch.from_numpy(view.raydir), samp_ray, slocw, spidx)
    valid = (spidx >= 0).any(-1)
    feat = out.feat[:S].cpu()[valid]

    def rel(a, b):
        return float(((a - b).abs() / torch.clamp(b.abs(), min=1.0)).max())
    ferr = rel(feat, fref[valid])
    # x30000 weights make block3.0's sums cancel over activations ~1e5: fp32's own summation-order noise
    # on this input is far above 1e-5 -- measured as the same oracle evaluated by torch on the GPU
    # against the CPU; the plain-fp32 path is held to a few times that floor
    with torch.no_grad():
        fgpu, _ = agg_ref.aggregate({k: v.to(DEV) for k, v in tp.items()}, {k: v.to(DEV) for k, v in big.items()},
                                    torch.from_numpy(view.campos).to(DEV), torch.from_numpy(view.camrotc2w).to(DEV),
                                    torch.from_numpy(view.raydir).to(DEV), samp_ray.to(DEV), slocw.to(DEV),
                                    spidx.to(DEV))
    floor = rel(fgpu.cpu()[valid], fref[valid])
    assert bool(torch.isfinite(out.rgb).all())
    print(f"x30000 block1.2 on the plain-fp32 path: max feature error {ferr:.3e}, fp32 floor (torch GPU vs CPU) "
          f"{floor:.3e} (|alpha| up to {float(fref[valid][:, 0].abs().max()):.3e})")
    assert ferr <= max(F32_TOL, 4.0 * floor)
    # the composite of those features: the golden path's own ray_march restatement
    with torch.no_grad():
        nnb = (spidx >= 0).sum(-1)
        fd, vd, ld = agg_ref.densify(R, o.SR, out.query.ray_ns[:R].long().cpu(),
                                     samp_ray, slocw, fref, nnb)
        color, _, _ = agg_ref.composite(fd, vd, ld, torch.from_numpy(view.camrotc2w), torch.from_numpy(view.campos))
    full = torch.where(vd.any(-1)[:, None], color, torch.ones_like(color))
    err = float((out.rgb.cpu() - full).abs().max())
    print(f"x30000 block1.2: max |rgb - oracle| = {err:.3e}")
    assert err <= max(F32_TOL, 4.0 * floor)
    out2 = bad.render(*args)   # later frames: the plain-fp32 path directly, the same result
    assert torch.equal(out2.rgb.cpu(), out.rgb.cpu())
    # a pipelined frame loop: the deferred check raises for the flagged frame and switches the renderer
    loop = HipRenderer(tab, big, o, DEV)
    loop.render(*args, check_range="deferred")
    with pytest.raises(_lib.SgnError, match="fp16 range"):
        loop.finish()
    assert loop.exact
    out3 = loop.render(*args, check_range="deferred")
    loop.finish()
    assert torch.equal(out3.rgb.cpu(), out.rgb.cpu())
    # PointAggregator (the sub-boundary) on the golden patch's gathered neighbours: the same recovery
    from test_api_gpu import _gathered
    agg = PointAggregator(big, o, DEV)
    dec, valid_a, _, _ = agg(**_gathered(pts, c))
    Rk, SRk = c["sample_pidx"].shape[:2]
    with torch.no_grad():
        fagg_ref, _ = agg_ref.aggregate(tp, big, torch.from_numpy(view.campos), torch.from_numpy(view.camrotc2w),
                                        torch.from_numpy(view.raydir[keep]), torch.arange(Rk).repeat_interleave(SRk),
                                        locw, pidx)
    fa = dec[0].reshape(-1, 4).cpu()
    v = (pidx >= 0).any(-1)
    aerr = float(((fa[v] - fagg_ref[v]).abs() / torch.clamp(fagg_ref[v].abs(), min=1.0)).max())
    print(f"x30000 block1.2, PointAggregator: max feature error {aerr:.3e}")
    assert aerr <= max(F32_TOL, 4.0 * floor)



@pytest.mark.parametrize("n_points,S,K", [(1_200_000, 300_000, 8), (5, 3, 1), (1_001, 7, 3)])
def test_frame_points_lists_the_named_points(n_points, S, K):
    """sgn_frame_points (the f32 renderer's projection subset): point 0 and every neighbour slot >= 0 of
    the first S samples, once each (slots past S * K ignored, ids >= n_points counted, not listed);
    the marks are left zero, so a second frame on the same buffers lists its own points only."""
    import ctypes
    from sgnerf_amd import _lib
    L = _lib.lib()
    g = torch.Generator().manual_seed(n_points + S)
    marks = torch.zeros(int(L.sgn_frame_points_mark_bytes(n_points)), dtype=torch.uint8, device=DEV)
    lst = torch.empty(n_points, dtype=torch.int32, device=DEV)
    cnt = torch.zeros(2, dtype=torch.int64, device=DEV)
    for frame in range(2):
        pidx = torch.randint(-1, min(n_points, 50_000 * (frame + 1)), ((S + 9) * K,), generator=g, dtype=torch.int32)
        pidx[S * K:] = n_points - 1                       # past the sample count: never read
        if n_points > 10:
            pidx[5] = n_points + 3                        # a query / table mismatch: counted only
        counters = torch.tensor([S, 0, 0, 0], dtype=torch.int32)
        pidx_d, counters_d = pidx.to(DEV), counters.to(DEV)   # alive until the launch has run
        _lib.check(L.sgn_frame_points(_lib.ptr(pidx_d), _lib.ptr(counters_d), S + 9, K, n_points,
                                      _lib.ptr(marks), _lib.ptr(lst), _lib.ptr(cnt), _lib.stream_handle()),
                   "sgn_frame_points")
        torch.cuda.synchronize()
        used = pidx[:S * K]
        used = used[(used >= 0) & (used < n_points)].long()
        want = torch.unique(torch.cat([used, torch.zeros(1, dtype=torch.long)]))
        n = int(cnt[0].item())
        assert n == want.numel()
        assert torch.equal(torch.sort(lst[:n].long().cpu()).values, want)
        assert int(cnt[1].item()) == (frame + 1 if n_points > 10 else 0)
        assert int(marks.count_nonzero().item()) == 0


@pytest.mark.parametrize("n", [5, 1001])   # less than one tile; no multiple of the 32- / 16 * NW16-point tile
@pytest.mark.parametrize("prec", ["f16", "f32"])
def test_point_project_list(prec, n):
    """sgn_point_project(_f32) over a device list: a permutation of every index equals the NULL / NULL
    call byte for byte, a strict subset writes its rows only, a zero count writes nothing."""
    import ctypes

    from sgnerf_amd import _lib
    from sgnerf_amd.weights import pack_mlp
    L = _lib.lib()
    f32 = prec == "f32"
    g = torch.Generator().manual_seed(n)
    tab = {k: (0.3 * torch.randn(n, w, generator=g)).to(DEV) for k, w in
           (("xyz", 3), ("embedding", 32), ("color", 3), ("dir", 3), ("conf", 1))}
    pt = _lib.PointTables()
    for k, t in tab.items():
        setattr(pt, k, t.data_ptr())
    pt.n_points = n
    packed = pack_mlp(init_mlp(0), DEV, prec)
    project = L.sgn_point_project_f32 if f32 else L.sgn_point_project
    nbytes = int((L.sgn_point_proj_bytes_f32 if f32 else L.sgn_point_proj_bytes)(n))
    rec = 64 if f32 else 0                    # f32: a 64-B record per point after the P rows
    row = nbytes // n - rec
    FILL = 0xA5

    def run(idx=None, count=None):
        proj = torch.full((nbytes,), FILL, dtype=torch.uint8, device=DEV)
        cnt = None if count is None else torch.tensor([count], dtype=torch.int64, device=DEV)
        _lib.check(project(ctypes.byref(pt), _lib.ptr(packed), _lib.ptr(idx), _lib.ptr(cnt), _lib.ptr(proj),
                           _lib.stream_handle()), "point projection")
        torch.cuda.synchronize()
        proj = proj.cpu()
        return torch.cat([proj[:n * row].view(n, row), proj[n * row:].view(n, rec)], dim=1)   # per point

    full = run()
    assert bool((full != FILL).any(dim=1).all())            # every point's row written
    perm = torch.randperm(n, generator=g).to(torch.int32)
    assert torch.equal(run(perm.to(DEV), n), full)
    part = perm[:n // 2]
    out = run(part.to(DEV), part.numel())
    listed = torch.zeros(n, dtype=torch.bool)
    listed[part.long()] = True
    assert 0 < int(listed.sum()) < n
    assert torch.equal(out[listed], full[listed])
    assert bool((out[~listed] == FILL).all())
    assert bool((run(perm.to(DEV), 0) == FILL).all())
