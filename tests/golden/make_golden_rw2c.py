"""Generates tests/golden/reference_rw2c.npz: rotated neural points (a non-identity Rw2c) run by the
reference's own PointAggregator and ray_march, as make_golden.py does for the unrotated cases
(same container-only imports, neighbour indices from the oracle, every float from the reference).

make_golden.make_case hard-codes Rw2c = eye(3); it is restated here with the NeuralPoints gather of
the matrix (neural_points.py:967): sampled_Rw2c = index_select(Rw2c, 0, clamp(pidx, 0)) as
[B,R,SR,K,3,3], or the [3,3] matrix itself.  viewmlp applies it at point_aggregators.py:565-569, :579,
:599 and :648.

Scene: scene.room_corner(20000, 1) from make_golden's corner_view (16 x 16 rays) with the alpha bias
OPAQUE_BIAS -- reference_opaque.npz's `sparse32` setting, partial K on most samples -- and that
file's aggregator weights (asserted equal here, so this file stores none).  The cloud is stored as its
generator call plus checksum.  The rotations are a palette [4,3,3] plus a uint8 index per point.

Usage:  python -B tests/golden/make_golden_rw2c.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

MIN_SHIFT = 1e-2   # max |decoded - decoded with identity| every case must reach


def axis_angle(axis, deg):
    """Rodrigues' formula in float64."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    t = np.deg2rad(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def palette():
    return np.stack([np.eye(3), axis_angle((0, 0, 1), 40.0), axis_angle((1, 2, 3), 75.0),
                     axis_angle((-1, 1, 0.5), 170.0)]).astype(np.float32)


def assign_parts(xyz):
    """Palette 0 / 1 / 2 by thirds of the cloud's x range: what editing produces (parts moved rigidly)."""
    x = xyz[:, 0].astype(np.float64)
    t = (x - x.min()) / (x.max() - x.min())
    return np.minimum((t * 3).astype(np.int64), 2).astype(np.uint8)


def assign_mixed(n, seed=5):
    return np.random.default_rng(seed).integers(0, 4, n).astype(np.uint8)


def run_case(pc, view, o, agg, refmods, Rw2c):
    """make_golden.make_case with the gathered Rw2c ([N,3,3] tensor, or [3,3])."""
    import oracle_query as oq
    from sgnerf_amd.hyper import grid_hyperparameters
    near_far_linear_ray_generation, ray_march, alpha_blend, radiance_render = refmods
    hy = grid_hyperparameters(o, torch.from_numpy(pc.xyz.min(0)), torch.from_numpy(pc.xyz.max(0)))
    campos = torch.from_numpy(view.campos)[None]
    rot = torch.from_numpy(view.camrotc2w)[None]
    raydir = torch.from_numpy(view.raydir)[None]
    R = raydir.shape[1]
    raypos, _, _, mid = near_far_linear_ray_generation(campos, raydir, o.z_depth_dim, near=view.near,
                                                       far=view.far, jitter=0.0)
    t_ref = mid[0, 0].contiguous()
    og = oq.OracleGrid(pc.xyz, hy, o)
    q = og.query(view.campos, view.raydir, t_ref.numpy())
    sample_pidx, sample_loc_w, ray_mask = oq.reference_layout(q)
    sample_pidx = torch.from_numpy(sample_pidx)[None].long()
    sample_loc_w = torch.from_numpy(sample_loc_w)[None]
    keep = torch.from_numpy(ray_mask.astype(bool))
    B, Rv, SR, K = sample_pidx.shape
    xyz = torch.from_numpy(pc.xyz)
    pers = mg.w2pers_points(xyz, rot, campos)
    mask = sample_pidx >= 0
    flat = torch.clamp(sample_pidx, min=0).view(-1)
    g = lambda t, c: torch.index_select(t, 1, flat).view(B, Rv, SR, K, c)  # noqa: E731
    sampled_embedding = g(torch.cat([xyz[None, ...], pers, torch.from_numpy(pc.embedding)[None]], dim=-1), 38)
    sampled_color = g(torch.from_numpy(pc.color)[None], 3)
    sampled_dir = g(torch.from_numpy(pc.dir)[None], 3)
    sampled_conf = g(torch.from_numpy(pc.conf)[None], 1)
    # neural_points.py:967
    sampled_Rw2c = Rw2c if Rw2c.dim() == 2 else torch.index_select(Rw2c, 0, flat).view(B, Rv, SR, K, 3, 3)
    sample_loc = mg.w2pers_samples(sample_loc_w, rot, campos)
    sample_ray_dirs = raydir[0][keep][None, :, None, :].expand(-1, -1, SR, -1).contiguous()
    vsize = np.asarray(o.vsize)
    with torch.no_grad():
        decoded, ray_valid, weight, conf_coef = agg(
            sampled_color, None, sampled_Rw2c, sampled_dir, sampled_conf, sampled_embedding[..., 6:],
            sampled_embedding[..., 3:6], sampled_embedding[..., :3], mask, sample_loc, sample_loc_w,
            sample_ray_dirs, vsize, 0)
        ray_dist = torch.cummax(sample_loc[..., 2], dim=-1)[0]   # neural_points_volumetric_model.py:569-577
        ray_dist = torch.cat([ray_dist[..., 1:] - ray_dist[..., :-1],
                              torch.full((ray_dist.shape[0], ray_dist.shape[1], 1), vsize[2])], dim=-1)
        m = ray_dist < 1e-8
        m = torch.logical_or(m, ray_dist > 2 * vsize[2]).to(torch.float32)
        ray_dist = ray_dist * (1.0 - m) + m * vsize[2]
        ray_dist *= ray_valid.float()
        ray_color, _, opacity, _, _, bg_t, _ = ray_march(ray_dist, ray_valid, decoded, radiance_render, alpha_blend,
                                                         torch.ones(1, 3))
    full = torch.ones(R, 3)
    full[keep] = ray_color[0]
    return dict(sample_pidx=sample_pidx[0].numpy().astype(np.int32), sample_loc_w=sample_loc_w[0].numpy(),
                ray_mask=ray_mask, decoded=decoded[0].numpy(), ray_valid=ray_valid[0].numpy(),
                weight=weight[0].numpy(), conf_coefficient=conf_coef[0].numpy(), opacity=opacity[0].numpy(),
                bg_transmission=bg_t[0, :, 0].numpy(), full_color=full.numpy())


def main():
    assert os.path.isdir(mg.REF), "the golden generator runs only where the reference checkout exists"
    sys.dont_write_bytecode = True
    sys.path.insert(0, mg.REF)
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    from models.aggregators.point_aggregators import PointAggregator
    from models.rendering.diff_ray_marching import near_far_linear_ray_generation, ray_march
    from models.rendering.diff_render_func import alpha_blend, radiance_render
    import sgnerf_amd  # noqa: F401
    from sgnerf_amd import scene
    from sgnerf_amd.opts import HotPathOpts

    agg = mg.seeded_aggregator(PointAggregator, 0, 1)
    with torch.no_grad():
        agg.alpha_branch[0].bias.add_(mg.OPAQUE_BIAS)
    stored = np.load(os.path.join(HERE, "reference_opaque.npz"))
    for k, v in agg.state_dict().items():   # the tests read the weights from reference_opaque.npz
        assert np.array_equal(stored[f"mlp/{k}"], v.detach().numpy()), k
    refmods = (near_far_linear_ray_generation, ray_march, alpha_blend, radiance_render)
    view = scene.room_view(16, 16, yaw=225.0, pitch=-30.0, campos=(2.3, 2.2, 0.8), focal=18.0)  # corner_view
    pc = scene.room_corner(20000, 1)
    n = pc.xyz.shape[0]
    pal = palette()
    index = {"rot_parts": assign_parts(pc.xyz), "rot_mixed": assign_mixed(n)}
    index["rot_mixed_k4"] = index["rot_mixed"]
    cases = {"rot_parts": (32, 8), "rot_mixed": (32, 8), "rot_mixed_k4": (24, 4), "rot_global": (32, 8)}
    out = {"corner/gen": np.array("room_corner:20000:1"), "corner/checksum": mg.cloud_checksum(pc),
           "mlp_from": np.array("reference_opaque.npz"), "palette": pal,
           "view/campos": view.campos, "view/camrotc2w": view.camrotc2w, "view/raydir": view.raydir,
           "view/near_far": np.array([view.near, view.far], np.float32)}
    for name, (SR, K) in cases.items():
        o = HotPathOpts(SR=SR, K=K)
        if name == "rot_global":
            Rw2c = torch.from_numpy(pal[2])
            out[f"{name}/global"] = np.uint8(2)
        else:
            Rw2c = torch.from_numpy(pal[index[name]])
            out[f"{name}/index"] = index[name]
        c = run_case(pc, view, o, agg, refmods, Rw2c)
        ident = run_case(pc, view, o, agg, refmods, torch.eye(3))
        pidx = c["sample_pidx"]
        nnb = (pidx >= 0).sum(-1)
        stats = {"valid samples": int((nnb > 0).sum()), "samples with 1..K-1 neighbours": int(((nnb > 0) & (nnb < K)).sum())}
        if name != "rot_global":
            mi = np.where(pidx >= 0, index[name][np.maximum(pidx, 0)].astype(np.int64), -1)
            lo = np.where(pidx >= 0, mi, 99).min(-1)
            stats["samples with >= 2 different matrices"] = int(((nnb > 0) & (mi.max(-1) != lo)).sum())
            later = (mi[..., 1:] >= 0) & (mi[..., 1:] != mi[..., :1])
            stats["samples whose slot-0 matrix differs from a later neighbour's"] = int(((nnb > 0) & later.any(-1)).sum())
        shift = float(np.abs(c["decoded"] - ident["decoded"]).max())
        print(name, stats, f"max |decoded - decoded_identity| = {shift:.3e}")
        assert all(v > 0 for v in stats.values()), stats
        assert shift >= MIN_SHIFT, shift
        # the rotation leaves the query, the weights and the mask alone
        for k in ("sample_pidx", "sample_loc_w", "ray_mask", "ray_valid", "weight", "conf_coefficient"):
            assert np.array_equal(c[k], ident[k]), k
        out.update({f"{name}/SR": np.int32(SR), f"{name}/K": np.int32(K), f"{name}/points": np.array("corner")})
        out.update({f"{name}/{k}": c[k] for k in ("sample_pidx", "sample_loc_w", "ray_mask", "decoded", "opacity",
                                                  "bg_transmission", "full_color")})
    path = os.path.join(HERE, "reference_rw2c.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) / 1e6, "MB")


if __name__ == "__main__":
    main()
