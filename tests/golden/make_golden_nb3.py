"""Generates tests/golden/reference_nb3.npz: the viewmlp without block3 (shading_feature_mlp_layer3 = 0, the
network of most SG-NeRF scripts) run by the reference's own PointAggregator and ray_march, as make_golden.py and
make_golden_rw2c.py do for the stock network (their helpers are imported; same container-only imports,
neighbour indices from the oracle, every float from the reference).

Cases (scene.room_corner(20000, 1) -- partial K on most samples -- seen through a 14 x 14 corner view, SR 24):
  base      the base network, K 8                         208,388 parameters
  base_k5   the same weights, K 5
  bp256     shading_feature_mlp_layer2_bpnet = 1, predict_semantic = 0 (block2_bpnet.0 on 256 inputs)   274,180
  bp352     ... predict_semantic = 1 (block2_bpnet.0 on [h | BPNet embedding 96])                       298,756
  rot       the base weights, a per-point Rw2c from make_golden_rw2c's palette

The weights are NOT stored (0.8 .. 1.2 MB of random floats per network): each network is sgnerf_amd.weights.
init_mlp's seeded draw (bias_std 0.01, alpha bias + OPAQUE_BIAS) loaded into the reference module with
load_state_dict(strict=True) -- which also pins init_mlp's keys and shapes to the reference's state dict -- and the
file keeps the seed, the reference's key order and a float64 checksum per tensor.  The cloud is its generator
call plus checksums (the BPNet table: scene.with_semantics(seed 22)).  The K-8 cases share one query (sample_pidx,
sample_loc_w, sample_loc, ray_mask, ray_valid, weight, conf_coefficient: asserted equal across them), stored once.

Usage:  python -B tests/golden/make_golden_nb3.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
import make_golden_rw2c as mr  # noqa: E402

OPAQUE_BIAS = 50.0
SEEDS = {"base": 31, "bp256": 32, "bp352": 33}
VARIANT = {"base": (0, 0), "bp256": (1, 0), "bp352": (1, 96)}
N_PARAMS = {"base": 208_388, "bp256": 274_180, "bp352": 298_756}
QUERY_KEYS = ("sample_pidx", "sample_loc_w", "sample_loc", "ray_mask", "ray_valid", "weight", "conf_coefficient")
CASE_KEYS = ("decoded", "opacity", "bg_transmission", "full_color")


def network(PointAggregator, key):
    """The reference module of a network, holding init_mlp's seeded weights; and those weights."""
    from sgnerf_amd.weights import init_mlp
    nl, dim = VARIANT[key]
    agg = PointAggregator(mg.reference_opt(shading_feature_mlp_layer3=0, shading_feature_mlp_layer2_bpnet=nl,
                                           predict_semantic=1 if dim else 0)).eval()
    st = init_mlp(SEEDS[key], bias_std=0.01, bpnet_layers=nl, bpnet_dim=dim, block3_layers=0)
    st["alpha_branch.0.bias"] = st["alpha_branch.0.bias"] + OPAQUE_BIAS
    keys = list(agg.state_dict())
    assert not any(k.startswith("block3.") for k in keys), keys
    assert sum(v.numel() for v in agg.state_dict().values()) == N_PARAMS[key]
    agg.load_state_dict(st, strict=True)
    return agg, st, keys


def run_case(pc, view, o, agg, refmods, Rw2c, bpnet):
    """make_golden_rw2c.run_case with the SG gather (neural_points.py:970-972) and sample_loc kept."""
    import oracle_query as oq
    from sgnerf_amd.hyper import grid_hyperparameters
    near_far_linear_ray_generation, ray_march, alpha_blend, radiance_render = refmods
    hy = grid_hyperparameters(o, torch.from_numpy(pc.xyz.min(0)), torch.from_numpy(pc.xyz.max(0)))
    campos = torch.from_numpy(view.campos)[None]
    rot = torch.from_numpy(view.camrotc2w)[None]
    raydir = torch.from_numpy(view.raydir)[None]
    R = raydir.shape[1]
    _, _, _, mid = near_far_linear_ray_generation(campos, raydir, o.z_depth_dim, near=view.near, far=view.far, jitter=0.0)
    q = oq.OracleGrid(pc.xyz, hy, o).query(view.campos, view.raydir, mid[0, 0].contiguous().numpy())
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
    sampled_conf = g(torch.from_numpy(pc.conf)[None], 1)
    sampled_label = None if bpnet is None else g(torch.from_numpy(bpnet)[None], bpnet.shape[1])
    sampled_Rw2c = Rw2c if Rw2c.dim() == 2 else torch.index_select(Rw2c, 0, flat).view(B, Rv, SR, K, 3, 3)
    sample_loc = mg.w2pers_samples(sample_loc_w, rot, campos)
    sample_ray_dirs = raydir[0][keep][None, :, None, :].expand(-1, -1, SR, -1).contiguous()
    vsize = np.asarray(o.vsize)
    outs = []
    with torch.no_grad():
        # the colour and dir inputs are not read: the reference's output is the same with None as with garbage
        for col, pdir in ((None, None), (torch.full((B, Rv, SR, K, 3), 7.5), torch.full((B, Rv, SR, K, 3), -3.25))):
            outs.append(agg(col, sampled_label, sampled_Rw2c, pdir, sampled_conf, sampled_embedding[..., 6:],
                            sampled_embedding[..., 3:6], sampled_embedding[..., :3], mask, sample_loc, sample_loc_w,
                            sample_ray_dirs, vsize, 0))
        for a, b in zip(*outs):
            assert torch.equal(a, b), "the reference read sampled_color / sampled_dir"
        decoded, ray_valid, weight, conf_coef = outs[0]
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
                sample_loc=sample_loc[0].numpy(), ray_mask=ray_mask, decoded=decoded[0].numpy(),
                ray_valid=ray_valid[0].numpy(), weight=weight[0].numpy(), conf_coefficient=conf_coef[0].numpy(),
                opacity=opacity[0].numpy(), bg_transmission=bg_t[0, :, 0].numpy(), full_color=full.numpy())


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

    refmods = (near_far_linear_ray_generation, ray_march, alpha_blend, radiance_render)
    view = scene.room_view(14, 14, yaw=225.0, pitch=-30.0, campos=(2.3, 2.2, 0.8), focal=16.0)
    pc = scene.with_semantics(scene.room_corner(20000, 1), seed=22)
    pal = mr.palette()
    index = mr.assign_mixed(pc.xyz.shape[0])
    out = {"corner/gen": np.array("room_corner:20000:1"), "corner/bpnet_seed": np.int32(22),
           "corner/checksum": np.concatenate([mg.cloud_checksum(pc), [np.float64(pc.bpnet).sum()]]),
           "palette": pal, "view/campos": view.campos, "view/camrotc2w": view.camrotc2w, "view/raydir": view.raydir,
           "view/near_far": np.array([view.near, view.far], np.float32)}
    nets = {}
    for key in SEEDS:
        agg, st, keys = network(PointAggregator, key)
        nets[key] = agg
        out.update({f"mlp_{key}/seed": np.int32(SEEDS[key]), f"mlp_{key}/variant": np.array(VARIANT[key], np.int32),
                    f"mlp_{key}/keys": np.array(keys), f"mlp_{key}/checksum": np.array([float(st[k].double().sum()) for k in keys])})
    eye = torch.eye(3)
    cases = {"base": ("base", 8, eye), "base_k5": ("base", 5, eye), "bp256": ("bp256", 8, eye), "bp352": ("bp352", 8, eye),
             "rot": ("base", 8, torch.from_numpy(pal[index]))}
    queries = {}
    for name, (key, K, Rw2c) in cases.items():
        nl, dim = VARIANT[key]
        o = HotPathOpts(SR=24, K=K, shading_feature_mlp_layer3=0, shading_feature_mlp_layer2_bpnet=nl,
                        predict_semantic=1 if dim else 0, semantic_guidance=1 if dim else 0)
        c = run_case(pc, view, o, nets[key], refmods, Rw2c, pc.bpnet if dim else None)
        qn = f"q{K}"
        if qn not in queries:
            queries[qn] = {k: c[k] for k in QUERY_KEYS}
            out.update({f"{qn}/{k}": c[k] for k in QUERY_KEYS})
            out.update({f"{qn}/SR": np.int32(24), f"{qn}/K": np.int32(K)})
        for k in QUERY_KEYS:   # neither the network nor the rotation moves the query, the weights or the mask
            assert np.array_equal(queries[qn][k], c[k]), (name, k)
        out.update({f"{name}/query": np.array(qn), f"{name}/mlp": np.array(key)})
        out.update({f"{name}/{k}": c[k] for k in CASE_KEYS})
        if name == "rot":
            out["rot/index"] = index
            shift = float(np.abs(c["decoded"] - out["base/decoded"]).max())
            assert shift >= mr.MIN_SHIFT, shift
            print("rot: max |decoded - decoded_identity| =", f"{shift:.3e}")
        nnb = (c["sample_pidx"] >= 0).sum(-1)
        bt = c["bg_transmission"]
        print(name, "valid rays", int(c["ray_mask"].sum()), "valid samples", int((nnb > 0).sum()),
              "samples with 1..K-1 neighbours", int(((nnb > 0) & (nnb < K)).sum()), "bg_t median", float(np.median(bt)),
              "max |decoded|", float(np.abs(c["decoded"]).max()))
        assert int(((nnb > 0) & (nnb < K)).sum()) > 0 and int((nnb == K).sum()) > 0
    path = os.path.join(HERE, "reference_nb3.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) / 1e6, "MB")


if __name__ == "__main__":
    main()
