"""Float64 restatement of the viewmlp without block3 (shading_feature_mlp_layer3 = 0; point_aggregators.py:
356-368 `self.block3 = passfunc`, :638-653, :743-786), on the scenes of agg_rows_ref.py and on the cases of
tests/golden/reference_nb3.npz (the reference's own PointAggregator, tests/golden/make_golden_nb3.py).

Per valid (sample, neighbour) row:
    h = LReLU(block1.2(LReLU(block1.0([emb | PE(emb, 3) | PE(dists, 5)]))))
    h = LReLU(block2_bpnet.0([h | BPNet embedding or nothing]))          with shading_feature_mlp_layer2_bpnet = 1
    alpha_k = softplus(alpha_branch.0(h) - 1)
per sample, with w_k the normalised inverse-distance weight times clamp(conf, 1e-4, 1):
    alpha_s = sum_k w_k alpha_k,  f_s = sum_k w_k h_k,  rgb = color_branch([f_s | PE(viewdir, 4)]) (unchanged)
The points' colour and dir are not read.  Rotated points (rot [N,3,3]): rule 1 (the world half of dists is R_p
(xyz_p - loc_s), the weights keep the unrotated offset) and rule 2 (the colour MLP's view direction is
R_{p0(s)} raydir) of rw2c_ref.py; rule 3 has no point direction to act on.

Everything is stated here from the raw inputs, on whatever device the scene's tensors live (the GPU tests
measure the fp32 floor as this same restatement in torch fp32 on the GPU against the CPU), so it shares no
layer with agg_rows_ref.chain, the stock network's restatement; test_nb3_ref_cpu.py pins the shared pieces
(row inputs, colour MLP) to it.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

import rw2c_ref as rw
from helpers import GOLDEN_DIR
from train_rows_ref import compact_lists, lrelu, row_index

from sgnerf_amd import scene as scenes
from sgnerf_amd.weights import init_mlp

GOLDEN = os.path.join(GOLDEN_DIR, "reference_nb3.npz")
CASES = ["base", "base_k5", "bp256", "bp352", "rot"]
VARIANT = {"base": (0, 0), "base_k5": (0, 0), "bp256": (1, 0), "bp352": (1, 96), "rot": (0, 0)}
N_PARAMS = {(0, 0): 208_388, (1, 0): 274_180, (1, 96): 298_756}
OPAQUE_BIAS = 50.0   # added to alpha_branch.0.bias of every golden network: opacity ~0.3 per sample


def lin(name, x, state):
    return F.linear(x, state[name + ".weight"].to(x), state[name + ".bias"].to(x))


def pe(x, freqs):
    """positional_encoding without the original (networks.py:175-192): (sin, cos) pairs, channel-major then
    frequency (train_rows_ref.pe on the tensor's own device)."""
    arg = x[..., :, None] * (2.0 ** torch.arange(freqs, dtype=x.dtype, device=x.device))
    return torch.stack([torch.sin(arg), torch.cos(arg)], dim=-1).reshape(x.shape[:-1] + (x.shape[-1] * freqs * 2,))


def w2pers(p, rot, campos):
    c = (p - campos) @ rot
    return torch.stack([c[..., 0] / c[..., 2], c[..., 1] / c[..., 2], c[..., 2]], dim=-1)


def row_inputs(sc, dtype=torch.float64, pers=None, rot=None):
    """dists [rows, 6] (the world half rotated with rot) and rw [rows, 2] = (w clamp(conf, 1e-4, 1), w), w the
    inverse-distance weight of the UNROTATED offset normalised over the sample's rows.  pers = (points' [N, 3],
    samples' [S, 3]): the caller's camera-space coordinates instead of the camera."""
    P, q = sc.points, sc.query
    t = lambda x: x.to(dtype)  # noqa: E731
    xyz, loc = t(P["xyz"])[sc.pid], t(q["samp_locw"])[sc.rs]
    if pers is None:
        campos, cam = (t(x) for x in sc.camera)
        pp, pl = w2pers(xyz, cam, campos), w2pers(loc, cam, campos)
    else:
        pp, pl = t(pers[0])[sc.pid], t(pers[1])[sc.rs]
    d = torch.cat([xyz - loc, torch.stack([pp[:, 0] * pp[:, 2] - pl[:, 0] * pl[:, 2], pp[:, 1] * pp[:, 2] - pl[:, 1] * pl[:, 2],
                                           pp[:, 2] - pl[:, 2]], dim=-1)], dim=-1)
    w = 1.0 / torch.clamp(d[:, :3].norm(dim=-1), min=1e-6)
    wsum = torch.zeros(sc.S, dtype=dtype, device=w.device).index_add(0, sc.rs, w)
    wn = w / torch.clamp(wsum, min=1e-8)[sc.rs]
    cf = torch.clamp(t(P["conf"]).reshape(-1)[sc.pid], 1e-4, 1.0)
    if rot is not None:
        d = torch.cat([rw.mv(t(rot)[sc.pid], d[:, :3]), d[:, 3:]], dim=-1)
    return d, torch.stack([wn * cf, wn], dim=-1)


def colour(fs, v, state):
    """color_branch on [f_s | PE(v, 4)] (sin block then cos block), sigmoid 1.002 - 0.001 (agg_rows_ref.colour_ref
    on the tensors' own device)."""
    arg = (v[:, :, None] * 2.0 ** torch.arange(4, dtype=fs.dtype, device=fs.device)).reshape(-1, 12)
    c = torch.cat([fs, torch.sin(arg), torch.cos(arg)], dim=-1)
    for name in ("color_branch.0", "color_branch.2", "color_branch.4"):
        c = lrelu(lin(name, c, state))
    return torch.sigmoid(lin("color_branch.6", c, state)) * 1.002 - 0.001


def chain(sc, state, dtype=torch.float64, pers=None, rot=None):
    """The whole network on a scene, on the device of the scene's tensors.  Returns dists, rw [rows, 2], h [rows,
    256] (the last row layer after its LeakyReLU), alpha_k [rows], fs [items, 256], alpha [items], v [items, 3],
    rgb [items, 3]."""
    assert not any(k.startswith("block3.") for k in state)
    d, rwt = row_inputs(sc, dtype, pers, rot)
    emb = sc.points["embedding"].to(dtype)[sc.pid]
    h = lrelu(lin("block1.0", torch.cat([emb, pe(emb, 3), pe(d, 5)], dim=-1), state))
    h = lrelu(lin("block1.2", h, state))
    if "block2_bpnet.0.weight" in state:
        assert rot is None, "rotation is built for the base network"
        if state["block2_bpnet.0.weight"].shape[1] > 256:
            h = torch.cat([h, sc.points["bpnet"].to(dtype)[sc.pid]], dim=-1)
        h = lrelu(lin("block2_bpnet.0", h, state))
    al = F.softplus(lin("alpha_branch.0", h, state).reshape(-1) - 1)
    w = rwt[:, 0]
    fs = torch.zeros(sc.items, 256, dtype=dtype, device=h.device).index_add(0, sc.item, w[:, None] * h)
    a_s = torch.zeros(sc.items, dtype=dtype, device=h.device).index_add(0, sc.item, w * al)
    v = sc.raydir.to(dtype)[sc.query["samp_ray"][:sc.S].long()]
    if rot is not None:   # rule 2: R of the point in slot 0 (clamped), for every sample
        v = rw.mv(rot.to(dtype)[torch.clamp(sc.query["pidx"][:sc.S, 0].long(), min=0)], v)
    v = v[sc.work.long()]
    return dict(dists=d, rw=rwt, h=h, alpha_k=al, fs=fs, alpha=a_s, v=v, rgb=colour(fs, v, state))


def rel(a, b):
    """max |a - b| / max(1, |b|): the project's error measure of the fp32 bar (tests/test_render_gpu.py)."""
    if a.numel() == 0:
        return 0.0
    return float(((a.double() - b.double()).abs() / b.double().abs().clamp(min=1.0)).max())


class _On:
    """A scene's tensors on another device (what `chain` reads)."""

    def __init__(self, sc, device):
        mv = lambda t: t.to(device) if torch.is_tensor(t) else t  # noqa: E731
        for k in ("points", "query", "camera", "raydir", "work", "rs", "rk", "pid", "item", "S", "K", "items"):
            v = getattr(sc, k)
            setattr(self, k, {a: mv(b) for a, b in v.items()} if isinstance(v, dict) else
                    tuple(mv(x) for x in v) if isinstance(v, tuple) else mv(v))


def floor(sc, state, device, pers=None, rot=None):
    """The fp32 floor as tests/test_render_gpu.py measures it: this restatement evaluated by torch in fp32 on
    `device` against the same on the CPU (fp32's own summation-order noise on this input), per output."""
    st = {k: v.to(device) for k, v in state.items()}
    prs = None if pers is None else tuple(p.to(device) for p in pers)
    with torch.no_grad():
        a = chain(_On(sc, device), st, torch.float32, prs, None if rot is None else rot.to(device))
        b = chain(sc, state, torch.float32, pers, rot)
    return {k: rel(a[k].cpu(), b[k]) for k in ("alpha", "rgb", "fs", "rw")}


# ---- the golden file -------------------------------------------------------------------------------
def golden_state(key):
    """The aggregator state of a golden network: init_mlp's seeded draw (the file stores the seed, the key order of
    the reference's state dict and a float64 checksum per tensor, not the 0.8 .. 1.2 MB of weights)."""
    g = np.load(GOLDEN, allow_pickle=False)
    nl, dim = (int(x) for x in g[f"mlp_{key}/variant"])
    st = init_mlp(int(g[f"mlp_{key}/seed"]), bias_std=0.01, bpnet_layers=nl, bpnet_dim=dim, block3_layers=0)
    st["alpha_branch.0.bias"] = st["alpha_branch.0.bias"] + OPAQUE_BIAS
    keys = [str(k) for k in g[f"mlp_{key}/keys"]]
    assert sorted(keys) == sorted(st), (keys, sorted(st))
    got = np.array([float(st[k].double().sum()) for k in keys])
    np.testing.assert_array_equal(got, g[f"mlp_{key}/checksum"], err_msg=f"regenerated weights {key} differ")
    return st


def golden_points():
    """The golden cloud (a seeded generator call, checked against the stored checksums) with its BPNet table."""
    g = np.load(GOLDEN, allow_pickle=False)
    fn, n, seed = str(g["corner/gen"]).split(":")
    pc = scenes.with_semantics(getattr(scenes, fn)(int(n), int(seed)), seed=int(g["corner/bpnet_seed"]))
    pts = dict(xyz=pc.xyz, embedding=pc.embedding, color=pc.color, dir=pc.dir, conf=pc.conf, bpnet=pc.bpnet)
    got = np.array([np.float64(pts[k]).sum() for k in ("xyz", "embedding", "color", "dir", "conf", "bpnet")])
    np.testing.assert_array_equal(got, g["corner/checksum"], err_msg="regenerated cloud differs")
    return pts


def load_case(name):
    """(points, state, case) of a golden case; `case` holds the view (campos, camrotc2w, raydir, near_far), SR, K,
    the query the case shares with others (sample_pidx, sample_loc_w, sample_loc, ray_mask, ray_valid, weight,
    conf_coefficient) and its own outputs (decoded, opacity, bg_transmission, full_color); `rot` [N,3,3] if rotated."""
    g = np.load(GOLDEN, allow_pickle=False)
    qn = str(g[f"{name}/query"])
    case = {k.split("/", 1)[1]: g[k] for k in g.files if k.split("/", 1)[0] in ("view", qn, name)}
    if f"{name}/index" in g.files:
        case["rot"] = g["palette"][g[f"{name}/index"].astype(np.int64)]
    return golden_points(), golden_state(str(g[f"{name}/mlp"])), case


class GoldenScene:
    """A golden case as the scene object `chain` reads: one sample per dense (valid ray, slot), its neighbours
    the oracle's (rw2c_ref.GoldenScene's construction on this file's layout)."""

    def __init__(self, pts, case):
        keep = case["ray_mask"].astype(bool)
        pidx = torch.from_numpy(case["sample_pidx"])          # [Rv, SR, K]
        Rv, SR, K = pidx.shape
        self.K, self.S, self.Rv, self.SR = K, Rv * SR, Rv, SR
        self.points = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in pts.items()}
        self.points["conf"] = self.points["conf"].reshape(-1, 1)
        self.N = self.points["xyz"].shape[0]
        self.camera = (torch.from_numpy(case["campos"]).reshape(3), torch.from_numpy(case["camrotc2w"]).reshape(3, 3))
        self.raydir = torch.from_numpy(case["raydir"])[torch.from_numpy(keep)]
        nnb = (pidx >= 0).sum(-1).reshape(-1).to(torch.int32)
        assert bool(((pidx >= 0).reshape(-1, K) == (torch.arange(K)[None, :] < nnb[:, None])).all())   # a prefix
        self.query = dict(samp_ray=torch.arange(Rv).repeat_interleave(SR).to(torch.int32),
                          samp_locw=torch.from_numpy(case["sample_loc_w"]).reshape(-1, 3), samp_nnb=nnb,
                          pidx=pidx.reshape(-1, K), S=self.S, S_cap=self.S)
        self.work, self.row_off, _ = compact_lists(nnb, self.S)
        self.items = self.work.numel()
        self.rs, self.rk, self.pid, self.item = row_index(self.query, K)
        self.rot = torch.from_numpy(case["rot"]) if "rot" in case else None

    def decoded(self, o):
        """[Rv, SR, 4] (alpha, rgb) of a chain's outputs, zeros where the sample has no neighbour."""
        out = torch.zeros(self.S, 4, dtype=o["alpha"].dtype)
        out[self.work.long(), 0] = o["alpha"]
        out[self.work.long(), 1:] = o["rgb"]
        return out.view(self.Rv, self.SR, 4)

    def slots(self, o):
        """weight [Rv, SR, K] (normalised, 0 on empty slots) of a chain's outputs."""
        w = torch.zeros(self.S, self.K, dtype=o["rw"].dtype)
        w[self.rs, self.rk] = o["rw"][:, 1]
        return w.view(self.Rv, self.SR, self.K)
