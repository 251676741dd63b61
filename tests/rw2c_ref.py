"""Float64 restatement of what a non-identity Rw2c (rotated neural points) changes in the aggregator, on top
of agg_rows_ref.py / train_rows_ref.py and their hand-built scenes.  Three rules (point_aggregators.py:565-569,
:579, :599, :648; R_p the point's matrix, R x meaning y_i = sum_j R[i][j] x_j):

  1. the world half of dists becomes R_p (xyz_p - loc_s) before its encoding; the pers half, the weights and
     their normalisation keep the unrotated offset;
  2. the view direction of a sample is v'_s = R_{p0(s)} raydir, p0(s) the point in its neighbour slot 0 (index
     clamped at 0), everywhere downstream: block3.0's extras and the colour MLP's PE;
  3. the point direction in block3.0's extras is R_p dir_p.

Only these are restated (row offsets, the extras, the sample view direction and with it the viewdir PE); every
layer is agg_rows_ref's.  `rot` is [N,3,3] (fp32); a [3,3] matrix is expanded by the caller (expand_rot).
"""
import numpy as np
import torch

import agg_rows_ref as ar
from train_rows_ref import compact_lists, row_index


def axis_angle(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    t = np.deg2rad(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def palette():
    """identity, Rz(40), 75 degrees about (1,2,3), 170 degrees about (-1,1,0.5): the golden file's palette."""
    return torch.from_numpy(np.stack([np.eye(3), axis_angle((0, 0, 1), 40.0), axis_angle((1, 2, 3), 75.0),
                                      axis_angle((-1, 1, 0.5), 170.0)]).astype(np.float32))


def palette_rot(n, seed=5):
    """[n,3,3]: every point draws one of the palette's four matrices (seeded)."""
    idx = torch.randint(0, 4, (n,), generator=torch.Generator().manual_seed(seed))
    return palette()[idx].contiguous()


def expand_rot(rot, n):
    rot = torch.as_tensor(rot)
    return rot.reshape(1, 3, 3).expand(n, 3, 3) if rot.dim() == 2 else rot


def mv(R, x):
    return torch.einsum("nij,nj->ni", R, x)


def sample_viewdirs(sc, rot, dtype=torch.float64):
    """v'_s [S,3] for every sample s < S (rule 2); samples without a neighbour read point 0 (the clamp)."""
    q = sc.query
    p0 = torch.clamp(q["pidx"][:sc.S, 0].long(), min=0)
    v = sc.raydir.to(dtype)[q["samp_ray"][:sc.S].long()]
    return mv(rot.to(dtype)[p0], v)


def row_inputs(sc, rot, dtype=torch.float64, vdir=None):
    """agg_rows_ref.row_inputs with the three rules: dists [rows,6], ext [rows,7], rw [rows,2] (unchanged).
    vdir: the samples' view directions to use instead of sample_viewdirs (a kernel's own output)."""
    d, _, rw = ar.row_inputs(sc, dtype)
    Rr = rot.to(dtype)[sc.pid]
    d = torch.cat([mv(Rr, d[:, :3]), d[:, 3:]], dim=-1)
    v = (sample_viewdirs(sc, rot, dtype) if vdir is None else vdir.to(dtype))[sc.rs]
    pd = mv(Rr, sc.points["dir"].to(dtype)[sc.pid])
    ext = torch.cat([sc.points["color"].to(dtype)[sc.pid], pd - v, (pd * v).sum(-1, keepdim=True)], dim=-1)
    return d, ext, rw


def chain(sc, state, rot, dtype=torch.float64):
    """agg_rows_ref.chain (base network) on the rotated row inputs and view directions."""
    assert "block2_bpnet.0.weight" not in state, "rotation is built for the base viewmlp"
    d, ext, rw = row_inputs(sc, rot, dtype)
    o = dict(rw=rw, dists=d, ext=ext)
    o["P"] = ar.proj_ref(sc.points["embedding"].to(dtype), state)
    o["z1"] = ar.z1_ref(o["P"][sc.pid], d, state)
    o["z2"] = ar.layer_ref("block1.2", ar.lrelu(o["z1"]), state)
    o["z3"] = ar.z3_ref(o["z2"], ext, state)
    o["fs"], o["alpha"], o["z4"], _ = ar.blend_ref(o["z3"], rw[:, 0], sc.item, sc.items, state)
    o["v"] = sample_viewdirs(sc, rot, dtype)[sc.work.long()]
    o["rgb"] = ar.colour_ref(o["fs"], o["v"], state)
    return o


def chain_bars(sc, state, rot):
    """agg_rows_ref.chain_bars for the rotated chain: float64 against the torch-fp32 floor, capped."""
    o64, o32 = chain(sc, state, rot), chain(sc, state, rot, dtype=torch.float32)
    b = dict(alpha=ar.chain_bar(o64["alpha"], o32["alpha"], True), rgb=ar.chain_bar(o64["rgb"], o32["rgb"], True),
             blend=ar.chain_bar(o64["rw"][:, 0], o32["rw"][:, 0], True),
             wnorm=ar.chain_bar(o64["rw"][:, 1], o32["rw"][:, 1], True), fs=ar.chain_bar(o64["fs"], o32["fs"]))
    for k in ("alpha", "rgb"):
        ar.capped(b[k], o64[k], k, unit=True)
    ar.capped(b["blend"], o64["rw"][:, 0], "blend", unit=True)
    ar.capped(b["wnorm"], o64["rw"][:, 1], "wnorm", unit=True)
    ar.capped(b["fs"], o64["fs"], "f_s")
    return b, o64


class GoldenScene:
    """A case of tests/golden/reference_rw2c.npz as the scene object the chains read: one sample per dense
    (valid ray, slot), its neighbours the oracle's; `rot` [N,3,3] from the palette."""

    def __init__(self, g, name, pts):
        keep = g[f"{name}/ray_mask"].astype(bool)
        pidx = torch.from_numpy(g[f"{name}/sample_pidx"])          # [Rv, SR, K]
        Rv, SR, K = pidx.shape
        self.K, self.S, self.Rv, self.SR = K, Rv * SR, Rv, SR
        self.points = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in pts.items()}
        self.points["conf"] = self.points["conf"].reshape(-1, 1)
        self.N = self.points["xyz"].shape[0]
        self.camera = (torch.from_numpy(g["view/campos"]).reshape(3), torch.from_numpy(g["view/camrotc2w"]).reshape(3, 3))
        self.raydir = torch.from_numpy(g["view/raydir"])[torch.from_numpy(keep)]
        nnb = (pidx >= 0).sum(-1).reshape(-1).to(torch.int32)
        assert bool(((pidx >= 0).reshape(-1, K) == (torch.arange(K)[None, :] < nnb[:, None])).all())   # a prefix
        self.query = dict(samp_ray=torch.arange(Rv).repeat_interleave(SR).to(torch.int32),
                          samp_locw=torch.from_numpy(g[f"{name}/sample_loc_w"]).reshape(-1, 3), samp_nnb=nnb,
                          pidx=pidx.reshape(-1, K), S=self.S, S_cap=self.S)
        self.work, self.row_off, _ = compact_lists(nnb, self.S)
        self.items = self.work.numel()
        self.rs, self.rk, self.pid, self.item = row_index(self.query, K)
        pal = torch.from_numpy(g["palette"])
        if f"{name}/index" in g.files:
            self.rot = pal[torch.from_numpy(g[f"{name}/index"]).long()]
        else:
            self.rot = pal[int(g[f"{name}/global"])].reshape(1, 3, 3).expand(self.N, 3, 3)

    def decoded(self, o):
        """[Rv, SR, 4] (alpha, rgb) of a chain's outputs, zeros where the sample has no neighbour."""
        out = torch.zeros(self.S, 4, dtype=o["alpha"].dtype)
        out[self.work.long(), 0] = o["alpha"]
        out[self.work.long(), 1:] = o["rgb"]
        return out.view(self.Rv, self.SR, 4)
