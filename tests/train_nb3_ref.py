"""What the tests of the training step of the viewmlp without block3 (opts.train_rows = 1) share: scene objects for
nb3_ref.chain built from train_rows_ref.synthetic_scene and from a sample-major query (HipTrainer.last_query), and the
step's reference for every variant -- autograd through nb3_ref.chain followed by train.composite_losses.

nb3_ref.chain clamps conf plainly (a rendered value needs no more).  Training differentiates the reference's
straight-through clamp (point_aggregators.py:863-865: d conf passes a clamped conf unchanged, as train.aggregate and
sgn_train_row_head have it), so `chain_feat` hands the chain the clamped values with conf's identity gradient
attached: the same values, and torch.clamp's gradient is 1 on them."""
import contextlib
from types import SimpleNamespace

import torch

import nb3_ref as nb
import train_rows_ref as rr

from sgnerf_amd.train import composite_losses

POINT_KEYS = ("embedding", "conf")


@contextlib.contextmanager
def default_dtype(dtype):
    """train.composite_losses allocates its dense tensors in torch's default dtype: float64 for the reference."""
    keep = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        yield
    finally:
        torch.set_default_dtype(keep)


class Scene:
    """The scene object nb3_ref.chain reads, from points (a dict of xyz / embedding / conf [N, 1] and, for the
    352-input block2_bpnet.0, bpnet), a camera (campos, rot), the rays and a sample-major query: samp_ray [S],
    samp_locw [S, 3], pidx [S, K] (-1 on empty slots, the valid ones a prefix), ray_soff [R].  Every tensor on the
    device of pidx."""

    def __init__(self, points, camera, raydir, q):
        pidx = q["pidx"].long()
        dev = pidx.device
        self.S, self.K = pidx.shape
        self.points = {k: v.to(dev) for k, v in points.items()}
        self.camera = tuple(t.to(dev) for t in camera)
        self.raydir = raydir.to(dev)
        nnb = (pidx >= 0).sum(-1)
        assert bool(((pidx >= 0) == (torch.arange(self.K, device=dev)[None, :] < nnb[:, None])).all())
        self.nnb = nnb
        self.query = dict(samp_ray=q["samp_ray"].long(), samp_locw=q["samp_locw"], pidx=pidx,
                          ray_soff=q["ray_soff"].long())
        self.work = torch.nonzero(nnb > 0).reshape(-1)
        self.items = self.work.numel()
        self.rs, self.rk = torch.nonzero(pidx >= 0, as_tuple=True)
        self.pid = pidx[self.rs, self.rk]
        self.item = (torch.cumsum((nnb > 0).long(), 0) - 1)[self.rs]


def synthetic(K, items):
    """train_rows_ref.synthetic_scene as a Scene (its counted samples; ray_soff is not meaningful there)."""
    points, camera, raydir, query = rr.synthetic_scene(K, items)
    S = query["S"]
    q = dict(samp_ray=query["samp_ray"][:S], samp_locw=query["samp_locw"][:S], pidx=query["pidx"][:S],
             ray_soff=torch.zeros(raydir.shape[0], dtype=torch.long))
    pts = dict(xyz=points["xyz"], embedding=points["embedding"], conf=points["conf"], color=points["color"],
               dir=points["dir"])
    return Scene(pts, camera, raydir, q)


def leaves(sc, state, dtype=torch.float64):
    """Differentiable copies in `dtype`: (the points dict with embedding and conf as leaves, the state as leaves)."""
    pts = {k: v.detach().to(dtype) if v.is_floating_point() else v for k, v in sc.points.items()}
    for k in POINT_KEYS:
        pts[k] = pts[k].clone().requires_grad_(True)
    st = {k: v.detach().to(sc.work.device, dtype).clone().requires_grad_(True) for k, v in state.items()}
    return pts, st


def chain_feat(sc, pts, st, dtype=torch.float64):
    """nb3_ref.chain on the leaves -> (its outputs, feat [S, 4] = (alpha, rgb), zeros on samples without a
    neighbour), conf through the straight-through clamp (module docstring)."""
    conf = pts["conf"]
    keep = sc.points
    # clamp(conf) + (conf - conf.detach()): exactly the clamped value (x - (x - c) need not be c in floating point)
    sc.points = dict(pts, conf=torch.clamp(conf, 1e-4, 1.0).detach() + (conf - conf.detach()))
    try:
        o = nb.chain(sc, st, dtype)
    finally:
        sc.points = keep
    feat = torch.zeros(sc.S, 4, dtype=dtype, device=sc.work.device)
    feat = feat.index_copy(0, sc.work, torch.cat([o["alpha"][:, None], o["rgb"]], dim=-1))
    return o, feat


def chain_loss(sc, state, opts, gt, dtype=torch.float64, bg=(1.0, 1.0, 1.0), depth=None):
    """The step's reference: autograd of train.composite_losses over nb3_ref.chain, evaluated in `dtype`.
    Returns (parts with "total", colour [R, 3], ray mask [R], gradients by name: every layer's weight and bias,
    points_embeding, points_conf)."""
    pts, st = leaves(sc, state, dtype)
    campos, rot = (t.to(dtype) for t in sc.camera)
    with default_dtype(dtype):
        _, feat = chain_feat(sc, pts, st, dtype)
        P = SimpleNamespace(points_conf=pts["conf"].reshape(-1, 1), xyz=pts["xyz"])
        q = dict(sc.query, samp_locw=sc.query["samp_locw"].to(dtype))
        if torch.is_tensor(bg):
            bg = bg.to(dtype)
        total, parts, full, mask, *_ = composite_losses(P, q, feat, sc.nnb > 0, campos, rot, sc.raydir.to(dtype),
                                                        gt.to(sc.work.device, dtype), opts, bg, depth=depth)
        total.backward()
    g = {k: (torch.zeros_like(v) if v.grad is None else v.grad) for k, v in st.items()}
    g["points_embeding"] = pts["embedding"].grad
    g["points_conf"] = pts["conf"].grad.reshape(-1, 1)
    parts["total"] = total.detach()
    return parts, full.detach(), mask, g


def min_preactivation(sc, state):
    """The smallest |LeakyReLU input| of the network on the scene, evaluated in float64: the row layers' (block1.0,
    block1.2, block2_bpnet.0) and the colour MLP's three.  LeakyReLU's derivative jumps from 0.01 to 1 at 0: an input
    inside the fp32 error of the forward may land on either side in an fp32 evaluation, and the gradients that pass
    through it differ by a factor of 100 between the two sides.  The tests print it with their errors."""
    st = {k: v.double() for k, v in state.items()}
    with torch.no_grad():
        d, _ = nb.row_inputs(sc)
        emb = sc.points["embedding"].double()[sc.pid]
        zs = [nb.lin("block1.0", torch.cat([emb, nb.pe(emb, 3), nb.pe(d, 5)], dim=-1), st)]
        zs.append(nb.lin("block1.2", nb.lrelu(zs[-1]), st))
        if "block2_bpnet.0.weight" in st:
            h = nb.lrelu(zs[-1])
            if st["block2_bpnet.0.weight"].shape[1] > 256:
                h = torch.cat([h, sc.points["bpnet"].double()[sc.pid]], dim=-1)
            zs.append(nb.lin("block2_bpnet.0", h, st))
        o = nb.chain(sc, st)
        arg = (o["v"][:, :, None] * 2.0 ** torch.arange(4, dtype=torch.float64)).reshape(-1, 12)
        c = torch.cat([o["fs"], torch.sin(arg), torch.cos(arg)], dim=-1)
        for name in ("color_branch.0", "color_branch.2", "color_branch.4"):
            zs.append(nb.lin(name, c, st))
            c = nb.lrelu(zs[-1])
    return min(float(z.abs().min()) for z in zs if z.numel())


def rel_l2(a, b):
    return float(torch.linalg.vector_norm(a.double().cpu() - b.double().cpu()) /
                 max(float(torch.linalg.vector_norm(b.double())), 1e-30))
