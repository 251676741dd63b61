"""Plain float64 references of the fp32 training step's per-row / per-item kernels (csrc/train_x3.hip)
and the seeded synthetic scene the CPU and GPU tests of those kernels share.

The formulas are the aggregator's (train.aggregate / train._pe / train._w2pers and the descriptions in
include/sgn_hip.h), written over COMPACT rows: row j is the valid (sample, neighbour) pair number j
in sample-major order, item i the i-th sample with a neighbour.  tests/test_train_rows_ref_cpu.py
chains them into the aggregator's whole forward and backward and checks every gradient against
float64 autograd through train.aggregate, so a GPU test that disagrees with one of them names a kernel.

Every reference takes (points, camera, raydir, query, K): `points` a dict of xyz / embedding / color /
dir / conf, `camera` = (campos, rot), `query` a dict of samp_ray / samp_locw / samp_nnb / pidx and the
sample count S.  Inputs of any float type are computed on in float64.
"""
import math

import torch

N_POINTS, N_RAYS = 257, 37


def _d(t):
    return t.detach().to(torch.float64)


def synthetic_scene(K, items, seed=11):
    """The shared scene: 257 points (so neighbours repeat everywhere), a fixed camera in front of them,
    37 unit rays and `items` samples with 1..K neighbours among ~30 % more without any.  All fp32 / int32
    CPU tensors.  Planted: embedding entries of 1e3 and 3e5 (x 4 crosses 2^20), conf outside [1e-4, 1]
    and exactly 0 / 1e-4 / 1, four samples exactly at a neighbour's position (the 1e-6 clamp of the
    weight), neighbour counts (K, 1) and (1, K) on adjacent items, samples and rows of slack after the
    counted ones (counters[0] = S < S_cap)."""
    g = torch.Generator().manual_seed(seed * 1000 + K * 100 + items % 97)
    N, R = N_POINTS, N_RAYS
    xyz = torch.rand(N, 3, generator=g) * 2 - 1
    emb = torch.randn(N, 32, generator=g)
    emb[3, 5], emb[3, 6], emb[100, 0], emb[256, 31], emb[256, 0] = 1e3, -1e3, 3e5, -3e5, 1e3
    conf = torch.rand(N, 1, generator=g) * 1.7 - 0.2
    conf[0], conf[1], conf[2], conf[255], conf[256] = 0.0, 1e-4, 1.0, 1e-4, 1.0
    color = torch.rand(N, 3, generator=g)
    pdir = torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1)
    yaw, pitch = math.radians(30.0), math.radians(-10.0)
    ry = torch.tensor([[math.cos(yaw), 0, math.sin(yaw)], [0, 1, 0], [-math.sin(yaw), 0, math.cos(yaw)]], dtype=torch.float64)
    rx = torch.tensor([[1, 0, 0], [0, math.cos(pitch), -math.sin(pitch)], [0, math.sin(pitch), math.cos(pitch)]],
                      dtype=torch.float64)
    rot = (ry @ rx).float()
    campos = torch.tensor([0.3, -0.2, -4.0])
    raydir = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1)
    S = items + int(round(items * 0.3 / 0.7)) + 2
    S_cap = S + 5
    pos = torch.sort(torch.randperm(S, generator=g)[:items]).values
    nnb = torch.zeros(S_cap, dtype=torch.int32)
    nnb[pos] = torch.randint(1, K + 1, (items,), generator=g, dtype=torch.int32)
    if items >= 4:
        nnb[pos[:4]] = torch.tensor([K, 1, 1, K], dtype=torch.int32)
    nnb[S:] = K   # slack samples: never listed, never read
    pidx = torch.randint(0, N, (S_cap, K), generator=g, dtype=torch.int32)
    pidx[torch.arange(K)[None, :] >= nnb[:, None]] = -1   # valid neighbours are a prefix of the K slots
    samp_ray = torch.randint(0, R, (S_cap,), generator=g, dtype=torch.int32)
    locw = xyz[torch.randint(0, N, (S_cap,), generator=g)] + 0.05 * torch.randn(S_cap, 3, generator=g)
    for j in range(min(4, items)):   # a sample exactly at its (first / last) neighbour
        s = int(pos[j])
        locw[s] = xyz[int(pidx[s, (int(nnb[s]) - 1) * (j & 1)])]
    counters = torch.tensor([S, items, 0, 0], dtype=torch.int32)
    points = dict(xyz=xyz, embedding=emb, color=color, dir=pdir, conf=conf)
    query = dict(samp_ray=samp_ray, samp_locw=locw.contiguous(), samp_nnb=nnb, pidx=pidx, counters=counters, S=S,
                 S_cap=S_cap)
    return points, (campos, rot), raydir, query


def compact_lists(samp_nnb, S):
    """work (the samples s < S with a neighbour, ascending), row_off (exclusive prefix sum of samp_nnb
    over s < S) and counts (items, rows): what sgn_train_lists computes, in torch."""
    n = samp_nnb[:S].to(torch.int64)
    work = torch.nonzero(n > 0).reshape(-1).to(torch.int32)
    row_off = (torch.cumsum(n, 0) - n).to(torch.int32)
    counts = torch.tensor([work.numel(), int(n.sum()), 0, 0], dtype=torch.int32)
    return work, row_off, counts


def row_index(query, K):
    """Per compact row: its sample, neighbour slot, point and item (int64)."""
    S = query["S"]
    n = query["samp_nnb"][:S].to(torch.int64)
    valid = torch.arange(K)[None, :] < n[:, None]
    rs, rk = torch.nonzero(valid, as_tuple=True)   # row-major: sample-major rows
    pid = query["pidx"][:S].to(torch.int64)[rs, rk]
    item_of_sample = torch.cumsum((n > 0).to(torch.int64), 0) - 1
    return rs, rk, pid, item_of_sample[rs]


def pe(x, freqs):
    """positional_encoding without the original: (sin, cos) pairs, channel-major then frequency."""
    arg = x[..., :, None] * (2.0 ** torch.arange(freqs, dtype=x.dtype))
    return torch.stack([torch.sin(arg), torch.cos(arg)], dim=-1).reshape(x.shape[:-1] + (x.shape[-1] * freqs * 2,))


def w2pers(p, rot, campos):
    c = (p - campos) @ rot
    return torch.stack([c[..., 0] / c[..., 2], c[..., 1] / c[..., 2], c[..., 2]], dim=-1), c


def row_dists(points, camera, query, K, dtype=torch.float64):
    """dists [rows, 6] of the rows: world-space offset point - sample, then the perspective-space one
    (x z, y z, z of the camera frame), evaluated in `dtype`."""
    rs, _, pid, _ = row_index(query, K)
    campos, rot = (t.to(dtype) for t in camera)
    xyz = points["xyz"].to(dtype)[pid]
    loc = query["samp_locw"].to(dtype)[rs]
    pp, _ = w2pers(xyz, rot, campos)
    pl, _ = w2pers(loc, rot, campos)
    return torch.cat([xyz - loc, torch.stack([pp[:, 0] * pp[:, 2] - pl[:, 0] * pl[:, 2],
                                              pp[:, 1] * pp[:, 2] - pl[:, 1] * pl[:, 2], pp[:, 2] - pl[:, 2]], dim=-1)], dim=-1)


def row_inputs_ref(points, camera, raydir, query, K):
    """x0 [rows, 288] = [emb | PE(emb, 3) | PE(dists, 5) | 1 | 0 0 0], ext [rows, 8] = [colour | dir - v |
    <dir, v> | 1], rw [rows, 2] = (w clamp(conf, 1e-4, 1), w) with w the inverse-distance weight
    normalised over the sample's rows, vpe [items, 32] = [sin | cos of v 2^f, f < 4 | 1 | 0 ...]."""
    rs, _, pid, _ = row_index(query, K)
    S, rows = query["S"], rs.numel()
    dists = row_dists(points, camera, query, K)
    emb = _d(points["embedding"])[pid]
    x0 = torch.cat([emb, pe(emb, 3), pe(dists, 5), torch.ones(rows, 1, dtype=torch.float64),
                    torch.zeros(rows, 3, dtype=torch.float64)], dim=-1)
    v = _d(raydir)[query["samp_ray"][:S].to(torch.int64)]
    vr, pd = v[rs], _d(points["dir"])[pid]
    ext = torch.cat([_d(points["color"])[pid], pd - vr, (pd * vr).sum(-1, keepdim=True),
                     torch.ones(rows, 1, dtype=torch.float64)], dim=-1)
    w = 1.0 / torch.clamp(dists[:, :3].norm(dim=-1), min=1e-6)
    wsum = torch.zeros(S, dtype=torch.float64).index_add(0, rs, w)
    wn = w / torch.clamp(wsum, min=1e-8)[rs]
    cf = torch.clamp(_d(points["conf"]).reshape(-1)[pid], 1e-4, 1.0)
    rw = torch.stack([wn * cf, wn], dim=-1)
    work = torch.nonzero(query["samp_nnb"][:S] > 0).reshape(-1)
    vi = v[work]
    arg = (vi[:, :, None] * (2.0 ** torch.arange(4, dtype=torch.float64))).reshape(-1, 12)
    vpe = torch.cat([torch.sin(arg), torch.cos(arg), torch.ones(work.numel(), 1, dtype=torch.float64),
                     torch.zeros(work.numel(), 7, dtype=torch.float64)], dim=-1)
    return x0, ext, rw, vpe


def lrelu(x):
    return torch.where(x > 0, x, x * 0.01)


def dlrelu(x):
    """LeakyReLU'(x) as torch defines it: 1 for x > 0, else 0.01 (x = 0 included)."""
    return torch.where(x > 0, torch.ones_like(x), torch.full_like(x, 0.01))


def colour_head_ref(h3, w6, b6):
    """rgb [items, 3] = sigmoid(h3 W6^T + b6) 1.002 - 0.001."""
    return torch.sigmoid(_d(h3) @ _d(w6).t() + _d(b6)) * 1.002 - 0.001


def colour_head_bwd_ref(h3, w6, b6, drgb):
    """From d rgb [items, 3]: dy3 [items, 128] = (W6^T dy4) LReLU'(h3) with dy4 = d rgb 1.002 sig (1 - sig)
    (h3 is color_branch.4's output after its LeakyReLU, whose sign is its pre-activation's), dW6 [3, 128],
    db6 [3] and max |dy3|."""
    h3, w6 = _d(h3), _d(w6)
    sg = torch.sigmoid(h3 @ w6.t() + _d(b6))
    dy4 = _d(drgb) * 1.002 * sg * (1 - sg)
    dy3 = (dy4 @ w6) * dlrelu(h3)
    return dy3, dy4.t() @ h3, dy4.sum(0), dy3.abs().max() if dy3.numel() else torch.zeros((), dtype=torch.float64)


def row_head_ref(points, camera, raydir, query, K, z4, dfs, dalpha, rw, wa, ba):
    """block3.2's LeakyReLU, the alpha branch and the K-blend, backward.  z4 [rows, 256] block3.2's
    pre-activation, dfs [items, 256] = d f_s, dalpha [items] = d alpha_s, rw [rows, 2] the blend weights
    (w conf, w), wa [256], ba [1].  With h4 = LReLU(z4), za = <wa, h4> + ba, alpha = softplus(za - 1),
    f_s = sum_k w_k conf_k h4_k, alpha_s = sum_k w_k conf_k alpha_k:
    delta4 [rows, 256], d conf [N] (conf's clamp is straight-through: d conf = d (w conf) w), dWa [256],
    dba [1], max |delta4|."""
    _, _, pid, item = row_index(query, K)
    z4, dfs, dalpha, rw, wa, ba = (_d(t) for t in (z4, dfs, dalpha, rw, wa, ba))
    wa = wa.reshape(-1)
    h4 = lrelu(z4)
    x = h4 @ wa + ba.reshape(()) - 1.0
    alpha = torch.nn.functional.softplus(x)
    wc, wn = rw[:, 0], rw[:, 1]
    dza = wc * dalpha[item] * torch.sigmoid(x)
    delta4 = (wc[:, None] * dfs[item] + dza[:, None] * wa[None, :]) * dlrelu(z4)
    dwc = (h4 * dfs[item]).sum(-1) + alpha * dalpha[item]
    n = points["conf"].shape[0]
    dconf = torch.zeros(n, dtype=torch.float64).index_add(0, pid, dwc * wn)
    amax = delta4.abs().max() if delta4.numel() else torch.zeros((), dtype=torch.float64)
    return delta4, dconf, dza @ h4, dza.sum().reshape(1), amax


def row_tail_ref(points, camera, raydir, query, K, dx0, dext):
    """The rows' point gradients: dx0 [rows, 224] = d [emb | PE(emb, 3)], dext [rows, 8] = d [colour |
    dir - v | <dir, v> | .] -> d emb [N, 32], d colour [N, 3], d dir [N, 3] (index_add over the rows)."""
    rs, _, pid, _ = row_index(query, K)
    dx0, dext = _d(dx0), _d(dext)
    n = points["xyz"].shape[0]
    emb = _d(points["embedding"])[pid]
    bands = 2.0 ** torch.arange(3, dtype=torch.float64)
    arg = emb[:, :, None] * bands
    dpe = dx0[:, 32:224].reshape(-1, 32, 3, 2)   # (channel, frequency, sin / cos)
    de = dx0[:, :32] + ((dpe[..., 0] * torch.cos(arg) - dpe[..., 1] * torch.sin(arg)) * bands).sum(-1)
    v = _d(raydir)[query["samp_ray"][:query["S"]].to(torch.int64)][rs]
    z = lambda c: torch.zeros(n, c, dtype=torch.float64)  # noqa: E731
    return (z(32).index_add(0, pid, de), z(3).index_add(0, pid, dext[:, :3]),
            z(3).index_add(0, pid, dext[:, 3:6] + dext[:, 6:7] * v))
