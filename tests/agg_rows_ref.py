"""Scenes and float64 references for the kernel tests of the fp32-faithful aggregator: k_point_proj16,
k_pair_slots, k_rows16, k_color16 (csrc/mlp_x3.hip) and k_rows_exact / k_color_exact (csrc/exact.hip).

Every reference evaluates ONE layer from given inputs, so the GPU test (test_agg_rows_gpu.py) can feed it
the kernel's own previous output (P, z1, z2, zb, z3, f_s are all readable) and a failure names one layer;
`chain` strings the same functions into the whole aggregator, in float64 or -- the "fp32 floor" -- in torch
fp32 on the CPU.  test_agg_rows_ref_cpu.py pins the chain to train.aggregate / oracle/agg_ref.py and
checks, without a GPU, every planting promised here and every cap on the bounds below (the bounds depend
on the reference alone).

Rows are the valid (sample, neighbour) pairs in sample-major order (train_rows_ref.row_index); item i is
the sample work[i], whatever the order of the work list.
"""
import math

import torch
import torch.nn.functional as F

from train_rows_ref import N_POINTS, N_RAYS, compact_lists, lrelu, pe, row_dists, row_index, w2pers
from train_rows_ref import row_inputs_ref  # noqa: F401  (ext and rw of the GPU tests; row_inputs below is pinned to it)

U = 2.0 ** -24
PE_ATOL = 2e-6       # sin / cos of an exact fp32 argument (test_train_rows_gpu.py::test_row_inputs holds it)
LOCAL = 2e-6         # one split-path layer, per element, of the tensor's max (sgn_x3_gemm, products 3)
F32_TOL = 1e-5       # the project's fp32 bar: x max(1, max |ref|)
CAP = 1e-5           # no bound on P, z, f_s above this fraction of the tensor's max


# ---- named neighbour-count lists ------------------------------------------------------------------
# k_pair_slots ranks the items of a 1024-item block per count and pairs 7+1, 6+2, 5+3, 4+4 in rank order, then
# the leftover 1..4s consecutively.  One block cannot hold everything the kernel can do: a leftover 1 means
# n1 > n7, so no 7 is unpaired (likewise 2 / 6 and 3 / 5), and the only leftover that can stay alone is the
# last of the chain, which is then the single leftover 4 that a 3+4 pair needs.  Hence two lists.
# PAIRS: two of each of 7+1, 6+2, 5+3, 4+4 (B rotated by nA - 4 = 3, 2, 1, 0), leftovers 1+1, 1+2, 2+3, 3+4, 8s
PAIRS = [8, 7, 1, 8, 6, 2, 5, 3, 4, 4, 8, 1, 7, 2, 6, 3, 5, 4, 4, 8, 8, 1, 1, 1, 2, 2, 3, 3, 4, 8]
# PAIRS_HI: one of each pair, unpaired 7, 7, 6, 5, the odd leftover (a 4) alone, 8s
PAIRS_HI = [7, 1, 8, 6, 2, 5, 3, 7, 6, 5, 8, 4, 4, 4, 8, 7]


def with_empties(counts, every=3):
    """The list with a sample without any neighbour after every `every`-th item (and one in front)."""
    out = [0]
    for i, c in enumerate(counts):
        out.append(c)
        if i % every == every - 1:
            out.append(0)
    return out


def pairs():
    return with_empties(PAIRS)


def pairs_hi():
    return with_empties(PAIRS_HI)


def pairs53():
    """Twenty 5+3 pairs among a few others: nB = 3 is the one B size at which a wrong rotation of B's weights
    inside its quad reorders a sum of three values (two values, or one, sum to the same bits in any order), and
    then only an ulp moves -- enough pairs that some sample's weight sum must differ."""
    return with_empties([5, 3] * 20 + [8, 6, 2, 7, 1] * 2)


def pairs75():
    """PAIRS padded to 75 items (three chunks of a 32-item workspace, each paired on its own)."""
    pad = [(5 * i) % 8 + 1 for i in range(75 - len(PAIRS))]
    return with_empties(PAIRS + pad)


def full(n):
    return [8] * n


def rand(K, items, seed=11):
    """`items` samples with 1..K neighbours at random among ~30 % more without any; the first four items
    have (K, 1, 1, K) neighbours like train_rows_ref.synthetic_scene."""
    g = torch.Generator().manual_seed(seed * 1000 + K * 100 + items % 97)
    S = items + int(round(items * 0.3 / 0.7)) + 2
    pos = torch.sort(torch.randperm(S, generator=g)[:items]).values
    n = torch.zeros(S, dtype=torch.int64)
    n[pos] = torch.randint(1, K + 1, (items,), generator=g)
    if items >= 4:
        n[pos[:4]] = torch.tensor([K, 1, 1, K])
    return n.tolist()


def pair_slots(counts):
    """The pairing rule of k_pair_slots restated: counts = the work items' neighbour counts in work-list
    order -> one entry (A item, nA, B item or -1, nB) per slot, in slot order (per 1024-item block the lead
    items in list order; blocks in order)."""
    out = []
    for b0 in range(0, len(counts), 1024):
        blk = [min(max(c, 1), 8) for c in counts[b0:b0 + 1024]]
        by = {c: [i for i, x in enumerate(blk) if x == c] for c in range(1, 9)}   # stable rank per count
        n = {c: len(by[c]) for c in by}
        p = {1: min(n[1], n[7]), 2: min(n[2], n[6]), 3: min(n[3], n[5]), 4: 2 * (n[4] // 2)}
        left = [i for c in (1, 2, 3, 4) for i in by[c][p[c]:]]
        partner, lead = {}, set(range(len(blk)))
        for c in (7, 6, 5):
            for r in range(p[8 - c]):
                partner[by[c][r]] = by[8 - c][r]
                lead.discard(by[8 - c][r])
        for r in range(0, p[4], 2):
            partner[by[4][r]] = by[4][r + 1]
            lead.discard(by[4][r + 1])
        for j in range(0, len(left) - 1, 2):
            partner[left[j]] = left[j + 1]
            lead.discard(left[j + 1])
        for i in sorted(lead):
            b = partner.get(i, -1)
            out.append((b0 + i, blk[i], b0 + b if b >= 0 else -1, blk[b] if b >= 0 else 0))
    return out


# ---- the scene ------------------------------------------------------------------------------------
class Scene:
    """257 points in a cube of side 0.5, a fixed camera 1.05 .. 2.2 in front of them (the measured E of the
    camera-space dists grows with that distance, and its term of z1's bound must stay under the cap), 37 unit rays
    and one sample per entry of `counts` (its neighbour count, 0 = a sample without a neighbour), all fp32 / int32
    CPU tensors.  Planted: conf exactly 0, 1e-4, 1 and outside
    [1e-4, 1]; the first four items exactly at a neighbour (the weight's 1e-6 clamp); five slack samples past
    counters[0] that no list names; |emb| <= 4 (emb is a direct input of block1.0: the row kernels carry it as
    fp16 hi / lo pairs).  shuffle: the work list in a seeded random order, as sgn_query writes it (unordered);
    bpnet: BPNet rows [N, 96]."""

    def __init__(self, K, counts, seed=11, shuffle=False, bpnet=False, n_points=N_POINTS):
        self.K = K
        g = torch.Generator().manual_seed(seed * 1000 + K * 100 + len(counts) % 97)
        N, R = n_points, N_RAYS
        xyz = torch.rand(N, 3, generator=g) * 0.5 - 0.25   # a small cube near the camera: see cam_E
        emb = torch.clamp(torch.randn(N, 32, generator=g) * 1.5, -4.0, 4.0)
        conf = torch.rand(N, 1, generator=g) * 1.7 - 0.2
        for i, v in ((0, 0.0), (1, 1e-4), (2, 1.0), (N - 2, 1e-4), (N - 1, 1.0)):
            if 0 <= i < N:
                conf[i] = v
        color = torch.rand(N, 3, generator=g)
        pdir = F.normalize(torch.randn(N, 3, generator=g), dim=-1)
        yaw, pitch = math.radians(30.0), math.radians(-10.0)
        ry = torch.tensor([[math.cos(yaw), 0, math.sin(yaw)], [0, 1, 0], [-math.sin(yaw), 0, math.cos(yaw)]], dtype=torch.float64)
        rx = torch.tensor([[1, 0, 0], [0, math.cos(pitch), -math.sin(pitch)], [0, math.sin(pitch), math.cos(pitch)]],
                          dtype=torch.float64)
        self.camera = (torch.tensor([0.15, -0.1, -1.75]), (ry @ rx).float())
        self.raydir = F.normalize(torch.randn(R, 3, generator=g), dim=-1)
        S = len(counts)
        S_cap = S + 5
        nnb = torch.full((S_cap,), K, dtype=torch.int32)   # slack samples: never listed, never read
        nnb[:S] = torch.tensor(counts, dtype=torch.int32).reshape(-1)[:S] if S else nnb[:0]
        assert int(nnb.max()) <= K and int(nnb.min()) >= 0
        pidx = torch.randint(0, N, (S_cap, K), generator=g, dtype=torch.int32)
        pidx[torch.arange(K)[None, :] >= nnb[:, None]] = -1   # valid neighbours are a prefix of the K slots
        samp_ray = torch.randint(0, R, (S_cap,), generator=g, dtype=torch.int32)
        locw = xyz[torch.randint(0, N, (S_cap,), generator=g)] + 0.05 * torch.randn(S_cap, 3, generator=g)
        work = torch.nonzero(nnb[:S] > 0).reshape(-1)
        for j in range(min(4, work.numel())):   # a sample exactly at its (first / last) neighbour
            s = int(work[j])
            locw[s] = xyz[int(pidx[s, (int(nnb[s]) - 1) * (j & 1)])]
        if shuffle:
            work = work[torch.randperm(work.numel(), generator=g)]
        self.items = work.numel()
        self.work = work.to(torch.int32)
        self.points = dict(xyz=xyz, embedding=emb, color=color, dir=pdir, conf=conf)
        if bpnet:
            self.points["bpnet"] = torch.randn(N, 96, generator=g)
        self.query = dict(samp_ray=samp_ray, samp_locw=locw.contiguous(), samp_nnb=nnb, pidx=pidx,
                          counters=torch.tensor([S, self.items, 0, 0], dtype=torch.int32), S=S, S_cap=S_cap)
        self.S, self.S_cap, self.N = S, S_cap, N
        self.rs, self.rk, self.pid, _ = row_index(self.query, K)
        self.rows = self.rs.numel()
        pos = torch.full((S_cap,), -1, dtype=torch.int64)
        pos[work.long()] = torch.arange(self.items)
        self.item = pos[self.rs]                    # per row: its item = the position of its sample in the work list
        _, self.row_off, _ = compact_lists(nnb, S)
        self.work_counts = [int(nnb[int(s)]) for s in work]

    def pers32(self):
        """fp32 of the float64 camera-space coordinates: what a caller of the compatibility path passes."""
        campos, rot = (t.double() for t in self.camera)
        pp, _ = w2pers(self.points["xyz"].double(), rot, campos)
        pl, _ = w2pers(self.query["samp_locw"].double(), rot, campos)
        return pp.float().contiguous(), pl.float().contiguous()


# ---- one-layer references (dtype = that of the inputs; weights cast to it) ---------------------------
def _w(state, name, like):
    return state[name + ".weight"].to(like.dtype), state[name + ".bias"].to(like.dtype)


def layer_shift(w):
    """s with max |W| 2^s < 2^14, as mlp_x3.hip's layer_shift: 14 - e of frexp(max |W|); 0 for a zero layer."""
    m = float(w.float().abs().max())
    if not (m > 0 and math.isfinite(m)):
        return 0
    return 14 - math.frexp(m)[1]


def proj_ref(emb, state):
    """P = 2^s0 (W0a [emb | PE(emb, 3)] + b0): the per-point part of block1.0, scaled as the kernel stores it."""
    w, b = _w(state, "block1.0", emb)
    return (F.linear(torch.cat([emb, pe(emb, 3)], dim=-1), w[:, :224], b)) * 2.0 ** layer_shift(state["block1.0.weight"])


def z1_ref(p_rows, dists, state):
    """block1.0's pre-activation of a row from its point's P and its dists [rows, 6]."""
    w, _ = _w(state, "block1.0", dists)
    return p_rows * 2.0 ** -layer_shift(state["block1.0.weight"]) + F.linear(pe(dists, 5), w[:, 224:284])


def layer_ref(name, x, state):
    return F.linear(x, *_w(state, name, x))


def zb_ref(z2, bp_rows, state):
    """SG: block2_bpnet.0 on [lrelu(z2) | bpnet[pid]] (bp_rows None: bpnet_dim 0)."""
    h = lrelu(z2)
    return layer_ref("block2_bpnet.0", h if bp_rows is None else torch.cat([h, bp_rows.to(h.dtype)], dim=-1), state)


def z3_ref(z_in, ext, state):
    """block3.0 on [lrelu(z2 or zb) | colour, dir - v, <dir, v>]."""
    return layer_ref("block3.0", torch.cat([lrelu(z_in), ext[:, :7].to(z_in.dtype)], dim=-1), state)


def blend_ref(z3, rw0, item, n_items, state):
    """The one cut the library does not expose: z4 = W4 lrelu(z3) + b4, h4 = lrelu(z4), alpha_k = softplus(<wa,
    h4> + ba - 1), f_s = sum_k rw0_k h4_k, alpha_s = sum_k rw0_k alpha_k.  Returns f_s, alpha_s, z4, alpha_k."""
    z4 = layer_ref("block3.2", lrelu(z3), state)
    h4 = lrelu(z4)
    al = F.softplus(layer_ref("alpha_branch.0", h4, state).reshape(-1) - 1)
    rw0 = rw0.to(z3.dtype)
    fs = torch.zeros(n_items, 256, dtype=z3.dtype).index_add(0, item, rw0[:, None] * h4)
    a_s = torch.zeros(n_items, dtype=z3.dtype).index_add(0, item, rw0 * al)
    return fs, a_s, z4, al


def colour_ref(fs, v, state, hidden=None):
    """The four colour layers on [f_s | PE(v, 4)] (sin block then cos block), then sigmoid 1.002 - 0.001."""
    v = v.to(fs.dtype)
    arg = (v[:, :, None] * 2.0 ** torch.arange(4, dtype=fs.dtype)).reshape(-1, 12)
    c = torch.cat([fs, torch.sin(arg), torch.cos(arg)], dim=-1)
    for name in ("color_branch.0", "color_branch.2", "color_branch.4"):
        z = layer_ref(name, c, state)
        if hidden is not None:
            hidden.append(z)
        c = lrelu(z)
    return torch.sigmoid(layer_ref("color_branch.6", c, state)) * 1.002 - 0.001


def row_inputs(sc, dtype, pers=None):
    """dists [rows, 6], ext [rows, 7], rw [rows, 2] evaluated in `dtype` from the fp32 inputs (float64: equal to
    train_rows_ref.row_inputs_ref).  pers = (points' [N, 3], samples' [S, 3]): the camera-space dists from these
    values instead of the camera."""
    P, q = sc.points, sc.query
    t = lambda x: x.to(dtype)  # noqa: E731
    if pers is None:
        d = row_dists(P, sc.camera, q, sc.K, dtype=dtype)
    else:
        pp, pl = t(pers[0])[sc.pid], t(pers[1])[sc.rs]
        d = torch.cat([t(P["xyz"])[sc.pid] - t(q["samp_locw"])[sc.rs],
                       torch.stack([pp[:, 0] * pp[:, 2] - pl[:, 0] * pl[:, 2], pp[:, 1] * pp[:, 2] - pl[:, 1] * pl[:, 2],
                                    pp[:, 2] - pl[:, 2]], dim=-1)], dim=-1)
    v = t(sc.raydir)[q["samp_ray"][:sc.S].long()][sc.rs]
    pd = t(P["dir"])[sc.pid]
    ext = torch.cat([t(P["color"])[sc.pid], pd - v, (pd * v).sum(-1, keepdim=True)], dim=-1)
    w = 1.0 / torch.clamp(d[:, :3].norm(dim=-1), min=1e-6)
    wsum = torch.zeros(sc.S, dtype=dtype).index_add(0, sc.rs, w)
    wn = w / torch.clamp(wsum, min=1e-8)[sc.rs]
    cf = torch.clamp(t(P["conf"]).reshape(-1)[sc.pid], 1e-4, 1.0)
    return d, ext, torch.stack([wn * cf, wn], dim=-1)


def chain(sc, state, dtype=torch.float64, pers=None):
    """The whole aggregator from the raw inputs through the one-layer references, in `dtype`.  Returns a dict:
    P [N, 256], z1, z2, (zb,) z3, z4 [rows, 256], rw [rows, 2], fs [items, 256], alpha [items], rgb [items, 3]
    and hidden = the largest |pre-activation| of any hidden layer (the fp16-range question)."""
    sg = "block2_bpnet.0.weight" in state
    d, ext, rw = row_inputs(sc, dtype, pers)
    o = dict(rw=rw, dists=d, ext=ext)
    o["P"] = proj_ref(sc.points["embedding"].to(dtype), state)
    o["z1"] = z1_ref(o["P"][sc.pid], d, state)
    o["z2"] = layer_ref("block1.2", lrelu(o["z1"]), state)
    zin = o["z2"]
    if sg:
        bp = sc.points.get("bpnet") if state["block2_bpnet.0.weight"].shape[1] > 256 else None
        zin = o["zb"] = zb_ref(o["z2"], None if bp is None else bp[sc.pid], state)
    o["z3"] = z3_ref(zin, ext, state)
    o["fs"], o["alpha"], o["z4"], _ = blend_ref(o["z3"], rw[:, 0], sc.item, sc.items, state)
    hid = []
    v = sc.raydir[sc.query["samp_ray"][sc.work.long()].long()]
    o["rgb"] = colour_ref(o["fs"], v, state, hid)
    tens = [o[k] for k in ("z1", "z2", "z3", "z4", "fs") if o[k].numel()] + ([o["zb"]] if sg and o["zb"].numel() else []) + \
           [h for h in hid if h.numel()]
    o["hidden"] = max([float(t.abs().max()) for t in tens], default=0.0)
    return o


def scale_block12(state, f):
    out = dict(state)
    out["block1.2.weight"] = state["block1.2.weight"] * f
    return out


def range_state(sc, state, target):
    """`state` with block1.2's weights scaled by a power of two so the float64 chain's largest hidden
    pre-activation is within a factor sqrt(2) of `target`."""
    f = 1.0
    for _ in range(6):
        h = chain(sc, scale_block12(state, f))["hidden"]
        step = 2.0 ** round(math.log2(target / h))
        if step == 1.0:
            break
        f *= step
    return scale_block12(state, f), f


# ---- bounds (functions of the reference alone) and their caps ------------------------------------------
def amax(t):
    return float(t.abs().max()) if t.numel() else 0.0


def cam_E(sc):
    """E of the camera-space dists: 4 x the fp32 - float64 difference of the aggregator's formula on these
    inputs, as test_train_rows_gpu.py::test_row_inputs measures it."""
    if sc.rows == 0:
        return 0.0
    d64 = row_dists(sc.points, sc.camera, sc.query, sc.K)
    d32 = row_dists(sc.points, sc.camera, sc.query, sc.K, dtype=torch.float32)
    return 4 * float((d32[:, 3:].double() - d64[:, 3:]).abs().max())


def bound_P(ref, state):
    """The local bar plus the 192 PE(emb) columns at PE_ATOL, carried by sum |w| over those columns."""
    w = state["block1.0.weight"].double()
    return LOCAL * amax(ref) + PE_ATOL * w[:, 32:224].abs().sum(1)[None, :] * 2.0 ** layer_shift(state["block1.0.weight"])


def bound_z1(ref, state, E):
    """The local bar plus the 60 PE(dists) columns: PE_ATOL for the world dists (exact fp32 arguments),
    PE_ATOL + 2^f E for the camera-space ones.  Column (c 5 + f) 2 + (sin | cos) of component c, frequency f."""
    w = state["block1.0.weight"].double()[:, 224:284].abs()
    e = torch.full((6, 5, 2), PE_ATOL, dtype=torch.float64)
    e[3:] += (2.0 ** torch.arange(5, dtype=torch.float64))[None, :, None] * E
    return LOCAL * amax(ref) + (w @ e.reshape(60))[None, :]


def bound_z3(ref, state):
    """The local bar plus the kernel's own ext inputs (dir - v, <dir, v>: at most 4 roundings of values <= 2)."""
    w = state["block3.0.weight"].double()[:, 256:263].abs().sum(1)
    return LOCAL * amax(ref) + 8 * U * w[None, :]


def bound_fs(z4, rw0, item, n_items):
    """block3.2's local bar through LeakyReLU (<= 1) and the blend (x sum_k rw0_k), the blend sum of <= 8 terms
    (2 9 u sum |terms|) and the kernel's own blend weights (32 u relative, the bar (c) holds them to)."""
    z4, rw0 = z4.double(), rw0.double()
    terms = torch.zeros(n_items, 256, dtype=torch.float64).index_add(0, item, rw0[:, None] * lrelu(z4).abs())
    wsum = torch.zeros(n_items, dtype=torch.float64).index_add(0, item, rw0)
    return LOCAL * amax(z4) * wsum[:, None] + (2 * 9 + 32) * U * terms


def chain_bar(ref64, ref32, unit=False):
    """max(2e-6 max |ref|, 4 x floor), floor = the torch-fp32 CPU evaluation's largest error against float64
    (measured on the reference, never on the kernel).  unit: the scale is max(1, max |ref|) (alpha, rgb, weights)."""
    s = amax(ref64)
    return max(LOCAL * (max(1.0, s) if unit else s), 4.0 * amax(ref32.double() - ref64))


def capped(bound, ref, what, unit=False):
    """The bound stays below F32_TOL max(1, max |ref|) (unit) or CAP max |ref|."""
    if ref.numel() == 0:
        return
    b = float(torch.as_tensor(bound).max())
    s = max(1.0, amax(ref)) if unit else amax(ref)
    assert b < (F32_TOL if unit else CAP) * s, f"{what}: bound {b:.3e} is not below 1e-5 x the reference's scale {s:.3e}"


def alpha_bar(z3, rw0, item, n_items, state, a64):
    """alpha_s from z3 crosses two layers with no cut between them (block3.2, then the 256-term alpha dot whose
    sum |wa| ~ 20 would carry block3.2's local bar far past F32_TOL): the chain bar of that two-layer piece, the
    floor being blend_ref in torch fp32 from the same z3."""
    a32 = blend_ref(z3.float(), rw0.float(), item, n_items, state)[1]
    return chain_bar(a64, a32, unit=True)


# ---- the scenes of the GPU tests, by name -------------------------------------------------------------
_SCENES = {
    "none": (8, lambda: []), "one": (8, lambda: [0, 1, 0]), "pairs": (8, pairs), "pairs_hi": (8, pairs_hi),
    "pairs_shuf": (8, pairs), "pairs53": (8, pairs53), "pairs75": (8, pairs75), "full4099": (8, lambda: full(4099)),
    "rand1_777": (1, lambda: rand(1, 777)), "rand3_777": (3, lambda: rand(3, 777)), "rand5_777": (5, lambda: rand(5, 777)),
    "rand8_300": (8, lambda: rand(8, 300)), "rand1_16387": (1, lambda: rand(1, 16387)),
}
for _n in (7, 8, 9, 15, 16, 17):
    _SCENES[f"full{_n}"] = (8, lambda _n=_n: full(_n))
_CACHE = {}


def scene(name):
    if name not in _CACHE:
        K, counts = _SCENES[name]
        _CACHE[name] = Scene(K, counts(), shuffle=name.endswith("_shuf"), bpnet=True)
    return _CACHE[name]


def check_caps(sc, state, o=None, pers=None):
    """Every cap of the local and chain bars on this scene, from the reference alone.  Returns the bounds."""
    o = o or chain(sc, state, pers=pers)
    b = dict(P=bound_P(o["P"], state), z1=bound_z1(o["z1"], state, cam_E(sc)), z2=LOCAL * amax(o["z2"]),
             z3=bound_z3(o["z3"], state), fs=bound_fs(o["z4"], o["rw"][:, 0], sc.item, sc.items))
    if "zb" in o:
        b["zb"] = LOCAL * amax(o["zb"])
    for k, v in b.items():
        capped(v, o["P" if k == "P" else k], k)
    b["alpha"] = alpha_bar(o["z3"], o["rw"][:, 0], sc.item, sc.items, state, o["alpha"])
    capped(b["alpha"], o["alpha"], "alpha_s", unit=True)
    return b, o


def chain_bars(sc, state, pers=None, o64=None):
    """The chain bars of alpha_s, f_s, rgb, blend and wnorm (float64 chain against the fp32 floor), capped."""
    o64 = o64 or chain(sc, state, pers=pers)
    o32 = chain(sc, state, dtype=torch.float32, pers=pers)
    b = dict(alpha=chain_bar(o64["alpha"], o32["alpha"], True), rgb=chain_bar(o64["rgb"], o32["rgb"], True),
             blend=chain_bar(o64["rw"][:, 0], o32["rw"][:, 0], True), wnorm=chain_bar(o64["rw"][:, 1], o32["rw"][:, 1], True),
             fs=chain_bar(o64["fs"], o32["fs"]))
    for k in ("alpha", "rgb"):
        capped(b[k], o64[k], k, unit=True)
    capped(b["blend"], o64["rw"][:, 0], "blend", unit=True)
    capped(b["wnorm"], o64["rw"][:, 1], "wnorm", unit=True)
    capped(b["fs"], o64["fs"], "f_s")
    return b, o64


# ---- point tables of the projection test -------------------------------------------------------------
def point_table(n, state):
    """n points for sgn_point_project_f32 (|emb| <= 4).  Below 100 points the tensor's max is too small for the
    PE(emb) term of the bound (it does not shrink with n) to stay under the cap, so point 0's embedding then lines
    up with block1.0's first row and a direct column sets the scale."""
    g = torch.Generator().manual_seed(77 + n)
    emb = torch.clamp(torch.randn(n, 32, generator=g) * 1.5, -4.0, 4.0)
    if n < 100:
        emb[0] = 4.0 * torch.sign(state["block1.0.weight"][0, :32])
    return dict(xyz=torch.randn(n, 3, generator=g), embedding=emb, color=torch.rand(n, 3, generator=g),
                dir=F.normalize(torch.randn(n, 3, generator=g), dim=-1), conf=torch.rand(n, 1, generator=g))


# ---- the colour stage alone ----------------------------------------------------------------------------
class ColourCase:
    """`items` work items among ~30 % samples that are none, 37 unit rays, an f_s the test writes itself
    (randn x 3) and a finite pre-filled feat; shuffle: a non-ascending work list."""

    def __init__(self, items, shuffle=False, seed=23):
        g = torch.Generator().manual_seed(seed * 1000 + items % 997)
        self.items = items
        self.S = S = items + int(round(items * 0.3 / 0.7)) + 2
        self.S_cap = S + 5
        self.raydir = F.normalize(torch.randn(N_RAYS, 3, generator=g), dim=-1)
        self.samp_ray = torch.randint(0, N_RAYS, (self.S_cap,), generator=g, dtype=torch.int32)
        work = torch.sort(torch.randperm(S, generator=g)[:items]).values
        if shuffle:
            work = work[torch.randperm(items, generator=g)]
        self.work = work.to(torch.int32)
        self.fs = torch.randn(items, 256, generator=g) * 3
        self.feat0 = torch.randn(self.S_cap, 4, generator=g)
        self.v = self.raydir[self.samp_ray[work].long()]


_COLOUR = {}


def colour_case(items, shuffle=False):
    if (items, shuffle) not in _COLOUR:
        _COLOUR[(items, shuffle)] = ColourCase(items, shuffle)
    return _COLOUR[(items, shuffle)]


def colour_bar(case, state, fs=None):
    """The colour stage's chain bar (f_s -> rgb, no cut in between) and its float64 reference."""
    fs = case.fs if fs is None else fs
    r64 = colour_ref(fs.double(), case.v, state)
    r32 = colour_ref(fs.float(), case.v, state)
    b = chain_bar(r64, r32, unit=True)
    capped(b, r64, "rgb", unit=True)
    return b, r64
