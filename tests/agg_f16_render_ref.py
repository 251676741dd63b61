"""Float64 references, with the kernels' own roundings, of the three f16 render kernels of csrc/mlp.hip:
k_point_proj (sgn_point_project), k_color<ROT> (sgn_aggregate, stages = 2) and the split block1.0 form of
k_agg_rows (sgn_aggregate with d_point_proj given, stages = 1), on top of agg_f16_ref.py, agg_rows_ref.py and
rw2c_ref.py.  test_agg_f16_render_ref_cpu.py proves them without a GPU (roundings off: agg_rows_ref's float64
functions; roundings on: fp32 torch emulations pass, planted errors fail); test_agg_f16_render_gpu.py calls the
C ABI.

k_point_proj: one layer, INTERVAL check (agg_f16_ref.py's docstring).  P = fp16(b0 + fp16(W0a) [fp16(emb) |
fp16(PE(emb, 3))]), 224 inputs, fp32 accumulate.  Two intervals, both asserted, no element excluded from either:
  "P (e_f)"  z0 from x = rn16(float64 sin / cos), E0 = (224 + 1) u (|b| + sum |w| |x|) + sum |w| e_f, e_f = 2^f E_PE the
             PE-column bound agg_f16_ref.py holds: every element in [rn16(z0 - E0), rn16(z0 + E0)].
  "P"        the same bound carried through the input's own fp16 rounding.  e_f bounds a PE value BEFORE it is rounded;
             the fp16 input then lies in [rn16(s - e_f), rn16(s + e_f)], one value on most columns and two neighbours
             (an fp16 ulp apart, 30 .. 100 x e_f) on the 9 % whose s sits within e_f of a rounding boundary.  z at the
             interval's midpoint, E = (224 + 1) u (|b| + sum |w| max |x|) + sum |w| d, d the column's half-width: tighter
             than E0 wherever no input straddles, and valid where one does.
k_point_proj's PE stayed on the float64 value's side of every boundary: no element left either interval on the MI355X.
Layout: P[p][t][h][r] = unit 32 t + acc_unit(r, h), acc_unit restated from mlp_layout.h (it is NOT
sgn_train_colmap(0)'s order, which is the chained B-operand order 16 ks + perm_acc).

k_color and the split k_agg_rows expose no tensor between their input and their output: CHAIN bars, measured on
the reference, never on the kernel.  floor = the largest per-element difference between the float64 model (fp16
weights, fp16 inputs, lrelu16 after every fp16 layer, everything after the last fp16 tensor at float64) and a torch
fp32 emulation of the same rounded chain (same fp16 weights and roundings, PE by the kernels' fp32 angle-doubling
recurrence, fp32 accumulation) on the same case; bar = max(2e-6 max(1, max |ref|), 4 x floor)
(agg_rows_ref.chain_bar).  What the floor consists of: the two evaluations round a hidden fp16 activation to
different neighbours where its pre-activation lies within the fp32 accumulation error of a rounding boundary, and
each such flip moves the output by its weight times an fp16 ulp.  The kernel's accumulation order is a third one.
Colour stage: 4 .. 9 % of the samples hold a flip (a sample without one agrees to 1e-7), and a flip moves rgb by
anything from 1e-6 to 1e-3.  So (a) the floor of a case below 300 samples is taken together with the 300-sample case
(colour_population: the largest of 0 .. 15 flips estimates nothing; on the MI355X the 32-sample case needed 33 x its
own floor, 0.68 of the bar of the population's), and (b) beside the bar the number of samples off the model by more
than 2e-6 is held to 4 x the emulation's share (check_colour): the one check that sees an error of a flip's own
size in every sample.  Figures (init_mlp(5, bias_std=0.1); the floors move a little with the host's BLAS):
    rgb floor 9.6e-5 .. 4.3e-4 up to 300 samples (3e-8 .. 3.8e-4 for the cases alone), 7.9e-4 .. 1.0e-3 at 65539; bar
    3.8e-4 .. 1.7e-3 and 3.2e-3 .. 4.0e-3.  A swapped layer-0 fragment moves rgb by 0.88 or more, a negated cos octave by
    0.13 or more: the bar is at most 0.018 of the smaller (COLOUR_CAP: a tenth).  A y1 packed toward zero moves rgb by
    1.1e-3 .. 2.3e-3, 0.3 .. 1.8 x the bar: no whole-case bar can stay a tenth below one flip's size, and (b) holds it.
    split rows: f_s floor 6.8e-4 .. 2.3e-3 (one or two fp16 ulps of the largest elements, max |f_s| 2.3 .. 7.7), bar 2.7e-3 ..
    9.2e-3, beside an interval bound of 1.2e-4 .. 2.8e-4 plus half an ulp for the unsplit kernel (which agg_f16_ref cuts
    at h3); alpha_s floor 8.6e-6 .. 5.9e-4, bar 3.5e-5 .. 2.4e-3, beside 2.0e-3 .. 4.5e-3.
out_blend / out_wnorm: agg_f16_ref.W_REL (32 u relative), exactly 0 on a listed sample's empty slots.
"""
import torch

import agg_f16_ref as fr
import agg_rows_ref as ar
import rw2c_ref as rw
from train_rows_ref import lrelu

U = fr.U
E_PE = fr.E_PE
C16H = torch.tensor(0.01).half()
COLOUR_CAP = 0.1      # the colour bar stays below this share of the smallest planted colour error's max |d rgb|


# ---- layout ------------------------------------------------------------------------------------------
def acc_unit(r, h):
    """mlp_layout.h: the unit of a 32-wide tile held by accumulator register r of lane-half h."""
    return (r & 3) + 8 * (r >> 2) + 4 * h


def proj_map(swap_h=False):
    """P[p]'s 256 fp16 positions [t][h][r] -> the block1.0 unit each holds (swap_h: the other lane-half's, a plant)."""
    return torch.tensor([32 * t + acc_unit(r, h ^ int(swap_h)) for t in range(8) for h in range(2) for r in range(16)],
                        dtype=torch.int64)


PM = proj_map()


# ---- positional encodings ----------------------------------------------------------------------------
def _rec32(x, freqs):
    """fp32 sin / cos [.., C, freqs] by the kernels' recurrence: octave 0 direct, then sin 2a = 2 sin a cos a,
    cos 2a = (cos a - sin a)(cos a + sin a)."""
    s, c = torch.sin(x), torch.cos(x)
    S, C = [s], [c]
    for _ in range(1, freqs):
        s, c = 2.0 * s * c, (c - s) * (c + s)
        S.append(s)
        C.append(c)
    return torch.stack(S, -1), torch.stack(C, -1)


def pe32(x, freqs):
    """block1.0's order (channel, octave, (sin, cos)) from the fp32 recurrence."""
    S, C = _rec32(x.float(), freqs)
    return torch.stack([S, C], -1).reshape(x.shape[:-1] + (x.shape[-1] * freqs * 2,))


def vpe(v, rec=False, neg_cos=None):
    """PE(viewdir, 4) in the colour MLP's order: the sin block [d 4 + f], then the cos block.  rec: the fp32
    recurrence, else sin / cos in v's dtype; neg_cos: the cos block negated at that octave (a plant)."""
    if rec:
        S, C = _rec32(v.float(), 4)
    else:
        arg = v[:, :, None] * (2.0 ** torch.arange(4, dtype=v.dtype, device=v.device))
        S, C = torch.sin(arg), torch.cos(arg)
    if neg_cos is not None:
        C = C.clone()
        C[..., neg_cos] = -C[..., neg_cos]
    return torch.cat([S.reshape(-1, 12), C.reshape(-1, 12)], dim=-1)


def _q(x, exact):
    return x if exact else fr.rn16(x)


def _act(z, exact):
    return lrelu(z) if exact else fr.lrelu16(fr.rn16(z))


def lrelu_pk(z32, toward_zero=False):
    """The kernels' lrelu_pk on an fp32 tensor: fp16 pack (toward_zero: truncated, a plant), max(v, v fp16(0.01))."""
    v = fr.rn16(z32.double(), toward_zero=True).half() if toward_zero else z32.half()
    return torch.maximum(v, v * C16H.to(v.device))


# ---- 1. k_point_proj ---------------------------------------------------------------------------------
def proj_model(emb, net, exact=False):
    """b0 + W0a [emb | PE(emb, 3)] in float64, before the store's fp16 rounding (natural unit order)."""
    e = emb.double()
    x = torch.cat([_q(e, exact), _q(fr.pe(e, 3), exact)], dim=-1)
    return x @ net.W0[:, :224].t() + net.b0


def check_proj(rep, cut, tile, emb, net):
    """tile: P rows [n, 256] fp16 in the kernel's layout; emb [n, 32] fp32, on net's device."""
    e = emb.double()
    s = fr.pe(e, 3)
    ef = ((2.0 ** torch.arange(3, dtype=torch.float64, device=e.device)) * E_PE)[None, :, None].expand(32, 3, 2).reshape(192)
    lo, hi = fr.rn16(s - ef), fr.rn16(s + ef)
    e16 = fr.rn16(e)
    W, Wa = net.W0[:, :224], net.W0[:, :224].abs()
    xm = torch.cat([e16, (lo + hi) / 2], dim=-1)
    xa = torch.cat([e16.abs(), torch.maximum(lo.abs(), hi.abs())], dim=-1)
    z = xm @ W.t() + net.b0
    E = 225 * U * (xa @ Wa.t() + net.b0.abs()) + ((hi - lo) / 2) @ Wa[:, 32:].t()
    got = fr.to_nat(tile, PM, 256)
    z0 = torch.cat([e16, fr.rn16(s)], dim=-1) @ W.t() + net.b0
    fr._interval(rep, cut, got, fr.rn16(z - E), fr.rn16(z + E), E, z, centre=fr.rn16(z0))
    E0 = 225 * U * (xa @ Wa.t() + net.b0.abs()) + (ef @ Wa[:, 32:].t())[None, :]
    fr._interval(rep, cut + " (e_f)", got, fr.rn16(z0 - E0), fr.rn16(z0 + E0), E0, z0)
    rep.count("lit_out", ((got < fr.rn16(z0 - E0)) | (got > fr.rn16(z0 + E0))).sum())
    rep.count("lit_n", got.numel())
    rep.count("straddle", (hi != lo).sum())
    rep.count("pe_cols", hi.numel())


def show_proj(rep, what):
    rep.show(what)
    x = rep.extra
    if x.get("lit_n"):
        print(f"{what} PE inputs whose interval holds two fp16 values: {x['straddle']} of {x['pe_cols']}; P elements outside "
              f"the interval of sum |w| e_f alone: {x['lit_out']} of {x['lit_n']}")


def proj_emu(emb, st, swap_h=False):
    """k_point_proj in torch fp32: P rows [n, 256] fp16 in the kernel's layout."""
    x = torch.cat([emb.float(), pe32(emb, 3)], dim=-1).half()
    z = x.float() @ st["block1.0.weight"][:, :224].half().float().t() + st["block1.0.bias"].float()
    return fr.from_nat(z, proj_map(swap_h))


# ---- 2. k_color --------------------------------------------------------------------------------------
COL = ("color_branch.0", "color_branch.2", "color_branch.4")


class ColNet:
    """The colour weights as k_color holds them, float64: fp16(W) of the three 128-unit layers (exact: W itself),
    fp32 biases and an fp32 head."""

    def __init__(self, state, device="cpu", exact=False):
        self.W = [(state[n + ".weight"] if exact else state[n + ".weight"].half()).double().to(device) for n in COL]
        self.b = [state[n + ".bias"].double().to(device) for n in COL]
        self.W3, self.b3 = state["color_branch.6.weight"].double().to(device), state["color_branch.6.bias"].double().to(device)


def colour_model(fs, v, cn, exact=False):
    """rgb [n, 3] float64 from f_s [n, 256] and the view directions [n, 3] (the kernel's own fp32 values)."""
    x = torch.cat([_q(fs.double(), exact), _q(vpe(v.double()), exact)], dim=-1)
    y = _act(x @ cn.W[0].t() + cn.b[0], exact)
    y = _act(y @ cn.W[1].t() + cn.b[1], exact)
    y = lrelu(y @ cn.W[2].t() + cn.b[2])
    return torch.sigmoid(y @ cn.W3.t() + cn.b3) * 1.002 - 0.001


def colour_emu(fs, v, st, plant=None):
    """k_color in torch fp32.  plant: "frag swap" (the 16-column fragment 3 of layer 0 swapped with fragment 4),
    "cos neg" (the cos block of PE(viewdir) negated at octave 2), "y1 rtz" (y1 packed toward zero)."""
    W = [st[n + ".weight"].half().float() for n in COL]
    b = [st[n + ".bias"].float() for n in COL]
    if plant == "frag swap":
        W[0] = torch.cat([W[0][:, :48], W[0][:, 64:80], W[0][:, 48:64], W[0][:, 80:]], dim=1)
    x = torch.cat([fs.half(), vpe(v, rec=True, neg_cos=2 if plant == "cos neg" else None).half()], dim=-1)
    y = lrelu_pk(x.float() @ W[0].t() + b[0], plant == "y1 rtz")
    y = lrelu_pk(y.float() @ W[1].t() + b[1])
    z = y.float() @ W[2].t() + b[2]
    y = torch.maximum(z, 0.01 * z)
    o = y @ st["color_branch.6.weight"].float().t() + st["color_branch.6.bias"].float()
    return torch.sigmoid(o) * 1.002 - 0.001


COLOUR_PLANTS = ("frag swap", "cos neg", "y1 rtz")


def case_viewdirs(case, rot=None):
    """The view direction of every sample of a ColourCase [S_cap, 3] fp32: its ray's, or (rot [N, 3, 3]) that ray
    turned by the Rw2c of the sample's slot-0 neighbour, as rw2c_ref.sample_viewdirs gives it."""
    if rot is None:
        return case.raydir[case.samp_ray.long()]
    g = torch.Generator().manual_seed(case.S_cap)
    case.query = dict(pidx=torch.randint(0, rot.shape[0], (case.S_cap, 1), generator=g, dtype=torch.int32), samp_ray=case.samp_ray)
    S, case.S = case.S, case.S_cap
    out = rw.sample_viewdirs(case, rot).float()
    case.S = S
    return out


POP = 300             # a colour case below this many samples measures its floor together with the POP-sample case


def colour_population(items, shuffle, rot):
    """The cases a colour bar is measured on, [(case, view directions of its listed samples)]: the case itself and,
    below POP samples, the POP-sample case of the same kind (ordered / shuffled, plain / rotated).  A case of 1 .. 257
    samples holds 0 .. 15 samples with a flipped rounding, each moving rgb by anything from 1e-6 to 1e-3: the largest
    of so few is no estimate of what one more flip, in the kernel's order, can do (MI355X: 6.7e-4 on the 32-sample
    case whose own two flips reach 2.0e-5, 33 x its floor)."""
    out = []
    for n in [items] + ([POP] if items < POP else []):
        c = ar.colour_case(n, shuffle)
        out.append((c, case_viewdirs(c, rw.palette_rot(ar.N_POINTS) if rot else None)[c.work.long()]))
    return out


def colour_bar(items, shuffle, rot, st, device="cpu"):
    """The colour stage's chain bar on a case: dict(bar, floor, ref = the float64 model [items, 3], emu = the fp32
    emulation, both of the case itself; v = its listed samples' view directions; moves = the planted errors' max |d rgb|;
    share = the emulation's noisy samples / samples), floor and moves being maxima, share the ratio, over
    colour_population.  The f_s the kernel reads is the case's, cast to fp16."""
    cn = ColNet(st, device)
    floor, scale, moves, first, nz, tot = 0.0, 1.0, {p: 0.0 for p in COLOUR_PLANTS}, None, 0, 0
    for c, v in colour_population(items, shuffle, rot):
        fs16 = c.fs.half()
        r64 = colour_model(fs16.to(device), v.to(device), cn).cpu()
        r32 = colour_emu(fs16, v, st)
        floor, scale = max(floor, ar.amax(r32.double() - r64)), max(scale, ar.amax(r64))
        for p in COLOUR_PLANTS:
            moves[p] = max(moves[p], ar.amax(colour_emu(fs16, v, st, p) - r32))
        first = first or dict(ref=r64, emu=r32, v=v, case=c)
        nz, tot = nz + noisy(r32, r64), tot + c.items
    return dict(first, bar=max(ar.LOCAL * scale, 4.0 * floor), floor=floor, moves=moves, share=nz / tot)


NOISE = 2e-6          # a sample is "noisy" when its rgb is off the float64 model by more than NOISE max(1, max |ref|)


def noisy(got, ref):
    """The number of samples whose rgb is off the float64 model by more than the project's fp32 noise bar: those in
    which some hidden fp16 activation was rounded to the other neighbour."""
    if ref.numel() == 0:
        return 0
    return int(((got.double().cpu() - ref).abs().max(1).values > NOISE * max(1.0, ar.amax(ref))).sum())


def check_colour(rep, cut, got, b):
    """rgb [n, 3] against the float64 model at the chain bar of colour_bar's dict b, and the number of noisy samples
    against 4 x the number the emulation's share of them on the population predicts for n samples (at least 4: the
    count is Poisson, and four times an expectation below one sample measures nothing).  The second check is what
    holds an error that moves every sample a little (fp16 packed toward zero: at most 1e-3 .. 2e-3, the size of one
    flipped rounding and so of the chain bar itself) -- the emulation is within NOISE on 91 .. 96 % of the samples, a
    truncating pack on 0 .. 3 %."""
    ref = b["ref"]
    fr._absbound(rep, cut, got.cpu(), ref, torch.full_like(ref, b["bar"]), torch.zeros_like(ref))
    allowed = max(4, int(4 * b["share"] * ref.shape[0] + 0.999))
    k = noisy(got, ref)
    rep.add(cut + " noisy samples", torch.tensor([k / allowed]), torch.tensor([k > allowed]), torch.zeros(()), torch.zeros(1))
    return k, allowed


# ---- 3. the split k_agg_rows ---------------------------------------------------------------------------
class RRows(fr.Rows):
    """agg_f16_ref.Rows with the render path's inputs: pers = (points' [N, 3], samples' [S, 3]) camera-space
    coordinates given by the caller, rot [N, 3, 3] / vdir [S.., 3] rotated neural points (rw2c_ref's rules; base
    network), plus the same inputs evaluated in torch fp32 for the emulation (d32, ext32, wgt32)."""

    def __init__(self, sc, n=None, bp16=None, pers=None, rot=None, vdir=None, exact=False):
        super().__init__(sc, n, bp16=bp16, exact=exact)
        keep = sc.item < self.n
        idx = (8 * sc.item + sc.rk)[keep]

        def inputs(dtype):
            if rot is not None:
                return rw.row_inputs(sc, rot, dtype, vdir)
            return ar.row_inputs(sc, dtype, pers)
        d64, e64, _ = inputs(torch.float64)
        if rot is not None:     # the world half: R_p times the kernel's own fp32 offset
            dw = (sc.points["xyz"][sc.pid] - sc.query["samp_locw"][sc.rs]).double()
            self.dists[idx, :3] = (d64[:, :3] if exact else rw.mv(rot.double()[sc.pid], dw))[keep]
            self.ext[idx] = e64[keep]
        if pers is not None:
            self.dists[idx, 3:] = d64[keep, 3:]
        d32, e32, w32 = inputs(torch.float32)
        z = lambda c: torch.zeros(8 * self.n, c)  # noqa: E731
        self.d32, self.ext32, self.wgt32 = z(6), z(7), torch.zeros(8 * self.n)
        self.d32[idx], self.ext32[idx], self.wgt32[idx] = d32[keep], e32[keep], w32[keep, 0]

    def chunk(self, i0, i1, device="cpu"):
        c = super().chunk(i0, i1, device)
        for k in ("d32", "ext32", "wgt32"):
            setattr(c, k, getattr(self, k)[8 * i0:8 * i1].to(device))
        return c


def rows_model(rc, net, Pn, exact=False):
    """The split aggregator on a chunk of rows: block1.0 = P[pid] + W0b PE(dists) (Pn [N, 256] float64, natural
    unit order: the table k_point_proj wrote; a masked slot reads P[0]), then agg_f16_ref's chain.  Returns
    blend_ref's dict (fs, alpha unrounded)."""
    x0, _ = fr.x0_ref(rc)
    z1 = Pn[rc.pid.clamp(min=0)] + _q(x0[:, 224:284], exact) @ net.W0[:, 224:284].t()
    h = _act(fr.dot(_act(z1, exact), net.W1, net.b1)[0], exact)
    if net.sg:
        h = _act(fr.dot(h if rc.bp is None or net.bp_dim == 0 else torch.cat([h, rc.bp], dim=1), net.WB, net.bB)[0], exact)
    h3 = _act(fr.dot(torch.cat([h, _q(rc.ext, exact)], dim=1), net.W2, net.b2)[0], exact)
    return fr.blend_ref(h3, rc, net)


ROW_PLANTS = ("h swap", "next tile", "ragged", "masked wgt")


def rows_emu(rc, st, tile, plant=None):
    """The split k_agg_rows in torch fp32 (CPU) on a chunk: tile = P rows [N, 256] fp16 in the kernel's layout.
    Returns f_s [n, 256] fp16 and alpha_s [n] fp32.  plant: "h swap" (items 4 .. 7 read P's other lane-half), "next
    tile" (items 4 .. 7 take the P rows of items 8 .. 11), "ragged" (the last 3 items never stored: NaN), "masked wgt"
    (a masked slot keeps its neighbour's weight)."""
    sg = "block2_bpnet.0.weight" in st
    w = lambda k: st[k + ".weight"].half().float()  # noqa: E731
    b = lambda k: st[k + ".bias"].float()  # noqa: E731
    Pn = fr.to_nat(tile, PM, 256).float()
    pid = rc.pid.clamp(min=0)
    p = Pn[pid]
    if plant == "h swap":
        p[32:64] = fr.to_nat(tile, proj_map(True), 256).float()[pid[32:64]]
    elif plant == "next tile":
        p[32:64] = Pn[pid[64:96]]
    z1 = p + pe32(rc.d32, 5).half().float() @ w("block1.0")[:, 224:284].t()
    h = lrelu_pk(lrelu_pk(z1).float() @ w("block1.2").t() + b("block1.2"))
    if sg:
        hb = h if rc.bp is None or st["block2_bpnet.0.weight"].shape[1] == 256 else torch.cat([h, rc.bp.half()], dim=1)
        h = lrelu_pk(hb.float() @ w("block2_bpnet.0").t() + b("block2_bpnet.0"))
    h3 = lrelu_pk(torch.cat([h, rc.ext32.half()], dim=1).float() @ w("block3.0").t() + b("block3.0"))
    z4 = h3.float() @ w("block3.2").t() + b("block3.2")
    h4 = torch.maximum(z4, z4 * 0.01)
    wgt, n = rc.wgt32.clone(), rc.n
    if plant == "masked wgt":
        m = int(torch.nonzero(~rc.valid)[3])
        wgt[m] = wgt[m - 1] if float(wgt[m - 1]) > 0 else 0.25
    wa, ba = st["alpha_branch.0.weight"].float().reshape(-1), st["alpha_branch.0.bias"].float()
    fs = (wgt[:, None] * h4).view(n, 8, 256).sum(1).half()
    al = (wgt * torch.nn.functional.softplus(h4 @ wa + ba - 1.0)).view(n, 8).sum(1)
    if plant == "ragged":
        fs[-3:], al[-3:] = float("nan"), float("nan")
    return fs, al


CHUNK = 8192     # items per float64 chunk (65536 rows), as test_agg_f16_gpu.py


def rows_bars(rows, st, tile, device="cpu"):
    """The chain bars of the split k_agg_rows on `rows` (an RRows) from the table `tile` (fp16, the kernel's layout):
    dict(fs, alpha = float64 references [n, ..] on the CPU, bar_fs, bar_alpha, floor_fs, floor_alpha, Efs, Ealpha =
    the largest interval bounds agg_f16_ref holds the unsplit kernel's f_s and alpha_s to)."""
    net = fr.Net(st, device)
    Pn = fr.to_nat(tile.to(device), PM, 256)
    out = dict(fs=[], alpha=[], e_fs=[], e_al=[], Efs=0.0, Ealpha=0.0)
    for i0 in range(0, rows.n, CHUNK):
        i1 = min(rows.n, i0 + CHUNK)
        o = rows_model(rows.chunk(i0, i1, device), net, Pn)
        out["fs"].append(o["fs"].cpu())
        out["alpha"].append(o["alpha"].cpu())
        out["Efs"], out["Ealpha"] = max(out["Efs"], ar.amax(o["Efs"])), max(out["Ealpha"], ar.amax(o["Ealpha"]))
        f32, a32 = rows_emu(rows.chunk(i0, i1), st, tile.cpu())
        out["e_fs"].append(f32)
        out["e_al"].append(a32)
    cat = lambda k, w: torch.cat(out[k]) if out[k] else torch.zeros((0,) + w)  # noqa: E731
    fs, alpha, e_fs, e_al = cat("fs", (256,)), cat("alpha", ()), cat("e_fs", (256,)), cat("e_al", ())
    return dict(fs=fs, alpha=alpha, emu_fs=e_fs, emu_alpha=e_al, bar_fs=ar.chain_bar(fs, e_fs), bar_alpha=ar.chain_bar(alpha, e_al, unit=True),
                floor_fs=ar.amax(e_fs.double() - fs), floor_alpha=ar.amax(e_al.double() - alpha), Efs=out["Efs"], Ealpha=out["Ealpha"])


def check_rows(rep, b, fs, alpha):
    """f_s [n, 256] fp16 and alpha_s [n] fp32 (CPU) against rows_bars' references at its chain bars."""
    fr._absbound(rep, "f_s", fs.cpu(), b["fs"], torch.full_like(b["fs"], b["bar_fs"]), torch.zeros_like(b["fs"]))
    fr._absbound(rep, "alpha_s", alpha.cpu(), b["alpha"], torch.full_like(b["alpha"], b["bar_alpha"]), torch.zeros_like(b["alpha"]))


def check_weights(rep, sc, rows, blend, wnorm):
    """out_blend / out_wnorm [S_cap K ..] (CPU): slot s K + k of a listed sample against the float64 weights at W_REL
    (an empty slot k < K: exactly 0); every slot of a sample outside the list must still be NaN (the caller's fill)."""
    K, n = sc.K, rows.n
    slot = (rows.samp[:, None] * K + torch.arange(K)[None, :]).reshape(-1)
    sel = (torch.arange(n)[:, None] * 8 + torch.arange(K)[None, :]).reshape(-1)
    for cut, got, ref in (("blend", blend, rows.wgt), ("wnorm", wnorm, rows.wn)):
        r = ref[sel]
        fr._absbound(rep, cut, got[slot], r, fr.W_REL * r.abs())
        rest = torch.ones(got.numel(), dtype=torch.bool)
        rest[slot] = False
        fr._flag(rep, cut + " untouched", not bool(torch.isnan(got[rest]).all()))
