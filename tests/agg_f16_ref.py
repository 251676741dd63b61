"""One-layer float64 references, with the kernels' own roundings, of the f16 training aggregator:
k_agg_rows<V, true> (sgn_aggregate_train_fwd, csrc/mlp.hip) and k_agg_bwd<SG> (sgn_aggregate_backward,
csrc/agg_train.hip).  test_agg_f16_gpu.py feeds every function here the tensor the kernel itself wrote on
the previous cut (the C ABI exposes x0, h1, h2, h2b, h3, f_s, alpha_s, h4, dza, d4 .. d1, db and the point
gradients), so a failure names one layer and no bound grows along the chain; test_agg_f16_ref_cpu.py proves
the references without a GPU (against agg_rows_ref.chain, torch autograd and train.aggregate), runs an fp32
torch emulation of every cut through every checker, plants errors, and caps every bound.

Layout.  Rows are PADDED: row = 8 * item + k (item = work-list position, k < 8), masked slots (k >= the
sample's neighbour count, or k >= K) included.  Saved / delta tiles are in the MFMA fragment column order;
sgn_train_colmap(0 / 1 / 2) maps a tile column to the unit / block1.0 input / block3.0 input it holds
(to_nat / from_nat).  Weights are fp16(W), round to nearest even; biases, the alpha weight and bias fp32.

Bounds, per element (u = 2^-24).  A dot product of n terms accumulated in fp32 in any order is within
E = (n + 1) u (|b| + sum |w| |x|) of the exact value.  A cut that ends in an fp16 rounding is checked by
INTERVAL: got must lie in [r(f(z - E)), r(f(z + E))] with r the (monotone) rounding and f the (monotone)
activation, so no element is excluded and nothing is added for the rounding itself.  lrelu16(v) = max(v,
fp16(v fp16(0.01))) is lrelu_pk's fp16 arithmetic (forward); the backward's LeakyReLU runs in fp32.  fp32
outputs (alpha_s, dza, the point gradients) take |got - ref| <= bound.  The one place a check gives way: d4's
LeakyReLU' mask is the sign of the recomputed z4, so where |z4| <= E either branch is accepted; the share of
such elements is capped at 0.1 % (AMBIG_CAP; 0.006 - 0.013 % measured on the CPU with the float64 chain and
init_mlp(5, bias_std=0.1) on rand8_300, rand3_777 and pairs).  Every other mask is read from a saved fp16
activation and is exact.  check_caps holds every bound below half an fp16 ulp of its tensor's max plus 1e-5
of it, so a bound can never swallow a wrong term.

Positional encodings.  The kernels take v_sin / v_cos at octave 0 and double the angle per octave, so the
error doubles too: a PE column at octave f lies within e_f = 2^f E_PE (plus 2^f cam_E for the camera-space
dists, agg_rows_ref.cam_E) of the float64 sin / cos of the kernel's own fp32 argument.  E_PE = 4e-6 holds at every
octave on the MI355X and was not raised; against the yardstick fp16(float64 sin / cos) 0.05 - 0.17 % of a scene's PE
elements differ (0.144 % on rand8_300; the fp32 torch emulation on the CPU: 0.009 %), each by one fp16 ulp.
"""
import ctypes

import torch
import torch.nn.functional as F

import agg_rows_ref as ar
from train_rows_ref import lrelu

U = 2.0 ** -24
C16 = 0.01000213623046875     # fp16(0.01), lrelu_pk's slope
E_PE = 4e-6                   # sin / cos at octave 0; octave f: 2^f E_PE
AMBIG_CAP = 1e-3              # share of d4 elements with |z4| <= E, per tensor
W_REL = 32 * U                # the kernel's own blend weights against float64 (the bar agg_rows_ref holds them to)
CAP_REL = 1e-5


def pe(x, freqs):
    """train_rows_ref.pe on x's own device: (sin, cos) pairs, channel-major then frequency."""
    arg = x[..., :, None] * (2.0 ** torch.arange(freqs, dtype=x.dtype, device=x.device))
    return torch.stack([torch.sin(arg), torch.cos(arg)], dim=-1).reshape(x.shape[:-1] + (x.shape[-1] * freqs * 2,))


# ---- fp16 arithmetic in float64 ------------------------------------------------------------------
def _q16(x):
    """The fp16 spacing q at |x| and 1 / q, both exact powers of two built from the float64 exponent field (a
    division or a pow on the device need not be exact)."""
    eb = x.double().abs().contiguous().view(torch.int64) >> 52
    eq = torch.clamp(eb - 10, min=1023 - 24)
    return (eq << 52).view(torch.float64), ((2046 - eq) << 52).view(torch.float64)


def ulp16(x):
    """The fp16 spacing at |x| (float64; 2^-24 below the normal range)."""
    return _q16(x)[0]


def rn16(x, toward_zero=False):
    """x rounded to fp16 (nearest, ties to even; toward_zero: truncated), as float64.  A direct rounding: the
    float64 -> fp32 -> fp16 route of a tensor cast rounds twice."""
    x = x.double()
    q, qi = _q16(x)
    return (torch.trunc(x * qi) if toward_zero else torch.round(x * qi)) * q


def lrelu16(v):
    """lrelu_pk on an fp16 value: max(v, fp16(v fp16(0.01)))."""
    return torch.maximum(v, rn16(v * C16))


# ---- layout --------------------------------------------------------------------------------------
_CM = None


def colmaps():
    """sgn_train_colmap(0 / 1 / 2) as int64 tensors (host function: no GPU needed)."""
    global _CM
    if _CM is None:
        from sgnerf_amd import _lib
        out = []
        for which, n in ((0, 256), (1, 288), (2, 272)):
            a = (ctypes.c_int32 * n)()
            assert _lib.lib().sgn_train_colmap(which, a, n) == 0
            out.append(torch.tensor(list(a), dtype=torch.int64))
        _CM = out
    return _CM


def to_nat(t, cm, width):
    """A tile in fragment column order -> float64 [rows, width] in reference column order."""
    cm = cm.to(t.device)
    keep = cm >= 0
    out = torch.zeros(t.shape[0], width, dtype=torch.float64, device=t.device)
    out[:, cm[keep]] = t[:, keep].double()
    return out


def from_nat(x, cm, dtype=torch.float16):
    """Reference column order -> fragment column order (padding columns 0)."""
    cm = cm.to(x.device)
    keep = cm >= 0
    out = torch.zeros(x.shape[0], cm.numel(), dtype=dtype, device=x.device)
    out[:, keep] = x[:, cm[keep]].to(dtype)
    return out


class Net:
    """The weights as the kernels hold them, float64 on `device`: fp16(W) (exact=True: W itself, the "roundings
    off" mode of the CPU test), fp32 biases, alpha weight and bias."""

    def __init__(self, state, device="cpu", exact=False):
        w = lambda n: (state[n + ".weight"] if exact else state[n + ".weight"].half()).double().to(device)  # noqa: E731
        b = lambda n: state[n + ".bias"].double().to(device)  # noqa: E731
        self.W0, self.b0, self.W1, self.b1 = w("block1.0"), b("block1.0"), w("block1.2"), b("block1.2")
        self.W2, self.b2, self.W3, self.b3 = w("block3.0"), b("block3.0"), w("block3.2"), b("block3.2")
        self.wa = state["alpha_branch.0.weight"].double().reshape(-1).to(device)
        self.ba = float(state["alpha_branch.0.bias"].double())
        self.sg = "block2_bpnet.0.weight" in state
        if self.sg:
            self.WB, self.bB = w("block2_bpnet.0"), b("block2_bpnet.0")
            self.bp_dim = self.WB.shape[1] - 256
        self.cm = [c.to(device) for c in colmaps()]


class Rows:
    """The padded rows of the first n work items of an agg_rows_ref.Scene, CPU float64 / int64: pid (-1 masked),
    wgt = w conf and wn = w (0 masked), emb, dists (the world half as the kernel's own fp32 subtraction -- exact:
    in float64 --, the camera half in float64), ext (colour, dir - v, <dir, v>), v (the row's ray), sample per item."""

    def __init__(self, sc, n=None, bp16=None, exact=False):
        n = sc.items if n is None else n
        assert 0 <= n <= sc.items
        self.n, self.N, self.K = n, sc.N, sc.K
        R = 8 * n
        keep = sc.item < n
        idx = (8 * sc.item + sc.rk)[keep]
        P, q = sc.points, sc.query
        d64, ext, rw = ar.row_inputs(sc, torch.float64)
        dw32 = d64[:, :3] if exact else (P["xyz"][sc.pid] - q["samp_locw"][sc.rs]).double()
        z = lambda *s: torch.zeros(*s, dtype=torch.float64)  # noqa: E731
        self.pid = torch.full((R,), -1, dtype=torch.int64)
        self.pid[idx] = sc.pid[keep]
        self.valid = self.pid >= 0
        self.wgt, self.wn, self.emb, self.dists, self.ext = z(R), z(R), z(R, 32), z(R, 6), z(R, 7)
        self.wgt[idx], self.wn[idx] = rw[keep, 0], rw[keep, 1]
        self.emb[idx] = P["embedding"][sc.pid[keep]].double()
        self.dists[idx] = torch.cat([dw32, d64[:, 3:]], dim=1)[keep]
        self.ext[idx] = ext[keep]
        self.samp = sc.work[:n].long()
        self.v = sc.raydir[q["samp_ray"][self.samp].long()].double().repeat_interleave(8, dim=0)
        self.camE = ar.cam_E(sc)
        self.bp = None
        if bp16 is not None:    # the fp16 BPNet table's rows; a masked slot reads point 0's (the kernel clamps the index)
            self.bp = bp16.cpu().double()[self.pid.clamp(min=0)]

    def chunk(self, i0, i1, device="cpu"):
        """Items [i0, i1) as an object of the same fields on `device`."""
        c = object.__new__(Rows)
        c.n, c.N, c.K, c.camE, c.i0 = i1 - i0, self.N, self.K, self.camE, i0
        for k in ("pid", "valid", "wgt", "wn", "emb", "dists", "ext", "v"):
            setattr(c, k, getattr(self, k)[8 * i0:8 * i1].to(device))
        c.bp = None if self.bp is None else self.bp[8 * i0:8 * i1].to(device)
        c.samp = self.samp[i0:i1].to(device)
        return c


# ---- the scenes of the GPU test (built here, not in agg_rows_ref._SCENES: that module's CPU test walks every
# named scene).  8195 items: the forward's persistent loop wraps past 256 workgroups x 32 items; 32771: a
# backward workgroup gets a second tile (the `more` prefetch) past 2048 workgroups x 16 items
def _nonzero(counts):
    return [c for c in counts if c]


_SCENES = {
    "rand8_300": (8, lambda: ar.rand(8, 300), False), "rand8_300_shuf": (8, lambda: ar.rand(8, 300), True),
    "rand4_300": (4, lambda: ar.with_empties(_nonzero(ar.rand(4, 300))), True), "rand1_300": (1, lambda: ar.rand(1, 300), False),
    "pairs": (8, ar.pairs, False), "rand3_8195": (3, lambda: ar.rand(3, 8195), False),
    "rand2_32771": (2, lambda: ar.rand(2, 32771), True),
}
SMALL_SCENES = ["rand8_300", "rand8_300_shuf", "rand4_300", "rand1_300", "pairs"]
_CACHE = {}


def scene(name):
    if name not in _CACHE:
        K, counts, shuffle = _SCENES[name]
        _CACHE[name] = ar.Scene(K, counts(), shuffle=shuffle, bpnet=True)
    return _CACHE[name]


def upstream(n, seed=7):
    """Seeded d f_s [n, 256], d alpha_s [n] and the pre-fill of the four point-gradient tensors (the ABI says +=)."""
    g = torch.Generator().manual_seed(seed * 1000 + n % 997)
    dfs, dalpha = torch.randn(n, 256, generator=g) * 0.02, torch.randn(n, generator=g) * 0.2
    g0 = {k: torch.randn(ar.N_POINTS, c, generator=g) * 1e-3 for k, c in (("embedding", 32), ("color", 3), ("dir", 3), ("conf", 1))}
    return dfs, dalpha, g0


def ambiguous_share(sc, state):
    """The share of block3.2 pre-activations with |z4| <= E on a scene, from the float64 chain alone."""
    o = ar.chain(sc, state)
    net = Net(state)
    z4, E = dot(lrelu(o["z3"]), net.W3, net.b3)
    return float((z4.abs() <= E).double().mean()) if z4.numel() else 0.0


# ---- the report ----------------------------------------------------------------------------------
class Report:
    """Worst error / bound ratio, failures, largest bound and reference scale per cut, over any number of chunks."""

    def __init__(self):
        self.ratio, self.fail, self.bmax, self.rmax, self.extra = {}, {}, {}, {}, {}

    def add(self, cut, ratio, bad, bound, ref):
        if ratio.numel() == 0:
            self.ratio.setdefault(cut, 0.0)
            return
        ratio = torch.nan_to_num(ratio, nan=float("inf"), posinf=float("inf"))
        self.ratio[cut] = max(self.ratio.get(cut, 0.0), float(ratio.max()))
        self.bmax[cut] = max(self.bmax.get(cut, 0.0), float(torch.as_tensor(bound).max()))
        self.rmax[cut] = max(self.rmax.get(cut, 0.0), float(ref.abs().max()))
        n = int(bad.sum())
        if n:
            i = int(torch.nonzero(bad.reshape(-1))[0])
            self.fail[cut] = self.fail.get(cut, "") + f"{n} of {bad.numel()} elements outside (first: flat index {i}, " \
                                                      f"ratio {float(ratio.reshape(-1)[i]):.3f}); "

    def count(self, key, n):
        self.extra[key] = self.extra.get(key, 0) + int(n)

    def failed(self):
        return sorted(self.fail)

    def show(self, what):
        print(f"{what} worst error / bound:", {k: round(v, 3) for k, v in self.ratio.items()})
        off = {k[4:]: round(100.0 * v / max(self.extra["n " + k[4:]], 1), 3) for k, v in self.extra.items() if k.startswith("off ")}
        if off:
            print(f"{what} % of elements off the error-free dot product's rounding:", off)
        if self.extra.get("d4_n"):
            print(f"{what} d4 elements with |z4| <= E: {self.extra.get('d4_ambiguous', 0)} of {self.extra['d4_n']} "
                  f"({100.0 * self.ambiguous_share():.4f} %)")
        if self.extra.get("pe_n"):
            print(f"{what} PE elements that differ from fp16(float64 reference): {self.extra.get('pe_diff', 0)} of "
                  f"{self.extra['pe_n']} ({100.0 * self.extra.get('pe_diff', 0) / self.extra['pe_n']:.3f} %)")

    def ambiguous_share(self):
        return self.extra.get("d4_ambiguous", 0) / max(self.extra.get("d4_n", 0), 1)

    def assert_ok(self, what):
        assert not self.fail, f"{what}: " + "; ".join(f"{k}: {v}" for k, v in self.fail.items())
        assert self.ambiguous_share() <= AMBIG_CAP, f"{what}: {self.ambiguous_share():.2e} of d4 is ambiguous"

    def check_caps(self, what):
        """Every bound below half an fp16 ulp of its tensor's max plus 1e-5 of it.  The bound of a cut that ends in
        an fp16 rounding is its E, before that rounding (the interval cuts add nothing for it; f_s's bound adds
        half an ulp of the element, which at the tensor's max is the limit's first term itself).  alpha_s and dza
        cross block3.2 and the alpha dot with no cut between them: block3.2's E, itself capped on the h4 cut, reaches
        them multiplied by sum |wa| ~ 20 (3e-3 .. 4.5e-3 on alpha_s <= 1.8, measured on the CPU), past any per-layer
        cap; the cap sees the rest of their bound.  The point gradients: their own (terms + rows) u sum |terms|
        has a cap of its own (check_point_grads), the carried parts (block3.2's E in g_conf, the PE's e_f in g_embedding)
        are capped where they arise."""
        for k, b in self.bmax.items():
            s = self.rmax[k]
            lim = 0.5 * float(ulp16(torch.tensor(s))) + CAP_REL * s
            assert b < lim, f"{what} {k}: bound {b:.3e} is not below {lim:.3e} (tensor max {s:.3e})"


def _interval(rep, cut, got, lo, hi, bound, ref, alt=None, centre=None):
    """lo <= got <= hi (or `alt`); the printed ratio is |got - mid| over the half-width plus half an fp16 ulp (0.5:
    lo and hi are neighbours and got is one of them).  centre: the value a dot product without any error rounds to;
    the share of elements off it is counted (it grows with any error, long before an element leaves its interval)."""
    got = got.double()
    if centre is not None:
        rep.count("off " + cut, (got != centre).sum())
        rep.count("n " + cut, got.numel())
    ok = (got >= lo) & (got <= hi)
    mid, hw = (lo + hi) / 2, (hi - lo) / 2
    ratio = (got - mid).abs() / (hw + 0.5 * ulp16(torch.maximum(lo.abs(), hi.abs())))
    if alt is not None:
        ok = ok | alt
        ratio = torch.where(alt, torch.zeros_like(ratio), ratio)
    rep.add(cut, ratio, ~ok, bound, ref)


def _absbound(rep, cut, got, ref, bound, capped=None):
    """|got - ref| <= bound.  capped: the part of the bound that check_caps sees (default: all of it)."""
    got = got.double()
    err = (got - ref).abs()
    ratio = torch.where(err > 0, err / bound.clamp(min=1e-300), torch.zeros_like(err))
    rep.add(cut, ratio, ~(err <= bound), bound if capped is None else capped, ref)


def _flag(rep, cut, bad):
    """An exact property (padding columns 0, masked rows 0, untouched points): ratio 0 or 2."""
    b = torch.full((1,), bool(bad))
    rep.add(cut, b.double() * 2, b, torch.zeros(()), torch.zeros(1))


# ---- values and bounds (no rounding of the result: the CPU test compares these with autograd) -----------
def dot(x, W, b=None, n=None):
    """z = b + x W^T in float64 and E = (n + 1) u (|b| + sum |w| |x|)."""
    n = W.shape[1] if n is None else n
    z, a = x @ W.t(), x.abs() @ W.abs().t()
    if b is not None:
        z, a = z + b, a + b.abs()
    return z, (n + 1) * U * a


def x0_ref(rc):
    """[emb | PE(emb, 3) | PE(dists, 5)] [rows, 284] and the PE columns' e_f (0 on masked rows: sin 0, cos 1 exactly)."""
    R, dev = rc.emb.shape[0], rc.emb.device
    ref = torch.cat([rc.emb, pe(rc.emb, 3), pe(rc.dists, 5)], dim=-1)
    f3 = 2.0 ** torch.arange(3, dtype=torch.float64, device=dev)
    f5 = 2.0 ** torch.arange(5, dtype=torch.float64, device=dev)
    e_emb = (f3 * E_PE)[None, :, None].expand(32, 3, 2).reshape(192)
    e_d = (f5 * E_PE)[None, :, None].expand(6, 5, 2).clone()
    e_d[3:] += (f5 * rc.camE)[None, :, None]
    e = torch.cat([torch.zeros(32, dtype=torch.float64, device=dev), e_emb, e_d.reshape(60)])
    return ref, e[None, :] * rc.valid[:, None].double()


def blend_ref(h3n, rc, net):
    """From block3.2's inputs [rows, 256] (natural order): z4, E4, h4 = lrelu(z4) in fp32 (no fp16 rounding) with
    its error, the alpha logit and alpha per row with theirs, f_s and alpha_s per item with theirs."""
    z4, E4 = dot(h3n, net.W3, net.b3)
    h4 = lrelu(z4)
    E4h = E4 + 2 * U * h4.abs()                       # the 0.01f product
    za = h4 @ net.wa + net.ba
    Eza_c = E4h @ net.wa.abs()                        # block3.2's E carried through the alpha dot (sum |wa| ~ 20)
    Eza = Eza_c + (256 + 2) * U * (h4.abs() @ net.wa.abs() + abs(net.ba) + 1.0)
    al = F.softplus(za - 1.0)
    Eal = Eza + 8 * U * al + 2 * U                    # softplus' <= 1; expf / log1pf
    n = rc.n
    terms = rc.wgt[:, None] * h4
    fs = terms.view(n, 8, 256).sum(1)
    Efs = (rc.wgt[:, None] * E4h).view(n, 8, 256).sum(1) + (10 * U + W_REL) * terms.abs().view(n, 8, 256).sum(1)
    a_s = (rc.wgt * al).view(n, 8).sum(1)
    Eas = (rc.wgt * Eal).view(n, 8).sum(1) + (10 * U + W_REL) * a_s
    return dict(z4=z4, E4=E4, h4=h4, E4h=E4h, za=za, Eza=Eza, Eza_c=Eza_c, al=al, Eal=Eal, fs=fs, Efs=Efs, alpha=a_s, Ealpha=Eas,
                Ealpha_c=(rc.wgt * Eza_c).view(n, 8).sum(1))


def head_ref(o, rc, net, dfs, dalpha, scale, dza=None):
    """dza [rows] and d4 [rows, 256] before the fp16 rounding, with bounds.  o: blend_ref's dict; dza: the kernel's
    own (d4 is built on it), default the reference's."""
    item = torch.arange(rc.wgt.shape[0], device=rc.wgt.device) // 8
    c = rc.wgt * dalpha.double()[item] * scale
    rdza = c * torch.sigmoid(o["za"] - 1.0)
    b_dza = c.abs() * (0.25 * o["Eza"] + 4 * U) + (W_REL + 6 * U) * rdza.abs()
    t1 = (rc.wgt * scale)[:, None] * dfs.double()[item]
    t2 = (rdza if dza is None else dza.double())[:, None] * net.wa[None, :]
    y = t1 + t2
    e = W_REL * t1.abs() + 3 * U * (t1.abs() + t2.abs())
    return rdza, b_dza, y, e


def masked(y, e, act_pos):
    """(y, e) through LeakyReLU' = 1 where act_pos else 0.01 (one more fp32 rounding for the product)."""
    m = torch.where(act_pos, torch.ones_like(y), torch.full_like(y, 0.01))
    v = m * y
    return v, m * e + U * v.abs()


def delta_ref(d, W, act):
    """(W^T d) LReLU'(act): d [rows, out] the next layer's deltas, W [out, in >= 256] its weights (the first 256
    input columns count), act [rows, 256] the saved activation whose sign is the mask."""
    y, E = dot(d, W[:, :256].t())
    return masked(y, E, act > 0)


def grad_rows(o, rc, net, d1n, d3n, dfs, dalpha):
    """Per-row point-gradient terms (scaled as the deltas are) and their bounds: dict name -> (value [rows, c],
    bound, sum |terms|, the carried part of the bound).  conf is unscaled (the kernel multiplies <h4, d f_s> by the scale and divides again)."""
    item = torch.arange(rc.wgt.shape[0], device=rc.wgt.device) // 8
    ye, Ee = dot(d3n, net.W2[:, 256:263].t(), n=256)
    ae = Ee / (257 * U)
    zc = torch.zeros_like(ye[:, :3])
    col = (ye[:, :3], Ee[:, :3], ae[:, :3], zc)
    va = rc.v.abs()
    dr = ye[:, 3:6] + ye[:, 6:7] * rc.v
    adr = ae[:, 3:6] + ae[:, 6:7] * va
    dirg = (dr, Ee[:, 3:6] + Ee[:, 6:7] * va + 3 * U * adr, adr, zc)
    df, da = dfs.double()[item], dalpha.double()[item]
    dt, adt = (o["h4"] * df).sum(-1), (o["h4"].abs() * df.abs()).sum(-1)
    val = (dt + o["al"] * da) * rc.wn
    aval = (adt + (o["al"] * da).abs()) * rc.wn
    c_conf = rc.wn * ((o["E4h"] * df.abs()).sum(-1) + o["Eza_c"] * da.abs())      # block3.2's E, carried
    e_conf = rc.wn * (258 * U * (adt + (o["al"] * da).abs()) + (o["Eal"] - o["Eza_c"]) * da.abs()) + (W_REL + 4 * U) * aval + c_conf
    conf = (val[:, None], e_conf[:, None], aval[:, None], c_conf[:, None])
    dx0, E0 = dot(d1n, net.W0[:, :224].t(), n=256)
    a0 = E0 / (257 * U)
    bands = 2.0 ** torch.arange(3, dtype=torch.float64, device=d1n.device)
    arg = rc.emb[:, :, None] * bands
    R = d1n.shape[0]
    dpe, ape, Epe = (t[:, 32:224].reshape(R, 32, 3, 2) for t in (dx0, a0, E0))
    de = dx0[:, :32] + ((dpe[..., 0] * torch.cos(arg) - dpe[..., 1] * torch.sin(arg)) * bands).sum(-1)
    ade = a0[:, :32] + ((ape[..., 0] + ape[..., 1]) * bands).sum(-1)
    c_de = ((dpe[..., 0].abs() + dpe[..., 1].abs()) * bands * bands * E_PE).sum(-1)     # the PE's e_f, carried
    e_de = E0[:, :32] + ((Epe[..., 0] + Epe[..., 1]) * bands).sum(-1) + c_de + 10 * U * ade
    emb = (de, e_de, ade, c_de)
    return dict(embedding=emb, color=col, dir=dirg, conf=conf)


class GradAcc:
    """Sums over the rows of each point (float64 index_add), chunk after chunk."""

    def __init__(self, N, device="cpu"):
        z = lambda c: torch.zeros(N, c, dtype=torch.float64, device=device)  # noqa: E731
        self.t = {k: [z(c), z(c), z(c), z(c)] for k, c in (("embedding", 32), ("color", 3), ("dir", 3), ("conf", 1))}
        self.cnt = torch.zeros(N, dtype=torch.float64, device=device)

    def add(self, rc, terms):
        pid = rc.pid[rc.valid]
        self.cnt.index_add_(0, pid, torch.ones_like(pid, dtype=torch.float64))
        for k, vals in terms.items():
            for acc, v in zip(self.t[k], vals):
                acc.index_add_(0, pid, v[rc.valid])


# ---- the cuts ------------------------------------------------------------------------------------
def check_forward(rep, rc, net, t):
    """One chunk of the forward.  t: x0 [rows, 288], h1, h3 [rows, 256], h2 [rows, 272], SG: h2b [rows, 256] (fp16,
    fragment order), fs [items, 256] (fp16, natural order), alpha [items] (fp32: out_feat[4 s] of the items).
    Returns blend_ref's dict."""
    cm0, cm1, cm2 = net.cm
    # x0
    x0 = t["x0"]
    ref, e = x0_ref(rc)
    got = to_nat(x0, cm1, 284)
    emb_bad = got[:, :32] != rn16(ref[:, :32])
    rep.add("x0 emb", emb_bad.double() * 2, emb_bad, torch.zeros(()), ref[:, :32])
    _flag(rep, "x0 pad", bool((x0[:, cm1 < 0] != 0).any()))
    _interval(rep, "x0 PE", got[:, 32:], rn16(ref[:, 32:] - e[:, 32:]), rn16(ref[:, 32:] + e[:, 32:]), e[:, 32:], ref[:, 32:])
    rep.count("pe_n", int(rc.valid.sum()) * 252)
    rep.count("pe_diff", (got[rc.valid, 32:] != rn16(ref[rc.valid, 32:])).sum())

    def hidden(cut, got_n, x, W, b):
        z, E = dot(x, W, b)
        _interval(rep, cut, got_n, lrelu16(rn16(z - E)), lrelu16(rn16(z + E)), E, z, centre=lrelu16(rn16(z)))

    hidden("h1", to_nat(t["h1"], cm0, 256), got, net.W0, net.b0)
    h1n = to_nat(t["h1"], cm0, 256)
    h2 = t["h2"]
    h2n = to_nat(h2, cm2, 263)
    if net.sg:
        hbn = to_nat(t["h2b"], cm0, 256)
        hidden("h2b", hbn, h1n, net.W1, net.b1)
        hidden("h2", h2n[:, :256], hbn if rc.bp is None or net.bp_dim == 0 else torch.cat([hbn, rc.bp], dim=1), net.WB, net.bB)
    else:
        hidden("h2", h2n[:, :256], h1n, net.W1, net.b1)
    e_ext = 8 * U * rc.valid[:, None].double().expand(-1, 7)      # 4 fp32 roundings of values <= 2; masked rows: exact 0
    _flag(rep, "h2 pad", bool((h2[:, cm2 < 0] != 0).any()))
    _interval(rep, "h2 ext", h2n[:, 256:], rn16(rc.ext - e_ext), rn16(rc.ext + e_ext), e_ext, rc.ext)
    h3n = to_nat(t["h3"], cm0, 256)
    hidden("h3", h3n, h2n, net.W2, net.b2)
    o = blend_ref(h3n, rc, net)
    # (the cap sees E_fs, as it sees E of the interval cuts: the result's own fp16 rounding is the limit's first term)
    _absbound(rep, "f_s", t["fs"], o["fs"], 0.5 * ulp16(o["fs"].abs() + o["Efs"]) + o["Efs"], o["Efs"])
    _absbound(rep, "alpha_s", t["alpha"], o["alpha"], o["Ealpha"], o["Ealpha"] - o["Ealpha_c"])
    return o


def check_backward(rep, rc, net, t, acc=None):
    """One chunk of the backward.  t: the saved h1, h2, h3 (SG: h2b), dfs [items, 256], dalpha [items], scale (float),
    and the kernel's h4, d4, d3, d2, d1 (SG: db) [rows, 256] and dza [rows].  acc: a GradAcc taking this chunk's
    point-gradient terms."""
    cm0, _, cm2 = net.cm
    nat = lambda k: to_nat(t[k], cm0, 256)  # noqa: E731
    h3n = nat("h3")
    o = blend_ref(h3n, rc, net)
    z4, E = o["z4"], o["E4"] + 2 * U * o["z4"].abs()
    _interval(rep, "h4", nat("h4"), rn16(lrelu(z4 - E)), rn16(lrelu(z4 + E)), E, z4, centre=rn16(lrelu(z4)))
    scale = float(t["scale"])
    rdza, b_dza, y, e = head_ref(o, rc, net, t["dfs"], t["dalpha"], scale, t["dza"])
    c = (rc.wgt * t["dalpha"].double().repeat_interleave(8) * scale).abs()
    _absbound(rep, "dza", t["dza"], rdza, b_dza, b_dza - 0.25 * c * o["Eza_c"])
    pos = z4 > 0
    v, ev = masked(y, e, pos)
    v2, ev2 = masked(y, e, ~pos)
    d4n = nat("d4")
    amb = z4.abs() <= o["E4"]
    alt = amb & (d4n >= rn16(v2 - ev2)) & (d4n <= rn16(v2 + ev2))
    _interval(rep, "d4", d4n, rn16(v - ev), rn16(v + ev), ev, v, alt, centre=rn16(v))
    rep.count("d4_n", amb.numel())
    rep.count("d4_ambiguous", amb.sum())

    def delta(cut, got_n, d_n, W, act_n):
        val, ee = delta_ref(d_n, W, act_n)
        _interval(rep, cut, got_n, rn16(val - ee), rn16(val + ee), ee, val, centre=rn16(val))

    d3n = nat("d3")
    delta("d3", d3n, d4n, net.W3, h3n)
    h2n = to_nat(t["h2"], cm2, 263)[:, :256]
    d2n = nat("d2")
    if net.sg:
        dbn = nat("db")
        delta("db", dbn, d3n, net.W2, h2n)
        delta("d2", d2n, dbn, net.WB, nat("h2b"))
    else:
        delta("d2", d2n, d3n, net.W2, h2n)
    d1n = nat("d1")
    delta("d1", d1n, d2n, net.W1, nat("h1"))
    if acc is not None:
        acc.add(rc, grad_rows(o, rc, net, d1n, d3n, t["dfs"], t["dalpha"]))
    return o


def masked_rows_zero(rc, t, sg):
    """d4, d3, d2, (db,) d1 and dza are exactly +-0 on every masked slot: the weight-gradient GEMMs sum over all
    8 n rows, and a masked row's x0 is not zero.  (The cuts imply it: d4's and dza's references are 0 with bound 0
    there, and a delta computed from an all-zero row is 0; this is the direct statement.)"""
    m = ~rc.valid
    names = ["d4", "d3", "d2", "d1"] + (["db"] if sg else [])
    return all(not bool((t[k][m] != 0).any()) for k in names + ["dza"])


def check_point_grads(rep, acc, g0, got, scale):
    """got = g0 + the rows' sums: within the rows' own bounds plus the atomic adds of a point's n rows onto g0 in
    any order ((n + 2) u (|g0| + sum |terms|)).  Points no valid row names keep their value."""
    for k in ("embedding", "color", "dir", "conf"):
        s, b, a, carried = acc.t[k]
        f = 1.0 if k == "conf" else 1.0 / scale
        base = g0[k].double().reshape(s.shape).to(s.device)
        ref = base + s * f
        bound = b * f + (acc.cnt[:, None] + 2) * U * (base.abs() + a * f)
        g = got[k].double().reshape(s.shape).to(s.device)
        # the cap of an fp32 sum: what is not carried stays below a quarter of the mean row's sum |terms| (a point's
        # rows and its pre-fill are what the kernel adds one by one), so it cannot swallow a wrong, dropped or leaked row
        # at any row count: at most (263 + 190 + 2) u = 2.7e-5 of sum |terms| against 1 / (4 x 191) = 1.3e-3 on the
        # 32771-item scene.  (The fp16-ulp cap of the tiles does not fit an fp32 sum that cancels: (256 + 7 + rows) u
        # sum |terms| is 3e-4 .. 4e-4 of g_embedding's max, measured on the CPU, against a limit of 2.4e-4 .. 4.9e-4 that
        # depends on where the max falls in its binade.)
        _flag(rep, "g cap", bool(((bound - carried * f) > 0.25 * (base.abs() + a * f) / (acc.cnt[:, None] + 1)).any()))
        _absbound(rep, "g_" + k, g, ref, bound, torch.zeros_like(bound))
        none = acc.cnt == 0
        _flag(rep, "g untouched", not torch.equal(g[none], base[none]))
