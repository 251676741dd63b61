"""The per-ray stage's kernels -- sgn_composite (k_composite), sgn_ray_march_dense (k_ray_march_dense) and
sgn_loss_train (k_loss_fwd, k_loss_reduce, k_loss_bwd) -- each called directly through the C ABI on the scenes
of tests/ray_stage_ref.py (hand-placed rays, a hand-built QueryOut) and compared element by element with that
module's float64 references (pinned to train.composite_losses / agg_ref and to finite differences in
test_ray_stage_ref_cpu.py).  Every output is pre-filled with a sentinel and followed by guard rows that must
stay as they were.  Each test prints its worst error / bound per output.

Bounds are per element, never a norm; u = 2^-24.  A sum of n fp32 terms (products rounded first) is within
2 n u sum|terms| of the exact value; an error passes on with the Lipschitz constant of what follows; every
expf / logf result is allowed 4 u relative (a choice with margin; the caps below keep it from hiding anything).

Forward, per slot (x = sigma dist, an fp32 product of fp32 inputs; the reference takes the same fp32 dist):
  e = exp(-x):   E_e  = (4 + x) u e            (expf, and x's rounding through e^-x)
  o = 1 - e:     E_o  = E_e + u o
  a = 1 - o + 1e-10 (the transmittance factor):  E_a = E_o + 2 u a   (two roundings; a <= 1 + 1e-10)
  (where x = 0 exactly -- no neighbour, alpha 0, a padding slot -- e = 1, o = 0 and a = 1.0f are exact and T
  passes unchanged: E_e = E_o = 0, E_a = 1e-10, the float64 reference's own 1 + 1e-10, and no rounding of T)
  T_{s+1} = T_s a_s:   E_T[s+1] = E_T[s] (a + E_a) + T_s E_a + u T_{s+1},   E_T[0] = 0
  w = o T:       E_w  = E_o T + o E_T + E_o E_T + u w
  rgb = sum c w + bg T_end:   E_rgb = sum c E_w + bg E_T[end] + 2 (n + 1) u (sum c w + bg T_end), n terms + 1
Two absolute floors ride along: 2^-149 per product that can underflow (gradual underflow rounds to a multiple
of the smallest denormal; the last products of d feat too), and 2^-52 per slot on E_T, the float64
reference's own rounding of (1 + 1e-10)^s against the kernel's exact 1 on rays that absorb nothing.
All absolute (the quantities live in [0, 1]); all relative errors of T would blow up where o rounds to 1
(a = 1e-10 in fp32 against ~e in float64), the absolute ones do not.

Backward (k_loss_bwd reads the forward's stored fp32 T, e, dist).  With g = 2 (rgb - gt) / (3 n) and
gc_s = g . c_s, the kernel forms d L / d o_s = gc_s T_s - U_s / a_s with U_s = sum_{i>s} gc_i w_i + (g . bg) T_end
accumulated from the end.  Every term of U_s carries T_{s+1} = T_s a_s as a factor -- in fp32 too, since
w_i = o_i T_i and T_i is the rounded product T_s a_s a_{s+1} .. -- so U_s / a_s = T_s V_s (1 + O(u)) with
  V_s = gc_{s+1} o_{s+1} + a_{s+1} V_{s+1},   V_end = g . bg,   |V_s| <= |g|_1 max(c, bg):
the division by a_s, as small as 1e-10, cancels against the factor a_s and never amplifies an error (only
T's underflow, < 2^-149 / 1e-10 in all, escapes the cancellation: 1e-30 is added).  So
  E_V[s-1] = E_gc o + |gc| E_o + E_gc E_o + 2 u |gc| o + (E_a + u a) |V_s| + (a + E_a) E_V[s] + u (|gc| o + a Vabs_s)
  (Vabs: the same recursion on absolute values, for the additions' roundings),
  E_dO = E_T (|gc| + |V|) + T (E_gc + E_V) + E_T (E_gc + E_V) + 3 u T (|gc| + |V|) + 1e-30,
  d sigma_s = dO e dist:  E = E_dO e dist + |dO| E_e dist + E_dO E_e dist + 2 u |d sigma|,
  d c_s = g w:            E = E_g w + |g| E_w + E_g E_w + u |g w|,
  E_g = 2 / (3 n) (E_rgb + u |rgb - gt|) + 2 u |g|,  E_gc = E_g . c + 6 u |g| . c  (three terms).
Losses: the longest addition chain is 3 terms per ray, 6 shuffle steps, 4 waves, the strided loop's trips, then
6 + 4 again (plus, for the zero-one sum, a lane's nv ceil(K / 8) + 1 terms); the colour error enters through
2 |full - gt|.  d conf of a point with m entries: 2 (m + 1) u (|start| + sum|terms|) plus the terms' own error;
point 0's empty entries count as the kernel adds them, one term per lane and ray.

Caps (conditions on the bounds, asserted): every forward bound < F32_TOL = 1e-5 (colour: x max(1, |ref|)), every
gradient / loss bound < GRAD_TOL_F32 = 1e-4 of the reference tensor's max abs.  Where a shape would break a cap
the scene's magnitudes are chosen lower (denser rays at SR >= 64, so that T has decayed by the late slots)."""
import ctypes
import functools

import pytest
import torch

import sgnerf_amd  # noqa: F401
from sgnerf_amd import _lib

import ray_stage_ref as rs

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
U = 2.0 ** -24
F32_TOL = 1e-5
GRAD_TOL_F32 = 1e-4
GUARD = 3
NAN = float("nan")
F32 = torch.float32
BG = (0.2, 0.5, 0.6)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a.cpu()), _bits(b.cpu()))


def _all_nan(t):
    return bool(torch.isnan(t).all())


def _ratio(got, ref, bound, what):
    """max |got - ref| / bound over the elements (an element may differ only where its bound is > 0), printed
    and asserted <= 1."""
    got, ref = got.detach().cpu().double(), ref.double()
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    if ref.numel() == 0:
        print(f"{what}: empty")
        return 0.0
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(ref)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
    err = (got - ref).abs()
    r = torch.where(err > 0, err / bound.clamp(min=1e-300), torch.zeros_like(err))
    worst = float(r.max())
    i = int(r.argmax())
    print(f"{what}: worst error / bound = {worst:.3f} (element {i}: error {float(err.reshape(-1)[i]):.3e}, "
          f"bound {float(bound.reshape(-1)[i]):.3e})")
    assert worst <= 1.0, f"{what}: element {i} off by {float(err.reshape(-1)[i]):.3e}, bound {float(bound.reshape(-1)[i]):.3e}"
    return worst


def _capped(bound, ref, what, cap=GRAD_TOL_F32):
    """The bound tensor stays below cap x the reference's scale."""
    if ref.numel() == 0:
        return
    b, s = float(torch.as_tensor(bound).max()), float(ref.abs().max())
    assert b < cap * s, f"{what}: bound {b:.3e} is not below {cap} x the reference's scale {s:.3e}"


def _capped_fwd(bound, what, ref=None):
    """A forward bound stays below F32_TOL (colour: x max(1, |ref|) per element)."""
    b = torch.as_tensor(bound, dtype=torch.float64)
    lim = F32_TOL * (torch.ones_like(b) if ref is None else ref.abs().clamp(min=1.0))
    assert bool((b < lim).all()), f"{what}: bound {float(b.max()):.3e} is not below F32_TOL"


# ---- bounds (CPU, float64, from the reference alone) ------------------------------------------------

def forward_bounds(sc, ref, n_terms):
    """E_o, E_e, E_a, E_T [R, SR], E_Tend [R], E_w [R, SR], E_rgb [R, 3] (before fill_invalid) as the module
    docstring derives them; n_terms [R] or int: the colour sum's terms per ray."""
    fd = rs.densify(sc, sc["feat"]).double()
    x = fd[..., 0] * ref["valid"].double() * ref["dist"].double()
    o, T, w, av = ref["o"], ref["T"], ref["w"], ref["av"]
    e = torch.exp(-x)
    live = (x != 0).double()        # x = 0 (no neighbour, alpha 0, padding): e = 1, o = 0, a = 1.0f, T unchanged, all exact
    Ee = ((4 + x) * U * e + 1e-37) * live
    Eo = Ee + U * o
    Ea = torch.where(x != 0, Eo + 2 * U * av, torch.full_like(x, rs.EPS_T))
    ET, cur = [], torch.zeros(T.shape[0], dtype=torch.float64)
    Tn = torch.cat([T[:, 1:], ref["bgT"][:, None]], dim=1)
    for s in range(T.shape[1]):
        ET.append(cur)
        cur = cur * (av[:, s] + Ea[:, s]) + T[:, s] * Ea[:, s] + (U * Tn[:, s] + 2.0 ** -149) * live[:, s] + 2.0 ** -52
    ET = torch.stack(ET, dim=1)
    Ew = Eo * T + o * ET + Eo * ET + U * w + 2.0 ** -149
    c, bg = fd[..., 1:4], ref["bg"].double()
    n = torch.as_tensor(n_terms, dtype=torch.float64).reshape(-1, 1)
    Ergb = (c * Ew[..., None]).sum(1) + bg * cur[:, None] + 2 * (n + 1) * U * ((c * w[..., None]).sum(1) + bg * ref["bgT"][:, None])
    return dict(e=e, Ee=Ee, Eo=Eo, Ea=Ea, ET=ET, ETend=cur, Ew=Ew, Ergb=Ergb, c=c)


def loss_bounds(sc, ref, fb, zo_w, start):
    """Bounds of d feat [S, 4], the four losses and d conf [N] (start: d conf's values before the call)."""
    R, SR, K, S = sc["R"], sc["SR"], sc["K"], sc["S"]
    n, mask = ref["n"], ref["mask"]
    m = mask.double()
    gs = 2.0 / max(3 * n, 1)
    diff = ref["full"] - sc["gt"].double()
    Efull = fb["Ergb"] * m[:, None]                       # a missed ray's colour is its background, bit for bit
    g = gs * diff * m[:, None]
    Eg = (gs * (Efull + U * diff.abs()) + 2 * U * g.abs()) * m[:, None]
    bg, c = ref["bg"].double(), fb["c"]
    V = (g * bg).sum(-1)
    Vabs = (g.abs() * bg).sum(-1)
    EV = (Eg * bg).sum(-1) + 6 * U * Vabs + 2 * U * V.abs()
    o, T, w, av, e, dist = ref["o"], ref["T"], ref["w"], ref["av"], fb["e"], ref["dist"].double()
    Eo, Ea, ET, Ew, Ee = fb["Eo"], fb["Ea"], fb["ET"], fb["Ew"], fb["Ee"]
    Edf = torch.zeros(R, SR, 4, dtype=torch.float64)
    for s in reversed(range(SR)):
        cs = c[:, s]
        gc = (g * cs).sum(-1)
        Egc = (Eg * cs).sum(-1) + 6 * U * (g.abs() * cs).sum(-1)
        Ts, os_, as_ = T[:, s], o[:, s], av[:, s]
        dO = Ts * (gc - V)
        EdO = ET[:, s] * (gc.abs() + V.abs()) + Ts * (Egc + EV) + ET[:, s] * (Egc + EV) + 3 * U * Ts * (gc.abs() + V.abs()) + 1e-30
        ed = e[:, s] * dist[:, s]
        Edf[:, s, 0] = EdO * ed + dO.abs() * Ee[:, s] * dist[:, s] + EdO * Ee[:, s] * dist[:, s] + 2 * U * (dO * ed).abs() + 2.0 ** -148
        Edf[:, s, 1:] = Eg * w[:, s, None] + g.abs() * Ew[:, s, None] + Eg * Ew[:, s, None] + U * (g * w[:, s, None]).abs() + 2.0 ** -149
        EV = (Egc * os_ + gc.abs() * Eo[:, s] + Egc * Eo[:, s] + 2 * U * gc.abs() * os_ + (Ea[:, s] + U * as_) * V.abs()
              + (as_ + Ea[:, s]) * EV + U * (gc.abs() * os_ + as_ * Vabs))
        Vabs = gc.abs() * os_ + as_ * Vabs
        V = gc * os_ + as_ * V
    sr = sc["samp_ray"][:S].long()
    slot = torch.arange(S) - sc["ray_soff"].long()[sr]
    Edfeat = Edf[sr, slot]
    # ---- losses
    nb = (R * 8 + 255) // 256
    chain = 3 + 6 + 4 + (nb + 255) // 256 + 6 + 4
    se = (diff ** 2).sum(-1)
    Ese = (2 * diff.abs() * Efull + Efull ** 2).sum(-1) + 10 * U * se
    L = ref["losses"]

    def summed(Eterms, terms, den, val, ch):
        return (float(Eterms.sum()) + 2 * ch * U * float(terms.abs().sum())) / den + 2 * U * abs(float(val))
    El = torch.zeros(4, dtype=torch.float64)
    El[0] = summed(Ese * m, se * m, max(3 * n, 1), L[0], chain)
    El[2] = summed(Ese * (1 - m), se * (1 - m), 3.0, L[2], chain)
    El[3] = summed(Ese, se, 3.0 * R, L[3], chain)
    conf32 = sc["conf"]
    inside, const = rs.zero_one_branch(conf32)
    val = torch.where(inside, conf32.double(), const)
    term = torch.log(val) + torch.log(1 - val)
    Eterm = 4 * U * (torch.log(val).abs() + torch.log(1 - val).abs()) + U + U * term.abs()
    pd = ref["pd"].clamp(min=0).long()
    nv_max = int(sc["ray_ns"].max()) if R else 0
    ch_zo = chain + nv_max * ((K + 7) // 8) + 1
    El[1] = summed(Eterm[pd] * m[:, None, None], term[pd] * m[:, None, None], max(n * SR * K, 1), L[1], ch_zo)
    # ---- d conf
    gz = zo_w / max(n * SR * K, 1)
    d = torch.where(inside, 1 / val - 1 / (1 - val), torch.zeros_like(val))
    Ed = torch.where(inside, gz * (3 * U / val + 4 * U / (1 - val)) + 4 * U * gz * d.abs(), torch.zeros_like(val))
    named = ref["pd"][mask]                                   # [n, SR, K]
    cnt = torch.bincount(named[named >= 0].long(), minlength=rs.N_POINTS).double()   # entries naming each point
    mcount, sabs, Esum = cnt.clone(), cnt * gz * d.abs(), cnt * Ed
    if bool(inside[0]) and n:                                 # the empty entries: one term gz d0 n_empty per lane and ray
        empty = (named < 0).sum(dim=1).double()               # [n, K]
        lanes = torch.zeros(n, 8, dtype=torch.float64)
        lanes.index_add_(1, torch.arange(K) % 8, empty)
        mcount[0] += float((lanes > 0).sum())
        sabs[0] += float(lanes.sum()) * gz * abs(float(d[0]))
        Esum[0] += float(lanes.sum()) * float(Ed[0]) + 2 * U * float(lanes.sum()) * gz * abs(float(d[0]))
    Edconf = 2 * (mcount + 1) * U * (start.double().abs() + sabs) + Esum
    return dict(Edfeat=Edfeat, Elosses=El, Edconf=Edconf, named=cnt > 0)


# ---- device side ---------------------------------------------------------------------------------

class Dev:
    """A scene's tensors on the device and its hand-built QueryOut."""

    def __init__(self, sc):
        up = lambda t: t.contiguous().to(DEV)  # noqa: E731
        self.d = {k: up(sc[k]) for k in ("conf", "campos", "rot", "ray_ns", "ray_soff", "samp_ray", "samp_locw", "samp_nnb",
                                         "pidx", "feat", "gt", "bg_ray")}
        self.d["none"] = torch.zeros(4, dtype=torch.int32, device=DEV)
        qo = self.qo = _lib.QueryOut()
        qo.samp_d = qo.work = qo.counters = self.d["none"].data_ptr()   # not read by these kernels
        for k in ("ray_ns", "ray_soff", "samp_ray", "samp_nnb", "pidx", "samp_locw"):
            setattr(qo, k, self.d[k].data_ptr())


# (R, SR, K, unit, bg_ray, camera, scene magnitudes); the zero-one weight alternates 1.0 (LossStage) / 1e-4 (the f32 step)
LOSS_CASES = [
    (1, 1, 1, 0, False, 0, {}),
    (31, 24, 8, 0, False, 0, {}),
    (33, 33, 3, 1, True, 1, {}),
    (65, 64, 16, 0, True, 0, dict(x_lo=-1.5)),
    (130, 128, 9, 1, False, 1, dict(x_lo=-1.3, rgb_max=0.6)),
    (37, 36, 8, 1, False, 0, {}),
    (8229, 4, 1, 0, False, 0, {}),        # 258 block partials: two trips of k_loss_reduce's strided loop
    (31, 24, 8, 1, True, 1, dict(conf0=0.0)),   # point 0 at the clamp: the empty entries carry no gradient
]


@functools.lru_cache(maxsize=None)
def loss_case(i):
    R, SR, K, unit, bgr, camera, kw = LOSS_CASES[i]
    zo_w = 1.0 if i % 2 == 0 else 1e-4
    sc = rs.ray_scene(R, SR, K, seed=20 + i, camera=camera, **kw)
    ref = rs.reference(sc, unit, bgr, bg=BG, zero_one_weight=zo_w)
    fb = forward_bounds(sc, ref, sc["ray_ns"].double())
    g = torch.Generator().manual_seed(i)
    scale = 0.1 * float(ref["dconf"].abs().max()) or 1e-6
    start = (scale * (0.25 + torch.rand(rs.N_POINTS + GUARD, generator=g)) * (1 - 2 * (torch.arange(rs.N_POINTS + GUARD) % 2))).to(F32)
    lb = loss_bounds(sc, ref, fb, zo_w, start[:rs.N_POINTS])
    return sc, ref, fb, lb, start, zo_w


def _loss_params(sc, unit, zo_w, bg_ray):
    lp = _lib.LossParams()
    lp.SR, lp.K, lp.vsize_z, lp.raydist_mode_unit = sc["SR"], sc["K"], rs.VZ, unit
    lp.bg[0], lp.bg[1], lp.bg[2] = BG
    lp.zero_one_weight, lp.zero_one_eps = zo_w, rs.ZO_EPS
    lp.bg_ray = bg_ray.data_ptr() if bg_ray is not None else None
    return lp


def _run_loss(sc, dv, unit, bgr, zo_w, start, R=None):
    R = sc["R"] if R is None else R
    SR, S_cap = sc["SR"], sc["S_cap"]
    d = dv.d
    out = dict(rgb=torch.full((sc["R"] + GUARD, 3), NAN, device=DEV), mask=torch.full((sc["R"] + GUARD,), 77, dtype=torch.int8, device=DEV),
               losses=torch.full((8 + GUARD,), NAN, device=DEV), dfeat=torch.full((S_cap + GUARD, 4), NAN, device=DEV),
               dconf=start.clone().to(DEV))
    ws = torch.empty(max(int(_lib.lib().sgn_loss_workspace_bytes(R, SR)), 16) + 64, dtype=torch.uint8, device=DEV)
    lp = _loss_params(sc, unit, zo_w, d["bg_ray"] if bgr else None)
    p = _lib.ptr
    _lib.check(_lib.lib().sgn_loss_train(ctypes.byref(lp), p(d["campos"]), p(d["rot"]), R, ctypes.byref(dv.qo), p(d["feat"]),
                                         p(d["gt"]), p(d["conf"]), p(out["rgb"]), p(out["mask"]), p(out["losses"]), p(out["dfeat"]),
                                         p(out["dconf"]), p(ws), ws.numel(), _lib.stream_handle()), "sgn_loss_train")
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


@pytest.mark.parametrize("i", range(len(LOSS_CASES)))
def test_loss_train(i):
    R, SR, K, unit, bgr, camera, _ = LOSS_CASES[i]
    sc, ref, fb, lb, start, zo_w = loss_case(i)
    print(f"case {LOSS_CASES[i]}, zero_one_weight {zo_w}, skipped plantings: {sc['skipped']}")
    S, N, n, mask = sc["S"], rs.N_POINTS, ref["n"], ref["mask"]
    # ---- caps: conditions on the bounds
    _capped_fwd(fb["Ergb"], "colour", ref["rgb"])
    _capped(lb["Edfeat"][:, 0], ref["dfeat"][:S, 0], "d feat.x")
    _capped(lb["Edfeat"][:, 1:], ref["dfeat"][:S, 1:], "d feat.yzw")
    for j in range(4):
        if float(ref["losses"][j]) != 0:
            _capped(lb["Elosses"][j], ref["losses"][j], f"losses[{j}]")
    want_dconf = start[:N].double() + ref["dconf"]
    _capped(lb["Edconf"], want_dconf, "d conf")
    dv = Dev(sc)
    out = _run_loss(sc, dv, unit, bgr, zo_w, start)
    again = _run_loss(sc, dv, unit, bgr, zo_w, start)
    # ---- guards, untouched entries, determinism
    assert _all_nan(out["rgb"][R:]) and bool((out["mask"][R:] == 77).all()) and _all_nan(out["losses"][8:])
    assert _all_nan(out["dfeat"][S:])                                         # guard rows and the samples past S
    assert _same_bits(out["dconf"][N:], start[N:])
    unnamed = ~lb["named"]
    unnamed[0] = False                                                         # point 0 takes the empty entries
    assert int(unnamed.sum()) >= 30 and _same_bits(out["dconf"][:N][unnamed], start[:N][unnamed])
    assert bool((start[:N][unnamed] != 0).all())
    assert torch.equal(out["mask"], again["mask"])
    for k in ("rgb", "losses", "dfeat"):                                       # everything but d conf (atomics) repeats bit for bit
        assert _same_bits(out[k], again[k]), k
    # ---- bit-exact parts
    assert torch.equal(out["mask"][:R].bool(), mask)
    L = out["losses"][:8]
    n32 = torch.tensor(float(n), dtype=F32)
    assert float(L[6]) == n and float(L[7]) == 0.0 and _same_bits(L[7:8], torch.zeros(1))
    den_c = torch.maximum(torch.tensor(3.0, dtype=F32) * n32, torch.tensor(1.0, dtype=F32))
    den_z = torch.maximum(n32 * torch.tensor(float(SR * K), dtype=F32), torch.tensor(1.0, dtype=F32))
    assert _same_bits(L[4:5], (torch.tensor(2.0, dtype=F32) / den_c).reshape(1))
    assert _same_bits(L[5:6], (torch.tensor(zo_w, dtype=F32) / den_z).reshape(1))
    bgv = ref["bg"].to(F32)
    assert _same_bits(out["rgb"][:R][~mask], bgv[~mask])                        # missed rays: their background, bit for bit
    sr = sc["samp_ray"][:S].long()
    assert bool((out["dfeat"][:S][~mask[sr]] == 0).all())                       # .. and no gradient to their samples
    # ---- per element
    Efull = fb["Ergb"] * mask.double()[:, None]
    _ratio(out["rgb"][:R], ref["full"], Efull, "rgb")
    _ratio(out["dfeat"][:S, 0], ref["dfeat"][:S, 0], lb["Edfeat"][:, 0], "d feat.x")
    _ratio(out["dfeat"][:S, 1:], ref["dfeat"][:S, 1:], lb["Edfeat"][:, 1:], "d feat.yzw")
    for j, name in enumerate(("colour", "zero-one", "missed", "all rays")):
        _ratio(L[j:j + 1], ref["losses"][j:j + 1], lb["Elosses"][j:j + 1], f"losses[{j}] ({name})")
    _ratio(out["dconf"][:N], want_dconf, lb["Edconf"], "d conf")
    _ratio(again["dconf"][:N], want_dconf, lb["Edconf"], "d conf (second run)")


def test_loss_train_no_ray():
    """R = 0: the call succeeds, d_losses is eight zeros, every other output keeps its sentinel."""
    sc, ref, fb, lb, start, zo_w = loss_case(1)
    out = _run_loss(sc, Dev(sc), 0, False, zo_w, start, R=0)
    assert _same_bits(out["losses"][:8], torch.zeros(8)) and _all_nan(out["losses"][8:])
    assert _all_nan(out["rgb"]) and bool((out["mask"] == 77).all()) and _all_nan(out["dfeat"]) and _same_bits(out["dconf"], start)


# ---- sgn_composite -------------------------------------------------------------------------------

def _scene_kw(SR):
    """The scene's magnitudes by SR, chosen so that the derived bounds keep their caps: denser rays from SR 64
    (T has decayed by the late slots), colours up to 0.6 from SR 100 (the colour sum's 2 (n + 1) u)."""
    return dict(x_lo=-2.0 if SR < 64 else -1.4, rgb_max=1.0 if SR < 100 else 0.6)


COMPOSITE_CASES = [(1, 1), (63, 4), (64, 24), (65, 32), (130, 33), (70, 36), (64, 64), (65, 100), (130, 128)]


def _run_composite(sc, dv, feat, unit, want_o, want_b):
    R, SR = sc["R"], sc["SR"]
    out = dict(rgb=torch.full((R + GUARD, 3), NAN, device=DEV), mask=torch.full((R + GUARD,), 77, dtype=torch.int8, device=DEV),
               bgT=torch.full((R + GUARD,), NAN, device=DEV),
               o=torch.full((R + GUARD, SR), NAN, device=DEV) if want_o else None,
               w=torch.full((R + GUARD, SR), NAN, device=DEV) if want_b else None)
    cp = _lib.CompositeParams()
    cp.SR, cp.vsize_z, cp.raydist_mode_unit = SR, rs.VZ, unit
    cp.bg[0], cp.bg[1], cp.bg[2] = BG
    p, d = _lib.ptr, dv.d
    _lib.check(_lib.lib().sgn_composite(ctypes.byref(cp), p(d["campos"]), p(d["rot"]), p(d["gt"]), R, None, 0, 0,
                                        ctypes.byref(dv.qo), p(feat), p(out["rgb"]), p(out["mask"]), p(out["bgT"]), p(out["o"]),
                                        p(out["w"]), _lib.stream_handle()), "sgn_composite")
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu()) for k, v in out.items()}


@pytest.mark.parametrize("i", range(len(COMPOSITE_CASES)))
def test_composite(i):
    R, SR = COMPOSITE_CASES[i]
    sc = rs.ray_scene(R, SR, 4, seed=40 + i, camera=i % 2, **_scene_kw(SR))
    print(f"(R, SR) = {(R, SR)}, skipped plantings: {sc['skipped']}")
    dv = Dev(sc)
    S = sc["S"]
    nan_feat = sc["feat"].clone()
    nan_feat[:S][sc["samp_nnb"][:S] == 0] = NAN
    nan_feat = nan_feat.to(DEV)
    pad = torch.arange(SR)[None, :] >= sc["ray_ns"].long()[:, None]
    for unit in (0, 1):
        ref = rs.reference(sc, unit, False, bg=BG)
        fb = forward_bounds(sc, ref, sc["ray_ns"].double())
        for k in ("Eo", "ET", "Ew"):
            _capped_fwd(fb[k], k)
        _capped_fwd(fb["ETend"], "bg T")
        _capped_fwd(fb["Ergb"], "colour", ref["rgb"])
        mask = ref["mask"]
        runs = {(wo, wb): _run_composite(sc, dv, dv.d["feat"], unit, wo, wb) for wo in (False, True) for wb in (False, True)}
        full = runs[(True, True)]
        for key, out in runs.items():
            assert _all_nan(out["rgb"][R:]) and bool((out["mask"][R:] == 77).all()) and _all_nan(out["bgT"][R:]), key
            for k in ("o", "w"):
                assert out[k] is None or _all_nan(out[k][R:]), (key, k)
            # the early-exit path (nothing staged) against the staged ones: the same bits
            assert _same_bits(out["rgb"], full["rgb"]) and torch.equal(out["mask"], full["mask"]) and _same_bits(out["bgT"], full["bgT"]), key
            for k in ("o", "w"):
                assert out[k] is None or _same_bits(out[k], full[k]), (key, k)
        withnan = _run_composite(sc, dv, nan_feat, unit, True, True)    # features of samples without a neighbour are ignored
        for k in ("rgb", "bgT", "o", "w"):
            assert _same_bits(withnan[k], full[k]), k
        assert torch.equal(withnan["mask"], full["mask"])
        assert torch.equal(full["mask"][:R].bool(), mask)
        bgv = ref["bg"].to(F32)
        assert _same_bits(full["rgb"][:R][~mask], bgv[~mask]) and bool((full["bgT"][:R][~mask] == 1).all())
        for k in ("o", "w"):
            assert bool((full[k][:R][~mask] == 0).all()) and bool((full[k][:R][pad] == 0).all()), k
        m = mask.double()
        tag = f"unit {unit}"
        _ratio(full["rgb"][:R], ref["full"], fb["Ergb"] * m[:, None], f"{tag} rgb")
        _ratio(full["bgT"][:R], ref["bgT_filled"], fb["ETend"] * m, f"{tag} bg T")
        _ratio(full["o"][:R], ref["o"], fb["Eo"], f"{tag} opacity")
        _ratio(full["w"][:R], ref["w"], fb["Ew"], f"{tag} blend weight")


# ---- one walk: the loss stage's colour, mask and depth are the composite's ----------------------------

def _run_walk(sc, dv, unit, bg, bg_ray):
    """sgn_composite_depth with the constant bg, and sgn_loss_train / sgn_loss_train_depth with bg or the per-ray
    bg_ray, on the scene's query and feat: the outputs both sides have."""
    R, SR = sc["R"], sc["SR"]
    p, d = _lib.ptr, dv.d
    L, st = _lib.lib(), _lib.stream_handle()
    f32 = dict(dtype=F32, device=DEV)
    comp = dict(rgb=torch.full((R, 3), NAN, **f32), mask=torch.full((R,), 77, dtype=torch.int8, device=DEV),
                bgT=torch.full((R,), NAN, **f32), depth=torch.full((R,), NAN, **f32))
    cp = _lib.CompositeParams()
    cp.SR, cp.vsize_z, cp.raydist_mode_unit = SR, rs.VZ, unit
    cp.bg[0], cp.bg[1], cp.bg[2] = bg
    stock = dict(rgb=torch.full((R, 3), NAN, **f32), mask=torch.full((R,), 77, dtype=torch.int8, device=DEV))
    _lib.check(L.sgn_composite(ctypes.byref(cp), p(d["campos"]), p(d["rot"]), p(d["gt"]), R, None, 0, 0, ctypes.byref(dv.qo),
                               p(d["feat"]), p(stock["rgb"]), p(stock["mask"]), None, None, None, st), "sgn_composite")
    _lib.check(L.sgn_composite_depth(ctypes.byref(cp), p(d["campos"]), p(d["rot"]), p(d["gt"]), R, None, 0, 0,
                                     ctypes.byref(dv.qo), p(d["feat"]), p(comp["rgb"]), p(comp["mask"]), p(comp["bgT"]), None,
                                     None, p(comp["depth"]), st), "sgn_composite_depth")
    lp = _lib.LossParams()
    lp.SR, lp.K, lp.vsize_z, lp.raydist_mode_unit = SR, sc["K"], rs.VZ, unit
    lp.bg[0], lp.bg[1], lp.bg[2] = bg
    lp.zero_one_weight, lp.zero_one_eps = 1e-4, rs.ZO_EPS
    lp.bg_ray = None if bg_ray is None else bg_ray.data_ptr()
    ws = torch.empty(max(int(L.sgn_loss_depth_workspace_bytes(R, SR)), 16), dtype=torch.uint8, device=DEV)
    gt_d = torch.ones(R, **f32)
    loss = {}
    for name in ("stock", "depth"):
        o = loss[name] = dict(rgb=torch.full((R, 3), NAN, **f32), mask=torch.full((R,), 77, dtype=torch.int8, device=DEV),
                              depth=torch.full((R,), NAN, **f32))
        args = (p(d["campos"]), p(d["rot"]), R, ctypes.byref(dv.qo), p(d["feat"]), p(d["gt"]), p(d["conf"]), p(o["rgb"]),
                p(o["mask"]), p(torch.empty(8, **f32)), p(torch.empty(sc["S_cap"], 4, **f32)), None, p(ws), ws.numel(), st)
        if name == "stock":
            _lib.check(L.sgn_loss_train(ctypes.byref(lp), *args), "sgn_loss_train")
        else:
            dp = _lib.LossDepth(gt_d.data_ptr(), None, 0.5, o["depth"].data_ptr())
            _lib.check(L.sgn_loss_train_depth(ctypes.byref(lp), ctypes.byref(dp), *args), "sgn_loss_train_depth")
    torch.cuda.synchronize()
    cpu = lambda m: {k: v.cpu() for k, v in m.items()}  # noqa: E731
    return cpu(stock), cpu(comp), cpu(loss["stock"]), cpu(loss["depth"])


@pytest.mark.parametrize("bgr", [False, True])
@pytest.mark.parametrize("unit", [0, 1])
@pytest.mark.parametrize("SR", [5, 36])
def test_loss_stage_walk_is_the_composites(SR, unit, bgr):
    """The contract csrc/ray_walk.h carries: on one query and one feat (zeros at samples without neighbours)
    sgn_loss_train's out_rgb / out_mask are sgn_composite's and sgn_loss_train_depth's out_depth is
    sgn_composite_depth's, bit for bit.  R = 70 crosses a 64-ray composite workgroup and a 32-ray loss block;
    SR = 5 is less than one 32-slot chunk and no multiple of 4, SR = 36 is two chunks.  With a per-ray background
    the composite side has no matching input: it runs with bg 0 (its colour is then the bare sum, x + 0 * T = x)
    and the loss stage's colour is that sum + bg_ray * T_end, the two roundings the kernel makes, for the rays
    with a valid sample; the others carry bg_ray itself."""
    R, K = 70, 3
    sc = rs.ray_scene(R, SR, K, seed=90 + SR, camera=1 if SR == 5 else 0, **_scene_kw(SR))
    # ---- the scene holds every case the walk distinguishes (from the inputs alone)
    S, ns = sc["S"], sc["ray_ns"].long()
    assert bool((sc["feat"][:S][sc["samp_nnb"][:S] == 0] == 0).all())
    _, valid, raw = rs.ray_dist_fp32(sc, unit)
    assert bool((ns == 0).any()) and bool((ns == SR).any()) and bool((ns == SR - 1).any())
    assert bool(((ns > 0) & ~valid.any(dim=1)).any())                       # samples, none with a neighbour
    c, r = sc["campos"], sc["rot"].reshape(-1)
    pos = rs.densify(sc, sc["samp_locw"])
    z = ((pos[..., 0] - c[0]) * r[2] + (pos[..., 1] - c[1]) * r[5]) + (pos[..., 2] - c[2]) * r[8]
    pair = torch.arange(1, SR)[None, :] < ns[:, None]                       # slots s, s + 1 both hold a sample
    assert bool(((z[:, 1:] == z[:, :-1]) & (raw[:, :-1] < 1e-8) & pair).any())
    assert bool(((raw[:, :-1] > 2 * rs.VZ) & pair).any())
    dv = Dev(sc)
    bg = (0.0, 0.0, 0.0) if bgr else BG
    stock, comp, loss, loss_d = _run_walk(sc, dv, unit, bg, dv.d["bg_ray"] if bgr else None)
    mask = comp["mask"].bool()
    assert torch.equal(mask, valid.any(dim=1)) and torch.equal(stock["mask"], comp["mask"])
    assert _same_bits(stock["rgb"], comp["rgb"])
    want = comp["rgb"]
    if bgr:
        want = torch.where(mask[:, None], comp["rgb"] + sc["bg_ray"] * comp["bgT"][:, None], sc["bg_ray"])
    for name, out in (("sgn_loss_train", loss), ("sgn_loss_train_depth", loss_d)):
        assert torch.equal(out["mask"], comp["mask"]), name
        assert _same_bits(out["rgb"], want), name
    assert _same_bits(loss_d["depth"], comp["depth"])
    assert _all_nan(loss["depth"])


# ---- sgn_ray_march_dense -------------------------------------------------------------------------

DENSE_CASES = [(1, 1), (255, 24), (257, 33), (256, 128)]


@pytest.mark.parametrize("i", range(len(DENSE_CASES)))
@pytest.mark.parametrize("with_bg", [False, True])
def test_ray_march_dense(i, with_bg):
    R, SR = DENSE_CASES[i]
    unit = i % 2
    sc = rs.ray_scene(R, SR, 2, seed=60 + i, camera=(i + 1) % 2, **_scene_kw(SR))
    print(f"(R, SR) = {(R, SR)}, skipped plantings: {sc['skipped']}")
    dist, valid, _ = rs.ray_dist_fp32(sc, unit)
    fd = rs.densify(sc, sc["feat"])
    bgv = torch.tensor(BG if with_bg else (0.0, 0.0, 0.0), dtype=F32).expand(R, 3)
    ref = rs.march_ref(dist, valid, fd.double(), bgv)
    ref.update(dist=dist, valid=valid, bg=bgv)
    fb = forward_bounds(sc, ref, SR)
    for k in ("Eo", "ET", "Ew"):
        _capped_fwd(fb[k], k)
    _capped_fwd(fb["ETend"], "bg T")
    _capped_fwd(fb["Ergb"], "colour", ref["rgb"])
    up = lambda t: t.contiguous().to(DEV)  # noqa: E731
    d_dist, d_valid, d_feat = up(dist), up(valid.to(torch.uint8)), up(fd)
    out = dict(rgb=torch.full((R + GUARD, 3), NAN, device=DEV), bgT=torch.full((R + GUARD,), NAN, device=DEV),
               **{k: torch.full((R + GUARD, SR), NAN, device=DEV) for k in ("o", "T", "w")})
    bg = (_lib.c_f32 * 3)(*BG) if with_bg else None
    p = _lib.ptr
    _lib.check(_lib.lib().sgn_ray_march_dense(p(d_dist), p(d_valid), p(d_feat), R, SR, bg, p(out["rgb"]), p(out["o"]), p(out["T"]),
                                              p(out["w"]), p(out["bgT"]), _lib.stream_handle()), "sgn_ray_march_dense")
    torch.cuda.synchronize()
    out = {k: v.cpu() for k, v in out.items()}
    for k, v in out.items():
        assert _all_nan(v[R:]), k
    assert bool((out["T"][:R, 0] == 1).all())                     # acc_t is the transmittance BEFORE the slot
    pad = torch.arange(SR)[None, :] >= sc["ray_ns"].long()[:, None]
    assert bool((out["o"][:R][pad] == 0).all()) and bool((out["w"][:R][pad] == 0).all())
    _ratio(out["rgb"][:R], ref["rgb"], fb["Ergb"], "rgb")
    _ratio(out["bgT"][:R], ref["bgT"], fb["ETend"], "bg T")
    _ratio(out["o"][:R], ref["o"], fb["Eo"], "opacity")
    _ratio(out["T"][:R], ref["T"], fb["ET"], "acc_t")
    _ratio(out["w"][:R], ref["w"], fb["Ew"], "blend weight")
