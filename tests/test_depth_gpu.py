"""Depth on the per-ray kernels -- sgn_composite_depth (k_composite<true>) and sgn_loss_train_depth (the DEPTH
instantiations of k_loss_fwd / k_loss_reduce / k_loss_bwd) -- called directly through the C ABI on the scenes of
tests/ray_stage_ref.py, as tests/test_ray_stage_gpu.py calls the stock entries (its helpers are used here:
sentinels, guard rows, _ratio, _capped, forward_bounds, loss_bounds), and compared element by element with
tests/depth_ref.py's float64 reference (pinned to train.composite_losses and to finite differences in
test_depth_ref_cpu.py).  Everything the stock entries also produce must equal their output bit for bit.

Bounds, per element, on top of test_ray_stage_gpu.py's (u = 2^-24, E_w its blend-weight bound).  z_s is the same
fp32 value in kernel and reference, so it carries no error.

Sums.  The kernel adds the terms t_k (w_k for W, fl(w_k z_k) for A) in ascending slot order.  One addition
s' = fl(s + t) is off by at most u |s + t| and by at most |t| (s is representable, and fl rounds to the nearest),
so with P_k the partial sums (taken with the terms' own errors, P_k + sum_{j<=k} E_j)
  R_W = sum_{k>=1} min(u P_k, w_k + E_w),   R_A = sum_k (u |w z| + 2^-149) + sum_{k>=1} min(u |PA_k|, |w_k z_k| + E_w |z_k|)
(the first addition, to 0, is exact).  A ray whose weights have decayed pays for its late slots no more than
their size, which keeps SR = 128 below the cap where 2 (n + 1) u sum|terms| would not (1.45e-5 there).
  E_W = sum E_w + R_W.
Depth.  With Wd = W + 1e-6f the reference has A = D Wd exactly, so the kernel's D' = A' / Wd' obeys
  D' - D = (dA - D dW) / Wd',   dA - D dW = sum_s dw_s (z_s - D) + rho_A - D rho_W:
  E_D = (sum_s E_w |z_s - D| + R_A + |D| R_W) / (Wd - E_W - u Wd) + 3 u |D|
(three roundings: W + 1e-6f, the division, and slack).  A ray of tiny W gets a wide bound from the same formula;
it is checked against it all the same.  A ray without a valid sample holds 0, bit for bit.
Loss.  t_r = (m (D - g))^2: E_t = 2 m |m (D - g)| E_D + (m E_D)^2 + 4 u t; the sum as the stock losses' chain
(one term per ray), then / R: E_L = (sum E_t + 2 chain u sum t) / R + 2 u L.
Gradient.  gD = w_d 2 m^2 (D - g) / R:  E_gD = (2 w_d m^2 / R) E_D + 8 u |gD|.
q_s = (z_s - D) / Wd:  E_q = (E_D + u |z_s - D|) / den + |q| (E_W + u Wd) / den + 2 u |q|,  den = Wd - E_W - u Wd.
The reverse pass takes gc'_s = gc_s + gD q_s in place of gc_s:
  E_gc' = E_gc + E_gD |q| + |gD| E_q + E_gD E_q + u |gD q| + u |gc'|,
and test_ray_stage_gpu.py's V recursion, E_dO and d sigma's bound go through unchanged with gc', E_gc' (V_end is
still g . bg: depth has no background term).

Caps (conditions on the bounds, asserted before anything runs): E_D < F32_TOL max(1, |D|) on every valid ray with
W >= 0.05, which are at least 80 % of the valid rays where R >= 31; E_L and the d feat.x bound below
GRAD_TOL_F32 of the reference's largest magnitude."""
import ctypes
import functools

import pytest
import torch

import sgnerf_amd  # noqa: F401
from sgnerf_amd import _lib

import depth_ref as dr
import ray_stage_ref as rs
import test_ray_stage_gpu as rsg
from test_ray_stage_gpu import BG, DEV, F32, F32_TOL, GUARD, NAN, U, Dev, _all_nan, _capped, _ratio, _same_bits

pytestmark = pytest.mark.gpu
W_MIN = 0.05
W_D = 0.5
ZO_W = 1e-4


# ---- bounds (CPU, float64, from the reference alone) ------------------------------------------------

def depth_bounds(z, w, Ew, D, W, mask):
    """E_D [R], E_W [R] and den [R] as the module docstring derives them."""
    zd, u1 = z.double(), U * (1 + 1e-3)
    t = w * zd
    Et = Ew * zd.abs()
    PW = torch.cumsum(w, 1) + torch.cumsum(Ew, 1)
    PA = torch.cumsum(t, 1).abs() + torch.cumsum(Et, 1)
    RW = torch.minimum(u1 * PW, w + Ew)
    RA = torch.minimum(u1 * PA, t.abs() + Et)
    RW[:, 0] = 0
    RA[:, 0] = 0
    RA = RA + (U * t.abs() + 2.0 ** -149) * (w != 0).double()
    EW = Ew.sum(1) + RW.sum(1)
    Wd = W + dr.EPS_D
    den = (Wd - EW - U * Wd).clamp(min=1e-300)
    num = (Ew * (zd - D[:, None]).abs()).sum(1) + RA.sum(1) + D.abs() * RW.sum(1)
    ED = (num / den + 3 * U * D.abs() + 2.0 ** -149) * mask.double()
    return ED, EW, den


def check_depth_caps(ED, D, W, mask, R, what):
    good = mask & (W >= W_MIN)
    lim = F32_TOL * D.abs().clamp(min=1.0)
    assert bool((ED[good] < lim[good]).all()), f"{what}: depth bound {float(ED[good].max()):.3e} is not below F32_TOL"
    share = float(good.sum()) / max(int(mask.sum()), 1)
    print(f"{what}: {int(good.sum())} of {int(mask.sum())} valid rays have W >= {W_MIN}; worst bound there "
          f"{float((ED[good] / lim[good]).max()) if bool(good.any()) else 0.0:.3f} of the cap")
    if R >= 31:
        assert share >= 0.8, f"{what}: only {share:.2f} of the valid rays have W >= {W_MIN}"


def depth_loss_bounds(sc, ref, fb, ED, EW, den, gt_d, gt_m, w_d):
    """(E_L, E d feat.x [S]) of the depth-supervised stage."""
    R, SR, S = sc["R"], sc["SR"], sc["S"]
    n, mask = ref["n"], ref["mask"]
    mk = mask.double()
    g_d = gt_d.double()
    md = (gt_d > 0).double() if gt_m is None else gt_m.double()
    D, W, z = ref["D"], ref["W"], ref["z"].double()
    # ---- the loss
    t = (md * (D - g_d)) ** 2
    Et = 2 * md * (md * (D - g_d)).abs() * ED + (md * ED) ** 2 + 4 * U * t
    nb = (R * 8 + 255) // 256
    chain = 3 + 6 + 4 + (nb + 255) // 256 + 6 + 4
    EL = (float(Et.sum()) + 2 * chain * U * float(t.sum())) / R + 2 * U * float(ref["l_depth"])
    # ---- the extra channel
    gD = w_d * 2 * md * md * (D - g_d) / R * mk
    EgD = ((2 * w_d * md * md / R) * ED + 8 * U * gD.abs()) * mk
    Wd = W + dr.EPS_D
    q = (z - D[:, None]) / Wd[:, None]
    Eq = (ED[:, None] + U * (z - D[:, None]).abs()) / den[:, None] + q.abs() * ((EW + U * Wd) / den)[:, None] + 2 * U * q.abs()
    # ---- test_ray_stage_gpu.loss_bounds' reverse pass with gc' = gc + gD q
    gs = 2.0 / max(3 * n, 1)
    diff = ref["full"] - sc["gt"].double()
    Efull = fb["Ergb"] * mk[:, None]
    g = gs * diff * mk[:, None]
    Eg = (gs * (Efull + U * diff.abs()) + 2 * U * g.abs()) * mk[:, None]
    bg, c = ref["bg"].double(), fb["c"]
    V = (g * bg).sum(-1)
    Vabs = (g.abs() * bg).sum(-1)
    EV = (Eg * bg).sum(-1) + 6 * U * Vabs + 2 * U * V.abs()
    o, T, av, e, dist = ref["o"], ref["T"], ref["av"], fb["e"], ref["dist"].double()
    Eo, Ea, ET, Ee = fb["Eo"], fb["Ea"], fb["ET"], fb["Ee"]
    Edf = torch.zeros(R, SR, dtype=torch.float64)
    for s in reversed(range(SR)):
        cs = c[:, s]
        gq = gD * q[:, s]
        gc = (g * cs).sum(-1) + gq
        Egc = ((Eg * cs).sum(-1) + 6 * U * (g.abs() * cs).sum(-1) + EgD * q[:, s].abs() + gD.abs() * Eq[:, s] + EgD * Eq[:, s]
               + U * gq.abs() + U * gc.abs())
        Ts, os_, as_ = T[:, s], o[:, s], av[:, s]
        dO = Ts * (gc - V)
        EdO = ET[:, s] * (gc.abs() + V.abs()) + Ts * (Egc + EV) + ET[:, s] * (Egc + EV) + 3 * U * Ts * (gc.abs() + V.abs()) + 1e-30
        ed = e[:, s] * dist[:, s]
        Edf[:, s] = EdO * ed + dO.abs() * Ee[:, s] * dist[:, s] + EdO * Ee[:, s] * dist[:, s] + 2 * U * (dO * ed).abs() + 2.0 ** -148
        EV = (Egc * os_ + gc.abs() * Eo[:, s] + Egc * Eo[:, s] + 2 * U * gc.abs() * os_ + (Ea[:, s] + U * as_) * V.abs()
              + (as_ + Ea[:, s]) * EV + U * (gc.abs() * os_ + as_ * Vabs))
        Vabs = gc.abs() * os_ + as_ * Vabs
        V = gc * os_ + as_ * V
    sr = sc["samp_ray"][:S].long()
    slot = torch.arange(S) - sc["ray_soff"].long()[sr]
    return EL, Edf[sr, slot]


# ---- sgn_composite_depth ---------------------------------------------------------------------------

COMPOSITE_CASES = [(1, 1), (63, 4), (64, 24), (65, 32), (130, 33), (64, 64), (130, 128)]


def _run_composite_depth(sc, dv, unit, want_o, want_b):
    R, SR = sc["R"], sc["SR"]
    out = dict(rgb=torch.full((R + GUARD, 3), NAN, device=DEV), mask=torch.full((R + GUARD,), 77, dtype=torch.int8, device=DEV),
               bgT=torch.full((R + GUARD,), NAN, device=DEV), depth=torch.full((R + GUARD,), NAN, device=DEV),
               o=torch.full((R + GUARD, SR), NAN, device=DEV) if want_o else None,
               w=torch.full((R + GUARD, SR), NAN, device=DEV) if want_b else None)
    cp = _lib.CompositeParams()
    cp.SR, cp.vsize_z, cp.raydist_mode_unit = SR, rs.VZ, unit
    cp.bg[0], cp.bg[1], cp.bg[2] = BG
    p, d = _lib.ptr, dv.d
    _lib.check(_lib.lib().sgn_composite_depth(ctypes.byref(cp), p(d["campos"]), p(d["rot"]), p(d["gt"]), R, None, 0, 0,
                                              ctypes.byref(dv.qo), p(d["feat"]), p(out["rgb"]), p(out["mask"]), p(out["bgT"]),
                                              p(out["o"]), p(out["w"]), p(out["depth"]), _lib.stream_handle()),
               "sgn_composite_depth")
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu()) for k, v in out.items()}


@pytest.mark.parametrize("camera", [0, 1])
@pytest.mark.parametrize("i", range(len(COMPOSITE_CASES)))
def test_composite_depth(i, camera):
    R, SR = COMPOSITE_CASES[i]
    sc = rs.ray_scene(R, SR, 4, seed=40 + i, camera=camera, **rsg._scene_kw(SR))
    dv = Dev(sc)
    z = dr.z_fp32(sc)
    for unit in (0, 1):
        ref = rs.reference(sc, unit, False, bg=BG)
        fb = rsg.forward_bounds(sc, ref, sc["ray_ns"].double())
        mask = ref["mask"]
        D, W, _ = dr.depth_of(ref["w"], z, mask)
        ED, _, _ = depth_bounds(z, ref["w"], fb["Ew"], D, W, mask)
        tag = f"(R, SR) = {(R, SR)}, camera {camera}, unit {unit}"
        check_depth_caps(ED, D, W, mask, R, tag)
        for wo, wb in ((True, True), (False, False)):      # staged rows, and the early-exit path
            stock = rsg._run_composite(sc, dv, dv.d["feat"], unit, wo, wb)
            out = _run_composite_depth(sc, dv, unit, wo, wb)
            again = _run_composite_depth(sc, dv, unit, wo, wb)
            for k in ("rgb", "bgT", "o", "w"):
                assert (out[k] is None and stock[k] is None) or _same_bits(out[k], stock[k]), (tag, k)
            assert torch.equal(out["mask"], stock["mask"])
            assert _all_nan(out["depth"][R:]), "guard rows"
            assert _same_bits(out["depth"], again["depth"])
            assert _same_bits(out["depth"][:R][~mask], torch.zeros(int((~mask).sum())))
            _ratio(out["depth"][:R], D, ED, f"{tag} depth (opacity / weights {'on' if wo else 'off'})")


# ---- sgn_loss_train_depth --------------------------------------------------------------------------

# (R, SR, K, unit, camera, scene magnitudes): test_ray_stage_gpu.LOSS_CASES' shapes and seeds
LOSS_CASES = [(1, 1, 1, 0, 0, {}, 20), (31, 24, 8, 0, 0, {}, 21), (33, 33, 3, 1, 1, {}, 22), (65, 64, 16, 0, 0, dict(x_lo=-1.5), 23),
              (8229, 4, 1, 0, 0, {}, 26)]


@functools.lru_cache(maxsize=None)
def loss_case(i, bgr):
    R, SR, K, unit, camera, kw, seed = LOSS_CASES[i]
    sc = rs.ray_scene(R, SR, K, seed=seed, camera=camera, **kw)
    fwd = dr.depth_map(sc, unit)
    gt_d, gt_m = dr.targets(sc, fwd["D"], seed=i)
    g = torch.Generator().manual_seed(i)
    refs = {}
    for name, m in (("null", None), ("explicit", gt_m)):
        ref = dr.reference(sc, unit, bgr, gt_d, m, W_D, bg=BG, zero_one_weight=ZO_W)
        fb = rsg.forward_bounds(sc, ref, sc["ray_ns"].double())
        refs[name] = (ref, fb, m)
    ref = refs["null"][0]
    scale = 0.1 * float(ref["dconf"].abs().max()) or 1e-6
    start = (scale * (0.25 + torch.rand(rs.N_POINTS + GUARD, generator=g)) * (1 - 2 * (torch.arange(rs.N_POINTS + GUARD) % 2))).to(F32)
    lb = rsg.loss_bounds(sc, ref, refs["null"][1], ZO_W, start[:rs.N_POINTS])
    return sc, gt_d, refs, start, lb


def _run_loss_depth(sc, dv, unit, bgr, start, gt_d, gt_m, w_d, R=None):
    R = sc["R"] if R is None else R
    SR, S_cap = sc["SR"], sc["S_cap"]
    d = dv.d
    out = dict(rgb=torch.full((sc["R"] + GUARD, 3), NAN, device=DEV), mask=torch.full((sc["R"] + GUARD,), 77, dtype=torch.int8, device=DEV),
               losses=torch.full((8 + GUARD,), NAN, device=DEV), dfeat=torch.full((S_cap + GUARD, 4), NAN, device=DEV),
               dconf=start.clone().to(DEV), depth=torch.full((sc["R"] + GUARD,), NAN, device=DEV))
    ws = torch.empty(max(int(_lib.lib().sgn_loss_depth_workspace_bytes(R, SR)), 16) + 64, dtype=torch.uint8, device=DEV)
    lp = rsg._loss_params(sc, unit, ZO_W, d["bg_ray"] if bgr else None)
    g_dev = gt_d.to(DEV)
    m_dev = None if gt_m is None else gt_m.to(DEV)
    dp = _lib.LossDepth(g_dev.data_ptr(), None if m_dev is None else m_dev.data_ptr(), w_d, out["depth"].data_ptr())
    p = _lib.ptr
    _lib.check(_lib.lib().sgn_loss_train_depth(ctypes.byref(lp), ctypes.byref(dp), p(d["campos"]), p(d["rot"]), R,
                                               ctypes.byref(dv.qo), p(d["feat"]), p(d["gt"]), p(d["conf"]), p(out["rgb"]),
                                               p(out["mask"]), p(out["losses"]), p(out["dfeat"]), p(out["dconf"]), p(ws),
                                               ws.numel(), _lib.stream_handle()), "sgn_loss_train_depth")
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


@pytest.mark.parametrize("bgr", [False, True])
@pytest.mark.parametrize("i", range(len(LOSS_CASES)))
def test_loss_train_depth(i, bgr):
    R, SR, K, unit, camera, _, _ = LOSS_CASES[i]
    sc, gt_d, refs, start, lb = loss_case(i, bgr)
    S, N = sc["S"], rs.N_POINTS
    dv = Dev(sc)
    stock = rsg._run_loss(sc, dv, unit, bgr, ZO_W, start)
    sr = sc["samp_ray"][:S].long()
    for name, (ref, fb, gt_m) in refs.items():
        tag = f"case {LOSS_CASES[i][:5]}, bg_ray {bgr}, mask {name}"
        mask = ref["mask"]
        D, W = ref["D"], ref["W"]
        ED, EW, den = depth_bounds(ref["z"], ref["w"], fb["Ew"], D, W, mask)
        check_depth_caps(ED, D, W, mask, R, tag)
        EL, Edx = depth_loss_bounds(sc, ref, fb, ED, EW, den, gt_d, gt_m, W_D)
        want_x = ref["dfeat_depth"][:S, 0]
        if float(ref["l_depth"]) != 0:      # (one ray whose explicit mask is 0: L_depth = 0 exactly)
            _capped(torch.tensor(EL), ref["l_depth"], "L_depth")
        _capped(Edx, want_x, "d feat.x")
        want_dconf = start[:N].double() + ref["dconf"]
        for w_d in (0.0, W_D):
            out = _run_loss_depth(sc, dv, unit, bgr, start, gt_d, gt_m, w_d)
            # ---- guards
            assert _all_nan(out["rgb"][R:]) and bool((out["mask"][R:] == 77).all()) and _all_nan(out["losses"][8:])
            assert _all_nan(out["dfeat"][S:]) and _all_nan(out["depth"][R:]) and _same_bits(out["dconf"][N:], start[N:])
            # ---- what the stock entry also writes: its bits
            assert _same_bits(out["rgb"], stock["rgb"]) and torch.equal(out["mask"], stock["mask"]), tag
            assert _same_bits(out["losses"][:7], stock["losses"][:7]), tag
            assert _same_bits(out["dfeat"][:S, 1:], stock["dfeat"][:S, 1:]), tag
            _ratio(out["dconf"][:N], want_dconf, lb["Edconf"], f"{tag}, weight {w_d}: d conf")
            # ---- depth and its loss
            assert _same_bits(out["depth"][:R][~mask], torch.zeros(int((~mask).sum())))
            _ratio(out["depth"][:R], D, ED, f"{tag}, weight {w_d}: depth")
            _ratio(out["losses"][7:8], ref["l_depth"].reshape(1), torch.tensor([EL]), f"{tag}, weight {w_d}: losses[7]")
            if w_d == 0.0:
                assert _same_bits(out["dfeat"][:S], stock["dfeat"][:S]), tag
            else:
                assert bool((out["dfeat"][:S][~mask[sr]] == 0).all())        # rays off the mask: no gradient
                _ratio(out["dfeat"][:S, 0], want_x, Edx, f"{tag}: d feat.x")
                if R >= 31:   # the depth term is far above the bound: a stage without it would fail here
                    assert float((want_x - ref["dfeat"][:S, 0]).abs().max()) > 100 * float(Edx.max())
        # rays off the mask hold D = 0 and still count in the loss: (m g)^2 / R each
        md = (gt_d > 0).double() if gt_m is None else gt_m.double()
        off = float((((md * gt_d.double()) ** 2) * (~mask).double()).sum()) / R
        if R in (31, 8229):   # (the two rays off the mask at R = 33 happen to have m g = 0; one mask's four at R = 65 too)
            assert off > 0
        assert off == 0 or off > 4 * EL, (off, EL)    # where they count, the loss check above sees them


def test_loss_train_depth_no_ray():
    """R = 0: the call succeeds, d_losses is eight zeros, every other output keeps its sentinel."""
    sc, gt_d, refs, start, lb = loss_case(1, False)
    out = _run_loss_depth(sc, Dev(sc), 0, False, start, gt_d, None, W_D, R=0)
    assert _same_bits(out["losses"][:8], torch.zeros(8)) and _all_nan(out["losses"][8:])
    assert _all_nan(out["rgb"]) and bool((out["mask"] == 77).all()) and _all_nan(out["dfeat"]) and _same_bits(out["dconf"], start)
    assert _all_nan(out["depth"])
