"""Float64 references of the per-ray stage (csrc/composite.hip: k_composite, k_ray_march_dense; csrc/loss.hip:
k_loss_fwd / k_loss_reduce / k_loss_bwd) and the seeded scene, with hand-placed rays, that the CPU and GPU
tests of those kernels share.

The formulas are those of include/sgn_hip.h, train.composite_losses and oracle/agg_ref.composite.
tests/test_ray_stage_ref_cpu.py pins them to both and checks the autograd gradients by finite differences,
so a GPU test that disagrees with this module names a kernel.

Every branch of the stage (the cummax, the two distance tests, the validity factor, the zero-one clamps)
is decided on fp32 values computed exactly as the kernels compute them (ray_dist_fp32, zero_one_branch);
the float64 arithmetic starts after the branches, so reference and kernel never sit on different sides of
a threshold."""
import math

import torch

VZ = 0.008            # vsize[2]
N_POINTS = 257
N_NAMED = 200         # random neighbours come from points [0, N_NAMED): the points after them are named by
                      # no ray except the planted conf values (points 1 .. 21)
ZO_EPS = 1e-3
EPS_T = float(torch.tensor(1e-10, dtype=torch.float32))   # the transmittance factor's 1e-10f
F32 = torch.float32

# (planting, smallest SR at which it fits), in the order in which rays are given out
PLANTINGS = [("full", 1), ("ns0", 1), ("no_nb", 1), ("ns1", 2), ("ns_sr_minus_1", 3), ("invalid_fml", 5),
             ("same_pos", 3), ("behind", 4), ("steps", 4), ("alpha0", 2), ("alpha_spread", 6), ("opaque_run", 7),
             ("ns32", 64), ("ns33", 64)]


def conf_plantings():
    """The 21 planted conf values: both clamps of the straight-through clamp (1e-4, 1), values outside them,
    the zero-one eps edges as fp32 evaluates them, and one fp32 step on either side of each."""
    eps = torch.tensor(ZO_EPS, dtype=F32)
    b = torch.stack([torch.tensor(v, dtype=F32) for v in (0.0, 1e-4, 1.0, 1.2, -0.1)] + [eps, torch.tensor(1.0) - eps])
    inf = torch.full_like(b, float("inf"))
    return torch.cat([b, torch.nextafter(b, inf), torch.nextafter(b, -inf)])


def ray_scene(R, SR, K, seed, camera=0, conf0=0.45, rgb_max=1.0, x_lo=-2.0):
    """CPU fp32 / int32 tensors of one scene: 257 points with conf, a camera, R rays of 0 .. SR samples
    (sample-major: ray_ns, ray_soff, samp_ray, samp_locw, samp_nnb, pidx with the valid neighbours as a prefix,
    feat = (alpha, r, g, b), zero on samples without a neighbour), gt, bg_ray; S < S_cap with five slack
    samples no ray names.  Samples lie along their ray with depth steps of vz x U(0.6, 1.4) from a first depth
    in [0.30, 0.40]; alpha x step is 10^U(x_lo, x_lo + 2).  camera 0 puts the world origin (the padding slots'
    position) at depth 0.1, behind every sample; camera 1 at 0.35 + SR vz / 2, ahead of some rays' last one.

    One ray each, where R and SR allow (scene['plant'] maps the name to the ray, scene['skipped'] lists the
    rest): full (ns = SR, all valid), ns0, no_nb (samples, none with a neighbour), ns1, ns_sr_minus_1,
    invalid_fml (first, a middle and the last sample invalid, each deeper than all before it), same_pos (two
    consecutive samples at one position), behind (a sample 0.5 vz behind its predecessor), steps (1.5 vz and
    3 vz: either side of the unit mode's 2 vz), alpha0 (alpha exactly 0 on a valid sample), alpha_spread
    (alpha x step over 1e-5 .. 300), opaque_run (six consecutive samples with alpha x dist >= 200), ns32 / ns33.
    conf holds conf_plantings() at points 1 .. 21, each named by a neighbour of a valid ray ('conf_values' is
    skipped where the scene has fewer than 21 such entries); conf[0] = conf0."""
    g = torch.Generator().manual_seed(seed * 7919 + R * 131 + SR * 17 + K)
    rnd = lambda *shape: torch.rand(*shape, generator=g, dtype=torch.float64)  # noqa: E731
    N = N_POINTS
    # ---- camera: a general rotation, so that the depth's three products all round
    yaw, pitch = math.radians(30.0), math.radians(-10.0)
    ry = torch.tensor([[math.cos(yaw), 0, math.sin(yaw)], [0, 1, 0], [-math.sin(yaw), 0, math.cos(yaw)]], dtype=torch.float64)
    rx = torch.tensor([[1, 0, 0], [0, math.cos(pitch), -math.sin(pitch)], [0, math.sin(pitch), math.cos(pitch)]],
                      dtype=torch.float64)
    rot64 = ry @ rx
    e1, e2, d = rot64[:, 0], rot64[:, 1], rot64[:, 2]    # depth of p = (p - campos) . d
    z0 = 0.1 if camera == 0 else 0.35 + 0.5 * SR * VZ
    campos64 = -z0 * d + 0.02 * e1 - 0.01 * e2
    # ---- rays and plantings
    ns = torch.randint(0, SR + 1, (R,), generator=g)
    plant, skipped = {}, []
    want = dict(full=SR, ns0=0, no_nb=min(SR, 5), ns1=1, ns_sr_minus_1=SR - 1, invalid_fml=min(SR, 7), same_pos=min(SR, 6),
                behind=min(SR, 6), steps=min(SR, 6), alpha0=min(SR, 4), alpha_spread=min(SR, 12), opaque_run=min(SR, 9),
                ns32=32, ns33=33)
    for name, min_sr in PLANTINGS:
        if len(plant) < R and SR >= min_sr:
            plant[name] = len(plant)
            ns[plant[name]] = want[name]
        else:
            skipped.append(name)
    soff = torch.cumsum(ns, 0) - ns
    S = int(ns.sum())
    S_cap = S + 5
    samp_ray = torch.repeat_interleave(torch.arange(R), ns)
    slot = torch.arange(S) - soff[samp_ray]
    off = {name: int(soff[r]) for name, r in plant.items()}
    # ---- depths
    step = VZ * (0.6 + 0.8 * rnd(S))
    if "same_pos" in plant:
        step[off["same_pos"] + 2] = 0.0
    if "behind" in plant:
        step[off["behind"] + 2] = -0.5 * VZ
    if "steps" in plant:
        step[off["steps"] + 1], step[off["steps"] + 2] = 1.5 * VZ, 3.0 * VZ
    step[slot == 0] = 0.0
    cs = torch.cumsum(step, 0)
    depth = (0.30 + 0.10 * rnd(R))[samp_ray] + cs - cs[soff[samp_ray]]   # a ray's first step is 0: cs there is the ray's base
    lat = 0.15 * (2 * rnd(R, 2) - 1)
    ray_vec = d[None] + lat[:, :1] * e1[None] + lat[:, 1:] * e2[None]
    locw = (campos64[None] + depth[:, None] * ray_vec[samp_ray]).to(F32)
    nxt = torch.cat([step[1:], torch.zeros(min(S, 1), dtype=torch.float64)])   # the step that closes a sample's interval
    last = slot == ns[samp_ray] - 1
    nxt = torch.where(last | (nxt < 1e-4), torch.full_like(nxt, VZ), nxt)
    # ---- neighbours
    nnb = torch.randint(1, K + 1, (S,), generator=g)
    nnb[rnd(S) < 0.25] = 0
    planted_ray = torch.zeros(R, dtype=torch.bool)
    planted_ray[:len(plant)] = True
    fix = planted_ray[samp_ray] & (nnb == 0)
    nnb[fix] = 1 + (torch.arange(S)[fix] % K)                      # planted rays: every sample valid ..
    if "no_nb" in plant:
        nnb[off["no_nb"]:off["no_nb"] + int(ns[plant["no_nb"]])] = 0   # .. except where the planting says otherwise
    if "invalid_fml" in plant:
        o_, n_ = off["invalid_fml"], int(ns[plant["invalid_fml"]])
        nnb[o_], nnb[o_ + n_ // 2], nnb[o_ + n_ - 1] = 0, 0, 0
    pidx = torch.randint(0, N_NAMED, (S_cap, K), generator=g)
    nnb_cap = torch.cat([nnb, torch.full((5,), K)])
    # ---- conf, its planted values named by valid entries of valid rays
    conf = (rnd(N) * 1.7 - 0.2).to(F32)
    cp = conf_plantings()
    conf[1:1 + cp.numel()] = cp
    conf[0] = conf0
    ray_valid = torch.zeros(R, dtype=torch.bool)
    ray_valid[samp_ray[nnb > 0]] = True
    es, ek = torch.nonzero((torch.arange(K)[None, :] < nnb[:, None]) & ray_valid[samp_ray][:, None], as_tuple=True)
    if es.numel() >= cp.numel():
        pick = torch.linspace(0, es.numel() - 1, cp.numel()).round().long()
        pidx[es[pick], ek[pick]] = torch.arange(1, 1 + cp.numel())
    else:
        skipped.append("conf_values")
    pidx[torch.arange(K)[None, :] >= nnb_cap[:, None]] = -1
    # ---- features
    x = 10.0 ** (x_lo + 2.0 * rnd(S))                                # alpha x step
    if "alpha_spread" in plant:
        o_, n_ = off["alpha_spread"], int(ns[plant["alpha_spread"]])
        x[o_:o_ + n_] = 10.0 ** torch.linspace(-5.0, math.log10(300.0), n_, dtype=torch.float64)
    alpha = x / nxt
    if "opaque_run" in plant:
        o_ = off["opaque_run"]
        alpha[o_] = 0.5 / VZ
        alpha[o_ + 1:o_ + 7] = 200.0 / (0.6 * VZ)
    if "alpha0" in plant:
        alpha[off["alpha0"] + 1] = 0.0
    feat = torch.cat([alpha[:, None], rgb_max * rnd(S, 3)], 1)
    feat = torch.where((nnb > 0)[:, None], feat, torch.zeros_like(feat))
    feat = torch.cat([feat, rnd(5, 4)]).to(F32)
    locw = torch.cat([locw, (rnd(5, 3) - 0.5).to(F32)])
    scene = dict(R=R, SR=SR, K=K, S=S, S_cap=S_cap, camera=camera, plant=plant, skipped=skipped,
                 xyz=(rnd(N, 3) * 2 - 1).to(F32), conf=conf, campos=campos64.to(F32), rot=rot64.to(F32).contiguous(),
                 ray_ns=ns.to(torch.int32), ray_soff=soff.to(torch.int32),
                 samp_ray=torch.cat([samp_ray, torch.zeros(5, dtype=torch.long)]).to(torch.int32),
                 samp_locw=locw.contiguous(), samp_nnb=nnb_cap.to(torch.int32), pidx=pidx.to(torch.int32).contiguous(),
                 feat=feat.contiguous(), gt=rnd(R, 3).to(F32), bg_ray=(rgb_max * rnd(R, 3)).to(F32))
    # no fp32 rounding decides a branch: a raw interval is exactly 0 or well above 1e-8, and well away from 2 vz
    raw = ray_dist_fp32(scene, 0)[2].double()
    assert bool(((raw == 0) | (raw > 1e-5)).all()) and bool(((raw - 2 * VZ).abs() > 1e-3 * VZ).all())
    return scene


def densify(scene, t, fill=0):
    """Sample-major [S_cap, ...] -> dense [R, SR, ...]; the slots after a ray's samples hold `fill`."""
    R, SR, S = scene["R"], scene["SR"], scene["S"]
    sr = scene["samp_ray"][:S].long()
    slot = torch.arange(S) - scene["ray_soff"].long()[sr]
    out = torch.full((R, SR) + tuple(t.shape[1:]), fill, dtype=t.dtype)
    return out.index_put((sr, slot), t[:S])


def ray_dist_fp32(scene, unit):
    """(dist [R, SR] fp32, valid [R, SR] bool, raw [R, SR] fp32) as the kernels decide them: the depth
    ((x - c0) r2 + (y - c1) r5) + (z - c2) r8 with every operation rounded to fp32 (pers_z's __f*_rn; the padding
    slots sit at the world origin), the running max, one subtraction (raw; the last slot's is vz), the two mask
    tests replacing the interval by vz, and the validity factor."""
    c, r = scene["campos"], scene["rot"].reshape(-1)
    p = densify(scene, scene["samp_locw"])
    z = ((p[..., 0] - c[0]) * r[2] + (p[..., 1] - c[1]) * r[5]) + (p[..., 2] - c[2]) * r[8]
    assert z.dtype == F32
    cm = torch.cummax(z, dim=-1)[0]
    vz = torch.tensor(VZ, dtype=F32)
    raw = torch.cat([cm[:, 1:] - cm[:, :-1], vz.expand(z.shape[0], 1)], dim=-1)
    mask = raw < torch.tensor(1e-8, dtype=F32)
    if unit:
        mask = mask | (raw > torch.tensor(2.0, dtype=F32) * vz)
    valid = densify(scene, scene["samp_nnb"] > 0, False)
    dist = torch.where(mask, vz, raw) * valid.to(F32)
    return dist, valid, raw


def march_ref(dist, valid, feat, bg=None):
    """ray_march in float64, slot by slot, differentiable in feat [R, SR, 4] (float64): o = 1 - exp(-sigma dist),
    T the exclusive product of (1 - o + 1e-10f), blend weight o T, rgb = sum c o T (+ bg T_end).  Returns a dict
    of o, T, w [R, SR], rgb [R, 3], bgT [R]."""
    dd, v = dist.double(), valid.double()
    o = 1.0 - torch.exp(-(feat[..., 0] * v) * dd)
    av = 1.0 - o + EPS_T
    Ts = [torch.ones(dd.shape[0], dtype=torch.float64)]
    for s in range(dd.shape[1]):
        Ts.append(Ts[-1] * av[:, s])
    T = torch.stack(Ts[:-1], dim=1)
    w = o * T
    rgb = (feat[..., 1:4] * w[..., None]).sum(dim=1)
    if bg is not None:
        rgb = rgb + bg.double() * Ts[-1][:, None]
    return dict(o=o, T=T, w=w, rgb=rgb, bgT=Ts[-1], av=av)


def fill_invalid(rgb, bgT, valid, bg):
    """Rays without a valid sample: the background colour, mask 0, background transmission 1."""
    mask = valid.any(dim=-1)
    return torch.where(mask[:, None], rgb, bg.double().expand_as(rgb)), mask, torch.where(mask, bgT, torch.ones_like(bgT))


def zero_one_branch(conf, eps=ZO_EPS):
    """Per conf value, decided in fp32 as zero_one() of csrc/loss.hip decides it: (inside, const) -- inside:
    the straight-through clamp's value cc = cd - (cd - clamp(cd, 1e-4, 1)) lies in [eps, 1 - eps], where the
    term's value is cd itself (cc = cd exactly there) and its derivative passes; const: the clamped value
    (eps or 1 - eps, float64 of the fp32 constants) elsewhere."""
    cd = conf.to(F32)
    e32 = torch.tensor(eps, dtype=F32)
    hi = torch.tensor(1.0, dtype=F32) - e32
    cc = cd - (cd - torch.clamp(cd, torch.tensor(1e-4, dtype=F32), torch.tensor(1.0, dtype=F32)))
    inside = (cc >= e32) & (cc <= hi)
    assert bool((cc[inside] == cd[inside]).all())
    return inside, torch.where(cc < e32, e32, hi).double()


def zero_one_terms(conf64, conf32, eps=ZO_EPS):
    """log(val) + log(1 - val) per point, float64, differentiable in conf64 inside the clamps."""
    inside, const = zero_one_branch(conf32, eps)
    val = torch.where(inside, conf64, const)
    return torch.log(val) + torch.log(1.0 - val)


def loss_ref(full, mask, gt, conf64, conf32, pd, eps=ZO_EPS):
    """The four losses as include/sgn_hip.h defines them, float64: the colour MSE over the valid rays,
    the zero-one mean over every (slot, k) of the valid rays (pd [R, SR, K]; empty entries, -1, read
    conf[0]), the missed rays' squared error / 3, the MSE over every ray.  Returns (losses [4], n)."""
    R, SR, K = pd.shape
    m = mask.double()
    n = int(mask.sum())
    se = ((full - gt.double()) ** 2).sum(dim=-1)
    terms = zero_one_terms(conf64, conf32, eps)
    zo = (terms[pd.clamp(min=0).long()] * m[:, None, None]).sum()
    return torch.stack([(se * m).sum() / max(3 * n, 1), zo / max(n * SR * K, 1), (se * (1 - m)).sum() / 3,
                        se.sum() / (3 * R)]), n


def reference(scene, unit, use_bg_ray, bg=(1.0, 1.0, 1.0), zero_one_weight=1e-4, eps=ZO_EPS):
    """The whole loss stage on a scene: ray_dist_fp32 + march_ref + fill_invalid + loss_ref, and by float64
    autograd d feat [S_cap, 4] = d losses[0] / d feat (zero on the slack samples) and d conf [N] =
    zero_one_weight x d losses[1] / d conf, which is what sgn_loss_train writes."""
    dist, valid, raw = ray_dist_fp32(scene, unit)
    feat = scene["feat"].double().requires_grad_(True)
    conf = scene["conf"].double().requires_grad_(True)
    bgv = scene["bg_ray"] if use_bg_ray else torch.tensor(bg, dtype=F32).expand(scene["R"], 3)
    m = march_ref(dist, valid, densify(scene, feat), bgv)
    full, mask, bgT = fill_invalid(m["rgb"], m["bgT"], valid, bgv)
    pd = densify(scene, scene["pidx"], -1)
    losses, n = loss_ref(full, mask, scene["gt"], conf, scene["conf"], pd, eps)
    dfeat = torch.autograd.grad(losses[0], feat, retain_graph=True, allow_unused=True)[0]
    dconf = torch.autograd.grad(zero_one_weight * losses[1], conf, allow_unused=True)[0]
    dfeat = torch.zeros_like(feat) if dfeat is None else dfeat
    dconf = torch.zeros_like(conf) if dconf is None else dconf
    det = {k: v.detach() for k, v in m.items()}
    return dict(det, dist=dist, valid=valid, raw=raw, bg=bgv, full=full.detach(), mask=mask, bgT_filled=bgT.detach(),
                pd=pd, losses=losses.detach(), n=n, dfeat=dfeat.detach(), dconf=dconf.detach())
