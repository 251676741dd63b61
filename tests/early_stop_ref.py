"""numpy float32 restatement of early ray termination (sgn_early_stop_tier, include/sgn_hip.h; the tier
loop of HipRenderer.render).

Two levels:
  * `decide` -- the tier decision from per-slot opacities: the transmittance T_b = prod_{s<b} (1 - o_s + 1e-10)
    in fp32, slot by slot as the composite multiplies it, the first boundary b with T_b <= eps is the ray's
    stop slot, every valid sample at or after it is skipped.
  * `tier` -- one call of the entry on a raw query (ray_ns, ray_soff, samp_nnb, samp_locw) and the feat
    buffer: T over the closed slots [0, lo) with the composite's arithmetic (pers z, running cummax, the
    distance replacement, o = 1 - exp(-sigma dist)), operation for operation in fp32, then the ids emitted,
    the ids zeroed, stop_slot and the counters.

The bound (early ray termination): a ray stopped at boundary a with T_a <= eps loses the weights
w_s = o_s T_s, s >= a, which sum to T_a - T_end + 1e-10 sum T_s; with colours in [-0.001, 1.001] and bg in
[0, 1] a channel moves by at most 1.001 eps, and bg_transmission rises by at most eps."""
import numpy as np

F = np.float32


def boundaries(slots, SR):
    """[0, b0, b1, ..., SR]: the boundaries of `slots` below SR between the frame's ends."""
    return [0] + [int(b) for b in slots if b < SR] + [int(SR)]


def transmittance(opacity):
    """T [R, SR + 1] fp32: T[:, b] = the transmittance a ray reaches slot b with (T[:, 0] = 1)."""
    o = np.asarray(opacity, F)
    R, SR = o.shape
    T = np.ones((R, SR + 1), F)
    for s in range(SR):
        T[:, s + 1] = T[:, s] * ((F(1.0) - o[:, s]) + F(1e-10))
    return T


def decide(opacity, valid, eps, slots):
    """(stop_slot [R] int32 (SR: never stopped), skipped [R, SR] bool) of rays with these per-slot opacities
    and valid flags, threshold eps and slot boundaries `slots`."""
    o = np.asarray(opacity, F)
    R, SR = o.shape
    T = transmittance(o)
    stop = np.full(R, SR, np.int32)
    for b in boundaries(slots, SR)[1:-1]:
        hit = (T[:, b] <= F(eps)) & (stop == SR)
        stop[hit] = b
    skipped = np.asarray(valid, bool) & (np.arange(SR)[None, :] >= stop[:, None])
    return stop, skipped


def pers_z(campos, rot, p):
    """Camera-space z of a world position, the composite's fp32 operation order."""
    c, r, p = np.asarray(campos, F), np.asarray(rot, F).reshape(9), np.asarray(p, F)
    sx, sy, sz = p[0] - c[0], p[1] - c[1], p[2] - c[2]
    return (sx * r[2] + sy * r[5]) + sz * r[8]


def ray_T(campos, rot, ns, off, samp_nnb, samp_locw, feat, SR, unit, vz, lo):
    """fp32 transmittance of one ray over its closed slots [0, lo) (lo < SR)."""
    vz = F(vz)
    ns = min(int(ns), SR)
    z0 = pers_z(campos, rot, np.zeros(3, F))
    locw = np.asarray(samp_locw, F).reshape(-1, 3)

    def z_at(s):
        return pers_z(campos, rot, locw[off + s]) if s < ns else z0
    T = F(1.0)
    if min(lo, ns) == 0:
        return T
    prev_cm = z_at(0)
    for s in range(min(lo, ns)):
        cm = np.maximum(prev_cm, z_at(s + 1))
        dist = F(cm - prev_cm)
        v = samp_nnb[off + s] > 0
        if dist < F(1e-8) or (unit and dist > F(2.0) * vz):
            dist = vz
        valid = F(1.0) if v else F(0.0)
        dist = F(dist * valid)
        sigma = F((F(feat[off + s, 0]) if v else F(0.0)) * valid)
        o = F(F(1.0) - np.exp(F(-sigma * dist), dtype=F))
        T = F(T * F(F(F(1.0) - o) + F(1e-10)))
        prev_cm = cm
    return T


def tier(campos, rot, ray_ns, ray_soff, samp_nnb, samp_locw, feat, SR, unit, vz, lo, hi, eps, stop_slot):
    """One sgn_early_stop_tier call.  Returns (emitted ids (sorted), zeroed ids (sorted), stop_slot after the
    call, T [R] fp32).  `feat` [S, 4] and `stop_slot` [R] are not modified."""
    R = len(ray_ns)
    stop = np.array(stop_slot, np.int32)
    emit, zero = [], []
    Ts = np.ones(R, F)
    for r in range(R):
        ns, off = min(int(ray_ns[r]), SR), int(ray_soff[r])
        T = Ts[r] = ray_T(campos, rot, ns, off, samp_nnb, samp_locw, feat, SR, unit, vz, lo)
        fin = bool(T <= F(eps))
        if fin and stop[r] == SR:
            stop[r] = lo
        ids = [off + s for s in range(lo, min(hi, ns)) if samp_nnb[off + s] > 0]
        (zero if fin else emit).extend(ids)
    return np.array(sorted(emit), np.int64), np.array(sorted(zero), np.int64), stop, Ts
