"""Float64 reference of the hole-probing kernel (csrc/probe.hip: k_probe behind sgn_probe) and the seeded
scene, with hand-placed rays, that the CPU and GPU tests of it share.

The formulas are those of include/sgn_hip.h (sgn_probe).  tests/test_probe_ref_cpu.py pins probe_ref to a
literal restatement of the reference's own lines (models/neural_points_volumetric_model.py:636-657) on dense
[1, R, SR, K, C] tensors, so a GPU test that disagrees with this module names the kernel.

The selected slot is decided on the fp32 opacities exactly as the kernel decides it (the first slot holding
the row maximum: a strict > scanning upwards); the float64 arithmetic on the same fp32 inputs starts after
that choice, so reference and kernel never select different samples."""
import functools

import torch

from ray_stage_ref import N_NAMED, N_POINTS, densify, ray_scene

F32 = torch.float32
REC = 48                      # floats per record (SGN_PROBE_RECORD)
# name -> (first float, channels) of the record; the words in between (3, 7, 11, 15) are zero padding
FIELDS = {"opacity": (0, 1), "far_dist": (1, 1), "avg_conf": (2, 1), "loc_w": (4, 3), "avg_color": (8, 3),
          "avg_dir": (12, 3), "avg_embedding": (16, 32)}
PADS = (3, 7, 11, 15)
P_NEAR, P_FAR = 250, 251      # points no ray_scene ray names (>= N_NAMED, past the planted conf values)

# (planting, smallest ns of the ray it takes, smallest K), in the order in which rays are given out
PLANTINGS = [("tie", 3, 1), ("all_zero", 1, 1), ("max_slot0", 2, 1), ("max_last", 2, 1), ("ones_run", 3, 1),
             ("pt0_near", 1, 2), ("pt0_far", 1, 2), ("nnb0", 2, 1)]
# plantings that reuse a ray of ray_scene's: (name, ray_scene's planting)
BORROWED = [("max_sr_minus_1", "full"), ("mask0_ns", "no_nb"), ("mask0_ns0", "ns0")]


@functools.lru_cache(maxsize=None)
def probe_scene(R, SR, K, seed=0):
    """ray_scene(R, SR, K, seed) (its tensors are copied, never edited) plus what sgn_probe reads: fp32
    embedding / color / dir tables for its 257 points (and its xyz / conf), blend [S_cap, K] (zero on empty
    slots), opacity [R, SR] (positive only on samples with a neighbour; zero on rays outside the mask) and
    mask [R] int8 (the ray has a sample with a neighbour).

    One ray each, where R, SR and K allow (scene['plant'] maps the name to the ray, scene['expect_j'] to the
    slot it must select, scene['skipped'] lists the rest):
      tie            the maximum twice, at slots a and a + 2: the first wins
      all_zero       a valid ray whose opacities are all 0: slot 0
      max_slot0, max_last, max_sr_minus_1   the maximum at slot 0, at slot ns - 1, at slot SR - 1 of a full ray
      ones_run       opacity exactly 1.0 on slots 1 .. : slot 1
      pt0_near       the selected sample has one neighbour (nnb = 1 < K), farther away than point 0: the
                     empty slots' point 0 wins the min
      pt0_far        the same with the neighbour 1e-3 away: it wins
      nnb0           the selected sample (slot 0, all opacities 0) has no neighbour: every slot reads point 0
      mask0_ns       a ray outside the mask that has samples (none with a neighbour)
      mask0_ns0      a ray outside the mask without samples"""
    sc = ray_scene(R, SR, K, seed)
    g = torch.Generator().manual_seed(seed * 104729 + R * 313 + SR * 29 + K)
    rnd = lambda *shape: torch.rand(*shape, generator=g, dtype=torch.float64)  # noqa: E731
    N, S, S_cap = N_POINTS, sc["S"], sc["S_cap"]
    ns, soff = sc["ray_ns"].long(), sc["ray_soff"].long()
    nnb, pidx = sc["samp_nnb"].clone(), sc["pidx"].clone()
    xyz, locw = sc["xyz"].clone(), sc["samp_locw"]
    # ray_scene plants conf one fp32 step either side of 0: subnormals, whose products with a blend weight
    # underflow in fp32, where no bound relative to |w x| can hold.  They become +-2^-60 here (still far
    # below every clamp): avg_conf's bound is about rounding, not about underflow.
    conf = sc["conf"].clone()
    tiny = (conf != 0) & (conf.abs() < 2.0 ** -126)
    conf[tiny] = torch.sign(conf[tiny]) * 2.0 ** -60
    plant, skipped, expect_j = {}, [], {}
    for name, theirs in BORROWED:
        if theirs in sc["plant"]:
            plant[name] = sc["plant"][theirs]
        else:
            skipped.append(name)
    # ---- rays of our own: the first unplanted rays long enough, every sample given a neighbour
    free = list(range(len(sc["plant"]), R))
    for name, min_ns, min_k in PLANTINGS:
        r = next((r for r in free if int(ns[r]) >= min_ns), None) if K >= min_k else None
        if r is None:
            skipped.append(name)
            continue
        free.remove(r)
        plant[name] = r
        for s in range(int(soff[r]), int(soff[r] + ns[r])):
            if nnb[s] == 0:
                nnb[s] = 1
                pidx[s, 0] = s % N_NAMED
    sel = {}   # the slot a planting's maximum goes to
    for name, point, offset in (("pt0_near", P_NEAR, 4.0), ("pt0_far", P_FAR, 1e-3)):
        if name in plant:
            r = plant[name]
            sel[name] = min(1, int(ns[r]) - 1)
            s = int(soff[r]) + sel[name]
            nnb[s] = 1
            pidx[s] = -1
            pidx[s, 0] = point
            xyz[point] = locw[s] + torch.tensor([offset, 0.0, 0.0], dtype=F32)
    if "nnb0" in plant:
        s = int(soff[plant["nnb0"]])
        nnb[s] = 0
        pidx[s] = -1
    assert bool(((pidx >= 0) == (torch.arange(K)[None, :] < nnb[:, None])).all())   # valid neighbours: a prefix
    # ---- tables, blend, opacity
    emb = (rnd(N, 32) * 2 - 1).to(F32)
    color = rnd(N, 3).to(F32)
    pdir = (rnd(N, 3) * 2 - 1).to(F32)
    have = pidx >= 0
    w = torch.where(have, 0.05 + rnd(S_cap, K), torch.zeros(S_cap, K, dtype=torch.float64))
    w = w / w.sum(-1, keepdim=True).clamp(min=1e-8)
    blend = (w * conf[pidx.clamp(min=0).long()].double().clamp(1e-4, 1.0)).to(F32)
    blend = torch.where(have, blend, torch.zeros_like(blend))
    samp_ray = sc["samp_ray"][:S].long()
    valid_ray = torch.zeros(R, dtype=torch.bool)
    valid_ray[samp_ray[nnb[:S] > 0]] = True
    o_s = torch.where(nnb[:S] > 0, 0.01 + 0.89 * rnd(S), torch.zeros(S, dtype=torch.float64)).to(F32)
    slot = torch.arange(S) - soff[samp_ray]
    opacity = torch.zeros(R, SR, dtype=F32).index_put((samp_ray, slot), o_s)
    opacity[~valid_ray] = 0.0
    top = torch.tensor(0.95, dtype=F32)
    for name, r in plant.items():
        n = int(ns[r])
        if name == "tie":
            a = min(1, n - 3)
            opacity[r, a] = opacity[r, a + 2] = 0.9375
            expect_j[name] = a
        elif name in ("all_zero", "nnb0"):
            opacity[r] = 0.0
            expect_j[name] = 0
        elif name == "max_slot0":
            opacity[r, 0] = top
            expect_j[name] = 0
        elif name == "max_last":
            opacity[r, n - 1] = top
            expect_j[name] = n - 1
        elif name == "max_sr_minus_1":
            assert n == SR
            opacity[r, SR - 1] = top
            expect_j[name] = SR - 1
        elif name == "ones_run":
            opacity[r, 1:min(n, 4)] = 1.0
            expect_j[name] = 1
        elif name in sel:
            opacity[r, sel[name]] = top
            expect_j[name] = sel[name]
    mask = valid_ray.to(torch.int8)
    # what the plantings claim
    for name in ("mask0_ns", "mask0_ns0"):
        if name in plant:
            assert mask[plant[name]] == 0 and (int(ns[plant[name]]) > 0) == (name == "mask0_ns")
    for name in expect_j:
        assert mask[plant[name]] == 1
    for name, nearer in (("pt0_near", True), ("pt0_far", False)):
        if name in plant:
            s = int(soff[plant[name]]) + sel[name]
            d0 = float((xyz[0].double() - locw[s].double()).norm())
            dn = float((xyz[int(pidx[s, 0])].double() - locw[s].double()).norm())
            assert (d0 < 0.9 * dn) if nearer else (dn < 0.1 * d0)
    return dict(R=R, SR=SR, K=K, S=S, S_cap=S_cap, plant=plant, skipped=skipped, expect_j=expect_j,
                ray_ns=sc["ray_ns"], ray_soff=sc["ray_soff"], samp_ray=sc["samp_ray"], samp_locw=locw,
                samp_nnb=nnb.contiguous(), pidx=pidx.contiguous(), xyz=xyz.contiguous(), conf=conf,
                embedding=emb, color=color, dir=pdir, blend=blend.contiguous(), opacity=opacity.contiguous(),
                mask=mask)


def select_slot(opacity):
    """[R] the first slot holding each row's maximum, as k_probe decides it on the fp32 values: slot 0,
    replaced by a later slot only when that one is strictly larger."""
    best, j = opacity[:, 0].clone(), torch.zeros(opacity.shape[0], dtype=torch.long)
    for s in range(1, opacity.shape[1]):
        up = opacity[:, s] > best
        best = torch.where(up, opacity[:, s], best)
        j = torch.where(up, torch.full_like(j, s), j)
    return j


def probe_ref(scene):
    """dict: j [R] (selected slot; 0 on rays outside the mask), rec [R, 48] float64 (the record
    include/sgn_hip.h defines: zero on rays outside the mask), sumabs [R, 48] float64 (sum over k of
    |w_k x_k| under each avg_* entry, zero elsewhere: what the kernel's fp32 rounding is measured against)."""
    R, K = scene["R"], scene["K"]
    m = scene["mask"] != 0
    j = torch.where(m, select_slot(scene["opacity"]), torch.zeros(R, dtype=torch.long))
    assert bool((j[m] < scene["ray_ns"].long()[m]).all())
    s = torch.where(m, scene["ray_soff"].long() + j, torch.zeros(R, dtype=torch.long))
    loc = scene["samp_locw"][s].double()
    p = scene["pidx"][s].clamp(min=0).long()          # [R, K]: empty slots read point 0
    w = scene["blend"][s].double()
    rec = torch.zeros(R, REC, dtype=torch.float64)
    sumabs = torch.zeros(R, REC, dtype=torch.float64)
    rec[:, 0] = scene["opacity"][torch.arange(R), j].double()
    rec[:, 1] = (scene["xyz"][p].double() - loc[:, None, :]).pow(2).sum(-1).sqrt().min(dim=-1)[0]
    rec[:, 4:7] = loc
    for name, tab in (("avg_conf", scene["conf"].reshape(-1, 1)), ("avg_color", scene["color"]), ("avg_dir", scene["dir"]),
                      ("avg_embedding", scene["embedding"])):
        o, c = FIELDS[name]
        terms = w[:, :, None] * tab[p].double()       # [R, K, C]
        rec[:, o:o + c] = terms.sum(1)
        sumabs[:, o:o + c] = terms.abs().sum(1)
    rec[~m] = 0.0
    sumabs[~m] = 0.0
    return dict(j=j, rec=rec, sumabs=sumabs)


def dense_inputs(scene):
    """The reference's dense tensors of the scene, float64 except the fp32 opacity: coarse_point_opacity
    [1, R, SR], sample_loc_w [1, R, SR, 3], weight * conf_coefficient [1, R, SR, K] and the gathered
    sampled_xyz / color / dir / conf / embedding [1, R, SR, K, C] (empty slots: point 0, neural_points.py:958-959)."""
    pd = densify(scene, scene["pidx"], -1).clamp(min=0).long()
    gather = lambda t: t.reshape(N_POINTS, -1)[pd].double()[None]  # noqa: E731
    return dict(opacity=scene["opacity"][None], sample_loc_w=densify(scene, scene["samp_locw"]).double()[None],
                weight_conf=densify(scene, scene["blend"]).double()[None], sampled_xyz=gather(scene["xyz"]),
                sampled_color=gather(scene["color"]), sampled_dir=gather(scene["dir"]),
                sampled_conf=gather(scene["conf"]), sampled_embedding=gather(scene["embedding"]))


def reference_lines_636_657(opacity, sample_loc_w, weight, sampled_xyz, sampled_color, sampled_dir, sampled_conf,
                            sampled_embedding):
    """models/neural_points_volumetric_model.py:636-657 restated line for line (`weight` is the reference's
    weight * conf_coefficient): dict of the eight outputs and opacity_ind [1, R]."""
    out = {}
    out["ray_max_shading_opacity"], opacity_ind = torch.max(opacity, dim=-1, keepdim=True)
    ind0 = opacity_ind[..., 0]
    opacity_ind = opacity_ind[..., None]
    out["ray_max_sample_loc_w"] = torch.gather(sample_loc_w, 2, opacity_ind.expand(-1, -1, -1, sample_loc_w.shape[-1])).squeeze(2)
    weight = torch.gather(weight, 2, opacity_ind.expand(-1, -1, -1, weight.shape[-1])).squeeze(2)[..., None]
    opacity_ind = opacity_ind[..., None]
    g5 = lambda t: torch.gather(t, 2, opacity_ind.expand(-1, -1, -1, t.shape[-2], t.shape[-1])).squeeze(2)  # noqa: E731
    xyz_max = g5(sampled_xyz)
    out["ray_max_far_dist"] = torch.min(torch.norm(xyz_max - out["ray_max_sample_loc_w"][..., None, :], dim=-1), axis=-1,
                                        keepdim=True)[0]
    out["shading_avg_color"] = torch.sum(g5(sampled_color) * weight, dim=-2)
    out["shading_avg_dir"] = torch.sum(g5(sampled_dir) * weight, dim=-2)
    out["shading_avg_conf"] = torch.sum(g5(sampled_conf) * weight, dim=-2)
    out["ray_max_sample_label"] = torch.zeros_like(out["shading_avg_conf"])
    out["shading_avg_embedding"] = torch.sum(g5(sampled_embedding) * weight, dim=-2)
    return out, ind0


# the eight output keys -> the record field each one is
KEY_FIELD = {"ray_max_shading_opacity": "opacity", "ray_max_sample_loc_w": "loc_w", "ray_max_far_dist": "far_dist",
             "shading_avg_color": "avg_color", "shading_avg_dir": "avg_dir", "shading_avg_conf": "avg_conf",
             "shading_avg_embedding": "avg_embedding"}


def check_records(got, ref, mask, what=""):
    """A kernel's records got [R, 48] (fp32) against probe_ref's: the copies (opacity, loc_w) bit for bit,
    every pad word and every word of a ray outside the mask +0.0,
      avg_*    |got - ref64| <= 2^-20 sum_k |w_k x_k|   (K + 1 <= 9 roundings of 2^-24 in a K-term fp32 sum of
               products, rounded up to 16)
      far_dist |got - ref64| <= 2^-20 ref64              (four roundings on the squared sum, halved by the root,
               plus the root's own)
    Prints the worst ratio to each bound before it asserts."""
    rec, sumabs = ref["rec"], ref["sumabs"]
    bits = lambda t: t.contiguous().view(torch.int32)  # noqa: E731
    for name in ("opacity", "loc_w"):
        o, c = FIELDS[name]
        assert torch.equal(bits(got[:, o:o + c]), bits(rec[:, o:o + c].to(F32))), f"{what}{name}: not a copy"
    assert int(bits(got[:, list(PADS)]).abs().max()) == 0, f"{what}pad words"
    out = mask == 0
    if bool(out.any()):
        assert int(bits(got[out]).abs().max()) == 0, f"{what}rays outside the mask"
    err = (got.double() - rec).abs()
    cols = [i for name in ("avg_conf", "avg_color", "avg_dir", "avg_embedding") for i in range(FIELDS[name][0], sum(FIELDS[name]))]
    far_bound, avg_bound = 2.0 ** -20 * rec[:, 1], 2.0 ** -20 * sumabs[:, cols]
    far_ratio = float((err[:, 1] / far_bound.clamp(min=1e-300)).max())
    avg_ratio = float((err[:, cols] / avg_bound.clamp(min=1e-300)).max())
    print(f"{what}far_dist error / bound {far_ratio:.3f}, avg error / bound {avg_ratio:.3f}")
    assert bool((err[:, 1] <= far_bound).all()), f"{what}far_dist: {far_ratio:.3e} x the bound"
    assert bool((err[:, cols] <= avg_bound).all()), f"{what}avg: {avg_ratio:.3e} x the bound"
