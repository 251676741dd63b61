"""tests/ray_stage_ref.py computes the function the project ships: its float64 march / losses / gradients agree
with train.composite_losses (the fp32 restatement that is pinned to oracle/agg_ref.py) and with
agg_ref.composite on the dense scatter, its scenes hold every planting they promise, and its autograd
gradients pass a float64 finite-difference check.  No GPU."""
import functools

import pytest
import torch

import agg_ref
import ray_stage_ref as rs
from sgnerf_amd.opts import HotPathOpts
from sgnerf_amd.train import PointParams, composite_losses

SCENES = [(37, 24, 8), (20, 33, 3), (9, 64, 16)]
BAR = 1e-5


@functools.lru_cache(maxsize=None)
def scene(R, SR, K, camera):
    return rs.ray_scene(R, SR, K, seed=3, camera=camera)


def _rel_max(a, b):
    """max |a - b| / max |b|: per element, relative to the tensor's largest entry."""
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp(min=1e-300))


@pytest.mark.parametrize("R,SR,K", SCENES)
@pytest.mark.parametrize("unit,bgr,camera", [(0, False, 0), (1, True, 1), (1, False, 0), (0, True, 1)])
def test_reference_agrees_with_composite_losses(R, SR, K, unit, bgr, camera):
    sc = scene(R, SR, K, camera)
    print("skipped plantings:", sc["skipped"])
    S = sc["S"]
    ref = rs.reference(sc, unit, bgr, zero_one_weight=1.0)
    N = rs.N_POINTS
    points = PointParams(sc["xyz"], torch.zeros(N, 32), torch.zeros(N, 3), torch.zeros(N, 3), sc["conf"], "cpu")
    q = {"ray_ns": sc["ray_ns"], "ray_soff": sc["ray_soff"], "samp_ray": sc["samp_ray"][:S], "samp_locw": sc["samp_locw"][:S],
         "pidx": sc["pidx"][:S]}
    feat = sc["feat"][:S].clone().requires_grad_(True)
    opts = HotPathOpts(SR=SR, K=K, raydist_mode_unit=unit)
    assert float(opts.vsize[2]) == rs.VZ
    tot, parts, full, mask = composite_losses(points, q, feat, sc["samp_nnb"][:S] > 0, sc["campos"], sc["rot"],
                                              torch.zeros(R, 3), sc["gt"], opts, bg=sc["bg_ray"] if bgr else (1.0, 1.0, 1.0),
                                              zero_one_weight=1.0, zero_eps=rs.ZO_EPS)
    tot.backward()
    assert torch.equal(mask, ref["mask"])
    assert 0 < ref["n"] < R or R < 3
    assert float((full.detach().double() - ref["full"]).abs().max()) <= BAR
    for i, k in enumerate(("ray_masked_coarse_raycolor", "conf_coefficient", "ray_miss_coarse_raycolor", "coarse_raycolor")):
        a, b = float(parts[k]), float(ref["losses"][i])
        assert abs(a - b) <= BAR * max(abs(b), 1e-12), (k, a, b)
    e_feat, e_conf = _rel_max(feat.grad, ref["dfeat"][:S]), _rel_max(points.points_conf.grad.reshape(-1), ref["dconf"])
    print(f"d feat {e_feat:.2e}, d conf {e_conf:.2e} of the tensor's max")
    assert e_feat <= BAR and e_conf <= BAR
    assert bool((ref["dfeat"][S:] == 0).all())


@pytest.mark.parametrize("R,SR,K", SCENES)
@pytest.mark.parametrize("unit,camera", [(0, 0), (1, 1)])
def test_dense_march_agrees_with_agg_ref(R, SR, K, unit, camera):
    sc = scene(R, SR, K, camera)
    dist, valid, _ = rs.ray_dist_fp32(sc, unit)
    fd = rs.densify(sc, sc["feat"])
    bg = torch.tensor([0.2, 0.5, 1.0])
    m = rs.march_ref(dist, valid, fd.double(), bg.expand(R, 3))
    color, opacity, bg_t = agg_ref.composite(fd, valid, rs.densify(sc, sc["samp_locw"]), sc["rot"], sc["campos"],
                                             vsize_z=rs.VZ, raydist_mode_unit=unit, bg=tuple(bg.tolist()))
    assert float((color.double() - m["rgb"]).abs().max()) <= BAR
    assert float((opacity.double() - m["o"]).abs().max()) <= BAR
    assert float((bg_t.double() - m["bgT"]).abs().max()) <= BAR


@pytest.mark.parametrize("camera", [0, 1])
def test_every_promised_planting_is_there(camera):
    """(37, 24, 8) and (20, 33, 3) promise every planting but ns32 / ns33 (SR < 64), (65, 64, 16) all of them."""
    for R, SR, K, absent in [(37, 24, 8, {"ns32", "ns33"}), (65, 64, 16, set()), (20, 33, 3, {"ns32", "ns33"})]:
        sc = scene(R, SR, K, camera)
        assert set(sc["skipped"]) == absent, sc["skipped"]
        P, ns, off, nnb, feat = sc["plant"], sc["ray_ns"], sc["ray_soff"], sc["samp_nnb"], sc["feat"]
        assert sc["S"] < sc["S_cap"] and int(ns.sum()) == sc["S"] and int(sc["samp_ray"][:sc["S"]].max()) < R
        seg = lambda name: slice(int(off[P[name]]), int(off[P[name]]) + int(ns[P[name]]))  # noqa: E731
        assert int(ns[P["ns0"]]) == 0 and int(ns[P["ns1"]]) == 1 and int(ns[P["ns_sr_minus_1"]]) == SR - 1
        assert int(ns[P["full"]]) == SR and bool((nnb[seg("full")] > 0).all())
        assert int(ns[P["no_nb"]]) > 0 and bool((nnb[seg("no_nb")] == 0).all())
        for unit in (0, 1):
            dist, valid, raw = rs.ray_dist_fp32(sc, unit)
            assert float(dist[P["full"], SR - 1]) == float(torch.tensor(rs.VZ, dtype=torch.float32))
            # invalid first / middle / last sample, each moving the cummax: the raw interval into it is > 0
            r, n = P["invalid_fml"], int(ns[P["invalid_fml"]])
            bad = [0, n // 2, n - 1]
            assert [bool(valid[r, s]) for s in range(n)] == [s not in bad for s in range(n)]
            assert all(float(raw[r, s - 1]) > 1e-5 for s in bad[1:]) and float(raw[r, 0]) > 1e-5
            assert float(raw[P["same_pos"], 1]) == 0.0 and torch.equal(sc["samp_locw"][seg("same_pos")][1], sc["samp_locw"][seg("same_pos")][2])
            assert float(raw[P["behind"], 1]) == 0.0 and float(dist[P["behind"], 1]) == float(torch.tensor(rs.VZ, dtype=torch.float32))
            a, b = float(raw[P["steps"], 0]), float(raw[P["steps"], 1])
            assert abs(a / rs.VZ - 1.5) < 0.01 and abs(b / rs.VZ - 3.0) < 0.01
            assert abs(float(dist[P["steps"], 1]) / rs.VZ - (1.0 if unit else 3.0)) < 0.01
            x = feat[seg("alpha_spread"), 0].double() * dist[P["alpha_spread"], :int(ns[P["alpha_spread"]])].double()
            assert float(x.min()) < 1e-4 and float(x.max()) > 100 and len(set(torch.floor(torch.log10(x)).tolist())) >= 6
            xo = feat[seg("opaque_run"), 0].double() * dist[P["opaque_run"], :int(ns[P["opaque_run"]])].double()
            assert bool((xo[1:7] > 110).all())
            T = rs.march_ref(dist, valid, rs.densify(sc, sc["feat"]).double())["T"][P["opaque_run"]]
            T32 = T.to(torch.float32)
            assert bool(((T32 > 0) & (T32 < 2.0 ** -126)).any()) and float(T32[7]) == 0.0   # through the denormals to 0
        assert float(feat[seg("alpha0")][1, 0]) == 0.0 and int(nnb[seg("alpha0")][1]) > 0
        if SR >= 64:
            assert int(ns[P["ns32"]]) == 32 and int(ns[P["ns33"]]) == 33
        # the world origin's depth against the rays' last samples
        c, r9 = sc["campos"], sc["rot"].reshape(-1)
        z0 = float(-c[0] * r9[2] - c[1] * r9[5] - c[2] * r9[8])
        _, _, raw = rs.ray_dist_fp32(sc, 0)
        lastraw = torch.stack([raw[r, int(ns[r]) - 1] for r in range(R) if 0 < int(ns[r]) < SR])
        if camera == 0:
            assert z0 < 0.29 and bool((lastraw == 0).all())
        else:
            assert bool((lastraw > 0).any()) and bool((lastraw == 0).any())
        # conf: every planted value present and named by a valid entry of a valid ray; point 0 inside the clamps
        cp = rs.conf_plantings()
        assert torch.equal(sc["conf"][1:22], cp) and len(set(cp.tolist())) == 21
        ref = rs.reference(sc, 0, False)
        pd = ref["pd"][ref["mask"]]
        assert set(range(1, 22)) <= set(pd[pd >= 0].tolist())
        inside, _ = rs.zero_one_branch(sc["conf"])
        assert bool(inside[0]) and rs.ZO_EPS < float(sc["conf"][0]) < 1 - rs.ZO_EPS
        assert int(inside[1:22].sum()) == 4        # eps and 1 - eps, and the step inside of each
        named = torch.zeros(rs.N_POINTS, dtype=torch.bool)
        named[pd[pd >= 0].long()] = True
        assert int((~named).sum()) >= 30           # points no valid ray names


def test_point0_at_clamp_scene():
    sc = rs.ray_scene(37, 24, 8, seed=3, conf0=0.0)
    inside, const = rs.zero_one_branch(sc["conf"])
    assert not bool(inside[0]) and float(rs.reference(sc, 0, False)["dconf"][0]) == 0.0


def test_autograd_gradients_pass_finite_differences():
    """Central differences in float64 (relative step 1e-6) at a dozen entries, six of feat (of losses[0]) and six
    of conf (of w losses[1]), drawn among those large enough for the quotient's own rounding: agreement 1e-6."""
    sc = scene(37, 24, 8, 1)
    w = 1.0
    dist, valid, _ = rs.ray_dist_fp32(sc, 1)
    pd = rs.densify(sc, sc["pidx"], -1)

    def total(feat, conf, which):
        m = rs.march_ref(dist, valid, rs.densify(sc, feat), sc["bg_ray"])
        full, mask, _ = rs.fill_invalid(m["rgb"], m["bgT"], valid, sc["bg_ray"])
        losses, _ = rs.loss_ref(full, mask, sc["gt"], conf, sc["conf"], pd)
        return losses[0] if which == "feat" else w * losses[1]

    ref = rs.reference(sc, 1, True, zero_one_weight=w)
    feat0, conf0 = sc["feat"].double(), sc["conf"].double()
    g = torch.Generator().manual_seed(5)
    checked = 0
    for which, grad, x0 in (("feat", ref["dfeat"], feat0), ("conf", ref["dconf"], conf0)):
        flat = grad.reshape(-1)
        f0 = abs(float(total(feat0, conf0, which)))
        # the difference quotient's own rounding noise, ~ 8 eps |f| / 2 h, stays below 3e-7 of the gradient
        cand = torch.nonzero(flat.abs() * x0.reshape(-1).abs() >= 8 * 2.2e-16 * f0 / (2 * 1e-6 * 3e-7)).reshape(-1)
        print(which, 'candidates:', cand.numel())
        assert cand.numel() >= 6, cand.numel()
        for i in cand[torch.randperm(cand.numel(), generator=g)[:6]].tolist():
            h = 1e-6 * abs(float(x0.reshape(-1)[i]))
            assert h > 0
            vals = []
            for sgn in (1.0, -1.0):
                x = x0.clone()
                x.reshape(-1)[i] += sgn * h
                vals.append(float(total(x, conf0, which) if which == "feat" else total(feat0, x, which)))
            fd = (vals[0] - vals[1]) / (2 * h)
            print(f"{which}[{i}]: autograd {float(flat[i]):.9e}, central difference {fd:.9e}")
            assert abs(fd - float(flat[i])) <= 1e-6 * abs(float(flat[i]))
            checked += 1
    assert checked == 12
