"""tests/agg_rows_ref.py proven without a GPU: its float64 chain equals train.aggregate, its fp32 chain the
oracle's aggregator; every planting the scenes promise is there; the restated pairing rule covers every pair
type of k_pair_slots; and every cap on the bounds of test_agg_rows_gpu.py holds on every scene that file uses
(the bounds are functions of the reference alone)."""
import pytest
import torch

import sgnerf_amd  # noqa: F401
from sgnerf_amd.train import PointParams, ViewMLP, aggregate
from sgnerf_amd.weights import init_mlp

import agg_ref
import agg_rows_ref as ar
import train_rows_ref as rr

BAR = 1e-10      # two float64 evaluations of one formula: only the summation order differs
VARIANTS = [(0, 0), (1, 96), (1, 0)]


def state_of(variant, seed=5):
    return init_mlp(seed, bias_std=0.1, bpnet_layers=variant[0], bpnet_dim=variant[1])


def _feat(sc, o):
    f = torch.zeros(sc.S, 4, dtype=o["rgb"].dtype)
    f[sc.work.long()] = torch.cat([o["alpha"][:, None], o["rgb"]], dim=-1)
    return f


@pytest.mark.parametrize("name", ["pairs", "rand3_777", "rand8_300"])
def test_float64_chain_is_train_aggregate(name):
    sc, st = ar.scene(name), state_of((0, 0))
    P, q = sc.points, sc.query
    campos, rot = sc.camera
    pp = PointParams(P["xyz"], P["embedding"], P["color"], P["dir"], P["conf"], "cpu").double()
    with torch.no_grad():
        feat, _, _ = aggregate(pp, ViewMLP(st).double(), campos.double(), rot.double(), sc.raydir.double(),
                               q["samp_ray"][:sc.S], q["samp_locw"][:sc.S].double(), q["pidx"][:sc.S])
    o = ar.chain(sc, st)
    got = _feat(sc, o)
    for c, what in ((slice(0, 1), "alpha_s"), (slice(1, 4), "rgb")):
        err, scale = float((got[:, c] - feat[:, c]).abs().max()), float(feat[:, c].abs().max())
        assert err <= BAR * scale, f"{what}: {err:.3e} over {scale:.3e}"
    # the module's row inputs are train_rows_ref's
    _, ext, rw, _ = rr.row_inputs_ref(P, sc.camera, sc.raydir, q, sc.K)
    assert float((o["ext"] - ext[:, :7]).abs().max()) < 1e-12 and float((o["rw"] - rw).abs().max()) < 1e-12
    assert float((o["dists"] - rr.row_dists(P, sc.camera, q, sc.K)).abs().max()) == 0.0


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", ["pairs", "rand3_777", "rand8_300"])
def test_fp32_chain_is_the_oracle(name, variant):
    sc, st = ar.scene(name), state_of(variant)
    q = sc.query
    pts = dict(sc.points)
    if variant != (1, 96):
        pts.pop("bpnet")
    campos, rot = sc.camera
    with torch.no_grad():
        feat, wgt = agg_ref.aggregate(pts, st, campos, rot, sc.raydir, q["samp_ray"][:sc.S], q["samp_locw"][:sc.S],
                                      q["pidx"][:sc.S].long())
    o = ar.chain(sc, st, dtype=torch.float32)
    err = float(((_feat(sc, o) - feat).abs() / feat.abs().clamp(min=1.0)).max())
    assert err <= 1e-5, err
    assert float((o["rw"][:, 0] - wgt[sc.rs, sc.rk]).abs().max()) <= 1e-5
    # and the float64 chain of every variant is that fp32 chain to fp32 rounding
    o64 = ar.chain(sc, st)
    assert float(((_feat(sc, o64) - feat.double()).abs() / feat.double().abs().clamp(min=1.0)).max()) <= 1e-5


def test_pers_chain_matches_the_camera_chain():
    sc, st = ar.scene("rand8_300"), state_of((0, 0))
    a, b = ar.chain(sc, st), ar.chain(sc, st, pers=sc.pers32())
    assert 0 < float((a["rgb"] - b["rgb"]).abs().max()) < 1e-4     # fp32-rounded pers coordinates: close, not equal


def _types(counts):
    """Pair types (nA, nB) of the restated rule on a work list's counts, and its slots."""
    slots = ar.pair_slots(counts)
    return slots, {(a, b) for _, a, _, b in slots}


def test_pair_lists_hold_every_pair_type():
    lo, tlo = _types(ar.PAIRS)
    hi, thi = _types(ar.PAIRS_HI)
    for t in ((7, 1), (6, 2), (5, 3), (4, 4)):
        assert sum(1 for _, a, _, b in lo if (a, b) == t) >= 2 and t in thi, t
    assert {(1, 1), (1, 2), (2, 3), (3, 4)} <= tlo            # the leftover chain
    assert {(7, 0), (6, 0), (5, 0), (4, 0), (8, 0)} <= thi       # unpaired 5, 6, 7, the odd leftover alone, 8s
    assert sum(1 for _, a, _, _ in lo if a == 8) >= 3
    assert len(lo) < len(ar.PAIRS) and len(hi) < len(ar.PAIRS_HI)
    for slots, counts in ((lo, ar.PAIRS), (hi, ar.PAIRS_HI), (ar.pair_slots(ar.scene("rand8_300").work_counts), None)):
        n = len(counts) if counts else 300
        seen = [0] * n
        for ia, na, ib, nb in slots:       # B sits at row max(nA, 4): it must fit the half
            seen[ia] += 1
            if ib >= 0:
                seen[ib] += 1
                assert max(na, 4) + nb <= 8 and nb >= 1
        assert seen == [1] * n             # each sample is A or B of exactly one slot
    # some 16-row set (two consecutive halves: a row set of the NS = 2 kernel's wave, and of NS = 1's) holds a B
    # sample in one half only
    for slots in (lo, hi):
        assert any((slots[j][2] >= 0) != (slots[j + 1][2] >= 0) for j in range(0, len(slots) - 1, 2))
    # the scene's work list carries these counts
    assert ar.scene("pairs").work_counts == ar.PAIRS and ar.scene("pairs_hi").work_counts == ar.PAIRS_HI
    assert sorted(ar.scene("pairs_shuf").work_counts) == sorted(ar.PAIRS)
    assert ar.scene("pairs75").items == 75
    assert sum(1 for _, a, _, b in ar.pair_slots(ar.scene("pairs53").work_counts) if (a, b) == (5, 3)) == 20


def test_scene_plants():
    sc = ar.scene("rand8_300")
    conf, emb, q = sc.points["conf"], sc.points["embedding"], sc.query
    assert float(conf.min()) < 0 and float(conf.max()) > 1 and bool((conf == 1e-4).any()) and bool((conf == 0).any())
    assert bool((conf == 1.0).any()) and float(emb.abs().max()) <= 4.0
    named = torch.unique(sc.pid)
    for v in (0.0, 1e-4, 1.0):
        assert bool((conf.reshape(-1)[named] == torch.tensor(v, dtype=torch.float32)).any()), v
    assert sc.S < sc.S_cap and int(q["counters"][0]) == sc.S and int(q["counters"][1]) == sc.items == 300
    assert bool((q["samp_nnb"][sc.S:] == sc.K).all())
    d = rr.row_dists(sc.points, sc.camera, q, sc.K)
    assert int((d[:, :3].norm(dim=-1) == 0).sum()) >= 4          # samples exactly at a neighbour
    assert 0.2 < float((q["samp_nnb"][:sc.S] == 0).float().mean()) < 0.4
    assert sc.points["bpnet"].shape == (ar.N_POINTS, 96)
    sh = ar.scene("pairs_shuf")
    assert not bool((sh.work[1:] > sh.work[:-1]).all())           # a non-ascending work list
    assert torch.equal(torch.sort(sh.work).values, ar.scene("pairs").work)
    cz = ((sc.points["xyz"].double() - sc.camera[0].double()) @ sc.camera[1].double())[:, 2]
    assert float(cz.min()) > 1.0                                   # every camera-space z well away from 0
    for name in ("pairs", "pairs_hi"):                             # empties are interleaved
        n = ar.scene(name).query["samp_nnb"][:ar.scene(name).S]
        assert int((n == 0).sum()) >= 5 and int(n[0]) == 0


def test_layer_shift_and_zero_layer():
    w = torch.zeros(4, 4)
    assert ar.layer_shift(w) == 0
    w[1, 2] = -0.75
    assert ar.layer_shift(w) == 14 and 0.75 * 2.0 ** 14 < 2 ** 14
    w[0, 0] = 1.0
    assert ar.layer_shift(w) == 13


GPU_SCENES = sorted(ar._SCENES)


@pytest.mark.parametrize("name", GPU_SCENES)
def test_caps_hold_on_every_gpu_scene(name):
    sc = ar.scene(name)
    variants = VARIANTS if name in ("pairs", "pairs_hi", "rand8_300", "pairs75") else [(0, 0)]
    for v in variants:
        st = state_of(v)
        b, o = ar.check_caps(sc, st)
        if sc.items and sc.rows <= 4000:
            ar.chain_bars(sc, st, o64=o)
    if name in ("rand8_300", "rand3_777"):
        ar.chain_bars(sc, state_of((0, 0)), pers=sc.pers32())


def test_projection_caps():
    """The bound of P stays under its cap on every table of the projection test, for both weight sets it bounds."""
    base = state_of((0, 0))
    big = dict(base)
    big["block1.0.weight"] = base["block1.0.weight"].clone()
    big["block1.0.weight"][7, 3] *= 1000.0
    for n in (1, 127, 128, 129, 32771):
        tab = ar.point_table(n, base)
        assert float(tab["embedding"].abs().max()) <= 4.0
        for st in (base, big):
            ref = ar.proj_ref(tab["embedding"].double(), st)
            ar.capped(ar.bound_P(ref, st), ref, f"P (n={n})")
    assert ar.layer_shift(big["block1.0.weight"]) < ar.layer_shift(base["block1.0.weight"]) - 6


def test_range_cases():
    sc, st = ar.scene("rand8_300"), state_of((0, 0))
    inside, f1 = ar.range_state(sc, st, 4.2e4)
    outside, f2 = ar.range_state(sc, st, 2.5e5)
    h1, h2 = ar.chain(sc, inside)["hidden"], ar.chain(sc, outside)["hidden"]
    assert 3e4 <= h1 <= 6e4 and h2 > 1e5 and f2 > f1 > 1
    ar.chain_bars(sc, inside)    # the caps hold on the scaled weights too


def test_colour_stage_caps():
    st = state_of((0, 0))
    for items in (1, 127, 128, 129, 32771):
        for shuffle in (False, True):
            case = ar.colour_case(items, shuffle)
            assert case.items < case.S < case.S_cap
            ar.colour_bar(case, st)
    c = ar.colour_case(129, True)
    assert not bool((c.work[1:] > c.work[:-1]).all())
