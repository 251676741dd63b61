"""The hand-built query scenes on the GPU, through HipGrid, run_query and QueryWorkspace.

Every comparison is bit-exact.  On the dyadic scenes the reference is the exact integer reference of
tests/query_scene_ref.py (and the C restatement is held to it as well); on the rounding scenes the
reference is the C restatement's full-table scan.  Every workspace tensor is filled with a sentinel
before each call and must come back untouched past the sample count, past the work count, past the
rays, and (sample-major) past the S-th pidx row; the workspace is two rays larger than the batch."""
import dataclasses

import numpy as np
import pytest
import torch

from helpers import assert_equal_arrays
import query_scene_ref as qs

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = -77777777
SENT_F = np.float32(-7.5e33)
MARCH = {"wave": "1000000000", "thread": "0"}   # SGN_MARCH_WAVE_MAX_RAYS: k_march_wave / k_march


def build_grid(sc, opts=None):
    from sgnerf_amd.querier import HipGrid
    return HipGrid(torch.from_numpy(sc.xyz).to(DEV).reshape(-1, 3), opts or sc.opts, hyper=sc.hyper)


def run(sc, grid, dense, count_traffic=False, labels=True):
    """One sgn_query on sentinel-filled buffers; every workspace tensor comes back as a numpy array."""
    from sgnerf_amd.querier import QueryWorkspace, run_query
    o = sc.opts
    ws = QueryWorkspace(sc.R + 2, o.SR, o.K, DEV, dense=dense)
    for name in ("ray_ns", "ray_soff", "samp_ray", "samp_d", "samp_nnb", "pidx", "work", "counters"):
        getattr(ws, name).fill_(SENT)
    ws.samp_locw.fill_(float(SENT_F))
    ws.scratch.zero_()   # the slot table starts from zeros, not from what an earlier call left there
    pl = rl = None
    if labels and sc.point_labels is not None:
        pl = torch.from_numpy(sc.point_labels).to(DEV)
        rl = torch.from_numpy(sc.ray_labels).to(DEV)
    run_query(grid, o, torch.from_numpy(sc.campos).to(DEV), torch.from_numpy(sc.raydir).to(DEV),
              torch.from_numpy(sc.t).to(DEV), sc.per_ray_t, ws, dense=dense, point_labels=pl, ray_labels=rl,
              seconds=sc.seconds, count_traffic=count_traffic)
    torch.cuda.synchronize()
    return {name: getattr(ws, name).cpu().numpy() for name in
            ("ray_ns", "ray_soff", "samp_ray", "samp_d", "samp_nnb", "pidx", "work", "counters", "samp_locw")}


def check_query(sc, out, ref, dense, what, traffic=None):
    """Every output of one call against a reference in the oracle's dense layout, and the sentinels."""
    o = sc.opts
    R, SR, K = sc.R, int(o.SR), int(o.K)
    ns = ref["ray_ns"]
    S = int(ns.sum())
    assert_equal_arrays(out["ray_ns"][:R], ns, f"{what}: ray_ns")
    assert_equal_arrays(out["ray_soff"][:R], np.concatenate([[0], np.cumsum(ns)[:-1]]).astype(np.int32), f"{what}: ray_soff")
    sr = np.repeat(np.arange(R), ns).astype(np.int32)
    slot = np.arange(S) - np.repeat(np.cumsum(ns) - ns, ns)
    nnb = (ref["pidx"][sr, slot] >= 0).sum(-1).astype(np.int32)
    assert out["counters"][0] == S, f"{what}: counters[0] {out['counters'][0]} vs {S}"
    assert out["counters"][1] == int((nnb > 0).sum()), f"{what}: counters[1]"
    if traffic is None:
        assert out["counters"][2] == 0 and out["counters"][3] == 0, f"{what}: counters[2..3] without count_traffic"
    else:
        assert (int(out["counters"][2]), int(out["counters"][3])) == tuple(traffic), \
            f"{what}: traffic counters {out['counters'][2:]} vs {traffic}"
    assert_equal_arrays(out["samp_ray"][:S], sr, f"{what}: samp_ray")
    assert_equal_arrays(out["samp_d"][:S], ref["ray_d"][sr, slot], f"{what}: samp_d")
    assert_equal_arrays(out["samp_locw"][:S * 3].reshape(S, 3), ref["loc_w"][sr, slot], f"{what}: samp_locw")
    assert_equal_arrays(out["samp_nnb"][:S], nnb, f"{what}: samp_nnb")
    if dense:
        assert_equal_arrays(out["pidx"][:R * SR * K].reshape(R, SR, K), ref["pidx"], f"{what}: dense pidx")
        used = R * SR * K
    else:
        assert_equal_arrays(out["pidx"][:S * K].reshape(S, K), ref["pidx"][sr, slot], f"{what}: sample-major pidx")
        used = S * K
    nwork = int(out["counters"][1])
    assert_equal_arrays(np.sort(out["work"][:nwork]), np.nonzero(nnb > 0)[0].astype(np.int32), f"{what}: work list")
    # sentinels
    for name, n in (("ray_ns", R), ("ray_soff", R), ("samp_ray", S), ("samp_d", S), ("samp_nnb", S), ("work", nwork),
                    ("pidx", used)):
        assert np.all(out[name][n:] == SENT), f"{what}: {name} written past {n}"
    assert np.all(out["samp_locw"][S * 3:].view(np.int32) == SENT_F.view(np.int32)), f"{what}: samp_locw written past {S}"


def same_outputs(a, b, what):
    """Two calls' outputs are identical; the work list's order is the only freedom."""
    for name in a:
        if name == "work":
            n = int(a["counters"][1])
            assert_equal_arrays(np.sort(a["work"][:n]), np.sort(b["work"][:n]), f"{what}: work")
            assert_equal_arrays(a["work"][n:], b["work"][n:], f"{what}: work tail")
        elif name == "counters":
            assert_equal_arrays(a[name][:2], b[name][:2], f"{what}: counters")
        else:
            assert_equal_arrays(a[name], b[name], f"{what}: {name}")


def check_grid(grid, g, og, what):
    coor_occ, coor_2_occ, numpnts, lists = (x.cpu().numpy() for x in grid.export())
    for ref, side in ((g, "exact"), (og, "oracle")):
        if ref is None:
            continue
        assert_equal_arrays(coor_occ, ref.coor_occ, f"{what}: coor_occ vs {side}")
        assert_equal_arrays(coor_2_occ, ref.coor_2_occ, f"{what}: coor_2_occ vs {side}")
        assert_equal_arrays(numpnts, ref.occ_numpnts, f"{what}: occ_numpnts vs {side}")
        assert_equal_arrays(lists, ref.occ_2_pnts, f"{what}: occ_2_pnts vs {side}")
    inf = grid.info()
    ref = g if g is not None else og
    occ_idx = int(ref.occ_idx)
    max_o, P = int(grid.opts.max_o), int(grid.opts.P)
    assert inf["n_points"] == grid.n_points
    assert inf["n_claimed"] == occ_idx
    assert inf["n_slots"] == min(occ_idx, max_o)
    assert inf["n_listed"] == int(np.minimum(ref.occ_numpnts, P).sum())
    assert inf["volume"] == int(np.prod(coor_occ.shape))


@pytest.mark.parametrize("name", qs.scene_names())
def test_dyadic_scene(name, monkeypatch):
    """Grid and query of one dyadic scene: both march kernels, both pidx layouts, twice (repeatability), and
    with count_traffic (k_knn<COUNT>; k_knn27 otherwise unless P = 64 or kernel_size 5)."""
    sc, g, q, _ = qs.scene_exact(name)
    og, oq_ = qs.oracle_run(sc)
    for k in ("ray_ns", "ray_d", "pidx", "loc_w"):
        assert_equal_arrays(oq_[k], q[k], f"{name}: oracle {k}")
    grid = build_grid(sc)
    check_grid(grid, g, og, name)
    first = {}
    for march, env in MARCH.items():
        monkeypatch.setenv("SGN_MARCH_WAVE_MAX_RAYS", env)
        for dense in (True, False):
            out = run(sc, grid, dense)
            check_query(sc, out, q, dense, f"{name}/{march}/{'dense' if dense else 'sample-major'}")
            if dense in first:                    # the other march kernel gave the same bytes
                same_outputs(first[dense], out, f"{name}: k_march_wave vs k_march")
            first[dense] = out
        again = run(sc, grid, False)
        same_outputs(first[False], again, f"{name}/{march}: second run")
        counted = run(sc, grid, False, count_traffic=True)
        check_query(sc, counted, q, False, f"{name}/{march}/count_traffic", traffic=q["traffic"])
        same_outputs(first[False], counted, f"{name}/{march}: count_traffic vs plain")
    print(f"\n  {name}: N {len(sc.xyz)} claimed {g.occ_idx} slots {g.n_slots} listed {g.n_listed} | R {sc.R} D {sc.D} "
          f"SR {sc.opts.SR} K {sc.opts.K} P {sc.opts.P} | S {int(q['ray_ns'].sum())} work {int(counted['counters'][1])} "
          f"traffic {tuple(int(x) for x in counted['counters'][2:])} | {len(sc.expect)} plantings", end="")
    grid.close()


def test_semantic_off_on_the_labelled_cloud():
    """The labelled scenes share knn_K4's cloud and rays: without labels the query is knn_K4's, with them it
    differs for seconds % 10 = 2 (some neighbour rejected) and not for 0 and 1."""
    base = qs.scene_exact("knn_K4")[2]
    for sec in (0, 1, 2):
        sc, _, q, _ = qs.scene_exact(f"knn_K4_sem{sec}")
        grid = build_grid(sc)
        out = run(sc, grid, True, labels=False)
        check_query(sc, out, base, True, f"sem{sec} without labels")
        assert np.array_equal(q["pidx"], base["pidx"]) == (sec < 2)
        grid.close()


QUERY_SIZES = ((3, 3, 3), (5, 5, 5), (2, 4, 1), (1, 1, 1), (3, 3, 3))


def test_set_query_size_walk():
    """3 -> 5 -> (2, 4, 1) -> 1 -> 3 on one grid: each stop equals a fresh build (and the exact reference) of
    that query_size; the slots and the lists never change."""
    base = qs.scene("grid_main")
    grid = build_grid(base)
    lists0 = [x.cpu().numpy() for x in grid.export()[1:]]
    for size in QUERY_SIZES:
        grid.set_query_size(size)
        sc = qs.Scene(**{**base.__dict__, "opts": dataclasses.replace(base.opts, query_size=size)})
        g = qs.exact_grid(sc)
        fresh = build_grid(sc)
        got, want = [x.cpu().numpy() for x in grid.export()], [x.cpu().numpy() for x in fresh.export()]
        for a, b, nm in zip(got, want, ("coor_occ", "coor_2_occ", "occ_numpnts", "occ_2_pnts")):
            assert_equal_arrays(a, b, f"query_size {size}: {nm} vs a fresh build")
        assert_equal_arrays(got[0], g.coor_occ, f"query_size {size}: coor_occ vs exact")
        for a, b in zip(got[1:], lists0):
            assert_equal_arrays(a, b, f"query_size {size}: slots and lists unchanged")
        assert grid.info() == fresh.info()
        # and the march sees the new flags
        out = run(sc, grid, True)
        check_query(sc, out, qs.exact_query(sc, g), True, f"query_size {size}")
        fresh.close()
    grid.close()


@pytest.mark.parametrize("variant", range(4))
def test_rounding_scene(variant, monkeypatch):
    """Non-dyadic scenes (depths a rounding step either side of every face and of the widened box, 1e-30 and
    subnormal direction components, coordinates just below 10): the oracle's full-table scan is the reference."""
    sc = qs.rounding_scene(variant)
    og, ref = qs.oracle_run(sc)
    grid = build_grid(sc)
    check_grid(grid, None, og, sc.name)
    assert int(ref["ray_ns"].sum()) > 100
    for march, env in MARCH.items():
        monkeypatch.setenv("SGN_MARCH_WAVE_MAX_RAYS", env)
        for dense in (True, False):
            check_query(sc, run(sc, grid, dense), ref, dense, f"{sc.name}/{march}/{dense}")
    print(f"\n  {sc.name}: N {len(sc.xyz)} claimed {og.occ_idx} | R {sc.R} D {sc.D} | S {int(ref['ray_ns'].sum())} "
          f"(rays with samples: {int((ref['ray_ns'] > 0).sum())})", end="")
    grid.close()
