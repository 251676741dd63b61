"""The hand-built query scenes without a GPU: on every dyadic scene the C restatement
(oracle/query_ref.c: OracleGrid, OracleGrid.query) equals the exact integer reference of
tests/query_scene_ref.py bit for bit, and every planting the scenes exist for is present, by name."""
import numpy as np
import pytest

from helpers import assert_equal_arrays
import query_scene_ref as qs

exact = qs.scene_exact
SCENES = {n: qs.scene(n) for n in qs.scene_names()}


@pytest.mark.parametrize("name", list(SCENES))
def test_oracle_equals_exact_reference(name):
    sc, g, q, _ = exact(name)
    og, oq_ = qs.oracle_run(sc)
    for k in ("coor_occ", "coor_2_occ", "occ_numpnts", "occ_2_pnts"):
        assert_equal_arrays(getattr(og, k), getattr(g, k), f"{name}: {k}")
    assert og.occ_idx == g.occ_idx
    for k in ("ray_ns", "ray_d", "pidx", "loc_w"):
        assert_equal_arrays(oq_[k], q[k], f"{name}: {k}")


@pytest.mark.parametrize("name", list(SCENES))
def test_scene_holds_its_plantings(name):
    sc, _, _, pl = exact(name)
    missing = [p for p in sc.expect if p not in pl]
    assert not missing, f"{name} lost its plantings {missing}"
    assert set(sc.expect) <= set(qs.ALL_PLANTINGS)


@pytest.mark.parametrize("planting", qs.ALL_PLANTINGS)
def test_planting_is_present(planting):
    """Each planting of the issue's table holds in a scene that declares it, at a reported place."""
    where = [n for n, sc in SCENES.items() if planting in sc.expect]
    assert where, f"no scene declares {planting}"
    for n in where:
        assert planting in exact(n)[3], f"{planting} is absent from {n}"


@pytest.mark.parametrize("SR", qs.MARCH_SR)
def test_every_SR_carries_the_slot_cut_off_plantings(SR):
    pl = exact(f"march_sr{SR}")[3]
    need = ["flagged_SR", "flagged_SR+1", "flagged_>>SR", "srth_at_8chunk_offset_7", "srth_at_8chunk_offset_0",
            "srth_at_64group_offset_63", "srth_at_64group_offset_0"] + (["flagged_SR-1"] if SR > 1 else [])
    assert not [p for p in need if p not in pl]
    # the offsets are counted from the span's d_lo, exact here (the directions are powers of two): the table's
    # `a` leading candidates lie before the widened box, so d_lo is their count
    q = exact(f"march_sr{SR}")[2]
    assert list(q["d_lo"][:10]) == [3, 3, 3, 3, 2, 2, 0, 1, 0, 0]


def test_march_kinds_of_rays():
    sc, g, q, pl = exact("march_sr8")
    assert q["ray_ns"][10] == 0 and q["d_lo"][10] == sc.D          # the whole table before the box
    assert q["ray_ns"][11] == 0 and q["d_hi"][11] == -1            # ... and after it
    assert q["ray_ns"][12] == 0                                    # pointing away
    sc, g, q, pl = exact("march_deep")
    assert q["ray_d"][0, 0] == 32766 and q["ray_ns"][0] == 1       # the top of the int16 slot table
    assert q["ray_ns"][1] == 0 and q["ray_d"][2, 0] == 16383
    for case in ("margin", "lo_edge", "hi_edge", "outside_lo", "outside_hi"):
        sc, g, q, pl = exact(f"camera_{case}")
        assert list(q["ray_ns"][:3]) == [0, 0, 0] and q["ray_ns"][3:5].min() > 0
    sc, g, q, pl = exact("corner")
    assert all(q["trace"][(0, s)]["voxel"] == (0, 0, 0) for s in range(q["ray_ns"][0]))


def test_knn_outcomes_by_hand():
    """The kNN plantings' results, worked out by hand from :653-672 (point indices through the regions)."""
    sc, g, q, pl = exact("knn_K4")
    K = 4
    r = sc.regions
    pid = q["pidx"][:, 0, :]
    # slot 0: list dropped by the `> 0` rule
    assert list(pid[r["slot0"]]) == [-1] * K
    # tie_far: points 1..K fill (the K-th at d2 = 4), point K + 1 ties the farthest and is not taken
    assert list(pid[r["tie_far"]]) == [1, 2, 3, 4]
    # tie_among: the farthest pair (d2 = 4) sits at positions 0 and 2 of the fill; the two d2 = 3 points that
    # follow take their places in that order, the third ties and is dropped
    base = 1 + K + 1
    assert list(pid[r["tie_among"]]) == [base + K, base + 1, base + K + 1, base + 3]
    # K duplicates at the sample itself: later candidates at 0 and 1 are not nearer than the farthest (0)
    fz = int(pid[r["full_at_zero"]][0])
    assert list(pid[r["full_at_zero"]]) == [fz, fz + 1, fz + 2, fz + 3]
    # r2: (5, 0, 0) at d2 == r2 kept, (5, 1, 0) one step beyond dropped, (4, 3, 0) at d2 == r2 kept, -1 tail
    e = int(pid[r["r2_edge"]][0])
    assert list(pid[r["r2_edge"]]) == [e, e + 2, -1, -1]
    assert list(pid[r["nnb_zero"]]) == [-1] * K
    assert (r["nnb_zero"], 0) in pl["nnb_zero_not_in_worklist"] and (r["r2_edge"], 0) in pl["nnb_partial_minus1_tail"]
    assert (r["k_in_layer0"], 0) in pl["exactly_K_in_layer0_nearer_in_layer1"]
    assert (r["km1_overfill"], 0) in pl["K-1_in_layer0_layer1_overfills"]
    assert (r["total1"], 0) in pl["layer1_total_1"]
    assert (r["runs"], 0) in pl["runs_0_1_2_3_adjacent"] and (r["runs"], 0) in pl["runs_of_length_1_adjacent"]
    assert (r["corner000"], 0) in pl["sample_in_voxel_000"] and (r["cornermax"], 0) in pl["sample_in_voxel_dims-1"]


def test_traffic_counts_by_hand():
    """One sample in the corner voxel of the kernel-3 scene: 1 word on layer 0, 7 in-grid words on layer 1."""
    sc, g, q, pl = exact("corner")
    S = int(q["ray_ns"].sum())
    assert q["traffic"][0] == S * 8
    sc, g, q, pl = exact("knn_kernel5")
    assert q["traffic"][0] > 0 and q["traffic"][1] > 0


@pytest.mark.parametrize("variant", range(4))
def test_rounding_scenes(variant):
    """The non-dyadic family builds, leaves the exact domain on purpose, and gives the oracle work: samples on
    the rays that reach the box, directions whose span divisions overflow."""
    sc = qs.rounding_scene(variant)
    assert not sc.exact and sc.per_ray_t == 1 and np.all(sc.t[:, 1:] > sc.t[:, :-1])
    v = float(sc.hyper.scaled_vsize[0])
    assert v != 2.0 ** round(np.log2(v))
    assert float(sc.xyz.max()) == 10.0 and float(sc.hyper.shift.min()) > 9.5
    og, q = qs.oracle_run(sc)
    assert (q["ray_ns"] > 20).sum() >= 4 and q["ray_ns"].max() < sc.opts.SR
    tiny = np.abs(sc.raydir)
    with np.errstate(over="ignore", divide="ignore"):
        assert np.isinf(np.float32(1.0) / tiny[(tiny > 0) & (tiny < 1e-38)]).all()
    assert ((tiny > 0) & (tiny < 1e-38)).any() and np.isclose(tiny, 1e-30, rtol=1e-3).any()
