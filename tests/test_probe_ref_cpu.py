"""CPU checks of the hole-probing feature (opt.prob = 1): the float64 helper the GPU tests compare sgn_probe
with (tests/probe_ref.py) against a literal restatement of the reference's lines
(models/neural_points_volumetric_model.py:636-657), fill_invalid's expansion of the eight maps (:192-203),
and sgn_probe's binding and argument checks (they return before any launch, so they need no GPU)."""
import ctypes

import pytest
import torch

import probe_ref as P
from sgnerf_amd import _lib
from sgnerf_amd import ray_marching as rm


# ---- (a) probe_ref is the reference's formula -----------------------------------------------------------
@pytest.mark.parametrize("R,SR,K", [(200, 24, 8), (65, 7, 3), (64, 64, 1), (63, 1, 8)])
def test_probe_ref_is_the_reference_lines(R, SR, K):
    """probe_ref on the sample-major scene == lines 636-657 on the dense [1, R, SR, K, C] tensors (torch.max,
    gather, sum(dim=-2), float64 on the CPU, where torch.max returns the first of tied slots): the selected
    slot equal, the values to 1e-12 relative, on every ray of the mask; zero records outside it (unmask)."""
    sc = P.probe_scene(R, SR, K)
    ref = P.probe_ref(sc)
    d = P.dense_inputs(sc)
    out, ind = P.reference_lines_636_657(d["opacity"], d["sample_loc_w"], d["weight_conf"], d["sampled_xyz"],
                                         d["sampled_color"], d["sampled_dir"], d["sampled_conf"], d["sampled_embedding"])
    m = sc["mask"] != 0
    assert torch.equal(ind[0][m], ref["j"][m])
    for name, e in sc["expect_j"].items():
        assert int(ref["j"][sc["plant"][name]]) == e, name
    for key, field in P.KEY_FIELD.items():
        o, c = P.FIELDS[field]
        torch.testing.assert_close(ref["rec"][m, o:o + c], out[key][0][m].double(), rtol=1e-12, atol=0, msg=key)
    assert float(out["ray_max_sample_label"].abs().max()) == 0.0
    assert float(ref["rec"][~m].abs().sum()) == 0.0 and float(ref["rec"][:, list(P.PADS)].abs().sum()) == 0.0


def test_probe_scene_plantings():
    """At R = 200, SR = 24, K = 8 every planting has its ray, and the rays do what their names say."""
    sc = P.probe_scene(200, 24, 8)
    assert sc["skipped"] == []
    assert set(sc["plant"]) == {n for n, _, _ in P.PLANTINGS} | {n for n, _ in P.BORROWED}
    ref = P.probe_ref(sc)
    ns, soff = sc["ray_ns"].long(), sc["ray_soff"].long()
    r = sc["plant"]["tie"]
    a = sc["expect_j"]["tie"]
    assert sc["opacity"][r, a] == sc["opacity"][r, a + 2] == sc["opacity"][r].max() > sc["opacity"][r, a + 1]
    assert float(sc["opacity"][sc["plant"]["ones_run"]].max()) == 1.0
    assert int((sc["opacity"][sc["plant"]["ones_run"]] == 1.0).sum()) >= 2
    d0 = lambda s: float((sc["xyz"][0].double() - sc["samp_locw"][s].double()).norm())  # noqa: E731
    for name, wins0 in (("pt0_near", True), ("pt0_far", False), ("nnb0", True)):
        r = sc["plant"][name]
        s = int(soff[r]) + sc["expect_j"][name]
        assert int(sc["samp_nnb"][s]) < sc["K"]
        assert (float(ref["rec"][r, 1]) == pytest.approx(d0(s), rel=1e-12)) == wins0, name
    assert int(sc["samp_nnb"][int(soff[sc["plant"]["nnb0"]])]) == 0
    assert float(ref["rec"][sc["plant"]["nnb0"], 2:].abs().sum()) > 0          # loc_w is there ..
    assert float(ref["sumabs"][sc["plant"]["nnb0"]].sum()) == 0                 # .. and every blend is zero
    assert int(ns[sc["plant"]["mask0_ns"]]) > 0 and int(ns[sc["plant"]["mask0_ns0"]]) == 0


# ---- (b) fill_invalid expands the eight maps ------------------------------------------------------------
def _compact_output(R, keep, SR=5, probe=True):
    g = torch.Generator().manual_seed(3)
    n = keep.numel()
    mask = torch.zeros(1, R, dtype=torch.int8)
    mask[0, keep] = 1
    out = {"ray_mask": mask, "coarse_raycolor": torch.rand(1, n, 3, generator=g),
           "coarse_point_opacity": torch.rand(1, n, SR, generator=g), "queried_shading": torch.zeros(1, n, 3),
           "coarse_is_background": torch.rand(1, n, 1, generator=g)}
    if probe:
        for k, c in zip(rm.PROBE_KEYS, (1, 3, 1, 1, 3, 3, 1, 32)):
            out[k] = torch.rand(1, n, c, generator=g) + 0.5
    return out


def test_fill_invalid_expands_probe_maps():
    R, keep = 9, torch.tensor([1, 2, 5, 8])
    comp = _compact_output(R, keep)
    before = {k: v.clone() for k, v in comp.items()}
    full = rm.fill_invalid(comp, {"bg_color": torch.ones(1, 3)})
    assert rm.PROBE_KEYS == ("ray_max_shading_opacity", "ray_max_sample_loc_w", "ray_max_sample_label", "ray_max_far_dist",
                             "shading_avg_color", "shading_avg_dir", "shading_avg_conf", "shading_avg_embedding")
    gone = torch.tensor([0, 3, 4, 6, 7])
    for k, c in zip(rm.PROBE_KEYS, (1, 3, 1, 1, 3, 3, 1, 32)):
        assert full[k].shape == (1, R, c), k
        assert torch.equal(full[k][0, keep], before[k][0]), k
        assert float(full[k][0, gone].abs().sum()) == 0.0, k


def test_fill_invalid_without_probe_maps_is_unchanged():
    R, keep = 9, torch.tensor([0, 4, 7])
    full = rm.fill_invalid(_compact_output(R, keep, probe=False), {"bg_color": torch.ones(1, 3)})
    assert set(full) == {"ray_mask", "coarse_raycolor", "coarse_point_opacity", "queried_shading", "coarse_is_background",
                         "coarse_mask"}


# ---- (c) binding and argument checks --------------------------------------------------------------------
def _probe_args(R=4, SR=3, K=2, out=0x1000):
    """Non-null addresses that are never read: every case below returns before a launch."""
    pt, q = _lib.PointTables(), _lib.QueryOut()
    for f in ("xyz", "embedding", "color", "dir", "conf"):
        setattr(pt, f, 0x1000)
    pt.n_points = 8
    for f in ("ray_ns", "ray_soff", "samp_locw", "pidx", "samp_nnb"):
        setattr(q, f, 0x1000)
    vp = ctypes.c_void_p
    return (ctypes.byref(pt), ctypes.byref(q), vp(0x1000), vp(0x1000), vp(0x1000), R, SR, K, vp(out) if out else None, None), (pt, q)


def test_sgn_probe_is_bound():
    assert "sgn_probe" in _lib.SIGNATURES
    assert _lib.ABI_VERSION >= 22 and _lib.lib().sgn_abi_version() == _lib.ABI_VERSION
    assert _lib.PROBE_RECORD == P.REC == 48


@pytest.mark.parametrize("kw,word", [(dict(K=0), "K"), (dict(K=9), "K"), (dict(SR=0), "SR"), (dict(out=0), "null")])
def test_sgn_probe_rejects_bad_arguments(kw, word):
    L = _lib.lib()
    args, keep = _probe_args(**kw)
    rc = L.sgn_probe(*args)
    assert rc < 0
    msg = L.sgn_last_error().decode()
    assert "invalid argument" in msg and word in msg, msg


def test_sgn_probe_no_rays_is_a_no_op():
    args, keep = _probe_args(R=0)
    assert _lib.lib().sgn_probe(*args) == 0
