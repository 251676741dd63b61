"""CPU tests of early ray termination: the restatement (tests/early_stop_ref.py) on the goldens' stored
reference opacities, the option validation, the binding, and that the option switched off plans no tiers."""
import os

import numpy as np
import pytest

import early_stop_ref as er
from helpers import GOLDEN_DIR
from sgnerf_amd import _lib
from sgnerf_amd.opts import HotPathOpts
from sgnerf_amd.render import HipRenderer, RenderOut

EPS = 1e-2
# valid samples skipped at eps = 1e-2, from the reference's own opacities (reference_opaque.npz)
SKIPPED = {
    (4, 8, 16): {"corner64": 49, "sparse32": 50, "opq_patch": 0},
    (4, 8, 12, 16, 20): {"corner64": 100, "sparse32": 78, "opq_patch": 0},
}


def _case(file, name):
    g = np.load(os.path.join(GOLDEN_DIR, file), allow_pickle=False)
    return g[f"{name}/opacity"], g[f"{name}/ray_valid"].astype(bool)


@pytest.mark.parametrize("slots", list(SKIPPED))
@pytest.mark.parametrize("name", ["corner64", "sparse32", "opq_patch"])
def test_skipped_counts_on_opaque_goldens(name, slots):
    op, valid = _case("reference_opaque.npz", name)
    stop, skipped = er.decide(op, valid, EPS, slots)
    assert int(skipped.sum()) == SKIPPED[slots][name]
    SR = op.shape[1]
    T = er.transmittance(op)
    bounds = er.boundaries(slots, SR)[1:-1]
    for r in range(op.shape[0]):
        hit = [b for b in bounds if T[r, b] <= np.float32(EPS)]
        assert stop[r] == (hit[0] if hit else SR)
    assert not skipped[np.arange(SR)[None, :] < stop[:, None]].any()
    # the bound: the weights a stopped ray loses sum to at most T at its stop slot (+ the 1e-10 terms)
    w = op * T[:, :-1]
    lost = np.where(skipped, w, 0).astype(np.float64).sum(1)
    Ta = T[np.arange(len(stop)), stop].astype(np.float64)
    assert (lost[stop < SR] <= Ta[stop < SR] + 1e-7).all() and (Ta[stop < SR] <= EPS).all()


@pytest.mark.parametrize("slots", list(SKIPPED))
@pytest.mark.parametrize("name", ["patch", "patch64", "dense"])
def test_transparent_goldens_skip_nothing(name, slots):
    op, valid = _case("reference_aggregator.npz", name)
    assert er.transmittance(op)[:, -1].min() >= 0.96
    stop, skipped = er.decide(op, valid, EPS, slots)
    assert int(skipped.sum()) == 0 and (stop == op.shape[1]).all()


def test_tier_restatement_agrees_with_the_decision():
    """The two levels of the restatement tied together on a synthetic query: `tier`'s transmittance (raw
    query + feat) equals `transmittance` of the per-slot opacities its arithmetic implies, bit for bit, and
    its stop slots, emitted and zeroed ids follow from that T."""
    rng = np.random.default_rng(3)
    R, SR, vz = 9, 12, 0.008
    campos, rot = np.array([0.1, -0.2, 0.3], np.float32), np.eye(3, dtype=np.float32)
    ns = np.array([0, 1, 4, 5, 12, 12, 7, 12, 3], np.int32)
    off = np.concatenate([[0], np.cumsum(ns)[:-1]]).astype(np.int32)
    S = int(ns.sum())
    locw = np.zeros((S, 3), np.float32)
    for r in range(R):
        locw[off[r]:off[r] + ns[r], 2] = 0.5 + vz * np.arange(ns[r]) + campos[2]
    nnb = np.where(rng.random(S) < 0.8, 3, 0).astype(np.int32)
    feat = np.zeros((S, 4), np.float32)
    feat[:, 0] = rng.choice([0.0, 5.0, 80.0, 400.0], S)
    for lo in (0, 4, 5):
        emit, zero, stop, T = er.tier(campos, rot, ns, off, nnb, locw, feat, SR, 1, vz, lo, lo + 3, EPS, np.full(R, SR))
        # the same T from per-slot opacities: intervals of the samples' pers z, the last one replaced by vz
        op = np.zeros((R, SR), np.float32)
        for r in range(R):
            for s in range(ns[r]):
                if nnb[off[r] + s] > 0:
                    z = [er.pers_z(campos, rot, locw[off[r] + j]) for j in (s, s + 1)] if s + 1 < ns[r] else [0, 0]
                    d = np.float32(z[1] - z[0])
                    d = np.float32(vz) if (d < 1e-8 or d > 2 * np.float32(vz)) else d
                    op[r, s] = np.float32(1) - np.exp(-feat[off[r] + s, 0] * d, dtype=np.float32)
        np.testing.assert_array_equal(T, er.transmittance(op)[:, lo])
        fin = T <= np.float32(EPS)
        assert (stop == np.where(fin, lo, SR)).all()
        assert lo == 0 or (fin.any() and not fin.all())
        ids = {int(off[r] + s) for r in range(R) for s in range(lo, min(lo + 3, ns[r])) if nnb[off[r] + s] > 0}
        assert set(emit) | set(zero) == ids and not set(emit) & set(zero)
        assert all(fin[np.searchsorted(off, i, side="right") - 1] for i in zero)


def test_option_defaults_and_tiers():
    o = HotPathOpts()
    assert o.early_stop == 0.0 and o.early_stop_slots == (4, 8, 16)
    assert o.check_supported().early_stop_tiers == ((0, 4), (4, 8), (8, 16), (16, 24))
    assert HotPathOpts(SR=16).early_stop_tiers == ((0, 4), (4, 8), (8, 16))          # boundaries >= SR are ignored
    assert HotPathOpts(SR=33, early_stop_slots=(5,)).early_stop_tiers == ((0, 5), (5, 33))
    assert HotPathOpts(SR=4).early_stop_tiers == ((0, 4),)
    assert HotPathOpts(early_stop=0.5, early_stop_slots=()).check_supported().early_stop_tiers == ((0, 24),)


@pytest.mark.parametrize("kw", [dict(early_stop=-1e-3), dict(early_stop=1.0), dict(early_stop=float("nan")),
                                dict(early_stop="0.1"), dict(early_stop_slots=(4, 4)), dict(early_stop_slots=(8, 4)),
                                dict(early_stop_slots=(0, 4)), dict(early_stop_slots=(-2,)),
                                dict(early_stop_slots=(4.5,)), dict(early_stop_slots=[4, 8])])
def test_option_validation_refuses(kw):
    with pytest.raises(NotImplementedError, match="early_stop"):
        HotPathOpts(**kw).check_supported()


@pytest.mark.parametrize("kw", [dict(early_stop=0.0), dict(early_stop=0), dict(early_stop=0.999),
                                dict(early_stop=np.float32(1e-3), early_stop_slots=(1, 2, 3, 400))])
def test_option_validation_accepts(kw):
    HotPathOpts(**kw).check_supported()


def test_from_opt_parses_the_options():
    import argparse
    ns = argparse.Namespace(early_stop=1e-3, early_stop_slots=[4, 12])
    o = HotPathOpts.from_opt(ns)
    assert o.early_stop == 1e-3 and o.early_stop_slots == (4, 12)
    assert HotPathOpts.from_opt(argparse.Namespace(early_stop_slots="4, 8,20")).early_stop_slots == (4, 8, 20)
    assert HotPathOpts.from_opt(argparse.Namespace(early_stop_slots=6)).early_stop_slots == (6,)
    o = HotPathOpts.from_opt(argparse.Namespace(early_stop=None, early_stop_slots=None))
    assert o.early_stop == 0.0 and o.early_stop_slots == (4, 8, 16)
    assert HotPathOpts.from_opt(argparse.Namespace()).early_stop == 0.0       # a reference Namespace: off


def _planner(**kw):
    """A HipRenderer shell carrying only what the tier planning reads (no device)."""
    r = HipRenderer.__new__(HipRenderer)
    r.opts = HotPathOpts(**kw).check_supported()
    r.exact = False
    r.es = None
    return r


def test_early_stop_off_plans_no_tiers_and_no_buffers():
    r = _planner()
    assert r._tiers() == () and r.es is None
    on = _planner(early_stop=1e-3, SR=24)
    assert on._tiers() == ((0, 4), (4, 8), (8, 16), (16, 24))
    # ignored: per-slot outputs, the hole probe, training options, the plain-fp32 range fallback
    assert on._tiers(want_probe=True) == () and on._tiers(want_weights=True) == () and on._tiers(want_blend=True) == ()
    assert _planner(early_stop=1e-3, is_train=1)._tiers() == ()
    on.exact = True
    assert on._tiers() == ()
    # the new RenderOut fields trail the old ones and default to None
    names = list(RenderOut.__dataclass_fields__)
    assert names[-3:] == ["stop_slot", "skipped", "tiers"] and names[-4] == "depth"
    assert all(RenderOut.__dataclass_fields__[n].default is None for n in names[-3:])


def test_entry_is_bound_and_validates():
    """sgn_early_stop_tier: bound with the header's signature, ABI still 23, arguments refused before any
    device work."""
    import ctypes
    assert "sgn_early_stop_tier" in _lib.SIGNATURES and _lib.ABI_VERSION == 23
    L = _lib.lib()
    assert L.sgn_abi_version() == 23
    cp = _lib.CompositeParams()
    cp.SR, cp.vsize_z, cp.raydist_mode_unit = 24, 0.008, 1
    q = _lib.QueryOut()
    one = ctypes.c_void_p(16)

    def call(lo, hi, eps, qq=q, feat=one):
        return L.sgn_early_stop_tier(ctypes.byref(cp), one, one, 4, ctypes.byref(qq), feat, lo, hi, eps, 96, one, one,
                                     None, one, None)
    assert call(0, 4, 0.01) == -2 and b"query outputs" in L.sgn_last_error()
    for name in ("ray_ns", "ray_soff", "samp_nnb", "samp_locw", "counters"):
        setattr(q, name, 16)
    for lo, hi, eps in ((4, 4, 0.01), (-1, 4, 0.01), (8, 25, 0.01), (24, 25, 0.01), (0, 4, 1.0), (0, 4, -0.1)):
        assert call(lo, hi, eps) == -2, (lo, hi, eps)
    assert call(0, 4, 0.01, feat=None) == -2 and b"null" in L.sgn_last_error()
    assert call(0, 4, 0.01, feat=ctypes.c_void_p(4)) == -2 and b"aligned" in L.sgn_last_error()


def test_plugin_options_reach_the_hot_path_options():
    """--sgn_early_stop / --sgn_early_stop_slots of the plugin: parsed, validated, and a model with the option
    on renders without the per-slot weight outputs (they need every sample)."""
    import argparse
    from sgnerf_amd.model import HipPointsVolumetricModel
    ap = HipPointsVolumetricModel.modify_commandline_options(argparse.ArgumentParser())
    off = ap.parse_args([])
    assert off.sgn_early_stop == 0.0 and off.sgn_early_stop_slots == "4,8,16"
    m = HipPointsVolumetricModel()
    m.initialize(off)
    assert m.opts.early_stop == 0.0 and m.opts.early_stop_slots == (4, 8, 16) and m._return_weights
    m.initialize(ap.parse_args(["--sgn_early_stop", "1e-3", "--sgn_early_stop_slots", "4,12"]))
    assert m.opts.early_stop == 1e-3 and m.opts.early_stop_slots == (4, 12) and not m._return_weights
    with pytest.raises(NotImplementedError, match="early_stop"):
        m.initialize(ap.parse_args(["--sgn_early_stop", "1.5"]))
