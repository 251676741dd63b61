"""Rotated neural points (a non-identity Rw2c) without a GPU: the float64 restatement of the three rules
(tests/rw2c_ref.py) against the reference's own outputs (tests/golden/reference_rw2c.npz), and the host side:
the identity shortcut, the NeuralPoints round trip, prune / grow, the table cache key and every refusal."""
import ctypes

import numpy as np
import pytest
import torch

import sgnerf_amd  # noqa: F401
from sgnerf_amd import _lib
from sgnerf_amd.ray_marching import NeuralPoints, PointAggregator
from sgnerf_amd.render import PointTables
from sgnerf_amd.weights import init_mlp

import agg_rows_ref as ar
import rw2c_ref as rw
from helpers import GOLDEN_DIR, golden_points, load_golden
from test_plugin_cpu import N, _model

CASES = ["rot_parts", "rot_mixed", "rot_mixed_k4", "rot_global"]


def _golden():
    return np.load(f"{GOLDEN_DIR}/reference_rw2c.npz", allow_pickle=False)


@pytest.mark.parametrize("name", CASES)
def test_chain_reproduces_reference(name):
    """The restatement's whole chain (float64) against the reference's decoded features, at the project's fp32
    bar; and the case really is rotated: the unrotated chain misses by 1e-2 or more."""
    g = _golden()
    sc = rw.GoldenScene(g, name, golden_points(g, "corner"))
    _, mlp, _ = load_golden(str(g["mlp_from"]), "sparse32")
    ref = torch.from_numpy(g[f"{name}/decoded"]).double()
    got = sc.decoded(rw.chain(sc, mlp, sc.rot))
    err = float(((got - ref).abs() / ref.abs().clamp(min=1.0)).max())
    plain = sc.decoded(ar.chain(sc, mlp))
    miss = float((plain - ref).abs().max())
    print(f"{name}: max |chain - reference| / max(1, |ref|) = {err:.3e}; unrotated chain misses by {miss:.3e}")
    assert err <= ar.F32_TOL
    assert miss >= 1e-2
    # what the file promises about its cases
    nnb = sc.query["samp_nnb"]
    assert int(((nnb > 0) & (nnb < sc.K)).sum()) > 0
    if name != "rot_global":
        idx = torch.from_numpy(g[f"{name}/index"]).long()
        mi = torch.where(sc.query["pidx"] >= 0, idx[sc.query["pidx"].clamp(min=0).long()], torch.full_like(sc.query["pidx"], -1).long())
        later = (mi[:, 1:] >= 0) & (mi[:, 1:] != mi[:, :1])
        assert int(later.any(-1).sum()) > 0


def test_identity_equals_unrotated_chain():
    sc = ar.scene("pairs")
    st = init_mlp(5, bias_std=0.1)
    eye = torch.eye(3).expand(sc.N, 3, 3)
    a, b = rw.chain(sc, st, eye), ar.chain(sc, st)
    for k in ("dists", "ext", "rw", "z1", "z3", "fs", "alpha", "rgb"):
        assert torch.equal(a[k], b[k]), k
    r = rw.chain(sc, st, rw.palette_rot(sc.N))
    assert torch.equal(r["rw"], b["rw"])                       # rule 1: the weights keep the unrotated offset
    assert torch.equal(r["dists"][:, 3:], b["dists"][:, 3:])   # the pers half is not rotated
    assert float((r["rgb"] - b["rgb"]).abs().max()) > 1e-3


def _tables(rot):
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.rand(*s, generator=g)  # noqa: E731
    return PointTables(r(7, 3), r(7, 32), r(7, 3), r(7, 3), r(7, 1), "cpu", rot=rot)


def test_identity_shortcut():
    assert _tables(None).rot is None
    assert _tables(torch.eye(3)).rot is None
    assert _tables(torch.eye(3).expand(7, 3, 3).contiguous()).rot is None
    pal = rw.palette()
    t = _tables(pal[2])
    assert t.rot.shape == (7, 9) and t.rot.is_contiguous() and torch.equal(t.rot, pal[2].reshape(1, 9).expand(7, 9))
    per = pal[torch.arange(7) % 4]
    assert torch.equal(_tables(per).rot, per.reshape(7, 9))
    nearly = torch.eye(3).expand(7, 3, 3).clone()
    nearly[3, 0, 1] = 1e-7
    assert _tables(nearly).rot is not None
    with pytest.raises(ValueError, match="Rw2c"):
        _tables(torch.eye(3).expand(5, 3, 3))


def _rot_model(tmp_path, **extra):
    m = _model(tmp_path, **extra)
    p = m.neural_points
    rot = rw.palette()[torch.arange(N) % 4].contiguous()
    m.neural_points = NeuralPoints(p.xyz, p.points_embeding, p.points_color, p.points_dir, p.points_conf, "cpu",
                                   points_feats=p.points_feats, points_label=p.points_label, Rw2c=rot)
    return m, rot


def test_neural_points_round_trip_and_version_key(tmp_path):
    m, rot = _rot_model(tmp_path)
    p = m.neural_points
    assert p.rotated()
    sd = p.state_dict()
    assert torch.equal(sd["neural_points.Rw2c"], rot)
    q = NeuralPoints.from_state_dict(sd, "cpu")
    assert q.Rw2c.shape == (N, 3, 3) and torch.equal(q.Rw2c, rot) and q.rotated()
    m.save_networks(3, {})
    sd = torch.load(tmp_path / "scene" / "3_net_ray_marching.pth", map_location="cpu", weights_only=True)
    assert torch.equal(NeuralPoints.from_state_dict(sd, "cpu").Rw2c, rot)
    # the table cache follows Rw2c: another tensor, or an in-place change
    k0 = p._version_key()
    p.Rw2c = rot.clone()
    k1 = p._version_key()
    p.Rw2c[0, 0, 0] += 1.0
    assert k0 != k1 and k1 != p._version_key()
    assert torch.equal(p.tables().rot[1:], rot.reshape(N, 9)[1:]) and float(p.tables().rot[0, 0]) == float(rot[0, 0, 0]) + 1.0
    # a [3,3] matrix, and the wrong length
    g = NeuralPoints(p.xyz, p.points_embeding, p.points_color, p.points_dir, p.points_conf, "cpu", Rw2c=rw.palette()[1])
    assert torch.equal(g.tables().rot, rw.palette()[1].reshape(1, 9).expand(N, 9))
    assert not NeuralPoints(p.xyz, p.points_embeding, p.points_color, p.points_dir, p.points_conf, "cpu").rotated()
    with pytest.raises(ValueError, match="Rw2c"):
        NeuralPoints(p.xyz, p.points_embeding, p.points_color, p.points_dir, p.points_conf, "cpu", Rw2c=rot[:5])
    # set_points takes it; without it a per-point table does not outlive its points
    g.set_points(p.xyz[:9], p.points_embeding[:, :9], p.points_color[:, :9], p.points_dir[:, :9], p.points_conf[:, :9], Rw2c=rot[:9])
    assert torch.equal(g.Rw2c, rot[:9])
    g.set_points(p.xyz[:4], p.points_embeding[:, :4], p.points_color[:, :4], p.points_dir[:, :4], p.points_conf[:, :4])
    assert not g.rotated()


def test_prune_and_grow_keep_rows_aligned(tmp_path):
    m, rot = _rot_model(tmp_path)
    conf = m.neural_points.points_conf[0, :, 0]
    thresh = float(conf.median())
    mask = conf >= thresh
    xyz = m.neural_points.xyz.clone()
    removed = m.prune_points(thresh)
    p = m.neural_points
    assert removed == int((~mask).sum()) and p.Rw2c.shape == (int(mask.sum()), 3, 3)
    assert torch.equal(p.Rw2c, rot[mask]) and torch.equal(p.xyz, xyz[mask])
    n0 = p.xyz.shape[0]
    g = torch.Generator().manual_seed(1)
    r = lambda *s: torch.rand(*s, generator=g)  # noqa: E731
    add = rw.palette()[torch.tensor([3, 1, 2])]
    m.grow_points(r(3, 3), r(3, 32), r(3, 3), r(3, 3), r(3, 1), add_Rw2c=add)
    p = m.neural_points
    assert torch.equal(p.Rw2c[:n0], rot[mask]) and torch.equal(p.Rw2c[n0:], add) and p.xyz.shape[0] == n0 + 3
    m.grow_points(r(2, 3), r(2, 32), r(2, 3), r(2, 3), r(2, 1))
    p = m.neural_points
    assert torch.equal(p.Rw2c[n0 + 3:], torch.eye(3).expand(2, 3, 3)) and torch.equal(p.Rw2c[n0:n0 + 3], add)
    # one matrix for every point covers new points as it is
    m.neural_points.Rw2c = rw.palette()[2]
    m.grow_points(r(2, 3), r(2, 32), r(2, 3), r(2, 3), r(2, 1))
    assert torch.equal(m.neural_points.Rw2c, rw.palette()[2])
    m.prune_points(0.0)
    assert torch.equal(m.neural_points.Rw2c, rw.palette()[2])
    with pytest.raises(ValueError, match="add_Rw2c"):
        m.grow_points(r(2, 3), r(2, 32), r(2, 3), r(2, 3), r(2, 1), add_Rw2c=add[:2])


def test_training_and_sg_refusals(tmp_path):
    m, _ = _rot_model(tmp_path)
    with pytest.raises(NotImplementedError, match="Rw2c"):
        m.setup_optimizer(m.opt)
    with pytest.raises(NotImplementedError, match="Rw2c"):
        m.optimize_parameters()
    sg, _ = _rot_model(tmp_path, shading_feature_mlp_layer2_bpnet=1)
    assert sg.opts.bpnet_variant[0]
    with pytest.raises(NotImplementedError, match="Rw2c"):
        sg._check_rotation()
    # identity stays welcome everywhere
    m.neural_points.Rw2c = torch.eye(3).expand(N, 3, 3).contiguous()
    m._check_rotation(training=True)
    sg.neural_points.Rw2c = torch.eye(3)
    sg._check_rotation()


def test_set_points_editing(tmp_path):
    """editing_set_points (neural_points.py:667-681): default_conf in (0, 1] overrides the confidences, Rw2c is
    kept, nothing is trainable.  set_points(editing=True) itself stays refused, and names the entry."""
    m = _model(tmp_path, default_conf=0.15)
    m.is_train = True
    m._sync_weights = lambda: None
    g = torch.Generator().manual_seed(2)
    r = lambda *s: torch.rand(*s, generator=g)  # noqa: E731
    rot = rw.palette()[torch.arange(9) % 4].contiguous()
    m.editing_set_points(r(9, 3), points_embedding=r(1, 9, 32), points_color=r(1, 9, 3), points_dir=r(1, 9, 3),
                         points_conf=r(1, 9, 1), Rw2c=rot)
    p = m.neural_points
    assert torch.equal(p.Rw2c, rot) and torch.equal(p.points_conf, torch.full((1, 9, 1), 0.15))
    assert m.trainer is None and m.optimizers == [] and m.net_ray_marching.neural_points is p
    m.opt.default_conf = -1.0
    conf = r(1, 9, 1)
    m.editing_set_points(r(9, 3), points_embedding=r(1, 9, 32), points_color=r(1, 9, 3), points_dir=r(1, 9, 3),
                         points_conf=conf, Rw2c=rot)
    assert torch.equal(m.neural_points.points_conf, conf)
    with pytest.raises(NotImplementedError, match="editing_set_points"):
        m.set_points(r(9, 3), points_embedding=r(1, 9, 32), points_color=r(1, 9, 3), points_dir=r(1, 9, 3),
                     points_conf=conf, Rw2c=rot, editing=True)
    # set_points without editing takes the rotation too (a non-training model: no optimizer to refuse it)
    m.is_train = False
    m.set_points(r(9, 3), points_embedding=r(1, 9, 32), points_color=r(1, 9, 3), points_dir=r(1, 9, 3),
                 points_conf=conf, Rw2c=rot)
    assert torch.equal(m.neural_points.Rw2c, rot)


def test_point_aggregator_refuses_rotation():
    agg = PointAggregator.__new__(PointAggregator)   # forward checks sampled_Rw2c before anything else
    agg.device = torch.device("cpu")
    z = torch.zeros(1, 2, 3, 4, 3)
    rot = rw.palette()[1].expand(1, 2, 3, 4, 3, 3)
    for bad in (rot, rw.palette()[2]):
        with pytest.raises(NotImplementedError, match="sampled_Rw2c"):
            agg.forward(z, None, bad, z, z[..., :1], z, z, z, z[..., 0] > 0, z[..., 0, :], z[..., 0, :], z[..., 0, :], None, 0)


def test_c_entries_refuse_rot_before_any_launch():
    """Every entry that takes sgn_point_tables and builds aggregator inputs, but is not built for rotation,
    returns an argument error naming rot (pointers are never dereferenced: the checks come first)."""
    L = _lib.lib()
    A = 4096   # a non-null, 16-byte aligned address that nothing reads
    p = ctypes.c_void_p(A)
    pt = _lib.PointTables()
    for k in ("xyz", "embedding", "color", "dir", "conf", "campos", "camrotc2w", "raydir", "rot", "samp_viewdir"):
        setattr(pt, k, A)
    pt.n_points = 8
    qo = _lib.QueryOut()
    for k, _ in qo._fields_:
        setattr(qo, k, A)
    saved, deltas, grads = _lib.AggSaved(), _lib.AggDeltas(), _lib.PointGrads()
    for s in (saved, deltas, grads):
        for k, _ in s._fields_:
            setattr(s, k, A)
    P, Q = ctypes.byref(pt), ctypes.byref(qo)
    big = 1 << 20

    def refused(rc, what):
        assert rc != 0, what
        msg = L.sgn_last_error().decode()
        assert "invalid argument" in msg and "rot" in msg, f"{what}: {msg}"

    refused(L.sgn_aggregate_train_fwd(0, 0, None, P, Q, 8, 8, p, p, p, ctypes.byref(saved), None, None), "train_fwd")
    refused(L.sgn_aggregate_backward(0, 0, P, Q, 8, 8, p, p, ctypes.byref(saved), None, p, p, p, ctypes.byref(deltas), None,
                                     ctypes.byref(grads), None), "backward")
    refused(L.sgn_aggregate_train_fwd_f32(0, 0, None, p, P, Q, 8, 8, p, p, p, p, None, p, None, p, big, None), "train_fwd_f32")
    refused(L.sgn_train_row_inputs(P, Q, 8, p, p, p, p, p, p, None), "row_inputs")
    refused(L.sgn_train_row_head(P, Q, 8, p, p, p, p, p, p, p, p, p, p, p, None), "row_head")
    refused(L.sgn_train_row_tail(P, Q, 8, p, p, p, p, ctypes.byref(grads), None), "row_tail")
    # the SG variants of the aggregate entries
    for nl, dim in ((1, 0), (1, 96)):
        refused(L.sgn_aggregate(nl, dim, p, p, P, Q, 8, 8, p, p, None, None, p, big, 3, None), f"aggregate {nl} {dim}")
        refused(L.sgn_aggregate_f32(nl, dim, p, p, P, Q, 8, 8, p, p, None, None, p, big, 3, None), f"aggregate_f32 {nl} {dim}")
        refused(L.sgn_aggregate_exact(nl, dim, p, P, Q, 8, 8, p, p, None, None, p, big, None), f"aggregate_exact {nl} {dim}")
    # rot without the samples' view directions, or with the caller's pers coordinates
    pt.samp_viewdir = None
    refused(L.sgn_aggregate_f32(0, 0, None, p, P, Q, 8, 8, p, p, None, None, p, big, 3, None), "no samp_viewdir")
    pt.samp_viewdir = A
    pt.pers = pt.samp_pers = A
    refused(L.sgn_aggregate_exact(0, 0, None, P, Q, 8, 8, p, p, None, None, p, big, None), "rot with pers")


def test_abi_23():
    assert _lib.ABI_VERSION == 23 and _lib.lib().sgn_abi_version() == 23
    names = [k for k, _ in _lib.PointTables._fields_]
    assert names[-2:] == ["rot", "samp_viewdir"] and ctypes.sizeof(_lib.PointTables) == 13 * 8
