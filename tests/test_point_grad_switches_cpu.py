"""CPU tests of the per-tensor training switches opt.feat_grad / color_grad / dir_grad / conf_grad /
xyz_grad (neural_points.py:410-416): the options, the reference trainer's freeze, the point Adam's
state under them.  The GPU side is tests/test_point_grad_switches_gpu.py."""
import argparse
import dataclasses

import numpy as np
import pytest
import torch

import oracle_query as oq
from helpers import hyper_for, make_view, small_room, t_table
from sgnerf_amd.opts import HotPathOpts
from sgnerf_amd.point_adam import NoPointAdam, PointAdam, _check_point_tensors
from sgnerf_amd.train import PointParams, Trainer, ViewMLP, loss_from_query
from sgnerf_amd.weights import init_mlp

O = HotPathOpts(SR=24)
NAMES = ("points_embeding", "points_color", "points_dir", "points_conf")


def test_defaults_are_all_trained():
    """HotPathOpts() trains the four tensors (scene241.sh:13-16), as before the switches existed."""
    o = HotPathOpts()
    assert (o.feat_grad, o.color_grad, o.dir_grad, o.conf_grad, o.xyz_grad) == (1, 1, 1, 1, 0)
    assert o.trained_points == NAMES
    assert o.check_supported() is o


def test_from_opt_picks_the_switches_up():
    """A driver's Namespace carries the real values (the reference's argparse default dir_grad 0 among
    them); any non-zero value means trained, as the reference's `> 0` test."""
    opt = argparse.Namespace(SR=24, feat_grad=1, color_grad=2, dir_grad=0, conf_grad=1, xyz_grad=0)
    o = HotPathOpts.from_opt(opt)
    assert (o.feat_grad, o.color_grad, o.dir_grad, o.conf_grad, o.xyz_grad) == (1, 2, 0, 1, 0)
    assert o.trained_points == ("points_embeding", "points_color", "points_conf")
    assert HotPathOpts.from_opt(argparse.Namespace(feat_grad=0, color_grad=0, dir_grad=0, conf_grad=0)).trained_points == ()
    assert HotPathOpts.from_opt(argparse.Namespace(SR=24)).trained_points == NAMES


def test_xyz_grad_is_refused():
    with pytest.raises(NotImplementedError, match="xyz_grad"):
        HotPathOpts(xyz_grad=1).check_supported()
    with pytest.raises(NotImplementedError, match="xyz_grad"):
        HotPathOpts.from_opt(argparse.Namespace(xyz_grad=1)).check_supported()


def _tiny():
    pc = small_room(20_000, seed=2)
    view = make_view(6, 8, yaw=30.0, pitch=-8.0)
    q = oq.OracleGrid(pc.xyz, hyper_for(pc, O), O).query(view.campos, view.raydir, t_table(O).numpy())
    rs, ss = np.nonzero(np.arange(O.SR)[None, :] < q["ray_ns"][:, None])
    ray_ns = torch.from_numpy(q["ray_ns"]).long()
    qd = {"ray_ns": ray_ns, "ray_soff": torch.cumsum(ray_ns, 0) - ray_ns, "samp_ray": torch.from_numpy(rs).long(),
          "samp_locw": torch.from_numpy(q["loc_w"][rs, ss]), "pidx": torch.from_numpy(q["pidx"][rs, ss]).long()}
    mlp = init_mlp(2, bias_std=0.01)
    mlp["alpha_branch.0.bias"] = mlp["alpha_branch.0.bias"] + 100.0
    gt = torch.rand(view.raydir.shape[0], 3, generator=torch.Generator().manual_seed(2))
    return pc, view, qd, mlp, gt


@pytest.mark.parametrize("frozen", [("points_dir",), ("points_conf",), ("points_embeding",),
                                    ("points_color", "points_dir"), NAMES])
def test_trainer_freezes_the_reference_way(frozen):
    """train.Trainer with switches off against plain autograd of loss_from_query with requires_grad_(False)
    set by hand: equal loss, equal gradients, none for the frozen tensors; after two steps the frozen
    tensors are bit-identical to their initial values, hold no Adam state though they are listed in the
    point group (the reference's way), and the trained ones moved."""
    pc, view, qd, mlp, gt = _tiny()
    sw = {"points_embeding": "feat_grad", "points_color": "color_grad", "points_dir": "dir_grad", "points_conf": "conf_grad"}
    o = dataclasses.replace(O, **{sw[k]: 0 for k in frozen})
    cam = (torch.from_numpy(view.campos), torch.from_numpy(view.camrotc2w), torch.from_numpy(view.raydir))
    pts = PointParams(pc.xyz, pc.embedding, pc.color, pc.dir, pc.conf, "cpu")
    tr = Trainer(pts, mlp, o, "cpu")
    parts, full, mask = tr.backward(*cam, 0.1, 8.0, gt, q=qd)
    assert int(mask.sum()) > 0
    # by hand
    hand = PointParams(pc.xyz, pc.embedding, pc.color, pc.dir, pc.conf, "cpu")
    for k in frozen:
        getattr(hand, k).requires_grad_(False)
    net = ViewMLP(mlp)
    total, parts_h, full_h, _ = loss_from_query(hand, net, qd, *cam, gt, O)
    total.backward()
    assert float(parts["total"]) == float(total.detach())
    assert torch.equal(full, full_h.detach())
    for k in NAMES:
        a, b = getattr(pts, k).grad, getattr(hand, k).grad
        if k in frozen:
            assert a is None and b is None
        else:
            assert torch.equal(a, b) and float(a.abs().sum()) > 0, k
    for pa, pb in zip(tr.mlp.parameters(), net.parameters()):
        assert torch.equal(pa.grad, pb.grad)
    # the zero-one term is reported whether conf trains or not
    ref_all = Trainer(PointParams(pc.xyz, pc.embedding, pc.color, pc.dir, pc.conf, "cpu"), mlp, O, "cpu")
    parts_all, _, _ = ref_all.backward(*cam, 0.1, 8.0, gt, q=qd)
    assert float(parts["conf_coefficient"]) == float(parts_all["conf_coefficient"]) != 0.0
    p0 = {k: getattr(pts, k).detach().clone() for k in NAMES}
    tr.apply()
    tr.step(*cam, 0.1, 8.0, gt, q=qd)
    assert len(tr.opt_pts.param_groups[0]["params"]) == 4
    for k in NAMES:
        p = getattr(pts, k)
        if k in frozen:
            assert torch.equal(p.detach(), p0[k]) and p not in tr.opt_pts.state
        else:
            assert not torch.equal(p.detach(), p0[k]) and "exp_avg" in tr.opt_pts.state[p]


def test_point_adam_state_refuses_other_switches():
    """A PointAdam state written under one switch set loads under the same set and raises a ValueError
    naming the switches under another -- also where the two sets train equally many tensors, which
    torch's own length check would let through."""
    mk = lambda: [torch.nn.Parameter(torch.zeros(5, w)) for w in (32, 3, 1)]  # noqa: E731
    a = PointAdam(mk(), lr=1e-3, names=("points_embeding", "points_color", "points_conf"))
    sd = a.state_dict()
    assert sd["param_groups"][0]["point_tensors"] == ["points_embeding", "points_color", "points_conf"]
    same = PointAdam(mk(), lr=1e-3, names=("points_embeding", "points_color", "points_conf"))
    same.load_state_dict(sd)
    assert same.state_dict()["param_groups"][0]["point_tensors"] == sd["param_groups"][0]["point_tensors"]
    other = PointAdam(mk(), lr=1e-3, names=("points_embeding", "points_dir", "points_conf"))
    with pytest.raises(ValueError, match=r"points_color.*points_dir.*dir_grad"):
        other.load_state_dict(sd)
    fewer = PointAdam(mk()[:2], lr=1e-3, names=("points_embeding", "points_color"))
    with pytest.raises(ValueError, match="dir_grad"):
        fewer.load_state_dict(sd)
    none = NoPointAdam(1e-3)
    with pytest.raises(ValueError, match="conf_grad"):
        none.load_state_dict(sd)
    none.load_state_dict(none.state_dict())
    with pytest.raises(ValueError):
        a.load_state_dict(none.state_dict())
    # a state from before the switches (no names): taken when the tensor count fits
    legacy = {"state": {}, "param_groups": [{k: v for k, v in sd["param_groups"][0].items() if k != "point_tensors"}]}
    _check_point_tensors(a.names, legacy)
    with pytest.raises(ValueError):
        _check_point_tensors(fewer.names, legacy)
    with pytest.raises(ValueError, match="one name per tensor"):
        PointAdam(mk(), lr=1e-3, names=("points_embeding",))
