"""Rotated neural points (a non-identity, per-point Rw2c) on the GPU: sgn_sample_viewdirs, the rotated
instantiations of k_rows16 / k_color16 and k_rows_exact / k_color_exact through the C ABI on the hand-built
scenes (float64 reference: tests/rw2c_ref.py), the three arithmetic paths through HipRenderer against the
reference's own outputs (tests/golden/reference_rw2c.npz), and the model plugin (editing_set_points,
checkpoints, the f32 range fallback)."""
import argparse
import ctypes
import functools

import numpy as np
import pytest
import torch

import sgnerf_amd  # noqa: F401
from sgnerf_amd import _lib, scene
from sgnerf_amd.render import HipRenderer, PointTables

import agg_rows_ref as ar
import rw2c_ref as rw
from helpers import GOLDEN_DIR, golden_points, load_golden
from test_agg_rows_gpu import GUARD, NAN, Dev, check_feat_untouched, check_slots, fs_of, new_ws, weights
from test_render_gpu import TOL, _dense_feat, _opts
from test_train_rows_gpu import _all_nan, _ratio, _same_bits

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
U = ar.U
CASES = ["rot_parts", "rot_mixed", "rot_mixed_k4", "rot_global"]


def L():
    return _lib.lib()


# ---- the hand-built scenes with a palette matrix per point ---------------------------------------------

@functools.lru_cache(maxsize=None)
def planted(name):
    """(scene, rot [N,3,3]) -- N = 257 points, no multiple of the projection tile (128); every point draws one of
    the palette's four matrices, so the neighbours of a sample (and paired samples) carry different ones."""
    sc = ar.Scene(3, ar.rand(3, 41), bpnet=True) if name == "rand3_41" else ar.scene(name)
    assert sc.N % 128 != 0
    return sc, rw.palette_rot(sc.N)


class RotDev(Dev):
    """Dev with the [N,9] table in pt.rot and, once sample_viewdirs() ran, its output in pt.samp_viewdir."""

    def __init__(self, sc, rot):
        super().__init__(sc)
        self.d["rot9"] = rot.reshape(sc.N, 9).contiguous().to(DEV)
        self.pt.rot = self.d["rot9"].data_ptr()
        self.d["viewdir"] = torch.full((sc.S_cap + GUARD, 3), NAN, device=DEV)

    def sample_viewdirs(self):
        _lib.check(L().sgn_sample_viewdirs(ctypes.byref(self.pt), ctypes.byref(self.qo), self.sc.S_cap, self.sc.K,
                                           _lib.ptr(self.d["viewdir"]), _lib.stream_handle()), "sgn_sample_viewdirs")
        torch.cuda.synchronize()
        self.pt.samp_viewdir = self.d["viewdir"].data_ptr()
        return self.d["viewdir"].cpu()


@functools.lru_cache(maxsize=None)
def rot_dev(name):
    sc, rot = planted(name)
    return RotDev(sc, rot)


def run(dv, exact, rotated=True):
    """sgn_aggregate_f32 (stages 3) or sgn_aggregate_exact on a RotDev: feat, blend, wnorm, f_s [items, 256] (CPU)."""
    sc = dv.sc
    _, packed, packed_x = weights()
    pt = dv.pt
    if not rotated:   # the same tables without the rotation
        pt = _lib.PointTables()
        for k, _ in pt._fields_:
            setattr(pt, k, getattr(dv.pt, k))
        pt.rot = pt.samp_viewdir = None
    n = sc.S_cap * sc.K
    blend, wnorm = (torch.full((n + GUARD,), NAN, device=DEV) for _ in range(2))
    feat0 = torch.randn(sc.S_cap + GUARD, 4, generator=torch.Generator().manual_seed(3 + sc.S_cap))
    feat = feat0.to(DEV)
    if exact:
        ws = torch.full(((sc.S_cap + GUARD) * 1024,), 255, dtype=torch.uint8, device=DEV)
        rc = L().sgn_aggregate_exact(0, 0, None, ctypes.byref(pt), ctypes.byref(dv.qo), sc.S_cap, sc.K, _lib.ptr(packed_x),
                                     _lib.ptr(feat), _lib.ptr(blend), _lib.ptr(wnorm), _lib.ptr(ws), sc.S_cap * 1024,
                                     _lib.stream_handle())
        _lib.check(rc, "sgn_aggregate_exact")
        torch.cuda.synchronize()
        fs = ws[:sc.items * 1024].view(torch.float32).view(sc.items, 256).cpu()
    else:
        ws = new_ws(sc.S_cap)
        rc = L().sgn_aggregate_f32(0, 0, None, _lib.ptr(dv.proj(packed)), ctypes.byref(pt), ctypes.byref(dv.qo), sc.S_cap, sc.K,
                                   _lib.ptr(packed), _lib.ptr(feat), _lib.ptr(blend), _lib.ptr(wnorm), _lib.ptr(ws), ws.numel(), 3,
                                   _lib.stream_handle())
        _lib.check(rc, "sgn_aggregate_f32")
        torch.cuda.synchronize()
        fs = fs_of(ws, sc.S_cap)[:sc.items].cpu()
    return dict(feat=feat.cpu(), feat0=feat0, blend=blend.cpu(), wnorm=wnorm.cpu(), fs=fs)


# ---- 1. sgn_sample_viewdirs ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["pairs", "rand3_41"])
def test_sample_viewdirs(name):
    """Per element against float64 within 4 u sum_j |R_ij v_j| (a product and two additions: at most three
    roundings; the fourth ulp covers the store); samples outside the work list and the guard rows keep their bits."""
    dv = rot_dev(name)
    sc, rot = planted(name)
    got = dv.sample_viewdirs()
    ref = rw.sample_viewdirs(sc, rot)                                                  # [S, 3] float64
    p0 = sc.query["pidx"][:sc.S, 0].long().clamp(min=0)
    v = sc.raydir.double()[sc.query["samp_ray"][:sc.S].long()]
    bound = 4 * U * (rot.double()[p0].abs() * v.abs()[:, None, :]).sum(-1)
    w = sc.work.long()
    worst = _ratio(got[w], ref[w], bound[w].clamp(min=1e-300), f"sample_viewdirs {name}")
    print(f"sample_viewdirs {name}: worst error / bound = {worst:.3f} over {w.numel()} samples")
    rest = torch.ones(sc.S_cap + GUARD, dtype=torch.bool)
    rest[w] = False
    assert _all_nan(got[rest])
    # slot 0 decides, not the row: some sample's later neighbour carries another matrix
    pid = sc.query["pidx"][:sc.S].long()
    other = (pid[:, 1:] >= 0) & (rot[pid[:, 1:].clamp(min=0)] != rot[p0][:, None]).flatten(2).any(-1)
    assert bool(other.any())


# ---- 2. the rotated row and colour kernels through the C ABI ------------------------------------------------

@pytest.mark.parametrize("exact", [False, True], ids=["x3", "exact"])
@pytest.mark.parametrize("name", ["pairs", "pairs53", "rand3_41"])
def test_rotated_rows_and_colour(name, exact):
    """f_s, alpha_s, rgb against rw2c_ref's float64 chain at the chain bars of agg_rows_ref (capped at the fp32
    bar); blend / wnorm at check_slots' 32 u, and with the bits of the unrotated run (rule 1: the weights keep
    the unrotated offset)."""
    dv = rot_dev(name)
    sc, rot = planted(name)
    dv.sample_viewdirs()
    what = f"rotated {'exact' if exact else 'x3'} {name}"
    r = run(dv, exact)
    bars, o = rw.chain_bars(sc, weights()[0], rot)
    w = sc.work.long()
    idx = sc.rs * sc.K + sc.rk
    got = dict(fs=r["fs"], alpha=r["feat"][w, 0], rgb=r["feat"][w, 1:], blend=r["blend"][idx], wnorm=r["wnorm"][idx])
    ref = dict(fs=o["fs"], alpha=o["alpha"], rgb=o["rgb"], blend=o["rw"][:, 0], wnorm=o["rw"][:, 1])
    out = {k: round(_ratio(got[k], ref[k], bars[k], f"{what} {k}"), 3) for k in got}
    print(f"{what} worst ratios (chain bar):", out)
    check_slots(sc, r["blend"], r["wnorm"], o["rw"], what)
    check_feat_untouched(sc, r["feat"], r["feat0"], rgb_written=True)
    plain = run(dv, exact, rotated=False)
    assert _same_bits(r["blend"], plain["blend"]) and _same_bits(r["wnorm"], plain["wnorm"])
    # ... and the rotation is really applied: the unrotated run is far outside the bar
    assert float((plain["feat"][w, 1:].double() - o["rgb"]).abs().max()) > 100 * bars["rgb"]
    r2 = run(dv, exact)
    assert _same_bits(r["feat"], r2["feat"]) and _same_bits(r["fs"], r2["fs"])


# ---- 3. the reference's own rotated frames through HipRenderer -------------------------------------------

@functools.lru_cache(maxsize=None)
def golden():
    g = np.load(f"{GOLDEN_DIR}/reference_rw2c.npz", allow_pickle=False)
    pts = golden_points(g, "corner")
    _, mlp, _ = load_golden(str(g["mlp_from"]), "sparse32")
    near, far = (float(x) for x in g["view/near_far"])
    view = scene.View(g["view/campos"], g["view/camrotc2w"], g["view/raydir"], None, None, 0, 0, near, far)
    return g, pts, mlp, view


def case_rot(g, name):
    """The case's Rw2c as the caller passes it: [N,3,3], or [3,3] for rot_global."""
    pal = torch.from_numpy(g["palette"])
    if f"{name}/index" in g.files:
        return pal[torch.from_numpy(g[f"{name}/index"]).long()]
    return pal[int(g[f"{name}/global"])]


def renderer(pts, mlp, o, rot, exact=False):
    tab = PointTables(pts["xyz"], pts["embedding"], pts["color"], pts["dir"], pts["conf"], DEV, rot=rot)
    r = HipRenderer(tab, mlp, o, DEV)
    r.exact = exact
    return r


def frame(r, view):
    out = r.render(torch.from_numpy(view.campos), torch.from_numpy(view.camrotc2w), torch.from_numpy(view.raydir),
                   view.near, view.far, want_blend=True)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("prec", ["f32", "f16", "exact"])
@pytest.mark.parametrize("name", CASES)
def test_render_matches_reference_rw2c(name, prec):
    """As test_render_gpu.py::test_render_matches_reference_golden, with its TOL table, on the rotated cases."""
    g, pts, mlp, view = golden()
    o = _opts(prec, SR=int(g[f"{name}/SR"]), K=int(g[f"{name}/K"]))
    rgb_tol, feat_tol = TOL[prec]
    out = frame(renderer(pts, mlp, o, case_rot(g, name), exact=prec == "exact"), view)
    R = view.raydir.shape[0]
    np.testing.assert_array_equal(out.ray_mask.cpu().numpy(), g[f"{name}/ray_mask"])
    err = np.abs(out.rgb.cpu().numpy() - g[f"{name}/full_color"]).max()
    keep = g[f"{name}/ray_mask"].astype(bool)
    bgt = np.abs(out.bg_transmission.cpu().numpy()[keep] - g[f"{name}/bg_transmission"]).max()
    op = np.abs(out.opacity.cpu().numpy()[keep] - g[f"{name}/opacity"]).max()
    dense = _dense_feat(out, R, o.SR)[0]
    ref = g[f"{name}/decoded"]
    ferr = (np.abs(dense[keep] - ref) / np.maximum(1.0, np.abs(ref))).max()
    print(f"{name} [{prec}]: max |rgb - reference| = {err:.3e}, bg_transmission {bgt:.3e}, opacity {op:.3e}, "
          f"decoded / max(1, |ref|) {ferr:.3e}")
    assert err <= rgb_tol
    assert bgt <= rgb_tol
    assert op <= feat_tol
    assert ferr <= feat_tol


def test_render_f16_unsplit_block10(monkeypatch):
    """sgn_aggregate without the point projection (block1.0 computed per row in full): the rotated
    instantiation of that form of k_agg_rows, which the renderer itself never launches, at the f16 bars."""
    g, pts, mlp, view = golden()
    name = "rot_mixed"
    o = _opts("f16", SR=int(g[f"{name}/SR"]), K=int(g[f"{name}/K"]))
    lib, orig = L(), L().sgn_aggregate
    calls = []

    def unsplit(nl, dim, bp, proj, *rest):
        calls.append(proj is not None)
        return orig(nl, dim, bp, None, *rest)
    monkeypatch.setattr(lib, "sgn_aggregate", unsplit)
    out = frame(renderer(pts, mlp, o, case_rot(g, name)), view)
    assert calls == [True, True]
    rgb_tol, feat_tol = TOL["f16"]
    keep = g[f"{name}/ray_mask"].astype(bool)
    err = np.abs(out.rgb.cpu().numpy() - g[f"{name}/full_color"]).max()
    ref = g[f"{name}/decoded"]
    ferr = (np.abs(_dense_feat(out, view.raydir.shape[0], o.SR)[0][keep] - ref) / np.maximum(1.0, np.abs(ref))).max()
    print(f"{name} [f16, block1.0 unsplit]: max |rgb - reference| = {err:.3e}, decoded / max(1, |ref|) {ferr:.3e}")
    assert err <= rgb_tol and ferr <= feat_tol


# ---- 4. identity is the stock path; the two forms of one matrix agree ----------------------------------------

@pytest.mark.parametrize("prec", ["f32", "f16", "exact"])
def test_identity_and_global_forms_bitwise(prec):
    g, pts, mlp, view = golden()
    o = _opts(prec, SR=32, K=8)
    n = pts["xyz"].shape[0]

    def bits(rot):
        r = renderer(pts, mlp, o, rot, exact=prec == "exact")
        out = frame(r, view)
        S = out.query.n_samples()
        valid = out.query.samp_nnb[:S] > 0   # feat rows of samples without a neighbour are never written
        return r, (out.rgb.clone(), out.feat[:S][valid].clone(), out.opacity.clone())
    _, base = bits(None)
    for rot in (torch.eye(3), torch.eye(3).expand(n, 3, 3).contiguous()):
        r, got = bits(rot)
        assert r.points.rot is None
        for a, b in zip(got, base):
            assert _same_bits(a.cpu(), b.cpu())
    pal2 = torch.from_numpy(g["palette"])[2]
    _, one = bits(pal2)
    r, per = bits(pal2.expand(n, 3, 3).contiguous())
    assert r.points.rot is not None
    for a, b in zip(per, one):
        assert _same_bits(a.cpu(), b.cpu())
    assert not _same_bits(one[1].cpu(), base[1].cpu())


# ---- 5. one rotated frame twice (a miscounted vmcnt allowance shows as run-to-run differences) --------------

def test_rotated_frame_repeats_bitwise():
    g, pts, mlp, view = golden()
    r = renderer(pts, mlp, _opts("f32", SR=32, K=8), case_rot(g, "rot_mixed"))
    a = frame(r, view)
    S = a.query.n_samples()
    valid = a.query.samp_nnb[:S] > 0
    feat = a.feat[:S][valid].clone()
    assert int(valid.sum()) > 1000
    b = frame(r, view)
    assert b.query.n_samples() == S and _same_bits(b.feat[:S][valid].cpu(), feat.cpu())


# ---- 6. the plugin ------------------------------------------------------------------------------------------

def _inputs(view):
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    R = view.raydir.shape[0]
    return {"campos": d(view.campos)[None], "raydir": d(view.raydir)[None], "camrotc2w": d(view.camrotc2w)[None],
            "near": torch.tensor([[[view.near]]]), "far": torch.tensor([[[view.far]]]),
            "bg_color": torch.tensor([[1.0, 1.0, 1.0]], dtype=torch.float32, device=DEV),
            "pixel_idx": torch.zeros(1, R, 2, device=DEV), "h": 1, "w": R}


def test_plugin_editing_and_checkpoint(tmp_path):
    from sgnerf_amd.model import HipPointsVolumetricModel
    g, pts, mlp, view = golden()
    name = "rot_parts"
    opt = argparse.Namespace(SR=int(g[f"{name}/SR"]), K=int(g[f"{name}/K"]), gpu_ids=[0], is_train=False,
                             checkpoints_dir=str(tmp_path), name="scene", resume_dir=str(tmp_path / "scene"),
                             bg_color="white", default_conf=-1.0)
    m = HipPointsVolumetricModel()
    m.initialize(opt)
    m.editing_set_points(points_xyz=pts["xyz"], points_embedding=pts["embedding"], points_conf=pts["conf"],
                         points_dir=pts["dir"], points_color=pts["color"], Rw2c=case_rot(g, name), aggregator_state=mlp)
    m.set_input(_inputs(view))
    out1 = {k: v.clone() for k, v in m.test().items()}
    err = np.abs(out1["coarse_raycolor"][0].cpu().numpy() - g[f"{name}/full_color"]).max()
    print(f"plugin {name}: max |coarse_raycolor - reference| = {err:.3e}")
    assert err <= TOL["f32"][0]
    np.testing.assert_array_equal(out1["ray_mask"][0].cpu().numpy(), g[f"{name}/ray_mask"])
    m.save_networks("latest")
    m2 = HipPointsVolumetricModel()
    m2.initialize(opt)
    m2.load_networks("latest")
    assert m2.neural_points.Rw2c.shape == (pts["xyz"].shape[0], 3, 3)
    m2.set_input(_inputs(view))
    out2 = m2.test()
    for k in ("coarse_raycolor", "coarse_point_opacity", "ray_mask", "weight"):
        assert torch.equal(out1[k], out2[k]), k


def test_f32_range_fallback_with_rotation():
    """block1.2's weights x 30000 push the hidden activations past fp16's range (the trick of
    test_render_gpu.py::test_f32_fp16_range_falls_back_to_plain_fp32): the rotated frame is re-rendered by
    sgn_aggregate_exact, and equals a render that took the plain-fp32 path from the start within 1e-5."""
    g, pts, mlp, view = golden()
    big = dict(mlp)
    big["block1.2.weight"] = mlp["block1.2.weight"] * 30000.0
    o = _opts("f32", SR=32, K=8)
    rot = case_rot(g, "rot_mixed")
    r = renderer(pts, big, o, rot)
    out = frame(r, view)
    assert r.exact, "the frame did not leave the split path"
    S = out.query.n_samples()
    rgb, feat = out.rgb.cpu().double(), out.feat[:S].cpu().double()
    valid = out.query.samp_nnb[:S].cpu() > 0
    rx = renderer(pts, big, o, rot, exact=True)
    ox = frame(rx, view)
    assert bool(torch.isfinite(feat[valid]).all())
    fx = ox.feat[:S].cpu().double()
    ferr = float(((feat[valid] - fx[valid]).abs() / fx[valid].abs().clamp(min=1.0)).max())
    err = float((rgb - ox.rgb.cpu().double()).abs().max())
    print(f"range fallback with rotation: max |rgb - exact| = {err:.3e}, decoded / max(1, |ref|) {ferr:.3e}")
    assert err <= 1e-5 and ferr <= 1e-5
    # and the unrotated cloud lands elsewhere: the fallback did rotate
    o0 = frame(renderer(pts, big, o, None, exact=True), view)
    assert float((o0.rgb.cpu().double() - rgb).abs().max()) > 1e-3
