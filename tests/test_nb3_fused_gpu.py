"""The viewmlp without block3 on the fused split-fp16 row kernel (opts.rows_fused = 1) on the GPU: the projection
and aggregate entries (sgn_point_project_f32_nb3, sgn_aggregate_f32_nb3: k_point_proj16, k_pair_slots, k_rows16
without block3, k_color16) called directly on the named scenes of tests/agg_rows_ref.py, then HipRenderer and the
model plugin against the reference's own outputs (tests/golden/reference_nb3.npz) and the plain-fp32 renderer.

The reference is tests/nb3_ref.py's float64 restatement on init_mlp(..., block3_layers=0) weights.  The bar is the
project's: max(1e-5, 4 x floor) x max(1, |ref|) per element, the floor measured as the same restatement in torch
fp32 on the GPU against the CPU, printed with the measured worst case per output (profiles/nb3_fused_tests.txt)."""
import argparse
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sgnerf_amd  # noqa: F401
from sgnerf_amd import _lib
from sgnerf_amd.model import HipPointsVolumetricModel
from sgnerf_amd.render import HipRenderer
from sgnerf_amd.weights import init_mlp, pack_mlp

import agg_rows_ref as ar
import nb3_ref as nb
from test_agg_rows_gpu import Dev, flag_of, fs_of
from test_api_gpu import _inputs
from test_nb3_gpu import _check_frame, _opts, _render, _tables, golden
from test_nb3_rows_gpu import _frame
from test_train_rows_gpu import _all_nan, _same_bits

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32_TOL = 1e-5
GUARD = 3
NAN = float("nan")
VARIANTS = [(0, 0), (1, 0), (1, 96)]
# One-pass capacity of the row launch: 256 workgroups x WG16_SAMPLES NS = 16 halves at NS = 2 (base, block2_bpnet on
# 352 inputs), 512 workgroups x 8 halves at NS = 1 (block2_bpnet on 256 inputs): 4096 halves either way, so
# full4099 (4099 samples of 8 neighbours, one per half) is the wrap case: three workgroups walk a second tile
P_ROWS = 4096
SCENES = ["none", "one", "pairs", "pairs_hi", "pairs_shuf", "pairs53", "pairs75", "full15", "full16", "full17", "rand1_777",
          "rand5_777", "rand8_300", "full%d" % (P_ROWS + 3)]
assert all(n in ar._SCENES for n in SCENES)
KEYS = ("feat", "blend", "wnorm")


def L():
    return _lib.lib()


def _id(v):
    return f"{v[0]}_{v[1]}" if isinstance(v, tuple) else None


@functools.lru_cache(maxsize=None)
def weights(variant=(0, 0)):
    st = init_mlp(7, bias_std=0.1, bpnet_layers=variant[0], bpnet_dim=variant[1], block3_layers=0)
    return st, pack_mlp(st, DEV, "fused", block3_layers=0)


@functools.lru_cache(maxsize=None)
def reference(name, variant=(0, 0)):
    """The float64 restatement of a scene, the fp32 floors and the bars, computed once and shared."""
    sc = ar.scene(name)
    st = weights(variant)[0]
    with torch.no_grad():
        o = nb.chain(sc, st)
    fl = nb.floor(sc, st, DEV)
    return o, fl, {k: max(F32_TOL, 4.0 * v) for k, v in fl.items()}


@functools.lru_cache(maxsize=None)
def dev(name, null_tables=True, garbage=False):
    """A scene on the device; colour and dir NULL, or present and filled with NaN (colour) and 1e30 (dir)."""
    sc = ar.scene(name)
    if garbage:
        keep = sc.points
        try:
            sc.points = dict(keep, color=torch.full_like(keep["color"], NAN), dir=torch.full_like(keep["dir"], 1e30))
            dv = Dev(sc)
        finally:
            sc.points = keep
    else:
        dv = Dev(sc)
    if null_tables:
        dv.pt.color = dv.pt.dir = None
    return dv


def project(pt, n, packed, idx=None):
    """sgn_point_project_f32_nb3 into a NaN-filled buffer with guard floats after it: the whole buffer (fp32)."""
    nbytes = int(L().sgn_point_proj_bytes_f32(n))
    buf = torch.full((nbytes // 4 + 16 * GUARD,), NAN, device=DEV)
    cnt = None if idx is None else torch.tensor([idx.numel()], dtype=torch.int64, device=DEV)
    _lib.check(L().sgn_point_project_f32_nb3(ctypes.byref(pt), _lib.ptr(packed), _lib.ptr(idx), _lib.ptr(cnt), _lib.ptr(buf),
                                             _lib.stream_handle()), "sgn_point_project_f32_nb3")
    torch.cuda.synchronize()
    assert _all_nan(buf[nbytes // 4:])
    return buf


def run(name, variant=(0, 0), stages=(3,), ws_items=None, null_tables=True, garbage=False):
    """sgn_aggregate_f32_nb3 on a scene (one call per entry of `stages`): feat, blend, wnorm (CPU, with guard rows),
    f_s of a full workspace, the range flag."""
    dv = dev(name, null_tables, garbage)
    sc = dv.sc
    _, packed = weights(variant)
    key = ("nb3", packed.data_ptr())
    if key not in dv._proj:
        dv._proj[key] = project(dv.pt, sc.N, packed)
    n = sc.S_cap * sc.K
    blend, wnorm = (torch.full((n + GUARD,), NAN, device=DEV) for _ in range(2))
    feat0 = torch.randn(sc.S_cap + GUARD, 4, generator=torch.Generator().manual_seed(3 + sc.S_cap))
    feat = feat0.to(DEV)
    nbytes = int(L().sgn_aggregate_workspace_bytes_f32(sc.S_cap if ws_items is None else ws_items))
    ws = torch.full((nbytes + 1024 * GUARD,), 255, dtype=torch.uint8, device=DEV)
    for st in stages:
        _lib.check(L().sgn_aggregate_f32_nb3(variant[0], variant[1], dv.bp(variant), _lib.ptr(dv._proj[key]), ctypes.byref(dv.pt),
                                             ctypes.byref(dv.qo), sc.S_cap, sc.K, _lib.ptr(packed), _lib.ptr(feat), _lib.ptr(blend),
                                             _lib.ptr(wnorm), _lib.ptr(ws), nbytes, st, _lib.stream_handle()),
                   "sgn_aggregate_f32_nb3")
    torch.cuda.synchronize()
    assert bool((ws[nbytes:] == 255).all()), "the workspace was written past its size"
    fs = fs_of(ws[:nbytes], sc.S_cap)[:sc.items].cpu() if ws_items is None else None
    return dict(feat=feat.cpu(), feat0=feat0, blend=blend.cpu(), wnorm=wnorm.cpu(), fs=fs, flag=flag_of(ws[:nbytes]))


def check(name, variant, r, what):
    """alpha, rgb, f_s, blend and wnorm at the bar; every word the kernels must not write keeps its bits."""
    sc = ar.scene(name)
    o, fl, bar = reference(name, variant)
    work, idx, n = sc.work.long(), sc.rs * sc.K + sc.rk, sc.S_cap * sc.K
    err = dict(alpha=nb.rel(r["feat"][work, 0], o["alpha"]), rgb=nb.rel(r["feat"][work, 1:], o["rgb"]),
               blend=nb.rel(r["blend"][idx], o["rw"][:, 0]), wnorm=nb.rel(r["wnorm"][idx], o["rw"][:, 1]))
    if r["fs"] is not None:
        err["fs"] = nb.rel(r["fs"], o["fs"])
    print(f"{what}: fp32 floor (torch GPU vs CPU) " + ", ".join(f"{k} {v:.2e}" for k, v in fl.items()) +
          "; max error / max(1, |ref|) " + ", ".join(f"{k} {v:.2e}" for k, v in err.items()))
    assert err["alpha"] <= bar["alpha"] and err["rgb"] <= bar["rgb"]
    assert err["blend"] <= bar["rw"] and err["wnorm"] <= bar["rw"]
    assert err.get("fs", 0.0) <= bar["fs"]
    assert r["flag"] == 0
    # samples without a neighbour, slack samples, guard rows; empty slots read 0
    is_item = torch.zeros(sc.S_cap + GUARD, dtype=torch.bool)
    is_item[work] = True
    assert _same_bits(r["feat"][~is_item], r["feat0"][~is_item])
    assert _all_nan(r["blend"][n:]) and _all_nan(r["wnorm"][n:])
    valid = torch.zeros(n, dtype=torch.bool)
    valid[idx] = True
    assert bool((r["blend"][:n][~valid] == 0).all()) and bool((r["wnorm"][:n][~valid] == 0).all())


# ---- 1. the projection entry -----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 127, 128, 129])
def test_point_project(n):
    """1, 127, 128 and 129 points (a tile is 128 points), every point and through an index list, colour and dir
    NULL: P against float64, the record's xyz and conf bit for bit."""
    st, packed = weights()
    tab = ar.point_table(n, st)
    d = {k: tab[k].contiguous().to(DEV) for k in ("xyz", "embedding", "conf")}
    pt = _lib.PointTables()
    for k, t in d.items():
        setattr(pt, k, t.data_ptr())
    pt.n_points = n
    buf = project(pt, n, packed).cpu()
    P, rec = buf[:n * 256].view(n, 256), buf[n * 256:n * 272].view(n, 16)
    assert _same_bits(rec[:, :4], torch.cat([tab["xyz"], tab["conf"]], dim=1))
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(n)).to(torch.int32).to(DEV)
    assert _same_bits(project(pt, n, packed, perm).cpu(), buf)          # the list call over a permutation

    def p_of(emb, state):
        w, b = state["block1.0.weight"].to(emb), state["block1.0.bias"].to(emb)
        return F.linear(torch.cat([emb, nb.pe(emb, 3)], dim=-1), w[:, :224], b)
    ref = p_of(tab["embedding"].double(), st)
    floor = nb.rel(p_of(d["embedding"], {k: v.to(DEV) for k, v in st.items()}).cpu(), p_of(tab["embedding"], st))
    got = P.double() * 2.0 ** -ar.layer_shift(st["block1.0.weight"])
    err = nb.rel(got, ref)
    print(f"projection n={n}: fp32 floor {floor:.2e}; max error / max(1, |ref|) P {err:.2e} (max |P| {float(ref.abs().max()):.2e})")
    assert err <= max(F32_TOL, 4.0 * floor)


# ---- 2. the aggregate entry on the named scenes ----------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_entry_base(name, monkeypatch):
    """Pairing of every kind, K 1 / 5 / 8, tiles of 15, 16 and 17 halves, the wrap case; a second run and a run with
    SGN_PAIR=0 give the same bits."""
    r = run(name)
    check(name, (0, 0), r, f"fused {name}")
    r2 = run(name)
    assert all(_same_bits(r[k], r2[k]) for k in KEYS + ("fs",))
    monkeypatch.setenv("SGN_PAIR", "0")
    r3 = run(name)
    assert all(_same_bits(r[k], r3[k]) for k in KEYS + ("fs",)), "SGN_PAIR=0"


# ---- 3. block2_bpnet.0 as the transposed last layer ------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS[1:], ids=_id)
@pytest.mark.parametrize("name", ["pairs", "rand8_300", "full17"])
def test_entry_bpnet(name, variant):
    check(name, variant, run(name, variant), f"fused {name} {variant}")


# ---- 4. chunked workspaces -------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS, ids=_id)
@pytest.mark.parametrize("ws_items", [8, 3])
def test_entry_chunked_workspace(variant, ws_items):
    """A workspace sized for 8 and for 3 items.  sgn_aggregate_workspace_bytes_f32 clamps both to 32 items (this
    entry's minimum, as sgn_aggregate_f32's), which hold full17's 22 samples in ONE chunk: these cases only show
    that a clamped workspace gives the full one's bits.  Chunking itself is test_entry_three_chunks below."""
    full = run("full17", variant)
    part = run("full17", variant, ws_items=ws_items)
    check("full17", variant, part, f"fused full17 {variant} workspace of {ws_items} items")
    assert all(_same_bits(full[k], part[k]) for k in KEYS)


@pytest.mark.parametrize("variant", VARIANTS, ids=_id)
def test_entry_three_chunks(variant):
    """pairs75 on a 32-item workspace: three chunks, each paired on its own; the stages alone are refused there."""
    sc = ar.scene("pairs75")
    assert sc.items == 75 and sc.S_cap > 75
    full = run("pairs75", variant)
    part = run("pairs75", variant, ws_items=32)
    check("pairs75", variant, part, f"fused pairs75 {variant} workspace of 32 items")
    assert all(_same_bits(full[k], part[k]) for k in KEYS)
    for st in (1, 2):
        with pytest.raises(_lib.SgnError, match="stages 1 and 2 called separately"):
            run("pairs75", variant, stages=(st,), ws_items=32)


# ---- 5. the stages called separately ---------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS, ids=_id)
def test_stages_separately(variant):
    both = run("pairs75", variant)
    split = run("pairs75", variant, stages=(1, 2))
    assert all(_same_bits(both[k], split[k]) for k in KEYS + ("fs",))
    rows_only = run("pairs75", variant, stages=(1,))
    assert _same_bits(rows_only["feat"][:, 1:], rows_only["feat0"][:, 1:])      # the colour words are stage 2's
    assert _same_bits(rows_only["feat"][:, 0], both["feat"][:, 0])


# ---- 6. colour and dir are not read ----------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS, ids=_id)
def test_entry_does_not_read_colour_and_dir(variant):
    """With the tables present, NaN in colour and 1e30 in dir: the same bits as with NULL."""
    a = run("rand8_300", variant)
    b = run("rand8_300", variant, null_tables=False, garbage=True)
    assert all(_same_bits(a[k], b[k]) for k in KEYS + ("fs",)) and b["flag"] == 0


# ---- 7. the renderer against the reference's outputs -----------------------------------------------------
def _fused_renderer(name, **kw):
    return HipRenderer(_tables(name, kw.pop("colour", False)), golden(name)[1], _opts(name, **kw), DEV, rows_fused=1)


@pytest.mark.parametrize("name", ["base", "bp256", "bp352"])
def test_renderer_matches_reference(name):
    """HipRenderer(rows_fused=1): ray_mask and the neighbour indices bit-exact, RGB and the decoded features within
    1e-5 of the reference's; both blobs packed, the renderer off the plain-fp32 path, the flag 0; rendered twice
    bitwise equal."""
    r = _fused_renderer(name)
    assert r.fused and not r.exact and r.packed is not None and r.packed_exact is not None and r.rows is None
    _, out = _render(name, r, want_blend=True)
    assert not r.exact and r._fused_frame and r._proj is not None and r._fp is not None
    assert int(r._ws_flag().item()) == 0
    _check_frame(name, out, "HipRenderer (rows_fused)")
    first = _frame(out)
    _, out2 = _render(name, r, want_blend=True)
    assert all(_same_bits(a, b) for a, b in zip(first, _frame(out2)))


def test_renderer_weights_blend_and_depth_match_plain_fp32():
    name = "base"
    _, plain = _render(name, want_weights=True, want_blend=True, want_depth=True)
    ref = {k: getattr(plain, k).clone() for k in ("wnorm", "blendw", "blend", "depth", "opacity", "rgb")}
    r = _fused_renderer(name)
    _, out = _render(name, r, want_weights=True, want_blend=True, want_depth=True)
    assert not r.exact and r._fused_frame
    S = int(out.query.counters[0])
    K = int(golden(name)[2]["K"])
    err = {}
    for k, v in ref.items():
        a, b = getattr(out, k), v
        if k in ("wnorm", "blend"):
            a, b = a.reshape(-1)[:S * K], b.reshape(-1)[:S * K]
        err[k] = nb.rel(a.cpu(), b.cpu())
    print("HipRenderer (rows_fused) against the plain-fp32 renderer: " + ", ".join(f"{k} {v:.2e}" for k, v in err.items()))
    assert all(v <= F32_TOL for v in err.values())
    assert float(ref["wnorm"].abs().max()) > 0 and float(ref["depth"].max()) > 0


def test_rotated_points_and_early_stop():
    """A non-identity Rw2c: the option is accepted and the frame is the plain-fp32 renderer's, bit for bit.
    early_stop = 0.01: accepted, the frame rendered in full on the fused kernel -- the frame without it, bit for bit."""
    _, plain = _render("rot", want_blend=True)
    want = _frame(plain)
    r = _fused_renderer("rot")
    _, out = _render("rot", r, want_blend=True)
    assert r.fused and not r._fused_frame and not r.exact and not r._pending
    assert all(_same_bits(a, b) for a, b in zip(want, _frame(out)))
    _, full = _render("base", _fused_renderer("base"))
    want = _frame(full, blend=False)
    es = _fused_renderer("base", early_stop=1e-2)
    _, oe = _render("base", es)
    assert es._fused_frame and not es.exact and oe.stop_slot is None and oe.skipped is None
    assert all(_same_bits(a, b) for a, b in zip(want, _frame(oe, blend=False)))


def test_refusals_on_construction():
    from dataclasses import replace
    st = golden("base")[1]
    with pytest.raises(NotImplementedError, match="rows_fused"):
        HipRenderer(_tables("base"), init_mlp(0), replace(_opts("base"), shading_feature_mlp_layer3=2), DEV, rows_fused=1)
    with pytest.raises(NotImplementedError, match="rows_fused"):
        HipRenderer(_tables("base"), st, replace(_opts("base"), K=16), DEV, rows_fused=1)
    with pytest.raises(NotImplementedError, match="rows_fused"):
        HipRenderer(_tables("base"), st, _opts("base"), DEV, rows_fused=1, rows_gemm=1)


# ---- 8. the range guard ----------------------------------------------------------------------------------
def _big():
    """block1.2 scaled by 4e5: its activations leave fp16 range (an out-of-range input, not a fault)."""
    st = golden("base")[1]
    big = dict(st)
    big["block1.2.weight"] = st["block1.2.weight"] * 4.0e5
    big["block1.2.bias"] = st["block1.2.bias"] * 4.0e5
    return big


def test_range_guard_falls_back_to_plain_fp32():
    name, big = "base", _big()
    plain = HipRenderer(_tables(name), big, _opts(name), DEV)
    _, po = _render(name, plain, want_blend=True)
    want = _frame(po)
    r = HipRenderer(_tables(name), big, _opts(name), DEV, rows_fused=1)
    assert not r.exact
    _, out = _render(name, r, want_blend=True, check_range="sync")
    assert r.exact and r._fused_frame       # the frame ran fused, was flagged and re-rendered
    assert all(_same_bits(a, b) for a, b in zip(want, _frame(out)))
    _, out2 = _render(name, r, want_blend=True)       # later frames go there directly
    assert r.exact and not r._fused_frame and all(_same_bits(a, b) for a, b in zip(want, _frame(out2)))
    # without the check the renderer keeps its path
    r2 = HipRenderer(_tables(name), big, _opts(name), DEV, rows_fused=1)
    _render(name, r2, check_range=False)
    assert not r2.exact and int(r2._ws_flag().item()) == 1


def test_deferred_range_check():
    """"deferred" raises at the next frame, and at finish(); an in-range frame leaves the flag 0 and raises nothing."""
    name, big = "base", _big()
    r = HipRenderer(_tables(name), big, _opts(name), DEV, rows_fused=1)
    _render(name, r, check_range="deferred")
    with pytest.raises(_lib.SgnError, match="fp16 range"):
        _render(name, r, check_range="deferred")
    assert r.exact
    r = HipRenderer(_tables(name), big, _opts(name), DEV, rows_fused=1)
    _render(name, r, check_range="deferred")
    with pytest.raises(_lib.SgnError, match="fp16 range"):
        r.finish()
    assert r.exact
    ok = _fused_renderer(name)
    _render(name, ok, check_range="deferred")
    _render(name, ok, check_range="deferred")
    ok.finish()
    assert not ok.exact and int(ok._ws_flag().item()) == 0


# ---- 9. the plugin ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["base", "bp256", "bp352"])
def test_model_test_matches_reference(name, tmp_path):
    """The plugin with rows_fused = 1 in the driver's namespace."""
    pts, st, c = golden(name)
    nl, dim = nb.VARIANT[name]
    n = pts["xyz"].shape[0]
    sd = {"neural_points.xyz": torch.from_numpy(pts["xyz"]), "neural_points.points_embeding": torch.from_numpy(pts["embedding"])[None],
          "neural_points.points_conf": torch.from_numpy(pts["conf"]).reshape(1, n, 1)}
    if dim:
        sd["neural_points.bpnet_points_embedding"] = torch.from_numpy(pts["bpnet"])[None]
        sd["neural_points.points_label"] = torch.zeros(n, 1, dtype=torch.int32)
    sd.update({"aggregator." + k: v for k, v in st.items()})
    (tmp_path / "scene").mkdir()
    torch.save(sd, tmp_path / "scene" / "5_net_ray_marching.pth")
    opt = argparse.Namespace(SR=int(c["SR"]), K=int(c["K"]), gpu_ids=[0], is_train=False, checkpoints_dir=str(tmp_path),
                             name="scene", bg_color="white", shading_feature_mlp_layer3=0,
                             shading_feature_mlp_layer2_bpnet=nl, predict_semantic=1 if dim else 0,
                             semantic_guidance=1 if dim else 0, rows_fused=1)
    m = HipPointsVolumetricModel()
    m.initialize(opt)
    assert m.opts.rows_fused == 1
    m.load_networks(5)
    inp = _inputs(c)
    if dim:
        inp["pixel_label"] = torch.zeros(1, c["raydir"].shape[0], 1, dtype=torch.int32, device=DEV)
    m.set_input(inp)
    out = m.test()
    r = m.net_ray_marching.renderer
    assert r.fused and r._fused_frame and not r.exact
    np.testing.assert_array_equal(out["ray_mask"][0].cpu().numpy(), c["ray_mask"])
    err = float(np.abs(out["coarse_raycolor"][0].cpu().numpy() - c["full_color"]).max())
    keep = c["ray_mask"].astype(bool)
    werr = float(np.abs(out["weight"][0].cpu().numpy()[keep] - c["weight"]).max())
    cerr = float(np.abs(out["conf_coefficient"][0].cpu().numpy()[keep] - c["conf_coefficient"]).max())
    print(f"model.test() rows_fused {name}: max |rgb - reference| = {err:.3e}, weight {werr:.3e}, conf_coefficient {cerr:.3e}")
    assert err <= F32_TOL and werr <= F32_TOL and cerr <= F32_TOL


def test_plugin_trains_and_tests_on_the_fused_path(tmp_path):
    """train_rows = 1 beside rows_fused = 1: the plugin sets up (the trainer's options carry rows_fused = 0), steps,
    and test() still renders on the fused kernel, with the stepped weights."""
    from test_train_nb3_gpu import batch, state_for
    pts, v = batch()
    ns = dict(SR=24, K=8, gpu_ids=[0], is_train=True, checkpoints_dir=str(tmp_path), name="scene", lr=5e-4, plr=2e-3,
              lr_decay_exp=0.1, lr_decay_iters=1_000_000, bg_color="white", shading_feature_mlp_layer3=0)
    inputs = {"campos": v["campos"][None].to(DEV), "raydir": v["raydir"][None].to(DEV), "camrotc2w": v["rot"][None].to(DEV),
              "near": torch.tensor([[[v["near"]]]]), "far": torch.tensor([[[v["far"]]]]), "gt_image": v["gt"][None].to(DEV)}
    opt = argparse.Namespace(**ns, train_rows=1, rows_fused=1)
    m = HipPointsVolumetricModel()
    m.initialize(opt)
    assert m.opts.train_rows == 1 and m.opts.rows_fused == 1 and m.opts.is_train == 0
    m.set_points(points_xyz=pts["xyz"], points_embedding=pts["embedding"][None], points_color=pts["color"][None],
                 points_dir=pts["dir"][None], points_conf=pts["conf"][None], aggregator_state=state_for("base"))
    m.setup(opt)
    m.init_scheduler(0, opt)
    assert m.trainer.opts.is_train == 1 and m.trainer.opts.rows_fused == 0 and m.trainer.opts.rows_gemm == 0
    m.set_input(inputs)
    before = m.test()["coarse_raycolor"].clone()
    r = m.net_ray_marching.renderer
    assert r.fused and r._fused_frame and not r.exact
    for step in range(2):
        parts = m.optimize_parameters(total_steps=step)
    assert bool(torch.isfinite(parts["total"]))
    after = m.test()["coarse_raycolor"].clone()
    r = m.net_ray_marching.renderer
    assert r.fused and r._fused_frame and not r.exact and not torch.equal(after, before)
