"""tests/agg_f16_render_ref.py proven without a GPU.

Layout: P's position map is a bijection of the 256 units, and not sgn_train_colmap(0).
Roundings off: in float64 with unrounded weights the three models are agg_rows_ref.proj_ref / colour_ref / chain
(given pers included) and rw2c_ref.chain for rotated points, to 1e-10.
Roundings on: the fp32 torch emulations of the three kernels pass every checker at the small counts.
Planted errors, on the emulations: each is caught.
Caps, for every case this file and test_agg_f16_render_gpu.py use: the colour bar below a tenth of what a swapped
fragment or a negated cos octave moves (a y1 packed toward zero moves no more than one flipped rounding does, 0.3 .. 1.8 x
the bar: the noisy-sample count holds it, see test_colour_bar_cap_and_plants), and agg_f16_ref's caps on every
interval E."""
import pytest
import torch

import sgnerf_amd  # noqa: F401
from sgnerf_amd.weights import init_mlp

import agg_f16_ref as fr
import agg_f16_render_ref as rr
import agg_rows_ref as ar
import rw2c_ref as rw

BAR = 1e-10
VARIANTS = [(0, 0), (1, 96), (1, 0)]
PROJ_N = [1, 31, 32, 33, 255, 256, 257]
COLOUR_ITEMS = [1, 31, 32, 33, 255, 256, 257, 300]
BIG = 65539


def state_of(variant=(0, 0)):
    return init_mlp(5, bias_std=0.1, bpnet_layers=variant[0], bpnet_dim=variant[1])


def _close(a, b, what):
    s, err = float(b.abs().max()), float((a - b).abs().max())
    assert err <= BAR * max(s, 1e-300), f"{what}: {err:.3e} over {s:.3e}"


# ---- layout ----------------------------------------------------------------------------------------
def test_proj_map_is_a_bijection_of_the_units():
    assert sorted(rr.PM.tolist()) == list(range(256))
    assert sorted(rr.proj_map(True).tolist()) == list(range(256)) and not torch.equal(rr.proj_map(True), rr.PM)
    # [t][h][r] -> 32 t + (r & 3) + 8 (r >> 2) + 4 h: the order pack_acc_order gives the biases, not the chained B order
    assert rr.PM[:4].tolist() == [0, 1, 2, 3] and rr.PM[4:8].tolist() == [8, 9, 10, 11] and rr.PM[16:20].tolist() == [4, 5, 6, 7]
    assert int(rr.PM[32 * 5 + 16 + 9]) == 32 * 5 + 1 + 16 + 4
    assert not torch.equal(rr.PM, fr.colmaps()[0])
    x = torch.randn(5, 256)
    assert torch.equal(fr.to_nat(fr.from_nat(x, rr.PM), rr.PM, 256), x.half().double())


# ---- roundings off -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [33, 257])
def test_proj_model_is_proj_ref(n):
    st = state_of()
    emb = ar.point_table(n, st)["embedding"]
    ref = ar.proj_ref(emb.double(), st) * 2.0 ** -ar.layer_shift(st["block1.0.weight"])
    _close(rr.proj_model(emb, fr.Net(st, exact=True), exact=True), ref, "P")


@pytest.mark.parametrize("rot", [False, True])
def test_colour_model_is_colour_ref(rot):
    st = state_of()
    c = ar.colour_case(257, True)
    v = rr.case_viewdirs(c, rw.palette_rot(ar.N_POINTS) if rot else None)[c.work.long()]
    _close(rr.colour_model(c.fs, v, rr.ColNet(st, exact=True), exact=True), ar.colour_ref(c.fs.double(), v, st), "rgb")
    if rot:     # case_viewdirs is rw2c_ref's rule 2, and not the plain ray
        pid = c.query["pidx"][c.work.long(), 0].long()
        ref = rw.mv(rw.palette_rot(ar.N_POINTS)[pid].double(), c.raydir[c.samp_ray[c.work.long()].long()].double())
        _close(v.double(), ref.float().double(), "v'")
        assert not torch.equal(v, c.v)


@pytest.mark.parametrize("variant", VARIANTS, ids=str)
@pytest.mark.parametrize("name,pers", [("pairs", False), ("rand4_300", False), ("rand8_300", True)])
def test_rows_model_is_the_float64_chain(name, pers, variant):
    sc, st = fr.scene(name), state_of(variant)
    p = sc.pers32() if pers else None
    net = fr.Net(st, exact=True)
    rows = rr.RRows(sc, bp16=sc.points["bpnet"] if variant == (1, 96) else None, pers=p, exact=True)
    o = rr.rows_model(rows, net, rr.proj_model(sc.points["embedding"], net, exact=True), exact=True)
    c = ar.chain(sc, st, pers=p)
    _close(o["fs"], c["fs"], "f_s")
    _close(o["alpha"], c["alpha"], "alpha_s")
    idx = 8 * sc.item + sc.rk
    _close(rows.wgt[idx], c["rw"][:, 0], "blend")
    _close(rows.wn[idx], c["rw"][:, 1], "wnorm")


def test_rotated_rows_model_is_rw2c_chain():
    sc, st = fr.scene("rand8_300"), state_of()
    rot = rw.palette_rot(sc.N)
    net = fr.Net(st, exact=True)
    rows = rr.RRows(sc, rot=rot, exact=True)
    o = rr.rows_model(rows, net, rr.proj_model(sc.points["embedding"], net, exact=True), exact=True)
    c = rw.chain(sc, st, rot)
    _close(o["fs"], c["fs"], "f_s")
    _close(o["alpha"], c["alpha"], "alpha_s")
    _close(rr.colour_model(c["fs"], c["v"], rr.ColNet(st, exact=True), exact=True), c["rgb"], "rgb")
    assert float((o["fs"] - ar.chain(sc, st)["fs"]).abs().max()) > 1e-3       # and the rotation matters


# ---- 1. k_point_proj: emulation, plant, caps ----------------------------------------------------------
def _proj_rep(n, st, tile=None, emb=None):
    emb = ar.point_table(n, st)["embedding"] if emb is None else emb
    rep = fr.Report()
    rr.check_proj(rep, "P", rr.proj_emu(emb, st) if tile is None else tile, emb, fr.Net(st))
    return rep


@pytest.mark.parametrize("n", PROJ_N + [1001, BIG])
def test_proj_emulation_passes_and_E_is_capped(n):
    """Every table size of the GPU test: the emulation inside its intervals, E under agg_f16_ref's cap."""
    rep = _proj_rep(n, state_of())
    rr.show_proj(rep, f"projection emulation n={n}")
    rep.assert_ok(f"n={n}")
    rep.check_caps(f"n={n}")


def test_proj_sg_blob_shares_w0a():
    a, b = state_of((0, 0)), state_of((1, 96))
    assert torch.equal(a["block1.0.weight"], b["block1.0.weight"]) and torch.equal(a["block1.0.bias"], b["block1.0.bias"])


def test_proj_plants_are_caught():
    st = state_of()
    emb = ar.point_table(257, st)["embedding"]
    assert _proj_rep(257, st, rr.proj_emu(emb, st, swap_h=True), emb).failed()[:1] == ["P"]
    t = rr.proj_emu(emb, st)
    t[100] = torch.roll(t[100], 16)                   # one point's fragments a half-tile off
    assert _proj_rep(257, st, t, emb).failed()[:1] == ["P"]
    t = rr.proj_emu(emb, st)
    t[-1] = float("nan")                              # the last point never stored
    assert _proj_rep(257, st, t, emb).failed()[:1] == ["P"]
    e2 = emb.clone()
    e2[7, 3] = -e2[7, 3]                              # a sign slip in one input
    assert _proj_rep(257, st, rr.proj_emu(e2, st), emb).failed()[:1] == ["P"]


# ---- 2. k_color: emulation, plants, the cap -------------------------------------------------------------
COLOUR_CASES = [(n, s, r) for n in COLOUR_ITEMS for s in (False, True) for r in (False, True)] + \
               [(BIG, False, False), (BIG, True, True)]


@pytest.mark.parametrize("items,shuffle,rot", COLOUR_CASES, ids=str)
def test_colour_bar_cap_and_plants(items, shuffle, rot):
    """Every colour case of the GPU test.  The emulation passes (the bar is 4 x its own distance, or more).  The chain
    bar is below a tenth of what a swapped fragment or a negated cos octave moves on the population the bar was measured
    on, and both are caught by it on every case of 31 samples or more (a single sample can sit where an octave's cos
    hardly matters: 2.2e-4 on the rotated one-sample case).  A y1 packed toward zero moves rgb by 1.1e-3 .. 2.3e-3 at
    most, the size of one flipped rounding and so of the floor itself (1e-4 .. 1e-3): no bar over a whole case can stay a
    tenth below it (bar / move 0.29 .. 1.75, printed), so it is held by the noisy-sample count instead, which must catch
    it on every case of 31 samples or more."""
    st = state_of()
    b = rr.colour_bar(items, shuffle, rot, st)
    c, v, bar, ref, emu, moves = b["case"], b["v"], b["bar"], b["ref"], b["emu"], b["moves"]
    fs16 = c.fs.half()
    out = {}
    for plant in (None,) + rr.COLOUR_PLANTS:
        rep = fr.Report()
        k, allowed = rr.check_colour(rep, "rgb", rr.colour_emu(fs16, v, st, plant), b)
        out[plant] = (rep.failed(), k)
    print(f"colour items={items} shuffled={shuffle} rotated={rot}: floor {b['floor']:.3e}, bar {bar:.3e}, planted "
          f"max |d rgb| " + ", ".join(f"{k} {m:.3e}" for k, m in moves.items()) + f"; bar / y1 rtz = {bar / moves['y1 rtz']:.4f}; "
          f"noisy samples allowed {allowed}; failed checks / noisy samples: {out}")
    assert bar >= 2e-6 * max(1.0, ar.amax(ref))
    assert bar < rr.COLOUR_CAP * min(moves["frag swap"], moves["cos neg"])
    assert out[None][0] == []
    if items >= 31:
        assert "rgb" in out["frag swap"][0] and "rgb" in out["cos neg"][0]
        assert "rgb noisy samples" in out["y1 rtz"][0]


# ---- 3. the split k_agg_rows: emulation, plants ---------------------------------------------------------
def _rows_case(name, variant, n=None, pers=False, rot=False):
    sc, st = fr.scene(name), state_of(variant)
    rows = rr.RRows(sc, n, bp16=sc.points["bpnet"].half() if variant == (1, 96) else None, pers=sc.pers32() if pers else None,
                    rot=rw.palette_rot(sc.N) if rot else None)
    return sc, st, rows, rr.proj_emu(sc.points["embedding"], st)


ROW_CASES = [(nm, v, None, False, False) for nm in fr.SMALL_SCENES for v in VARIANTS] + \
            [("rand8_300", (0, 0), n, False, False) for n in (1, 3, 4, 5, 31, 32, 33)] + \
            [("rand8_300", (0, 0), None, True, False), ("rand8_300", (0, 0), 33, False, True), ("rand8_300", (0, 0), None, False, True)]


@pytest.mark.parametrize("name,variant,n,pers,rot", ROW_CASES, ids=str)
def test_rows_emulation_passes(name, variant, n, pers, rot):
    sc, st, rows, tile = _rows_case(name, variant, n, pers, rot)
    b = rr.rows_bars(rows, st, tile)
    rep = fr.Report()
    rr.check_rows(rep, b, b["emu_fs"], b["emu_alpha"])
    K = sc.K
    blend, wnorm = (torch.full((sc.S_cap * K,), float("nan")) for _ in range(2))
    slot = (rows.samp[:, None] * K + torch.arange(K)[None, :]).reshape(-1)
    sel = (torch.arange(rows.n)[:, None] * 8 + torch.arange(K)[None, :]).reshape(-1)
    blend[slot], wnorm[slot] = rows.wgt32[sel], rows.wn[sel].float()
    rr.check_weights(rep, sc, rows, blend, wnorm)
    rep.show(f"rows emulation {name} {variant} n={n} pers={pers} rot={rot}")
    print(f"  f_s floor {b['floor_fs']:.3e} bar {b['bar_fs']:.3e} (max |f_s| {ar.amax(b['fs']):.3e}; unsplit interval bound E_fs "
          f"{b['Efs']:.3e}); alpha_s floor {b['floor_alpha']:.3e} bar {b['bar_alpha']:.3e} (max {ar.amax(b['alpha']):.3e}; "
          f"E_alpha {b['Ealpha']:.3e})")
    rep.assert_ok(name)
    assert len(rep.ratio) == 6


@pytest.mark.parametrize("variant", [(0, 0), (1, 96)], ids=str)
@pytest.mark.parametrize("plant", rr.ROW_PLANTS)
def test_rows_planted_error_is_caught(plant, variant):
    """On 35 items (two 32-item workgroup tiles, the second ragged with 3 items)."""
    sc, st, rows, tile = _rows_case("rand8_300", variant, 35)
    b = rr.rows_bars(rows, st, tile)
    fs, al = rr.rows_emu(rows.chunk(0, rows.n), st, tile, plant)
    rep = fr.Report()
    rr.check_rows(rep, b, fs, al)
    print(plant, "->", rep.fail)
    assert rep.failed(), f"{plant} passed"
    if plant == "ragged":
        assert rep.failed() == ["alpha_s", "f_s"]


def test_masked_slot_reads_point_0_with_weight_zero():
    """The reference's statement of load_proj's clamp: replacing P[0] changes nothing when no valid row names point 0
    (the weight of a masked slot is an exact zero), and does when one does."""
    sc, st = fr.scene("rand8_300"), state_of()
    rows = rr.RRows(sc)
    tile = rr.proj_emu(sc.points["embedding"], st)
    t2 = tile.clone()
    t2[0] = (torch.randn(256) * 3).half()
    c = rows.chunk(0, rows.n)
    names0 = (c.pid.view(-1, 8) == 0).any(1)
    assert int(names0.sum()) > 0 and int((~c.valid).sum()) > 0
    f1, a1 = rr.rows_emu(c, st, tile)
    f2, a2 = rr.rows_emu(c, st, t2)
    assert torch.equal(f1[~names0], f2[~names0]) and torch.equal(a1[~names0], a2[~names0])
    assert not torch.equal(f1[names0], f2[names0])
