"""The three f16 render kernels of csrc/mlp.hip -- k_point_proj (sgn_point_project), k_color<ROT> (sgn_aggregate,
stages = 2) and the split block1.0 form of k_agg_rows (sgn_aggregate with d_point_proj, stages = 1; the only form the
renderer launches) -- called directly through the C ABI and compared per element with the float64 references of
tests/agg_f16_render_ref.py (proven on the CPU in test_agg_f16_render_ref_cpu.py).

Cuts.  P is checked by interval from the embedding; the row kernel reads the table sgn_point_project itself wrote, so it
is cut at P and none of the projection's error enters; the colour stage runs alone on an f_s (and, rotated, a
samp_viewdir) the test writes.  Bars: agg_f16_render_ref.py's docstring.  Every output is pre-filled (NaN, 0xFF bytes, or
finite random values where the kernel must leave words alone) in exact-size buffers with GUARD rows behind them, which
must keep their bits; nothing out of range is probed.

Item counts are the smallest at which the kernels change path: a wave takes 32 points (projection) or 32 items
(colour), a workgroup 8 waves, the grid at most 256 workgroups -- 65539 = 256 x 8 x 32 + 3 is the persistent loops' second
trip with a ragged last tile; the row kernel's wave takes 4 items, its workgroup 32, 8195 = 256 x 32 + 3 is where the
prefetch of the next tile's P rows crosses into the second trip.  Counts below 300 run on the first n items of the
300-item scene.  Each test prints its worst error / bound ratio per output."""
import ctypes
import functools

import pytest
import torch

import sgnerf_amd  # noqa: F401
from sgnerf_amd import _lib
from sgnerf_amd.weights import init_mlp, pack_mlp

import agg_f16_ref as fr
import agg_f16_render_ref as rr
import agg_rows_ref as ar
import rw2c_ref as rw
from test_agg_rows_gpu import Dev
from test_train_rows_gpu import _all_nan, _same_bits

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
VARIANTS = [(0, 0), (1, 96), (1, 0)]
GUARD = 3
NAN = float("nan")
FILL = 255           # byte fill of the fp16 buffers: 0xFFFF is a NaN
PCHUNK = 8192        # points per float64 chunk of the projection check
BIG_PROJ = BIG_COLOUR = 256 * 8 * 32 + 3
BIG_ROWS = 256 * 32 + 3


def L():
    return _lib.lib()


def _id(v):
    return f"{v[0]}_{v[1]}" if isinstance(v, tuple) else None


@functools.lru_cache(maxsize=None)
def weights(variant=(0, 0)):
    """(state, the f16 blob, Net on the device)."""
    st = init_mlp(5, bias_std=0.1, bpnet_layers=variant[0], bpnet_dim=variant[1])
    return st, pack_mlp(st, DEV), fr.Net(st, DEV)


# ---- 1. k_point_proj -------------------------------------------------------------------------------------------------
def project(emb, variant=(0, 0), idx=None, count=None):
    """sgn_point_project over emb [n, 32] (device) into a 0xFF-filled exact-size table with guard rows: [n + GUARD, 256]
    fp16 in the kernel's layout."""
    n = emb.shape[0]
    assert int(L().sgn_point_proj_bytes(n)) == n * 512
    buf = torch.full(((n + GUARD) * 512,), FILL, dtype=torch.uint8, device=DEV)
    pt = _lib.PointTables()
    pt.xyz = pt.embedding = pt.color = pt.dir = pt.conf = emb.data_ptr()      # only the embedding is read
    pt.n_points = n
    cnt = None if count is None else torch.tensor([count], dtype=torch.int64, device=DEV)
    _lib.check(L().sgn_point_project(ctypes.byref(pt), _lib.ptr(weights(variant)[1]), _lib.ptr(idx), _lib.ptr(cnt), _lib.ptr(buf),
                                     _lib.stream_handle()), "sgn_point_project")
    torch.cuda.synchronize()
    return buf.view(torch.float16).view(n + GUARD, 256)


def check_table(rep, tile, emb, rows=None):
    """The rows `rows` (default: all) of a table against the interval reference, in chunks on the device."""
    net = weights()[2]
    rows = torch.arange(emb.shape[0], device=DEV) if rows is None else rows.to(DEV)
    for i0 in range(0, rows.numel(), PCHUNK):
        r = rows[i0:i0 + PCHUNK]
        rr.check_proj(rep, "P", tile[r], emb[r], net)


PROJ_CASES = [(n, (0, 0)) for n in (1, 31, 32, 33, 255, 256, 257, BIG_PROJ)] + [(33, (1, 96)), (257, (1, 96))]


@pytest.mark.parametrize("n,variant", PROJ_CASES, ids=_id)
def test_point_project(n, variant):
    """Every element of P inside its interval; the guard rows keep their bytes; a second run gives the same bits.  The SG
    blob holds W0a at other offsets (block2_bpnet's sections follow it) and must give the base blob's bits."""
    emb = ar.point_table(n, weights()[0])["embedding"].contiguous().to(DEV)
    tile = project(emb, variant)
    assert bool((tile[n:].view(torch.uint8) == FILL).all()), "a guard row was written"
    rep = fr.Report()
    check_table(rep, tile[:n], emb)
    rr.show_proj(rep, f"point_project n={n} {variant}")
    rep.assert_ok(f"point_project n={n} {variant}")
    rep.check_caps(f"point_project n={n}")
    assert torch.equal(project(emb, variant).view(torch.int16), tile.view(torch.int16))
    if variant != (0, 0):
        assert torch.equal(project(emb, (0, 0)).view(torch.int16), tile.view(torch.int16))
    del tile, emb
    if n > 10000:
        torch.cuda.empty_cache()


def test_point_project_list():
    """n = 1001, a shuffled strict subset of half the points, *d_count below the list's length: the counted entries'
    rows pass the interval check, every other row and the guard rows keep their fill; count 0 writes nothing."""
    n = 1001
    emb = ar.point_table(n, weights()[0])["embedding"].contiguous().to(DEV)
    g = torch.Generator().manual_seed(n)
    lst = torch.randperm(n, generator=g)[:n // 2].to(torch.int32)
    count = lst.numel() - 37
    tile = project(emb, idx=lst.to(DEV), count=count)
    listed = torch.zeros(n + GUARD, dtype=torch.bool)
    listed[lst[:count].long()] = True
    assert 0 < int(listed.sum()) == count < lst.numel() < n
    assert bool((tile[~listed.to(DEV)].view(torch.uint8) == FILL).all()), "a row outside the counted list was written"
    rep = fr.Report()
    check_table(rep, tile, emb, lst[:count].long())
    rr.show_proj(rep, "point_project list")
    rep.assert_ok("point_project list")
    full = project(emb)
    assert torch.equal(tile[listed.to(DEV)].view(torch.int16), full[listed.to(DEV)].view(torch.int16))
    assert bool((project(emb, idx=lst.to(DEV), count=0).view(torch.uint8) == FILL).all())


# ---- 2. k_color<false> / k_color<true> -------------------------------------------------------------------------------
class ColDev:
    """A ColourCase on the device: the tables k_color reads (counters, work, samp_ray, raydir / samp_viewdir), dummies
    for the rest, a full-size workspace whose first rows hold fp16(f_s)."""

    def __init__(self, c, rot):
        self.case = c
        up = lambda t: t.contiguous().to(DEV)  # noqa: E731
        self.viewdir = rr.case_viewdirs(c, rw.palette_rot(ar.N_POINTS) if rot else None)       # [S_cap, 3] fp32
        work = torch.cat([c.work, torch.full((c.S_cap - c.items,), -1, dtype=torch.int32)])
        self.d = d = dict(raydir=up(c.raydir), samp_ray=up(c.samp_ray), work=up(work),
                          counters=up(torch.tensor([c.S, c.items, 0, 0], dtype=torch.int32)),
                          nowork=up(torch.tensor([c.S, 0, 0, 0], dtype=torch.int32)),
                          f=torch.zeros(64, device=DEV), i=torch.zeros(c.S_cap * 8 + 64, dtype=torch.int32, device=DEV))
        pt = self.pt = _lib.PointTables()
        pt.xyz = pt.embedding = pt.color = pt.dir = pt.conf = pt.campos = pt.camrotc2w = d["f"].data_ptr()   # not read by stage 2
        pt.n_points = 1
        pt.raydir = d["raydir"].data_ptr()
        if rot:
            d["rot9"] = up(rw.palette_rot(ar.N_POINTS).reshape(-1, 9))
            d["viewdir"] = up(torch.cat([self.viewdir, torch.zeros(GUARD, 3)]))
            pt.n_points, pt.rot, pt.samp_viewdir = ar.N_POINTS, d["rot9"].data_ptr(), d["viewdir"].data_ptr()
        qo = self.qo = _lib.QueryOut()
        qo.ray_ns = qo.ray_soff = qo.samp_d = qo.samp_nnb = qo.pidx = d["i"].data_ptr()
        qo.samp_locw = d["f"].data_ptr()
        qo.samp_ray, qo.work, qo.counters = d["samp_ray"].data_ptr(), d["work"].data_ptr(), d["counters"].data_ptr()
        self.nb = int(L().sgn_aggregate_workspace_bytes(c.S_cap))
        assert self.nb == max(c.S_cap, 32) * 512
        self.ws = torch.full((self.nb + 512 * GUARD,), FILL, dtype=torch.uint8, device=DEV)
        self.ws[:c.items * 512].view(torch.float16).view(c.items, 256).copy_(c.fs.half())

    def run(self, counters="counters"):
        c = self.case
        self.qo.counters = self.d[counters].data_ptr()
        feat = torch.cat([c.feat0, torch.full((GUARD, 4), NAN)]).to(DEV)
        ws0 = self.ws.clone()
        _lib.check(L().sgn_aggregate(0, 0, None, None, ctypes.byref(self.pt), ctypes.byref(self.qo), c.S_cap, 8,
                                     _lib.ptr(weights()[1]), _lib.ptr(feat), None, None, _lib.ptr(self.ws), self.nb, 2,
                                     _lib.stream_handle()), "sgn_aggregate stages 2")
        torch.cuda.synchronize()
        assert torch.equal(self.ws, ws0), "the colour stage wrote into the workspace"
        return feat.cpu()


COLOUR_ITEMS = [1, 31, 32, 33, 255, 256, 257, 300, BIG_COLOUR]


@pytest.mark.parametrize("rot", [False, True], ids=["plain", "rotated"])
@pytest.mark.parametrize("shuffle", [False, True], ids=["ordered", "shuffled"])
@pytest.mark.parametrize("items", COLOUR_ITEMS)
def test_colour_stage(items, shuffle, rot):
    """rgb of the listed samples within the chain bar and the noisy-sample count; feat[:, 0], the samples outside the
    list and the rows past S keep their bits; two runs give the same bits; counters[1] = 0 writes nothing."""
    c = ar.colour_case(items, shuffle)
    cd = ColDev(c, rot)
    st = weights()[0]
    w = c.work.long()
    v = cd.viewdir[w]
    assert rot != torch.equal(v, c.v)
    b = rr.colour_bar(items, shuffle, rot, st, DEV)
    bar, ref, emu = b["bar"], b["ref"], b["emu"]
    assert torch.equal(b["v"], v)
    feat = cd.run()
    feat0 = torch.cat([c.feat0, torch.full((GUARD, 4), NAN)])
    listed = torch.zeros(c.S_cap + GUARD, dtype=torch.bool)
    listed[w] = True
    assert _same_bits(feat[:, 0], feat0[:, 0]) and _same_bits(feat[~listed], feat0[~listed])
    rep = fr.Report()
    k, allowed = rr.check_colour(rep, "rgb", feat[w, 1:], b)
    what = f"colour items={items} {'shuffled' if shuffle else 'ordered'} {'rotated' if rot else 'plain'}"
    rep.show(what)
    print(f"{what}: floor {b['floor']:.3e} (the case alone {ar.amax(emu.double() - ref):.3e}), bar {bar:.3e}, worst error "
          f"{ar.amax(feat[w, 1:].double() - ref):.3e}; noisy samples {k} (emulation {rr.noisy(emu, ref)}, allowed {allowed}) of {items}")
    rep.assert_ok(what)
    assert _same_bits(cd.run(), feat)
    assert _same_bits(cd.run("nowork"), feat0)
    del cd
    if items > 10000:
        torch.cuda.empty_cache()


# ---- 3. the split k_agg_rows -------------------------------------------------------------------------------------------
class RDev(Dev):
    """test_agg_rows_gpu.Dev with, optionally, a palette Rw2c per point and the samples' rotated view directions written
    from rw2c_ref.sample_viewdirs, and a pidx table in which no row names point 0."""

    def __init__(self, sc, pers=False, rot=False, no_p0=False):
        super().__init__(sc, pers)
        self.rot = self.vdir = None
        if rot:
            self.rot = rw.palette_rot(sc.N)
            self.vdir = rw.sample_viewdirs(sc, self.rot).float()                                  # [S, 3]
            self.d["rot9"] = self.rot.reshape(sc.N, 9).contiguous().to(DEV)
            self.d["viewdir"] = torch.cat([self.vdir, torch.zeros(sc.S_cap + GUARD - sc.S, 3)]).to(DEV)
            self.pt.rot, self.pt.samp_viewdir = self.d["rot9"].data_ptr(), self.d["viewdir"].data_ptr()
        if no_p0:
            p = sc.query["pidx"].clone()
            p[p == 0] = 1
            self.d["pidx"] = p.contiguous().to(DEV)
            self.qo.pidx = self.d["pidx"].data_ptr()


@functools.lru_cache(maxsize=None)
def dev(name, pers=False, rot=False):
    return RDev(fr.scene(name), pers, rot)


@functools.lru_cache(maxsize=None)
def bp16(name):
    """sgn_bpnet_pack's fp16 table of the scene's BPNet rows."""
    dv = dev(name)
    out = torch.full((dv.sc.N, 96), NAN, dtype=torch.float16, device=DEV)
    _lib.check(L().sgn_bpnet_pack(_lib.ptr(dv.d["bpnet"]), dv.sc.N, 96, _lib.ptr(out), _lib.stream_handle()), "sgn_bpnet_pack")
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), dv.sc.points["bpnet"].half())
    return out


def table(dv, variant):
    """P of the scene's points, as sgn_point_project wrote it (test_point_project holds it to its intervals)."""
    return project(dv.d["emb"], variant)


def run_agg(dv, variant, n, stages, proj, name=None, ws_items=None, into=None):
    """sgn_aggregate over S_capacity = n into exact-size pre-filled buffers (into: the buffers of an earlier call).
    ws_items: a workspace of that many items instead of max(n, 32)."""
    sc = dv.sc
    items = max(n if ws_items is None else ws_items, 32)
    nb = int(L().sgn_aggregate_workspace_bytes(items))
    assert nb == items * 512
    if into is None:
        feat0 = torch.randn(sc.S_cap + GUARD, 4, generator=torch.Generator().manual_seed(3 + sc.S_cap))
        nK = sc.S_cap * sc.K
        into = dict(feat0=feat0, feat=feat0.to(DEV), ws=torch.full((nb + 512 * GUARD,), FILL, dtype=torch.uint8, device=DEV),
                    blend=torch.full((nK + GUARD,), NAN, device=DEV), wnorm=torch.full((nK + GUARD,), NAN, device=DEV), nb=nb, n=n)
    t = into
    assert t["nb"] == nb
    bp = _lib.ptr(bp16(name)) if variant[1] else None
    _lib.check(L().sgn_aggregate(variant[0], variant[1], bp, _lib.ptr(proj), ctypes.byref(dv.pt), ctypes.byref(dv.qo), n, sc.K,
                                 _lib.ptr(weights(variant)[1]), _lib.ptr(t["feat"]), _lib.ptr(t["blend"]), _lib.ptr(t["wnorm"]),
                                 _lib.ptr(t["ws"]), nb, stages, _lib.stream_handle()), "sgn_aggregate")
    torch.cuda.synchronize()
    return t


def fs_of(t):
    return t["ws"][:t["nb"]].view(torch.float16).view(-1, 256)


def check_untouched(sc, t, n, rgb_written=False):
    """f_s rows of items >= n and the workspace's guard bytes, feat[:, 1:], samples outside the list, guard rows."""
    fs = fs_of(t)
    assert bool((fs[n:].view(torch.uint8) == FILL).all()), "an f_s row of an item >= n was written"
    assert bool((t["ws"][t["nb"]:] == FILL).all()), "workspace guard bytes written"
    feat, feat0 = t["feat"].cpu(), t["feat0"]
    mine = torch.zeros(feat.shape[0], dtype=torch.bool)
    mine[sc.work[:n].long()] = True
    assert _same_bits(feat[~mine], feat0[~mine]), "a sample outside the list was written"
    if not rgb_written:
        assert _same_bits(feat[:, 1:], feat0[:, 1:])
    nK = sc.S_cap * sc.K
    assert _all_nan(t["blend"][nK:]) and _all_nan(t["wnorm"][nK:])


def check_rows_run(name, variant, n=None, pers=False, rot=False):
    dv = dev(name, pers, rot)
    sc = dv.sc
    n = sc.items if n is None else n
    st = weights(variant)[0]
    what = f"rows {name}[:{n}] {variant}{' pers' if pers else ''}{' rotated' if rot else ''}"
    proj = table(dv, variant)
    t = run_agg(dv, variant, n, 1, proj, name)
    check_untouched(sc, t, n)
    rows = rr.RRows(sc, n, bp16=bp16(name) if variant == (1, 96) else None, pers=dv.pers if pers else None, rot=dv.rot, vdir=dv.vdir)
    b = rr.rows_bars(rows, st, proj[:sc.N], DEV)
    rep = fr.Report()
    rr.check_rows(rep, b, fs_of(t)[:n], t["feat"][sc.work[:n].long().to(DEV), 0])
    rr.check_weights(rep, sc, rows, t["blend"][:sc.S_cap * sc.K].cpu(), t["wnorm"][:sc.S_cap * sc.K].cpu())
    rep.show(what)
    print(f"{what}: f_s floor {b['floor_fs']:.3e} bar {b['bar_fs']:.3e} (max |f_s| {ar.amax(b['fs']):.3e}; the unsplit kernel's interval "
          f"bound E_fs {b['Efs']:.3e}); alpha_s floor {b['floor_alpha']:.3e} bar {b['bar_alpha']:.3e} (max {ar.amax(b['alpha']):.3e}; "
          f"E_alpha {b['Ealpha']:.3e})")
    rep.assert_ok(what)
    t2 = run_agg(dv, variant, n, 1, proj, name)                          # a second run: the same bits
    for k in ("feat", "ws", "blend", "wnorm"):
        assert _same_bits(t[k].cpu(), t2[k].cpu()), f"{what}: {k} differs between two runs"
    return t


@pytest.mark.parametrize("variant", VARIANTS, ids=_id)
@pytest.mark.parametrize("name", fr.SMALL_SCENES)
def test_rows(name, variant):
    """K = 8 in order and shuffled, K = 4 with empty samples interleaved (shuffled), K = 1, the pairing lists."""
    check_rows_run(name, variant)


ROW_COUNTS = [(n, (0, 0)) for n in (1, 3, 4, 5, 31, 32, 33)] + [(n, v) for n in (5, 33) for v in VARIANTS[1:]]


@pytest.mark.parametrize("n,variant", ROW_COUNTS, ids=_id)
def test_rows_item_counts(n, variant):
    """S_capacity = n below the work count: waves without an item, ragged tiles, one and two workgroups."""
    check_rows_run("rand8_300", variant, n)


@pytest.mark.parametrize("variant", VARIANTS, ids=_id)
def test_rows_second_trip(variant):
    """8195 items: 256 workgroups x 32 + 3 -- three workgroups' pnext prefetch names a tile of the second trip, the
    others' must be skipped; the last tile is ragged."""
    assert fr.scene("rand3_8195").items == BIG_ROWS
    check_rows_run("rand3_8195", variant)
    torch.cuda.empty_cache()


def test_rows_given_pers():
    """pt->pers / samp_pers given: the camera-space dists are single fp32 operations on the caller's values."""
    check_rows_run("rand8_300", (0, 0), pers=True)


@pytest.mark.parametrize("n", [33, 300])
def test_rows_rotated(n):
    """k_agg_rows<SP, false, true>: per-point Rw2c on the world offset and the point direction, the sample's rotated view
    direction (written by the test); blend / wnorm keep the unrotated run's bits (the weights read the unrotated offset)."""
    t = check_rows_run("rand8_300", (0, 0), n, rot=True)
    dv = dev("rand8_300")
    plain = run_agg(dv, (0, 0), n, 1, table(dv, (0, 0)), "rand8_300")
    assert _same_bits(t["blend"].cpu(), plain["blend"].cpu()) and _same_bits(t["wnorm"].cpu(), plain["wnorm"].cpu())
    assert not _same_bits(fs_of(t)[:n].cpu(), fs_of(plain)[:n].cpu())


@pytest.mark.parametrize("variant,rot", [((0, 0), False), ((1, 96), False), ((0, 0), True)], ids=_id)
def test_chunked_stages3_equals_stages_1_then_2(variant, rot):
    """stages = 3 into a 32-item workspace launches both kernels per chunk of 32 items (item0 = 32, 64, ...; every chunk's
    f_s rows at the workspace's start): feat, blend and wnorm equal, bit for bit, stages = 1 then stages = 2 into a full
    workspace."""
    name = "rand8_300"
    dv = dev(name, False, rot)
    sc = dv.sc
    proj = table(dv, variant)
    full = run_agg(dv, variant, sc.S_cap, 1, proj, name)
    alpha_only = full["feat"].clone()
    run_agg(dv, variant, sc.S_cap, 2, proj, name, into=full)
    check_untouched(sc, full, sc.items, rgb_written=True)
    w = sc.work.long().to(DEV)
    assert _same_bits(full["feat"][:, 0].cpu(), alpha_only[:, 0].cpu()) and not _same_bits(full["feat"][w, 1:].cpu(), alpha_only[w, 1:].cpu())
    part = run_agg(dv, variant, sc.S_cap, 3, proj, name, ws_items=32)
    assert bool((part["ws"][part["nb"]:] == FILL).all()), "workspace guard bytes written"
    for k in ("feat", "blend", "wnorm"):
        assert _same_bits(full[k].cpu(), part[k].cpu()), k
    both = run_agg(dv, variant, sc.S_cap, 3, proj, name)
    for k in ("feat", "blend", "wnorm", "ws"):
        assert _same_bits(full[k].cpu(), both[k].cpu()), k


def test_masked_slots_read_p0_with_weight_zero():
    """A masked slot (k >= the sample's neighbour count) runs the whole chain on P[0] (load_proj clamps its index) and
    must enter the blend with a weight of exactly 0: with no valid row naming point 0, other finite values in P[0]
    change no output bit.  P[0] must be FINITE -- 0 x inf is a NaN -- which is why sgn_frame_points always lists point 0."""
    name = "rand8_300"
    sc = fr.scene(name)
    dv = RDev(sc, no_p0=True)
    assert int((sc.query["samp_nnb"][sc.work.long()] < sc.K).sum()) > 0 and not bool((dv.d["pidx"] == 0).any())
    proj = table(dv, (0, 0))
    a = run_agg(dv, (0, 0), sc.S_cap, 3, proj, name)
    p2 = proj.clone()
    p2[0] = (torch.randn(256, generator=torch.Generator().manual_seed(1)) * 3).half().to(DEV)
    assert not torch.equal(p2[0], proj[0]) and bool(torch.isfinite(p2[0]).all())
    b = run_agg(dv, (0, 0), sc.S_cap, 3, p2, name)
    for k in ("feat", "blend", "wnorm", "ws"):
        assert _same_bits(a[k].cpu(), b[k].cpu()), k
