"""The fp32-faithful aggregator's kernels -- k_point_proj16, k_pair_slots, k_rows16 (save and render
instantiations), k_color16 (csrc/mlp_x3.hip) and k_rows_exact / k_color_exact (csrc/exact.hip) -- called
directly through the C ABI on the hand-built scenes of tests/agg_rows_ref.py and compared per element with
that module's float64 references (proven on the CPU in test_agg_rows_ref_cpu.py).

The chain of four 256-wide layers is cut wherever the library exposes a tensor: P (the projection buffer), z1 /
z2 / zb / z3 (the save mode), f_s (the workspace), the colour stage alone (stages = 2 on an f_s the test
writes).  Each layer is compared with a float64 evaluation of that ONE layer on the input the kernel itself
produced, so a failure names a layer and the bound does not grow along the chain.

Bounds (agg_rows_ref.py; u = 2^-24), per element:
  local bar   2e-6 x the reference tensor's max for one split-path layer (the bar DESIGN 4.1 holds sgn_x3_gemm's
              three-product mode to), plus the error of inputs the kernel computes itself: PE at 2e-6 (2e-6 + 2^f E
              for the camera-space dists), carried by sum |w| over those columns only; f_s: block3.2's bar through
              the blend plus (2 9 + 32) u sum |terms|
  chain bar   max(2e-6 max |ref|, 4 x the fp32 floor) where no cut exists: z3 -> alpha_s (block3.2 and the alpha
              dot), f_s -> rgb, the caller-given pers coordinates, the plain-fp32 kernels
  caps        every bound on alpha_s / rgb / blend / wnorm < 1e-5 max(1, max |ref|), on P / z / f_s < 1e-5 max |ref|
Every output is pre-filled (NaN, or random bits where the kernel must leave finite values alone) and has guard
rows; lists are built in torch.  Each test prints its worst error / bound ratios."""
import ctypes
import functools
import time

import pytest
import torch

import sgnerf_amd  # noqa: F401
from sgnerf_amd import _lib
from sgnerf_amd.weights import init_mlp, pack_mlp

import agg_rows_ref as ar
import train_rows_ref as rr
from test_train_rows_gpu import _all_nan, _bits, _ratio, _same_bits

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
U = ar.U
GUARD = 3
NAN = float("nan")
# One-pass capacities of the launches (grid-stride loops wrap past them; each wrap case is the capacity + 3):
#   k_point_proj16  sgn_point_project_f32: min(tiles, 256) workgroups x 16 NW16 = 128 points
#   k_rows16        aggregate_f32: wmax workgroups x WG16_SAMPLES NS halves = 512 x 8 (save) = 256 x 16 (render)
#   k_color16       aggregate_f32: wcmax = 256 workgroups x 16 NWC = 128 items
#   k_rows_exact    sgn_aggregate_exact: 2048 workgroups x 2 NW = 8 items
P_PROJ, P_ROWS, P_COLOUR, P_EXACT = 32768, 4096, 32768, 16384
assert "full%d" % (P_ROWS + 3) in ar._SCENES and "rand1_%d" % (P_EXACT + 3) in ar._SCENES     # the wrap scenes, by name
VARIANTS = [(0, 0), (1, 96), (1, 0)]
# k_rows16's render instantiation (NS = 2) sums every row's dot products, the K-blend and alpha in the order of the
# save instantiation (NS = 1): found bit-identical on the MI355X, asserted from then on
RENDER_EQUALS_SAVE = True
T0 = time.time()


def L():
    return _lib.lib()


def _id(v):
    return f"{v[0]}_{v[1]}" if isinstance(v, tuple) else None


@functools.lru_cache(maxsize=None)
def weights(variant=(0, 0), kind="base", scene="rand8_300"):
    """(state, blob of the split path, blob of the plain-fp32 path) of a weight set."""
    st = init_mlp(5, bias_std=0.1, bpnet_layers=variant[0], bpnet_dim=variant[1])
    if kind == "big":      # one entry 1000 x the rest: the layer's shift leaves the small weights few low bits
        st["block1.0.weight"] = st["block1.0.weight"].clone()
        st["block1.0.weight"][7, 3] *= 1000.0
    elif kind == "zero":   # layer_shift returns 0 for an all-zero layer: P = b0 exactly
        st["block1.0.weight"] = torch.zeros_like(st["block1.0.weight"])
    elif kind == "inside":
        st, _ = ar.range_state(ar.scene(scene), st, 4.2e4)
    elif kind == "outside":
        st, _ = ar.range_state(ar.scene(scene), st, 2.5e5)
    return st, pack_mlp(st, DEV, "f32"), pack_mlp(st, DEV, "exact")


class Dev:
    """A scene's tensors on the device with hand-built PointTables / QueryOut."""

    def __init__(self, sc, pers=False):
        self.sc = sc
        up = lambda t: t.contiguous().to(DEV)  # noqa: E731
        P, q = sc.points, sc.query
        pad = lambda t: torch.cat([t.to(torch.int32), torch.full((sc.S_cap - t.numel(),), -1, dtype=torch.int32)])  # noqa: E731
        d = self.d = dict(xyz=up(P["xyz"]), emb=up(P["embedding"]), color=up(P["color"]), dir=up(P["dir"]), conf=up(P["conf"]),
                          bpnet=up(P["bpnet"]), campos=up(sc.camera[0]), rot=up(sc.camera[1]), raydir=up(sc.raydir),
                          samp_ray=up(q["samp_ray"]), samp_locw=up(q["samp_locw"]), samp_nnb=up(q["samp_nnb"]),
                          pidx=up(q["pidx"]), counters=up(q["counters"]), work=up(pad(sc.work)), row_off=up(pad(sc.row_off)),
                          none=torch.zeros(4, dtype=torch.int32, device=DEV))
        pt = self.pt = _lib.PointTables()
        pt.xyz, pt.embedding, pt.color, pt.dir, pt.conf = (d[k].data_ptr() for k in ("xyz", "emb", "color", "dir", "conf"))
        pt.n_points = sc.N
        pt.campos, pt.camrotc2w, pt.raydir = d["campos"].data_ptr(), d["rot"].data_ptr(), d["raydir"].data_ptr()
        if pers:
            self.pers = sc.pers32()
            d["pers"], d["samp_pers"] = up(self.pers[0]), up(self.pers[1])
            pt.pers, pt.samp_pers = d["pers"].data_ptr(), d["samp_pers"].data_ptr()
        qo = self.qo = _lib.QueryOut()
        qo.ray_ns = qo.ray_soff = qo.samp_d = d["none"].data_ptr()   # not read by these kernels
        for k in ("samp_ray", "samp_nnb", "pidx", "work", "counters", "samp_locw"):
            setattr(qo, k, d[k].data_ptr())
        self._proj = {}

    def bp(self, variant):
        return _lib.ptr(self.d["bpnet"]) if variant[1] else None

    def proj(self, packed):
        """The projection buffer of a weight blob (sgn_point_project_f32 over every point), cached."""
        key = packed.data_ptr()
        if key not in self._proj:
            self._proj[key] = project(self.pt, self.sc.N, packed)
        return self._proj[key]


@functools.lru_cache(maxsize=None)
def dev(name, pers=False):
    return Dev(ar.scene(name), pers)


def project(pt, n, packed, idx=None):
    """sgn_point_project_f32 into a NaN-filled buffer with guard floats after it: the whole buffer (fp32)."""
    nb = int(L().sgn_point_proj_bytes_f32(n))
    assert nb == n * (1024 + 64)
    buf = torch.full((nb // 4 + 16 * GUARD,), NAN, device=DEV)
    cnt = None if idx is None else torch.tensor([idx.numel()], dtype=torch.int64, device=DEV)
    _lib.check(L().sgn_point_project_f32(ctypes.byref(pt), _lib.ptr(packed), _lib.ptr(idx), _lib.ptr(cnt), _lib.ptr(buf),
                                         _lib.stream_handle()), "sgn_point_project_f32")
    torch.cuda.synchronize()
    assert _all_nan(buf[nb // 4:])
    return buf


def split_proj(buf, n):
    return buf[:n * 256].view(n, 256), buf[n * 256:n * 272].view(n, 16)


def new_ws(S_cap, items=None):
    """An aggregate workspace for `items` (default: every) work items, every byte 0xFF (NaN as fp32)."""
    nb = int(L().sgn_aggregate_workspace_bytes_f32(S_cap if items is None else items))
    return torch.full((nb,), 255, dtype=torch.uint8, device=DEV)


def fs_of(ws, S_cap):
    """The f_s rows of a full workspace, [max(S_cap, 32), 256] fp32."""
    assert int(L().sgn_aggregate_fs_offset_f32(ws.numel(), S_cap)) == 0
    n = max(S_cap, 32)
    return ws[:n * 1024].view(torch.float32).view(n, 256)


def slots_of(ws, S_cap):
    """k_pair_slots' entries in a full workspace (after the f_s rows and the row table; the count is the tail's
    first word): sorted (A item, nA, B item or -1, nB)."""
    n = max(S_cap, 32)
    cnt = int(ws[n * 1072:n * 1072 + 4].view(torch.int32).item())
    e = ws[n * 1056:n * 1056 + 16 * cnt].view(torch.int32).view(cnt, 4).cpu()
    out = []
    for a, b, _, _ in e.tolist():
        nb = (b >> 28) & 15
        out.append((a & 0x0FFFFFFF, (a >> 28) & 15, (b & 0x0FFFFFFF) if nb else -1, nb))
    return sorted(out)


def flag_of(ws):
    off = int(L().sgn_aggregate_flag_offset_f32(ws.numel()))
    return int(ws[off:off + 4].view(torch.int32).item())


def feat0_of(sc, salt=3):
    return torch.randn(sc.S_cap + GUARD, 4, generator=torch.Generator().manual_seed(salt + sc.S_cap))


def run_save(name, variant=(0, 0), compact=False):
    """sgn_aggregate_train_fwd_f32 on a scene: feat, z1, z2, zb, z3 (CPU) and f_s."""
    dv = dev(name)
    sc = dv.sc
    _, packed, _ = weights(variant)
    nrow = (sc.rows if compact else sc.S_cap * sc.K) + GUARD
    z = [torch.full((nrow, 256), NAN, device=DEV) for _ in range(4)]
    feat0 = feat0_of(sc)
    feat = feat0.to(DEV)
    ws = new_ws(sc.S_cap)
    _lib.check(L().sgn_aggregate_train_fwd_f32(variant[0], variant[1], dv.bp(variant), _lib.ptr(dv.proj(packed)), ctypes.byref(dv.pt),
                                               ctypes.byref(dv.qo), sc.S_cap, sc.K, _lib.ptr(packed), _lib.ptr(feat), _lib.ptr(z[0]),
                                               _lib.ptr(z[1]), _lib.ptr(z[2]) if variant[0] else None, _lib.ptr(z[3]),
                                               _lib.ptr(dv.d["row_off"]) if compact else None, _lib.ptr(ws), ws.numel(),
                                               _lib.stream_handle()), "sgn_aggregate_train_fwd_f32")
    torch.cuda.synchronize()
    return dict(feat=feat.cpu(), feat0=feat0, z1=z[0].cpu(), z2=z[1].cpu(), zb=z[2].cpu(), z3=z[3].cpu(), fs=fs_of(ws, sc.S_cap).cpu())


@functools.lru_cache(maxsize=None)
def saved(name, variant=(0, 0)):
    """The save-mode run (NULL row_off) that the render-mode tests compare with."""
    return run_save(name, variant)


def run_render(name, variant=(0, 0), stages=1, pers=False, kind="base", ws_items=None, exact=False, ws_bytes=None):
    """sgn_aggregate_f32 (or sgn_aggregate_exact): feat, blend, wnorm (CPU), the workspace, the return code."""
    dv = dev(name, pers)
    sc = dv.sc
    _, packed, packed_x = weights(variant, kind)
    n = sc.S_cap * sc.K
    blend, wnorm = (torch.full((n + GUARD,), NAN, device=DEV) for _ in range(2))
    feat0 = feat0_of(sc)
    feat = feat0.to(DEV)
    if exact:
        ws = torch.full(((sc.S_cap + GUARD) * 1024,), 255, dtype=torch.uint8, device=DEV)
        rc = L().sgn_aggregate_exact(variant[0], variant[1], dv.bp(variant), ctypes.byref(dv.pt), ctypes.byref(dv.qo), sc.S_cap, sc.K,
                                     _lib.ptr(packed_x), _lib.ptr(feat), _lib.ptr(blend), _lib.ptr(wnorm), _lib.ptr(ws),
                                     sc.S_cap * 1024 if ws_bytes is None else ws_bytes, _lib.stream_handle())
    else:
        ws = new_ws(sc.S_cap, ws_items)
        rc = L().sgn_aggregate_f32(variant[0], variant[1], dv.bp(variant), _lib.ptr(dv.proj(packed)), ctypes.byref(dv.pt),
                                   ctypes.byref(dv.qo), sc.S_cap, sc.K, _lib.ptr(packed), _lib.ptr(feat), _lib.ptr(blend),
                                   _lib.ptr(wnorm), _lib.ptr(ws), ws.numel(), stages, _lib.stream_handle())
    torch.cuda.synchronize()
    return dict(feat=feat.cpu(), feat0=feat0, blend=blend.cpu(), wnorm=wnorm.cpu(), ws=ws, rc=rc)


def _ok(r, what):
    _lib.check(r["rc"], what)
    return r


def check_feat_untouched(sc, feat, feat0, rgb_written):
    """feat.x of the work items (and rgb if the colour stage ran) is the kernel's; every other word keeps its bits."""
    is_item = torch.zeros(sc.S_cap + GUARD, dtype=torch.bool)
    is_item[sc.work.long()] = True
    assert _same_bits(feat[~is_item], feat0[~is_item])     # samples without a neighbour, slack samples, guard rows
    if not rgb_written:
        assert _same_bits(feat[:, 1:], feat0[:, 1:])


def check_slots(sc, blend, wnorm, rw, what):
    """blend / wnorm per element against rw at 32 u |ref|; exactly 0 on every invalid slot; sum_k wnorm = 1."""
    n = sc.S_cap * sc.K
    assert _all_nan(blend[n:]) and _all_nan(wnorm[n:])
    idx = sc.rs * sc.K + sc.rk
    valid = torch.zeros(n, dtype=torch.bool)
    valid[idx] = True
    assert bool((blend[:n][~valid] == 0).all()) and bool((wnorm[:n][~valid] == 0).all())
    for got, ref, nm in ((blend, rw[:, 0], "blend"), (wnorm, rw[:, 1], "wnorm")):
        b = 32 * U * ref.abs()
        ar.capped(b, ref, nm, unit=True)
        _ratio(got[idx], ref, b.clamp(min=1e-300), f"{what} {nm}")
    tot = wnorm[:n].view(sc.S_cap, sc.K).double().sum(1)[sc.work.long()]
    assert float((tot - 1).abs().max()) <= 16 * U if sc.items else True


def check_chain(sc, st, got, what, pers=None):
    """alpha_s, rgb, f_s, blend, wnorm (those given in `got`) against the float64 chain at the chain bar."""
    bars, o = ar.chain_bars(sc, st, pers=pers)
    idx = sc.rs * sc.K + sc.rk
    ref = dict(alpha=o["alpha"], rgb=o["rgb"], fs=o["fs"], blend=o["rw"][:, 0], wnorm=o["rw"][:, 1])
    out = {}
    for k, t in got.items():
        t = t[idx] if k in ("blend", "wnorm") else t
        out[k] = round(_ratio(t, ref[k], bars[k], f"{what} {k}"), 3)
    print(f"{what} worst ratios (chain bar):", out)
    return o


# ---- a. sgn_point_project_f32 ----------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["base", "big", "zero"])
@pytest.mark.parametrize("n", [1, 127, 128, 129, P_PROJ + 3, "scene"])
def test_point_project(n, kind):
    if n == "scene":       # the table the row tests read: their z1 check starts from this P
        tab, n = ar.scene("rand8_300").points, ar.N_POINTS
    else:
        tab = ar.point_table(n, weights()[0])
    st, packed, _ = weights((0, 0), kind)
    d = {k: tab[k].contiguous().to(DEV) for k in ("xyz", "embedding", "color", "dir", "conf")}
    pt = _lib.PointTables()
    for k, t in d.items():
        setattr(pt, k, t.data_ptr())
    pt.n_points = n
    buf = project(pt, n, packed).cpu()
    P, rec = split_proj(buf, n)
    # the 64-B record, bit for bit: [xyz, conf | colour, 0 | dir, 0 | 0 0 0 0]
    z1, z4 = torch.zeros(n, 1), torch.zeros(n, 4)
    assert _same_bits(rec, torch.cat([tab["xyz"], tab["conf"], tab["color"], z1, tab["dir"], z1, z4], dim=1))
    g = torch.Generator().manual_seed(n)
    perm = torch.randperm(n, generator=g).to(torch.int32).to(DEV)
    assert _same_bits(project(pt, n, packed, perm).cpu(), buf)          # the list call over a permutation
    if kind == "zero":
        assert ar.layer_shift(st["block1.0.weight"]) == 0
        assert _same_bits(P, st["block1.0.bias"][None, :].expand(n, 256))
        return
    ref = ar.proj_ref(tab["embedding"].double(), st)
    b = ar.bound_P(ref, st)
    ar.capped(b, ref, "P")
    _ratio(P, ref, b, f"P (n={n}, {kind} weights, shift {ar.layer_shift(st['block1.0.weight'])})")


# ---- b. the save mode: k_pair_slots + k_rows16<.., SAVE, NS = 1> ------------------------------------

SAVE_SCENES = ["none", "one", "pairs", "pairs_hi", "pairs_shuf", "pairs53", "full7", "full8", "full9", "full15", "full16", "full17",
               "rand1_777", "rand3_777", "rand5_777", "full4099", "rand8_300"]
SG_SCENES = ["pairs", "pairs_hi", "rand8_300"]
SAVE_CASES = [(n, (0, 0)) for n in SAVE_SCENES] + [(n, v) for n in SG_SCENES for v in VARIANTS[1:]]


def _check_save(name, variant, compact, r):
    """One save-mode run against the one-layer references, each fed with the kernel's own previous output."""
    sc, (st, packed, _) = ar.scene(name), weights(variant)
    dv = dev(name)
    what = f"save {name} {variant}{' compact' if compact else ''}"
    rows, items, K = sc.rows, sc.items, sc.K
    idx = torch.arange(rows) if compact else sc.rs * K + sc.rk
    keep = torch.zeros(r["z1"].shape[0], dtype=torch.bool)
    keep[idx] = True
    names = ["z1", "z2", "z3"] + (["zb"] if variant[0] else [])
    for k in names:
        assert _all_nan(r[k][~keep]), f"{what}: {k} wrote a row without a neighbour / a guard row"
    if not variant[0]:
        assert _all_nan(r["zb"])
    z = {k: r[k][idx] for k in names}
    P = sc.points
    worst = {}
    # z1 from the kernel's P (test_point_project) and the dists: the world part one fp32 subtraction (the kernel's own
    # argument, exact), the camera-space part in float64
    Pk, _ = split_proj(dv.proj(packed).cpu(), sc.N)
    d64 = rr.row_dists(P, sc.camera, sc.query, K)
    dk = torch.cat([(P["xyz"][sc.pid] - sc.query["samp_locw"][sc.rs]).double(), d64[:, 3:]], dim=1)
    ref = ar.z1_ref(Pk[sc.pid].double(), dk, st)
    b = ar.bound_z1(ref, st, ar.cam_E(sc))
    ar.capped(b, ref, "z1")
    worst["z1"] = _ratio(z["z1"], ref, b, f"{what} z1")
    ref = ar.layer_ref("block1.2", rr.lrelu(z["z1"].double()), st)
    ar.capped(ar.LOCAL * ar.amax(ref), ref, "z2")
    worst["z2"] = _ratio(z["z2"], ref, ar.LOCAL * ar.amax(ref), f"{what} z2")
    zin = z["z2"]
    if variant[0]:
        ref = ar.zb_ref(z["z2"].double(), P["bpnet"][sc.pid] if variant[1] else None, st)
        ar.capped(ar.LOCAL * ar.amax(ref), ref, "zb")
        worst["zb"] = _ratio(z["zb"], ref, ar.LOCAL * ar.amax(ref), f"{what} zb")
        zin = z["zb"]
    _, ext, rw, _ = rr.row_inputs_ref(P, sc.camera, sc.raydir, sc.query, K)
    ref = ar.z3_ref(zin.double(), ext, st)
    b = ar.bound_z3(ref, st)
    ar.capped(b, ref, "z3")
    worst["z3"] = _ratio(z["z3"], ref, b, f"{what} z3")
    # f_s and alpha_s from the kernel's z3 through the one cut the library does not expose
    fs_r, a_r, z4_r, _ = ar.blend_ref(z["z3"].double(), rw[:, 0], sc.item, items, st)
    b = ar.bound_fs(z4_r, rw[:, 0], sc.item, items)
    ar.capped(b, fs_r, "f_s")
    worst["f_s"] = _ratio(r["fs"][:items], fs_r, b.clamp(min=1e-300), f"{what} f_s")
    assert bool((_bits(r["fs"][items:sc.S_cap]) == -1).all())          # f_s rows past the items: untouched
    b = ar.alpha_bar(z["z3"], rw[:, 0], sc.item, items, st, a_r)
    ar.capped(b, a_r, "alpha_s", unit=True)
    worst["alpha_s"] = _ratio(r["feat"][sc.work.long(), 0], a_r, b, f"{what} alpha_s")
    check_feat_untouched(sc, r["feat"], r["feat0"], rgb_written=False)
    print(f"{what} worst ratios:", {k: round(v, 3) for k, v in worst.items()})


@pytest.mark.parametrize("name,variant", SAVE_CASES, ids=_id)
def test_save_mode(name, variant):
    r = saved(name, variant)
    _check_save(name, variant, False, r)
    r2 = run_save(name, variant)                                         # two runs: the same bits
    for k in ("feat", "z1", "z2", "zb", "z3", "fs"):
        assert _same_bits(r[k], r2[k]), k


@pytest.mark.parametrize("name,variant", [("pairs", (0, 0)), ("pairs_hi", (0, 0)), ("rand5_777", (0, 0)), ("one", (0, 0)),
                                          ("none", (0, 0)), ("rand8_300", (1, 96))], ids=_id)
def test_save_mode_compact_rows(name, variant):
    """d_row_off given: the rows at row_off[s] + k.  Same values as the NULL form, bit for bit."""
    sc = ar.scene(name)
    r = run_save(name, variant, compact=True)
    _check_save(name, variant, True, r)
    r0 = saved(name, variant)
    idx = sc.rs * sc.K + sc.rk
    for k in ("z1", "z2", "z3") + (("zb",) if variant[0] else ()):
        assert _same_bits(r[k][:sc.rows], r0[k][idx]), k
    assert _same_bits(r["feat"], r0["feat"]) and _same_bits(r["fs"], r0["fs"])


@pytest.mark.parametrize("name,variant", [("pairs", v) for v in VARIANTS] + [("pairs_hi", v) for v in VARIANTS] +
                         [("pairs_shuf", (0, 0)), ("pairs53", (0, 0)), ("rand8_300", (1, 96)), ("rand8_300", (1, 0))], ids=_id)
def test_pairing_does_not_change_a_bit(name, variant, monkeypatch):
    """SGN_PAIR=0 (read per call) runs every sample alone in its half: the same bits in every output, in the save
    and the render instantiation."""
    r = saved(name, variant)
    rr1 = _ok(run_render(name, variant, stages=3), "sgn_aggregate_f32")
    monkeypatch.setenv("SGN_PAIR", "0")
    r0 = run_save(name, variant)
    rr0 = _ok(run_render(name, variant, stages=3), "sgn_aggregate_f32")
    for k in ("feat", "z1", "z2", "zb", "z3", "fs"):
        assert _same_bits(r[k], r0[k]), k
    sc = ar.scene(name)
    for k in ("feat", "blend", "wnorm"):
        assert _same_bits(rr1[k], rr0[k]), k
    assert _same_bits(fs_of(rr1["ws"], sc.S_cap)[:sc.items].cpu(), fs_of(rr0["ws"], sc.S_cap)[:sc.items].cpu())


# ---- c. the render mode: sgn_aggregate_f32(stages = 1), k_rows16<.., NS = 2> --------------------------

@pytest.mark.parametrize("name,variant", SAVE_CASES, ids=_id)
def test_render_mode(name, variant):
    sc = ar.scene(name)
    st = weights(variant)[0]
    what = f"render {name} {variant}"
    r = _ok(run_render(name, variant, stages=1), "sgn_aggregate_f32")
    _, _, rw, _ = rr.row_inputs_ref(sc.points, sc.camera, sc.raydir, sc.query, sc.K)
    check_slots(sc, r["blend"], r["wnorm"], rw, what)
    check_feat_untouched(sc, r["feat"], r["feat0"], rgb_written=False)
    fs = fs_of(r["ws"], sc.S_cap).cpu()
    assert bool((_bits(fs[sc.items:sc.S_cap]) == -1).all())
    # k_pair_slots' table is what the restated rule gives (blocks of 1024 items land in atomic order: compared sorted)
    assert slots_of(r["ws"], sc.S_cap) == sorted(ar.pair_slots(sc.work_counts))
    s = saved(name, variant)
    same = _same_bits(r["feat"], s["feat"]) and _same_bits(fs[:sc.items], s["fs"][:sc.items])
    da = float((r["feat"][sc.work.long(), 0].double() - s["feat"][sc.work.long(), 0].double()).abs().max()) if sc.items else 0.0
    df = float((fs[:sc.items].double() - s["fs"][:sc.items].double()).abs().max()) if sc.items else 0.0
    print(f"{what}: render vs save mode bit-identical: {same} (max |d alpha_s| {da:.3e}, max |d f_s| {df:.3e})")
    if RENDER_EQUALS_SAVE:
        assert same
    elif sc.items and sc.rows <= 4000:
        check_chain(sc, st, dict(alpha=r["feat"][sc.work.long(), 0], fs=fs[:sc.items]), what)
    r2 = _ok(run_render(name, variant, stages=1), "sgn_aggregate_f32")
    assert _same_bits(r["feat"], r2["feat"]) and _same_bits(r["blend"], r2["blend"]) and _same_bits(r["wnorm"], r2["wnorm"])


@pytest.mark.parametrize("name", ["rand8_300", "rand3_777"])
def test_render_mode_given_pers(name):
    """pt->pers / samp_pers given (the PERS instantiations): the camera-space dists are single fp32 operations on the
    given values; everything against the float64 chain that starts from those same fp32 values."""
    sc = ar.scene(name)
    st = weights()[0]
    r = _ok(run_render(name, stages=1, pers=True), "sgn_aggregate_f32")
    n = sc.S_cap * sc.K
    idx = sc.rs * sc.K + sc.rk
    valid = torch.zeros(n, dtype=torch.bool)
    valid[idx] = True
    assert bool((r["blend"][:n][~valid] == 0).all()) and bool((r["wnorm"][:n][~valid] == 0).all()) and _all_nan(r["blend"][n:])
    _, _, rw, _ = rr.row_inputs_ref(sc.points, sc.camera, sc.raydir, sc.query, sc.K)
    check_slots(sc, r["blend"], r["wnorm"], rw, f"render {name} pers")     # the weights read the world dists only
    check_feat_untouched(sc, r["feat"], r["feat0"], rgb_written=False)
    fs = fs_of(r["ws"], sc.S_cap).cpu()
    check_chain(sc, st, dict(alpha=r["feat"][sc.work.long(), 0], fs=fs[:sc.items], blend=r["blend"], wnorm=r["wnorm"]),
                f"render {name} pers", pers=dev(name, True).pers)


# ---- d. the colour stage alone: sgn_aggregate_f32(stages = 2), k_color16 ------------------------------

class ColourDev:
    def __init__(self, case):
        self.case = c = case
        up = lambda t: t.contiguous().to(DEV)  # noqa: E731
        work = torch.cat([c.work, torch.full((c.S_cap - c.items,), -1, dtype=torch.int32)])
        self.d = d = dict(raydir=up(c.raydir), samp_ray=up(c.samp_ray), work=up(work),
                          counters=up(torch.tensor([c.S, c.items, 0, 0], dtype=torch.int32)),
                          f=torch.zeros(64, device=DEV), i=torch.zeros(c.S_cap * 8 + 64, dtype=torch.int32, device=DEV))
        pt = self.pt = _lib.PointTables()
        pt.xyz = pt.embedding = pt.color = pt.dir = pt.conf = pt.campos = pt.camrotc2w = d["f"].data_ptr()   # not read by stage 2
        pt.n_points = 1
        pt.raydir = d["raydir"].data_ptr()
        qo = self.qo = _lib.QueryOut()
        qo.ray_ns = qo.ray_soff = qo.samp_d = qo.samp_nnb = qo.pidx = d["i"].data_ptr()
        qo.samp_locw = d["f"].data_ptr()
        qo.samp_ray, qo.work, qo.counters = d["samp_ray"].data_ptr(), d["work"].data_ptr(), d["counters"].data_ptr()
        self.ws = new_ws(c.S_cap)
        self.proj = torch.zeros(272, device=DEV)

    def run(self, fs, feat0):
        c = self.case
        fs_of(self.ws, c.S_cap)[:c.items] = fs.to(DEV)
        feat = torch.cat([feat0, torch.full((GUARD, 4), NAN)]).to(DEV)
        _, packed, _ = weights()
        _lib.check(L().sgn_aggregate_f32(0, 0, None, _lib.ptr(self.proj), ctypes.byref(self.pt), ctypes.byref(self.qo), c.S_cap, 8,
                                         _lib.ptr(packed), _lib.ptr(feat), None, None, _lib.ptr(self.ws), self.ws.numel(), 2,
                                         _lib.stream_handle()), "sgn_aggregate_f32 stages 2")
        torch.cuda.synchronize()
        return feat.cpu(), flag_of(self.ws)


def _check_colour(c, feat, feat0, fs, skip=None, what=""):
    assert _all_nan(feat[c.S_cap:]) and _same_bits(feat[:c.S_cap, 0], feat0[:, 0])       # guard rows; alpha is not this stage's
    is_item = torch.zeros(c.S_cap, dtype=torch.bool)
    is_item[c.work.long()] = True
    assert _same_bits(feat[:c.S_cap][~is_item], feat0[~is_item])
    bar, ref = ar.colour_bar(c, weights()[0], fs)
    got = feat[c.work.long(), 1:]
    if skip is not None:
        keep = torch.ones(c.items, dtype=torch.bool)
        keep[skip] = False
        got, ref = got[keep], ref[keep]
    return _ratio(got, ref, bar, f"colour stage rgb {what}")


@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("items", [0, 1, 127, 128, 129, P_COLOUR + 3])
def test_colour_stage(items, shuffle):
    c = ar.colour_case(items, shuffle)
    cd = ColourDev(c)
    feat, flag = cd.run(c.fs, c.feat0)
    _check_colour(c, feat, c.feat0, c.fs, what=f"(items={items}, shuffled={shuffle})")
    assert flag == 0
    feat2, _ = cd.run(c.fs, c.feat0)
    assert _same_bits(feat, feat2)


def test_colour_stage_range_flag():
    """The flag at sgn_aggregate_flag_offset_f32: set by a sample whose activations leave fp16 range or whose alpha
    is not finite, cleared by the next call's colour stage; the other samples of a flagged call are unharmed."""
    c = ar.colour_case(129)
    cd = ColourDev(c)
    assert cd.run(c.fs, c.feat0)[1] == 0
    fs = c.fs.clone()
    fs[77] = 1e6
    feat, flag = cd.run(fs, c.feat0)
    assert flag == 1
    _check_colour(c, feat, c.feat0, fs, skip=77, what="(one f_s row of 1e6: the other samples)")
    assert cd.run(c.fs, c.feat0)[1] == 0
    f0 = c.feat0.clone()
    f0[int(c.work[5]), 0] = NAN
    feat, flag = cd.run(c.fs, f0)
    assert flag == 1
    _check_colour(c, feat, f0, c.fs, what="(a NaN alpha)")
    feat, flag = cd.run(c.fs, c.feat0)
    assert flag == 0
    _check_colour(c, feat, c.feat0, c.fs, what="(clean again)")


# ---- e. fp16 range at kernel level --------------------------------------------------------------------

def test_range_inside_and_outside():
    """block1.2 scaled so the float64 chain's largest hidden activation is ~4.2e4 (inside fp16's range: flag 0, every
    bar holds) and ~2.5e5 (outside: the flag is raised)."""
    name = "rand8_300"
    sc = ar.scene(name)
    st = weights((0, 0), "inside")[0]
    h = ar.chain(sc, st)["hidden"]
    assert 3e4 <= h <= 6e4
    r = _ok(run_render(name, stages=3, kind="inside"), "sgn_aggregate_f32")
    assert flag_of(r["ws"]) == 0
    check_feat_untouched(sc, r["feat"], r["feat0"], rgb_written=True)
    w = sc.work.long()
    check_chain(sc, st, dict(alpha=r["feat"][w, 0], rgb=r["feat"][w, 1:], fs=fs_of(r["ws"], sc.S_cap)[:sc.items].cpu(),
                             blend=r["blend"], wnorm=r["wnorm"]), f"range inside (hidden {h:.3e})")
    assert ar.chain(sc, weights((0, 0), "outside")[0])["hidden"] > 1e5
    r = _ok(run_render(name, stages=3, kind="outside"), "sgn_aggregate_f32")
    assert flag_of(r["ws"]) == 1
    r = _ok(run_render(name, stages=3), "sgn_aggregate_f32")     # the unscaled weights: clean
    assert flag_of(r["ws"]) == 0


# ---- f. a workspace smaller than S_capacity items: the chunked host path ---------------------------------

@pytest.mark.parametrize("variant", [(0, 0), (1, 96)], ids=_id)
def test_chunked_workspace(variant):
    name = "pairs75"
    sc = ar.scene(name)
    assert sc.items == 75 and sc.S_cap > 75
    small = int(L().sgn_aggregate_workspace_bytes_f32(32))
    assert int(L().sgn_aggregate_fs_offset_f32(small, sc.S_cap)) == -1
    assert int(L().sgn_aggregate_fs_offset_f32(int(L().sgn_aggregate_workspace_bytes_f32(sc.S_cap)), sc.S_cap)) == 0
    for stages in (1, 2):        # the stages alone need every item's f_s row: an argument error, nothing launched
        assert run_render(name, variant, stages=stages, ws_items=32)["rc"] != 0
    full = _ok(run_render(name, variant, stages=3), "sgn_aggregate_f32")
    part = _ok(run_render(name, variant, stages=3, ws_items=32), "sgn_aggregate_f32 (32-item workspace)")
    for k in ("feat", "blend", "wnorm"):
        assert _same_bits(full[k], part[k]), k
    assert flag_of(part["ws"]) == 0
    check_feat_untouched(sc, part["feat"], part["feat0"], rgb_written=True)
    w = sc.work.long()
    check_chain(sc, weights(variant)[0], dict(alpha=part["feat"][w, 0], rgb=part["feat"][w, 1:], blend=part["blend"],
                                              wnorm=part["wnorm"]), f"chunked {variant}")
    xfull = _ok(run_render(name, variant, exact=True), "sgn_aggregate_exact")
    xpart = _ok(run_render(name, variant, exact=True, ws_bytes=3 * 1024), "sgn_aggregate_exact (3-KiB workspace)")
    for k in ("feat", "blend", "wnorm"):
        assert _same_bits(xfull[k], xpart[k]), k
    assert bool((xpart["ws"][3 * 1024:] == 255).all())     # a 3-item workspace: nothing past it written


# ---- g. sgn_aggregate_exact ----------------------------------------------------------------------------

@pytest.mark.parametrize("name,variant,pers", [("pairs", (0, 0), False), ("pairs", (1, 96), False), ("pairs", (1, 0), False),
                                               ("pairs_hi", (0, 0), False), ("rand3_777", (0, 0), False),
                                               ("rand3_777", (0, 0), True), ("pairs", (0, 0), True),
                                               (f"rand1_{P_EXACT + 3}", (0, 0), False)], ids=_id)
def test_exact(name, variant, pers):
    sc = ar.scene(name)
    r = _ok(run_render(name, variant, pers=pers, exact=True), "sgn_aggregate_exact")
    n = sc.S_cap * sc.K
    idx = sc.rs * sc.K + sc.rk
    valid = torch.zeros(n, dtype=torch.bool)
    valid[idx] = True
    assert bool((r["blend"][:n][~valid] == 0).all()) and bool((r["wnorm"][:n][~valid] == 0).all())
    assert _all_nan(r["blend"][n:]) and _all_nan(r["wnorm"][n:])
    check_feat_untouched(sc, r["feat"], r["feat0"], rgb_written=True)
    ws = r["ws"].cpu()
    assert bool((ws[sc.items * 1024:] == 255).all())        # f_s rows past the items, and the guard
    fs = ws[:sc.items * 1024].view(torch.float32).view(sc.items, 256)
    w = sc.work.long()
    check_chain(sc, weights(variant)[0], dict(alpha=r["feat"][w, 0], rgb=r["feat"][w, 1:], fs=fs, blend=r["blend"], wnorm=r["wnorm"]),
                f"exact {name} {variant}{' pers' if pers else ''}", pers=dev(name, True).pers if pers else None)
    r2 = _ok(run_render(name, variant, pers=pers, exact=True), "sgn_aggregate_exact")
    assert _same_bits(r["feat"], r2["feat"])


def test_zz_file_time():
    print(f"tests/test_agg_rows_gpu.py: {time.time() - T0:.1f} s since import")
