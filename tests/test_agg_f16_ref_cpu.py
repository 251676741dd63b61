"""tests/agg_f16_ref.py proven without a GPU.

Roundings off: in float64, with the weights unrounded, its forward functions are agg_rows_ref.chain (z1 .. z4, f_s,
alpha_s) and its backward functions torch autograd of that chain (the deltas as dL/dz per layer, the embedding,
colour and direction gradients) to 1e-10; conf's straight-through clamp is pinned to sgnerf_amd.train.aggregate.
Roundings on: an fp32 torch emulation of every cut (fp16 casts where the kernels cast, fp32 dots, the padded row
layout and the column maps applied) passes every checker, with every bound under its cap.
Planted errors: each makes the named cut's checker fail, and only that one.
The ambiguity cap: the share of d4 elements with |z4| <= E, from the float64 chain alone, on every scene of
test_agg_f16_gpu.py."""
import copy

import pytest
import torch
import torch.nn.functional as F

import sgnerf_amd  # noqa: F401
from sgnerf_amd.train import PointParams, ViewMLP, aggregate
from sgnerf_amd.weights import init_mlp

import agg_f16_ref as fr
import agg_rows_ref as ar
from train_rows_ref import lrelu, pe

BAR = 1e-10
VARIANTS = [(0, 0), (1, 96), (1, 0)]
C16H = torch.tensor(0.01).half()


def state_of(variant, seed=5):
    return init_mlp(seed, bias_std=0.1, bpnet_layers=variant[0], bpnet_dim=variant[1])


def _close(a, b, what):
    s = float(b.abs().max())
    err = float((a - b).abs().max())
    assert err <= BAR * max(s, 1e-300), f"{what}: {err:.3e} over {s:.3e}"


# ---- roundings off --------------------------------------------------------------------------------
def _exact_chain(sc, st, variant):
    """The module's forward functions strung together in float64 with unrounded weights, on padded rows."""
    net = fr.Net(st, exact=True)
    rows = fr.Rows(sc, bp16=sc.points["bpnet"] if variant == (1, 96) else None, exact=True)
    x0, _ = fr.x0_ref(rows)
    z = {}
    z["z1"], _ = fr.dot(x0, net.W0, net.b0)
    z["z2"], _ = fr.dot(lrelu(z["z1"]), net.W1, net.b1)
    zin = z["z2"]
    if net.sg:
        h = lrelu(z["z2"])
        zin = z["zb"] = fr.dot(h if rows.bp is None else torch.cat([h, rows.bp], dim=1), net.WB, net.bB)[0]
    z["z3"], _ = fr.dot(torch.cat([lrelu(zin), rows.ext], dim=1), net.W2, net.b2)
    o = fr.blend_ref(lrelu(z["z3"]), rows, net)
    return net, rows, z, o


@pytest.mark.parametrize("variant", VARIANTS, ids=str)
@pytest.mark.parametrize("name", ["pairs", "rand4_300"])
def test_forward_functions_are_the_float64_chain(name, variant):
    sc, st = fr.scene(name), state_of(variant)
    _, rows, z, o = _exact_chain(sc, st, variant)
    c = ar.chain(sc, st)
    idx = 8 * sc.item + sc.rk
    for k in z:
        _close(z[k][idx], c[k], k)
    _close(o["z4"][idx], c["z4"], "z4")
    _close(o["fs"], c["fs"], "f_s")
    _close(o["alpha"], c["alpha"], "alpha_s")
    # masked slots hold the encoding of zeros and a zero weight
    m = ~rows.valid
    x0, e = fr.x0_ref(rows)
    assert bool((x0[m][:, :32] == 0).all()) and bool((x0[m][:, 32::2] == 0).all()) and bool((x0[m][:, 33::2] == 1).all())
    assert bool((e[m] == 0).all()) and bool((rows.wgt[m] == 0).all()) and int(m.sum()) > 0


@pytest.mark.parametrize("variant", [(0, 0), (1, 96)], ids=str)
def test_backward_functions_are_autograd_of_the_chain(variant):
    sc, st = fr.scene("pairs"), state_of(variant)
    net, rows, z, o = _exact_chain(sc, st, variant)
    n, N = sc.items, sc.N
    dfs, dalpha, _ = fr.upstream(n)
    dfs, dalpha = dfs.double(), dalpha.double()
    sg = copy.copy(sc)
    sg.points = {k: v.double().requires_grad_(k in ("embedding", "color", "dir")) for k, v in sc.points.items()}
    c = ar.chain(sg, st)
    L = (c["fs"] * dfs).sum() + (c["alpha"] * dalpha).sum()
    zs = ["z4", "z3"] + (["zb"] if net.sg else []) + ["z2", "z1"]
    g = torch.autograd.grad(L, [c[k] for k in zs] + [sg.points[k] for k in ("embedding", "color", "dir")])
    gz = dict(zip(zs, g))
    idx = 8 * sc.item + sc.rk
    zero = torch.zeros(())
    _, _, y, _ = fr.head_ref(o, rows, net, dfs, dalpha, 1.0)
    d4, _ = fr.masked(y, zero, o["z4"] > 0)
    d3, _ = fr.delta_ref(d4, net.W3, z["z3"])
    if net.sg:
        db, _ = fr.delta_ref(d3, net.W2, z["zb"])
        d2, _ = fr.delta_ref(db, net.WB, z["z2"])
        _close(db[idx], gz["zb"], "db")
    else:
        d2, _ = fr.delta_ref(d3, net.W2, z["z2"])
    d1, _ = fr.delta_ref(d2, net.W1, z["z1"])
    for k, d in (("z4", d4), ("z3", d3), ("z2", d2), ("z1", d1)):
        _close(d[idx], gz[k], "d" + k[1])
        assert bool((d[~rows.valid] == 0).all())
    acc = fr.GradAcc(N)
    acc.add(rows, fr.grad_rows(o, rows, net, d1, d3, dfs, dalpha))
    for k, gk in zip(("embedding", "color", "dir"), g[len(zs):]):
        _close(acc.t[k][0], gk, "g_" + k)


def test_conf_gradient_is_train_aggregates_straight_through_clamp():
    sc, st = fr.scene("pairs"), state_of((0, 0))
    net, rows, z, o = _exact_chain(sc, st, (0, 0))
    n = sc.items
    _, dalpha, _ = fr.upstream(n)
    dalpha = dalpha.double()
    drgb = torch.randn(n, 3, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    P, q = sc.points, sc.query
    pp = PointParams(P["xyz"], P["embedding"], P["color"], P["dir"], P["conf"], "cpu").double()
    campos, rot = sc.camera
    feat, _, _ = aggregate(pp, ViewMLP(st).double(), campos.double(), rot.double(), sc.raydir.double(), q["samp_ray"][:sc.S],
                           q["samp_locw"][:sc.S].double(), q["pidx"][:sc.S])
    w = sc.work.long()
    ((feat[w, 0] * dalpha).sum() + (feat[w, 1:] * drgb).sum()).backward()
    # d f_s of the same loss, from the chain's colour stage
    fs = o["fs"].clone().requires_grad_(True)
    v = sc.raydir[q["samp_ray"][w].long()]
    (ar.colour_ref(fs, v, st) * drgb).sum().backward()
    acc = fr.GradAcc(sc.N)
    zero = torch.zeros(8 * n, 256, dtype=torch.float64)
    acc.add(rows, fr.grad_rows(o, rows, net, zero, zero, fs.grad, dalpha))
    got, ref = acc.t["conf"][0], pp.points_conf.grad
    _close(got, ref, "g_conf")
    cf = P["conf"].reshape(-1)
    out = (cf < 1e-4) | (cf > 1.0)
    touched = acc.cnt > 0
    assert int((out & touched).sum()) > 0 and bool((got[out & touched] != 0).any())    # straight through: no clamp mask


# ---- roundings on: an fp32 emulation of the kernels --------------------------------------------------
def lrelu_pk(z32, toward_zero=False):
    v = fr.rn16(z32.double(), toward_zero=True).half() if toward_zero else z32.half()
    return torch.maximum(v, v * C16H)


class Emu:
    """The two kernels in torch fp32 on the CPU, writing the tensors in the kernels' layout."""

    def __init__(self, sc, st, variant, n=None):
        self.variant, self.sg = variant, variant[0] == 1
        self.rows = fr.Rows(sc, n, bp16=sc.points["bpnet"].half() if variant == (1, 96) else None)
        self.net = fr.Net(st)
        self.cm = fr.colmaps()
        w = lambda k: st[k + ".weight"].half().float()  # noqa: E731
        b = lambda k: st[k + ".bias"].float()  # noqa: E731
        self.W = {i: w(k) for i, k in enumerate(("block1.0", "block1.2", "block3.0", "block3.2"))}
        self.b = {i: b(k) for i, k in enumerate(("block1.0", "block1.2", "block3.0", "block3.2"))}
        if self.sg:
            self.W["B"], self.b["B"] = w("block2_bpnet.0"), b("block2_bpnet.0")
        self.T = {k: v.t().contiguous() for k, v in self.W.items()}     # the transposed blob, packed on its own
        self.wa, self.ba = st["alpha_branch.0.weight"].float().reshape(-1), st["alpha_branch.0.bias"].float()

    def forward(self, rtz=None):
        r, cm0, cm1, cm2 = self.rows, *self.cm
        emb, d = r.emb.float(), r.dists.float()
        x0 = torch.cat([emb, pe(emb, 3), pe(d, 5)], dim=-1).half()
        lay = lambda i, x, name: lrelu_pk(x.float() @ self.W[i].t() + self.b[i], rtz == name)  # noqa: E731
        h1 = lay(0, x0, "h1")
        h2 = lay(1, h1, "h2b" if self.sg else "h2")
        t = dict(x0=fr.from_nat(x0, cm1), h1=fr.from_nat(h1, cm0))
        if self.sg:
            t["h2b"] = fr.from_nat(h2, cm0)
            h2 = lay("B", h2 if r.bp is None else torch.cat([h2, r.bp.half()], dim=1), "h2")
        ext = r.ext.float().half()
        h2x = torch.cat([h2, ext], dim=1)
        t["h2"] = fr.from_nat(h2x, cm2)
        h3 = lay(2, h2x, "h3")
        t["h3"] = fr.from_nat(h3, cm0)
        z4 = h3.float() @ self.W[3].t() + self.b[3]
        h4 = torch.maximum(z4, z4 * 0.01)
        wgt, n = r.wgt.float(), r.n
        t["fs"] = (wgt[:, None] * h4).view(n, 8, 256).sum(1).half()
        t["alpha"] = (wgt * F.softplus(h4 @ self.wa + self.ba - 1.0)).view(n, 8).sum(1)
        return t

    def backward(self, t, dfs, dalpha, scale, g0, hook=None, act_hook=None, wgt_d4=None):
        """hook(name, tensor): replaces a stored tensor (natural order) right after it is computed, the later layers
        reading the replaced one; act_hook(name, act): the activation a layer's mask is read from; wgt_d4: the
        weights of d4's first term."""
        r, cm0, _, cm2 = self.rows, *self.cm
        hook = hook or (lambda k, x: x)
        act_hook = act_hook or (lambda k, a: a)
        nat = lambda k: fr.to_nat(t[k], cm0, 256).float()  # noqa: E731
        h3, h1 = nat("h3"), nat("h1")
        h2 = fr.to_nat(t["h2"], cm2, 263).float()[:, :256]
        item = torch.arange(8 * r.n) // 8
        wgt, wn = r.wgt.float(), r.wn.float()
        z4 = h3 @ self.W[3].t() + self.b[3]
        h4 = torch.maximum(z4, z4 * 0.01)
        x1 = h4 @ self.wa + self.ba - 1.0
        al = F.softplus(x1)
        das = dalpha[item] * scale
        dz = wgt * das * torch.sigmoid(x1)
        d = ((wgt if wgt_d4 is None else wgt_d4) * scale)[:, None] * dfs[item] + dz[:, None] * self.wa[None, :]
        mk = lambda y, a: torch.where(a > 0, y, 0.01 * y).half()  # noqa: E731
        o = dict(h4=hook("h4", h4.half()), dza=dz, d4=hook("d4", mk(d, h4)))
        o["d3"] = hook("d3", mk(o["d4"].float() @ self.T[3].t(), act_hook("d3", h3)))
        y2 = o["d3"].float() @ self.T[2].t()
        if self.sg:
            o["db"] = hook("db", mk(y2[:, :256], act_hook("db", h2)))
            o["d2"] = hook("d2", mk(o["db"].float() @ self.T["B"].t()[:, :256], act_hook("d2", nat("h2b"))))
        else:
            o["d2"] = hook("d2", mk(y2[:, :256], act_hook("d2", h2)))
        o["d1"] = hook("d1", mk(o["d2"].float() @ self.T[1].t(), act_hook("d1", h1)))
        dx0 = o["d1"].float() @ self.T[0].t()
        bands = torch.tensor([1.0, 2.0, 4.0])
        emb = r.emb.float()
        arg = emb[:, :, None] * bands
        dpe = dx0[:, 32:224].reshape(-1, 32, 3, 2)
        de = dx0[:, :32] + ((dpe[..., 0] * torch.cos(arg) - dpe[..., 1] * torch.sin(arg)) * bands).sum(-1)
        v = r.v.float()
        dwgt = (h4 * dfs[item]).sum(-1) * scale + al * das
        inv = 1.0 / scale
        terms = dict(embedding=de * inv, color=y2[:, 256:259] * inv, dir=(y2[:, 259:262] + y2[:, 262:263] * v) * inv,
                     conf=(dwgt * wn * inv)[:, None])
        g = {k: g0[k].clone().index_add_(0, r.pid[r.valid], terms[k][r.valid]) for k in terms}
        out = {k: (fr.from_nat(x, cm0) if k != "dza" else x) for k, x in o.items()}
        return out, g


def _check(emu, fwd, bwd, g, dfs, dalpha, scale, g0):
    rep = fr.Report()
    rc = emu.rows.chunk(0, emu.rows.n)
    fr.check_forward(rep, rc, emu.net, fwd)
    acc = fr.GradAcc(emu.rows.N)
    keys = ("h1", "h2", "h3") + (("h2b",) if emu.sg else ())
    fr.check_backward(rep, rc, emu.net, dict(bwd, dfs=dfs, dalpha=dalpha, scale=scale, **{k: fwd[k] for k in keys}), acc)
    fr.check_point_grads(rep, acc, g0, g, scale)
    return rep


EMU_CASES = [(n, v, 4096.0) for n in fr.SMALL_SCENES for v in VARIANTS] + [(n, v, 1.0) for n in ("rand8_300", "pairs") for v in VARIANTS]


@pytest.mark.parametrize("name,variant,scale", EMU_CASES, ids=str)
def test_fp32_emulation_passes_every_checker(name, variant, scale):
    sc, st = fr.scene(name), state_of(variant)
    emu = Emu(sc, st, variant)
    dfs, dalpha, g0 = fr.upstream(sc.items)
    fwd = emu.forward()
    bwd, g = emu.backward(fwd, dfs, dalpha, scale, g0)
    rep = _check(emu, fwd, bwd, g, dfs, dalpha, scale, g0)
    rep.show(f"emulation {name} {variant} scale {scale}")
    rep.assert_ok(name)
    rep.check_caps(name)
    assert fr.masked_rows_zero(emu.rows, dict(bwd), emu.sg)
    assert len(rep.ratio) == (22 if variant[0] == 0 else 24), sorted(rep.ratio)      # every cut ran


def _shift_item(x):
    x = x.clone()
    x[8 * 5:8 * 6] = torch.roll(x[8 * 5:8 * 6], 1, 0)
    return x


def _planted(kind, variant):
    """(forward tensors, backward tensors, gradients, emu, upstream) with one error planted."""
    sc, st = fr.scene("rand8_300"), state_of(variant)
    n = 5 if kind == "ragged" else None       # 40 rows: the second 32-row tile has 8
    emu = Emu(sc, st, variant, n)
    dfs, dalpha, g0 = fr.upstream(emu.rows.n)
    kw, rtz = {}, None
    if kind == "weight swap":         # one element of the transposed block3.2 weight swapped with its neighbour
        T = emu.T[3]
        T[17, 40], T[17, 41] = T[17, 41].clone(), T[17, 40].clone()
    elif kind == "wrong mask":        # block1.2's mask read from h2's tile for one 32-row tile
        h2 = fr.to_nat(emu.forward()["h2"], emu.cm[2], 263).float()[:, :256]
        kw["act_hook"] = lambda k, a: torch.cat([h2[:32], a[32:]]) if k == "d1" else a
    elif kind == "row shift":         # item 5's block1.2 deltas shifted by a row
        kw["hook"] = lambda k, x: _shift_item(x) if k == "d2" else x
    elif kind == "toward zero":       # h3 = lrelu16(fp16 toward zero (z3))
        rtz = "h3"
    elif kind == "masked wgt":        # a masked row's d4 takes its neighbour row's weight
        m = torch.nonzero(~emu.rows.valid)[3]
        w = emu.rows.wgt.float().clone()
        w[m] = w[m - 1] if float(w[m - 1]) > 0 else 0.25
        kw["wgt_d4"] = w
    elif kind == "ragged":            # the last 8 rows of the ragged tile never stored: the pre-fill stays
        kw["hook"] = lambda k, x: torch.cat([x[:-8], torch.full_like(x[-8:], float("nan"))]) if k == "h4" else x
    fwd = emu.forward(rtz)
    bwd, g = emu.backward(fwd, dfs, dalpha, 4096.0, g0, **kw)
    return _check(emu, fwd, bwd, g, dfs, dalpha, 4096.0, g0)


PLANTS = [("weight swap", "d3"), ("wrong mask", "d1"), ("row shift", "d2"), ("toward zero", "h3"), ("masked wgt", "d4"),
          ("ragged", "h4")]


@pytest.mark.parametrize("variant", [(0, 0), (1, 96)], ids=str)
@pytest.mark.parametrize("kind,cut", PLANTS)
def test_planted_error_fails_its_cut_and_only_it(kind, cut, variant):
    rep = _planted(kind, variant)
    print(kind, "->", rep.fail)
    assert rep.failed() == [cut], f"{kind}: failed {rep.failed()}, expected [{cut}]"


# ---- the ambiguity cap, from the reference alone --------------------------------------------------------
@pytest.mark.parametrize("name", sorted(fr._SCENES))
def test_ambiguity_cap(name):
    big = fr.scene(name).items > 1000
    for variant in ([(0, 0)] if big else VARIANTS):
        share = fr.ambiguous_share(fr.scene(name), state_of(variant))
        print(f"{name} {variant}: |z4| <= E on {100 * share:.4f} % of block3.2's pre-activations")
        assert share <= fr.AMBIG_CAP


def test_rn16_is_the_direct_rounding():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(200000, generator=g) * torch.logspace(-9, 4, 200000)       # fp32 values: one rounding to fp16
    x = torch.cat([x, torch.tensor([0.0, -0.0, 1.0, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 65504.0, 1.00048828125, -1.00146484375])])
    assert torch.equal(fr.rn16(x.double()), x.half().double())
    t = fr.rn16(x.double(), toward_zero=True)
    assert bool((t.abs() <= x.double().abs()).all()) and bool(((t - x.double()).abs() < fr.ulp16(x.double())).all())
    v = x.half()
    assert torch.equal(fr.lrelu16(v.double()), torch.maximum(v, v * C16H).double())
