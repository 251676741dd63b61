"""GPU tests of what the HIP training steps carry from one step to the next: the f32 step's
partial point projection, the per-capacity caches of both steps and the row-sparse point Adam's replay,
over four views of different batch sizes that read mostly different point rows.

Trainer A runs the four steps.  Before each of steps 2-4 a fresh trainer B (and B', for the run-to-run
spread) is built from A's state through public surfaces only -- sync_points(), clones of the point
tensors, mlp_state(), both optimizers' state_dict(), step_count -- and runs that one step under the same
seed: whatever A carried over (projection rows made with older weights, buffers sized for another
batch, rows behind the optimizer's step) must not show."""
import copy
from dataclasses import replace
from types import SimpleNamespace

import pytest
import torch

import train_state_ref as ts
from helpers import small_room
from sgnerf_amd.opts import HotPathOpts
from sgnerf_amd.render import HipRenderer, PointTables
from sgnerf_amd.train import PointParams
from sgnerf_amd.train_hip import HipTrainer
from sgnerf_amd.weights import init_mlp
from test_train_cpu import O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
N_POINTS, SEED = 60_000, 7
POINTS = ("points_embeding", "points_color", "points_dir", "points_conf")


def _config(name):
    pc = small_room(N_POINTS, seed=SEED)
    mlp = init_mlp(SEED, bias_std=0.01)
    mlp["alpha_branch.0.bias"] = mlp["alpha_branch.0.bias"] + 100.0   # as test_train_cpu._setup
    c = SimpleNamespace(name=name, pc=pc, opts=O, mlp=mlp, precision="f32", graph=None, bp=None, sg=False)
    if name.startswith("f16"):
        c.precision, c.graph = "f16", name == "f16_graph"
    elif name == "sg_f32":
        import math
        g = torch.Generator().manual_seed(11)
        bound = math.sqrt(6.0 / (256 + 96 + 256)) * 0.5
        c.mlp["block2_bpnet.0.weight"] = (torch.rand(256, 256 + 96, generator=g) * 2 - 1) * bound
        c.mlp["block2_bpnet.0.bias"] = torch.randn(256, generator=g) * 0.01
        c.bp = torch.rand(N_POINTS, 96, generator=g) - 0.5
        c.opts = replace(O, shading_feature_mlp_layer2_bpnet=1, predict_semantic=1, semantic_guidance=1)
        c.sg = True
    elif name == "nb3_rows":
        c.opts = HotPathOpts(SR=O.SR, shading_feature_mlp_layer3=0, is_train=1, train_rows=1).check_supported()
        c.mlp = init_mlp(3, bias_std=0.05, block3_layers=0)
    return c


def _make(c, st=None):
    """A fresh trainer on the initial state, or on a snapshot of another trainer's."""
    pc = c.pc
    if st is None:
        points = PointParams(pc.xyz, pc.embedding, pc.color, pc.dir, pc.conf, DEV)
        mlp = c.mlp
    else:
        points = PointParams(pc.xyz, st["points_embeding"], st["points_color"], st["points_dir"], st["points_conf"], DEV)
        mlp = st["mlp"]
    tr = HipTrainer(points, mlp, replace(c.opts), DEV, precision=c.precision, bpnet=c.bp)
    if c.graph is not None:
        tr.use_graph = c.graph
    if st is not None:
        tr.opt_net.load_state_dict(copy.deepcopy(st["opt_net"]))
        tr.opt_pts.load_state_dict(copy.deepcopy(st["opt_pts"]))
        tr.step_count = st["step_count"]
    return tr


def _snapshot(tr):
    tr.sync_points()
    st = {k: getattr(tr.points, k).detach().clone() for k in POINTS}
    st["mlp"] = {k: v.detach().clone() for k, v in tr.mlp_state().items()}
    st["opt_net"] = copy.deepcopy(tr.opt_net.state_dict())
    st["opt_pts"] = copy.deepcopy(tr.opt_pts.state_dict())
    st["step_count"] = tr.step_count
    return st


def _backward(tr, c, i):
    """Step i + 1's forward and backward; returns the outputs, clones of the gradients and the step's rows."""
    v = ts.view(i)
    R = v.raydir.shape[0]
    d = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
    gt = torch.rand(R, 3, generator=torch.Generator().manual_seed(i)).to(DEV)
    labels = (torch.zeros(N_POINTS, dtype=torch.int32), torch.ones(R, dtype=torch.int32), 10) if c.sg else None
    torch.manual_seed(100 + i + 1)
    parts, full, mask = tr.backward(d(v.campos), d(v.camrotc2w), d(v.raydir), 0.1, 8.0, gt, labels)
    torch.cuda.synchronize()
    grads = {k: getattr(tr.points, k).grad.detach().clone() for k in tr.trained}
    grads["mlp"] = tr.mlp.flat.grad.detach().clone()
    pb = tr.opt_pts._rows[0]   # the step's pend list: int64 count, int32 rows from byte 16
    n = int(pb[:8].view(torch.int64).item())
    assert int(pb[8:16].view(torch.int64).item()) == 0
    rows = torch.sort(pb[16:].view(torch.int32)[:n].long()).values.cpu()
    assert torch.equal(rows, ts.touched_from_pidx(tr.last_query["pidx"].cpu().numpy()))
    return SimpleNamespace(parts={k: float(x) for k, x in parts.items()}, full=full.clone(), mask=mask.clone(),
                           grads=grads, rows=rows)


def _spread_check(what, a, b, b2, f32, log, bad):
    """A against B per element under 4 x |B - B'| + 4 u max|B| (capped at 1e-5 max|B| at f32)."""
    a, b, b2 = a.double(), b.double(), b2.double()
    top = float(b.abs().max())
    spread = (b - b2).abs()
    margin = 4 * spread + 4 * U * top
    if f32:
        margin = margin.clamp(max=1e-5 * top)
    err = (a - b).abs()
    ratio = float((err / margin.clamp_min(1e-300)).max()) if top > 0 else float(err.max() > 0)
    log.append(f"{what}: max|B| {top:.3e} spread {float(spread.max()) / max(top, 1e-300):.2e} "
               f"|A-B| {float(err.max()) / max(top, 1e-300):.2e} of max, worst |A-B| / margin {ratio:.3f}")
    if ratio > 1.0:
        bad.append(f"{what}: |A - B| / margin {ratio:.3f}")


@pytest.mark.parametrize("name", ["f32", "f16_graph", "f16_eager", "sg_f32", "nb3_rows"])
def test_carried_state_equals_a_fresh_trainer(name):
    c = _config(name)
    f32 = c.precision == "f32"
    A = _make(c)
    touched, log, bad = [], [], []
    for i in range(4):
        B = B2 = None
        if i >= 1:
            st = _snapshot(A)
            B, B2 = _make(c, st), _make(c, st)
        ra = _backward(A, c, i)
        touched.append(ra.rows)
        if B is not None:
            rb, rb2 = _backward(B, c, i), _backward(B2, c, i)
            tag = f"{name} step {i + 1}"
            assert torch.equal(ra.rows, rb.rows) and torch.equal(ra.mask, rb.mask) and int(ra.mask.sum()) > 0
            if f32:   # the forward has no atomics: loss parts and colour bit for bit
                if ra.parts != rb.parts:
                    bad.append(f"{tag}: loss parts {ra.parts} != {rb.parts}")
                if not torch.equal(ra.full, rb.full):
                    bad.append(f"{tag}: colour differs, max {float((ra.full - rb.full).abs().max()):.3e}")
            else:
                log.append(f"{tag}: B == B' colour {torch.equal(rb.full, rb2.full)} parts {rb.parts == rb2.parts}; "
                           f"A == B colour {torch.equal(ra.full, rb.full)} parts {ra.parts == rb.parts}")
                _spread_check(f"{tag} colour", ra.full, rb.full, rb2.full, False, log, bad)
                for k in ra.parts:
                    m = 4 * abs(rb.parts[k] - rb2.parts[k]) + 4 * U * abs(rb.parts[k])
                    if abs(ra.parts[k] - rb.parts[k]) > m:
                        bad.append(f"{tag}: loss part {k} {ra.parts[k]!r} vs {rb.parts[k]!r}, margin {m:.3e}")
            for k in ra.grads:
                assert float(rb.grads[k].abs().max()) > 0
                same = torch.equal(rb.grads[k], rb2.grads[k])
                if k == "mlp" and f32 and same:   # reduced in fixed order: bit for bit
                    log.append(f"{tag} grad mlp: B == B', A == B {torch.equal(ra.grads[k], rb.grads[k])}")
                    if not torch.equal(ra.grads[k], rb.grads[k]):
                        d = (ra.grads[k] - rb.grads[k]).abs().max() / rb.grads[k].abs().max()
                        bad.append(f"{tag}: flat MLP gradient differs from the fresh trainer's ({float(d):.2e} of max) "
                                   "while two fresh trainers agree bit for bit")
                else:
                    if k == "mlp" and f32:
                        log.append(f"{tag} grad mlp: B != B' on this GPU, spread rule")
                    _spread_check(f"{tag} grad {k}", ra.grads[k], rb.grads[k], rb2.grads[k], f32, log, bad)
            # the update: rows the step did not touch replay one zero-gradient step, exactly
            before = {k: st[k] for k in A.trained}
            for t in (A, B):
                t.apply()
                t.sync_points()
            rest = torch.ones(N_POINTS, dtype=torch.bool)
            rest[ra.rows] = False
            rest = rest.to(DEV)
            slept = touched[i - 1][~torch.isin(touched[i - 1], ra.rows)].to(DEV)   # moved by the replay alone
            assert slept.numel() > 0
            for k, pa, pb_ in zip(A.trained, A.point_params, B.point_params):
                if not torch.equal(pa.detach()[rest], pb_.detach()[rest]):
                    bad.append(f"{tag}: untouched rows of {k} differ after the update")
                if torch.equal(pa.detach()[slept], before[k][slept]):
                    bad.append(f"{tag}: the previous step's rows of {k} did not move in this step's replay")
                for key in ("exp_avg", "exp_avg_sq"):
                    if not torch.equal(A.opt_pts.state[pa][key][rest], B.opt_pts.state[pb_][key][rest]):
                        bad.append(f"{tag}: untouched rows of {k}.{key} differ after the update")
            if f32 and torch.equal(ra.grads["mlp"], rb.grads["mlp"]) and not torch.equal(A.mlp.flat, B.mlp.flat):
                bad.append(f"{tag}: equal flat gradients, different flat parameters")
        else:
            A.apply()
    fresh, sleepers = ts.check_condition(touched)   # the condition on the inputs, from the GPU's own lists
    log.append(f"{name}: rows per step {[t.numel() for t in touched]}, fresh {['%.2f' % f for f in fresh]}, "
               f"sleepers {sleepers.numel()}")
    print("\n".join(log))
    assert not bad, "\n".join(bad)


def test_render_after_training_equals_a_renderer_on_cloned_state():
    """A HipRenderer over trainer A's live point tensors (built before training, so whatever it caches
    predates the four steps) renders a fifth view, after sync_points() and set_mlp(), bit for bit as a
    renderer built from clones of the final state."""
    c = _config("f32")
    A = _make(c)
    P = A.points
    o = replace(O, precision="f32")
    live = HipRenderer(PointTables(P.xyz, P.points_embeding.detach(), P.points_color.detach(), P.points_dir.detach(),
                                   P.points_conf.detach(), DEV), c.mlp, o, DEV)
    assert live.points.embedding.data_ptr() == P.points_embeding.data_ptr()   # live, not a copy
    v = ts.view(4)
    d = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
    args = (d(v.campos), d(v.camrotc2w), d(v.raydir), 0.1, 8.0)
    first = live.render(*args).rgb.clone()
    for i in range(4):
        _backward(A, c, i)
        A.apply()
    A.sync_points()
    live.set_mlp(A.mlp_state())
    got = live.render(*args)
    got = [x.clone() for x in (got.rgb, got.ray_mask, got.bg_transmission, got.opacity)]
    st = _snapshot(A)
    fresh = HipRenderer(PointTables(c.pc.xyz, st["points_embeding"], st["points_color"], st["points_dir"],
                                    st["points_conf"], DEV), st["mlp"], o, DEV)
    ref = fresh.render(*args)
    assert int(got[1].sum()) > 0 and not torch.equal(got[0], first)   # the training moved the picture
    for x, y in zip(got, (ref.rgb, ref.ray_mask, ref.bg_transmission, ref.opacity)):
        assert torch.equal(x, y)
