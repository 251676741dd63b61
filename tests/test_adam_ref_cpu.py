"""CPU checks of tests/adam_ref.py, the float64 references tests/test_adam_gpu.py holds the Adam
kernels to: the one-step reference against torch.optim.Adam on float64 tensors, the lazy row model
against the dense one, and the error bound against an fp32 emulation of adam_el's operations."""
import numpy as np
import torch

import adam_ref as ar

BETAS = (0.9, 0.999)


def test_one_step_reference_matches_torch_adam_float64():
    g = torch.Generator().manual_seed(1)
    sizes = (7, 130, 1003)
    p0 = [torch.randn(n, generator=g, dtype=torch.float64) for n in sizes]
    tp = [torch.nn.Parameter(x.clone()) for x in p0]
    opt = torch.optim.Adam(tp, lr=2e-3, betas=BETAS, eps=1e-8, foreach=False)
    p = [x.clone() for x in p0]
    m = [torch.zeros_like(x) for x in p0]
    v = [torch.zeros_like(x) for x in p0]
    for it in range(20):
        lr = 2e-3 * 0.93 ** it
        opt.param_groups[0]["lr"] = lr
        for i, n in enumerate(sizes):
            gr = torch.randn(n, generator=g, dtype=torch.float64) * 10.0 ** (it % 5 - 3)
            gr[::5] = 0.0
            tp[i].grad = gr.clone()
            p[i], m[i], v[i] = ar.adam_step(p[i], gr, m[i], v[i], lr, BETAS, 1e-8, it + 1)
        opt.step()
        for i in range(len(sizes)):
            torch.testing.assert_close(p[i], tp[i].detach(), rtol=1e-12, atol=1e-12)
            torch.testing.assert_close(m[i], opt.state[tp[i]]["exp_avg"], rtol=1e-12, atol=1e-14)
            torch.testing.assert_close(v[i], opt.state[tp[i]]["exp_avg_sq"], rtol=1e-12, atol=1e-16)


def test_lazy_row_model_equals_dense_exactly():
    g = torch.Generator().manual_seed(2)
    n, widths, steps = 97, (5, 3, 1), 40
    p0 = [torch.randn(n, w, generator=g) for w in widths]
    dense, lazy = ar.DenseAdam(p0), ar.LazyRowAdam(p0)
    sleepers = torch.tensor([90, 91, 92])
    for it in range(steps):
        rows = torch.unique(torch.randint(0, 90, (12,), generator=g))
        if it in (2, 33):
            rows = torch.unique(torch.cat([rows, sleepers]))   # touched at step 3, next at step 34
        lr = 2e-3 * 0.97 ** it
        gs = [torch.randn(rows.numel(), w, generator=g, dtype=torch.float64) for w in widths]
        full = []
        for w, gr in zip(widths, gs):
            f = torch.zeros(n, w, dtype=torch.float64)
            f[rows] = gr
            full.append(f)
        lazy.bring(rows, it)
        for i in range(len(widths)):   # a row equals the dense state whenever it is read
            assert torch.equal(lazy.p[i][rows], dense.p[i][rows])
        dense.step(full, lr)
        lazy.step(rows, gs, lr)
    assert int(lazy.last.min()) < steps   # some rows still sleep: the flush has work to do
    lazy.flush()
    assert torch.equal(lazy.last, torch.full((n,), steps))
    for i in range(len(widths)):
        assert torch.equal(lazy.p[i], dense.p[i])
        assert torch.equal(lazy.m[i], dense.m[i])
        assert torch.equal(lazy.v[i], dense.v[i])


def _adam_el_fp32(p, g, m, v, lr, betas, eps, step):
    """adam_el's operation sequence in numpy float32 (every operation rounded once, no contraction)."""
    f = np.float32
    b1, b2 = betas
    ss, bs = ar.adam_constants(lr, betas, step)
    b1f, b2f, o1, o2, ssf, bsf, ef = f(b1), f(b2), f(1.0 - b1), f(1.0 - b2), f(ss), f(bs), f(eps)
    m = b1f * m + o1 * g
    v = b2f * v + o2 * g * g
    d = np.sqrt(v) / bsf + ef
    return p - ssf * m / d, m, v


def test_bound_covers_an_fp32_emulation_and_stays_below_the_bar():
    """The bound of adam_step_bound holds for numpy's fp32 evaluation of the same operation sequence
    (worst ratio below 1, and not vacuous: above 0.05), over gradients from 1e-12 to 1e4, carried
    moments and steps 1 .. 100000; its max stays below 1e-6 of max(|p|, lr) and of the moments' max."""
    g = torch.Generator().manual_seed(3)
    n = 20_000
    worst = [0.0, 0.0, 0.0]
    for step in (1, 2, 10, 1000, 100000):
        lr = 2e-3
        p = torch.randn(n, generator=g)
        mag = 10.0 ** (torch.rand(n, generator=g) * 16 - 12)
        gr = torch.randn(n, generator=g).sign() * mag
        m = torch.randn(n, generator=g) * mag * (step > 1)
        v = ((0.05 + torch.rand(n, generator=g)) * mag * mag * (step > 1)).float()
        m = m.float()
        gr = gr.float()
        got = _adam_el_fp32(p.numpy(), gr.numpy(), m.numpy(), v.numpy(), lr, BETAS, 1e-8, step)
        ref = ar.adam_step(p, gr, m, v, lr, BETAS, 1e-8, step)
        bnd = ar.adam_step_bound(p, gr, m, v, lr, BETAS, 1e-8, step)
        for i in range(3):
            err = (torch.from_numpy(got[i]).double() - ref[i]).abs()
            assert bool((err <= bnd[i]).all()), (step, i, float((err / bnd[i].clamp_min(1e-300)).max()))
            worst[i] = max(worst[i], float((err / bnd[i].clamp_min(1e-300)).max()))
        assert float(bnd[0].max()) < 1e-6 * max(float(p.abs().max()), lr)
        assert float(bnd[1].max()) < 1e-6 * float(ref[1].abs().max())
        assert float(bnd[2].max()) < 1e-6 * float(ref[2].abs().max())
    print("fp32 emulation, worst error / bound (p, m, v):", ["%.3f" % w for w in worst])
    assert min(worst) > 0.05


def test_train_state_views_meet_the_sleeper_condition():
    """The four views of tests/test_train_state_gpu.py on the oracle's query of small_room(60_000): steps
    2-4 each read at least 20 % rows the step before did not touch, and step 4 reads rows that step 1
    touched and steps 2-3 did not (row 0 is read by every step and is not one of them)."""
    import oracle_query as oq
    import train_state_ref as ts
    from helpers import hyper_for, small_room, t_table
    from test_train_cpu import O
    pc = small_room(60_000, seed=7)
    grid = oq.OracleGrid(pc.xyz, hyper_for(pc, O), O)
    touched = []
    for i in range(4):
        v = ts.view(i)
        assert v.raydir.shape[0] == (192, 63, 192, 110)[i]
        q = grid.query(v.campos, v.raydir, t_table(O).numpy())
        valid = np.arange(O.SR)[None, :] < q["ray_ns"][:, None]
        touched.append(ts.touched_from_pidx(q["pidx"][valid]))
    fresh, sleepers = ts.check_condition(touched)
    print("rows per step", [t.numel() for t in touched], "fresh fractions", ["%.2f" % f for f in fresh],
          "sleepers", sleepers.numel())
    assert 0 not in sleepers.tolist() and sleepers.numel() >= 10
