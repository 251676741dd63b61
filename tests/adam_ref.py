"""float64 references of the Adam kernels (csrc/optim.hip): one dense step with its per-element fp32
error bound, and a model of the row-sparse contract of sgn_adam_rows.

The update is torch.optim.Adam's (no weight decay, no amsgrad):
    m' = b1 m + (1 - b1) g;  v' = b2 v + (1 - b2) g^2
    p' = p - (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps),  bc_i = 1 - b_i^step
with every constant formed in double."""
import math

import torch

U = 2.0 ** -24   # unit roundoff of fp32
TINY = 2.0 ** -149   # fp32's subnormal spacing


def adam_constants(lr, betas, step):
    """(step_size, bc2_sqrt) of one step, in double: lr / (1 - b1^step), sqrt(1 - b2^step)."""
    b1, b2 = betas
    return lr / (1.0 - b1 ** step), math.sqrt(1.0 - b2 ** step)


def sched_entry(lr, betas, step):
    """The two fp32 constants sgn_adam_rows keeps per step (d_sched[2 (step - 1)], [2 (step - 1) + 1])."""
    ss, bs = adam_constants(lr, betas, step)
    return torch.tensor([ss, bs], dtype=torch.float64).float()


def adam_step(p, g, m, v, lr, betas, eps, step):
    """One Adam step in float64 on (p, g, m, v) of any dtype; returns new (p, m, v), inputs untouched."""
    p, g, m, v = (x.double() for x in (p, g, m, v))
    b1, b2 = betas
    ss, bs = adam_constants(lr, betas, step)
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    p = p - ss * m / (v.sqrt() / bs + eps)
    return p, m, v


def adam_step_bound(p, g, m, v, lr, betas, eps, step):
    """Per-element bounds (bp, bm, bv) of |kernel - adam_step| when the kernel runs adam_el's fp32
    operations on the same fp32 inputs, u = 2^-24, first order in u with 1 % for the higher orders:

      m' = fl(fl(b1f m) + fl(omb1f g)): each product carries its constant's rounding and its own (2 u),
           the sum one more on both terms                       -> bm = 3 u (|b1 m| + |omb1 g|)
      v' = fl(fl(b2f v) + fl(fl(omb2f g) g)): 2 u, 3 u, + 1 u    -> bv = u (3 b2 v + 4 omb2 g^2)
      s  = fl(sqrt(v')):   s (bv / (2 v') + u)                   (correctly rounded sqrt)
      q  = fl(s / bsf):    the constant and the divide           -> dq = q (bv / (2 v') + 3 u)
      d  = fl(q + epsf):   dd = dq + u eps + u d
      n  = fl(ssf m'):     dn = |ss| bm + 2 u |ss m'|
      r  = fl(n / d):      dr = dn / d + |r| dd / d + u |r|
      p' = fl(p - r):      bp = dr + u |p - r|
    A result below 2^-126 is rounded to fp32's subnormal spacing instead (a sleeping row's m gets there
    within ~850 zero-gradient steps): TINY = 2^-149 is added per such chain (bm, bv, dn, dr).
    """
    p, g, m, v = (x.double() for x in (p, g, m, v))
    b1, b2 = betas
    ss, bs = adam_constants(lr, betas, step)
    t1, t2 = (b1 * m).abs(), ((1.0 - b1) * g).abs()
    bm = 3 * U * (t1 + t2) + TINY
    bv = U * (3 * b2 * v + 4 * (1.0 - b2) * g * g) + TINY
    m1 = b1 * m + (1.0 - b1) * g
    v1 = b2 * v + (1.0 - b2) * g * g
    q = v1.sqrt() / bs
    rel_v = torch.where(v1 > 0, bv / v1.clamp_min(1e-300), torch.zeros_like(v1))
    rel_s = torch.where(rel_v < 1e-3, 0.5 * rel_v, rel_v)   # |sqrt(a) - sqrt(b)| <= |a - b| / sqrt(a) always
    dq = q * (rel_s + 3 * U)
    d = q + eps
    dd = dq + U * eps + U * d
    n = ss * m1
    dn = abs(ss) * bm + 2 * U * n.abs() + TINY
    r = n / d
    dr = dn / d + r.abs() * dd / d + U * r.abs() + TINY
    bp = dr + U * (p - r).abs()
    return 1.01 * bp, 1.01 * bm, 1.01 * bv


class DenseAdam:
    """Dense float64 Adam over a list of tensors sharing a step count."""

    def __init__(self, params, betas=(0.9, 0.999), eps=1e-8):
        self.p = [x.double().clone() for x in params]
        self.m = [torch.zeros_like(x) for x in self.p]
        self.v = [torch.zeros_like(x) for x in self.p]
        self.betas, self.eps, self.step_count = betas, eps, 0

    def step(self, grads, lr):
        self.step_count += 1
        for i, g in enumerate(grads):
            self.p[i], self.m[i], self.v[i] = adam_step(self.p[i], g, self.m[i], self.v[i], lr, self.betas,
                                                        self.eps, self.step_count)


class LazyRowAdam:
    """The row-sparse contract of sgn_adam_rows in float64: last[r] is the step row r holds; bringing a
    row forward replays the steps it missed at g = 0, each with its own constants (lrs[k - 1] is step
    k's lr), and a step with a gradient is that step's update on the rows brought to the step before."""

    def __init__(self, params, betas=(0.9, 0.999), eps=1e-8):
        self.p = [x.double().clone() for x in params]
        self.m = [torch.zeros_like(x) for x in self.p]
        self.v = [torch.zeros_like(x) for x in self.p]
        self.last = torch.zeros(self.p[0].shape[0], dtype=torch.long)
        self.betas, self.eps, self.lrs = betas, eps, []

    def bring(self, rows, upto):
        """Rows `rows` (distinct) to step `upto` by zero-gradient steps."""
        rows = torch.as_tensor(rows, dtype=torch.long)
        for k in range(int(self.last[rows].min()) + 1 if rows.numel() else upto + 1, upto + 1):
            sel = rows[self.last[rows] < k]
            for i in range(len(self.p)):
                z = torch.zeros_like(self.p[i][sel])
                self.p[i][sel], self.m[i][sel], self.v[i][sel] = adam_step(
                    self.p[i][sel], z, self.m[i][sel], self.v[i][sel], self.lrs[k - 1], self.betas, self.eps, k)
            self.last[sel] = k

    def step(self, rows, grads, lr):
        """Step len(lrs) + 1 on `rows` (distinct; grads[i] holds their rows' gradients, [len(rows), w])."""
        rows = torch.as_tensor(rows, dtype=torch.long)
        t = len(self.lrs) + 1
        self.bring(rows, t - 1)
        self.lrs.append(lr)
        for i, g in enumerate(grads):
            self.p[i][rows], self.m[i][rows], self.v[i][rows] = adam_step(
                self.p[i][rows], g, self.m[i][rows], self.v[i][rows], lr, self.betas, self.eps, t)
        self.last[rows] = t

    def flush(self):
        self.bring(torch.arange(self.last.numel()), len(self.lrs))


def replay_zero_grad(p, m, v, last, lrs, betas, eps, upto):
    """Rows [n, w] (float64) brought from last[r] to step `upto` by zero-gradient steps, step k with
    lr lrs[k - 1]: returns (p, m, v) and the per-element sums over the replayed steps of
    adam_step_bound: the per-step bound times the number of replayed steps, each step's own."""
    p, m, v = p.double().clone(), m.double().clone(), v.double().clone()
    bp, bm, bv = torch.zeros_like(p), torch.zeros_like(m), torch.zeros_like(v)
    z = torch.zeros_like(p)
    for k in range(int(last.min()) + 1, upto + 1):
        sel = (last < k).reshape(-1, 1)
        p1, m1, v1 = adam_step(p, z, m, v, lrs[k - 1], betas, eps, k)
        b = adam_step_bound(p, z, m, v, lrs[k - 1], betas, eps, k)
        p, m, v = torch.where(sel, p1, p), torch.where(sel, m1, m), torch.where(sel, v1, v)
        bp = bp + torch.where(sel, b[0], z)
        bm = bm + torch.where(sel, b[1], z)
        bv = bv + torch.where(sel, b[2], z)
    return (p, m, v), (bp, bm, bv)
